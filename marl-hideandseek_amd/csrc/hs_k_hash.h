// The SimHash encoder (hs_hash_encode, hs_hash_encode_backward): the reference's HashNet (scripts/jax_policy.py:170-218)
// over k_pack's rows.  A row's 296 columns are projected onto 8 directions, the 8 sign bits are a bin number, the bin
// selects a row of a [256][32] table, and the row is LayerNormed.  include/hideseek.h states the arithmetic.
//
// Forward (k_hash_fwd).  It moves 296 elements in and one byte and 32 channels out per row; the 8 x 296 fmaf are noise.
//   table     the LayerNorm of a table row depends on the parameters alone, so a workgroup normalises the 256 rows once
//             into LDS (32 KB): each of its 8 half-waves takes every 8th row, a lane a channel, hs_rows.h's row_norm over
//             32 lanes.  Every workgroup holds the same bits.
//   stage     a wave takes kHashSub = 2 consecutive rows per round and a workgroup of four waves kHashRows = 8:
//             grid-stride over rounds.  Each wave stages its own rows, widened to f32, into its own piece of LDS with
//             k_embed's emb_stage_rows: lane i loads the i-th 16 bytes of them (rows are 16-byte aligned by contract, and
//             a row is 37 or 74 such pieces).  Widening is exact, so every element type leaves the same image.
//   dot       lane l owns the columns l, l + 64, ..., l + 256 (the last where l < 40) and keeps proj's 8 x 5 values of them
//             in registers for the whole call; per row it reads its 5 columns from LDS (64 consecutive dwords per read:
//             no conflict) and makes 8 partial sums.
//   reduce    the header's butterfly over 64 lanes, folded: at the step m = 1 a lane hands its partner the sums of the
//             bits it does not keep (even lanes keep the even bits), so 4 exchanges carry 8 sums; m = 2 takes 2, m = 4 one,
//             and lane l is left with bit l & 7 for m = 8, 16, 32.  Float addition commutes, so each value is the
//             butterfly's, bit for bit, in 10 exchanges where 48 were.  m = 1, 2 are DPP quad permutes; the rest go
//             through the LDS crossbar (__shfl_xor).  One ballot of lanes 0 .. 7 is the bin.
//   store     lanes 0 .. 31 gather and store the first row's channels, 32 .. 63 the second's: 64 consecutive elements.
// LDS: 32 KB table + 9.25 KB rows; 40 registers of proj.  Nothing in a row's bin or features depends on the grid, on the
// row's position or on n.
//
// Backward.  The substance is G[b][c], the 256-bin sum of the rows' gradients, with plain loads and stores in a fixed
// order, so that the same inputs give the same bits on every call:
//   k_hash_bwd_bins   one workgroup per CU at the most (kHashMaxGridBwd = 256), four waves, each with a private slice
//                     [256][32] f32 of LDS (4 x 32 KB = 128 KB of the CU's 160).  A wave takes 2 rows per round, a
//                     half-wave a row and a lane a channel; the next round's gradient and bin are loaded before this
//                     round's are added.  Where the two halves hold the same bin the first half adds, the wave waits for
//                     its LDS traffic, then the second half adds (else both add at once, to different addresses): the
//                     order inside a slice is row order.  The slices are
//                     added as ((w0 + w1) + w2) + w3 into the workgroup's slice of the workspace.
//   k_partials_sum    hs_rows.h's, the instance k_embed uses: 8 segments over the workgroups' slices, into G, the last
//                     slice of the workspace.
//   k_hash_bwd_table  one workgroup: half-wave h takes the bins 32 h .. 32 h + 31 in ascending order, recomputes the
//                     LayerNorm of the table row, writes d table (hs_rows.h's row_norm_bwd over 32 lanes; +0 for a bin
//                     whose G is all zero) and keeps its segment of d gamma and d beta in registers; the 8 segments are
//                     added in ascending order.  It also writes the +0 of the proj range.
// No scratch.  The three kernels are templates, emitted where their launches (at the end of hideseek.hip) name them.
#pragma once
#include "hs_k_embed.h"                    // emb_stage_rows and, through it, the row's layout and hs_rows.h

namespace hs {

constexpr int kHashBits = 8, kHashBins = 256, kHashFeat = 32;
constexpr int kHashProj = kHashBits * kPackRow;                                // the parameters: proj | table | gamma | beta
constexpr int kHashTableAt = kHashProj, kHashGammaAt = kHashTableAt + kHashBins * kHashFeat, kHashBetaAt = kHashGammaAt + kHashFeat;
constexpr int kHashParams = kHashBetaAt + kHashFeat;
constexpr int kHashSub = 2, kHashRows = kRowsWaves * kHashSub;                 // rows per wave and per workgroup in a round
constexpr int kHashCols = (kPackRow + 63) / 64, kHashTail = kPackRow - 64 * (kHashCols - 1);   // columns per lane; lanes that own a last one
constexpr int kHashMaxGrid = 1024;                                             // forward: 256 CUs x 4 workgroups (LDS: 41 KB each)
constexpr int kHashMaxGridBwd = 256;                                           // backward: a workgroup per CU (LDS: 128 KB each)
constexpr int kHashHalves = kRowsThreads / kHashFeat;                          // half-waves of a workgroup: the segments of the last sums
constexpr int kHashSlice = kHashBins * kHashFeat;
static_assert(kHashFeat == 32 && kHashSub * kHashFeat == 64, "a half-wave holds a row's channels");
static_assert(kHashCols == 5 && kHashTail == 40 && kHashBits == 8, "the lanes' columns and the fold of the butterfly");
static_assert(kHashBins % kHashHalves == 0 && kHashBins / kHashHalves == 32, "a half-wave takes 32 consecutive bins");

struct HashArgs {
    const void *rows;                     // [n][kPackRow], 16-byte aligned
    const float *params;                  // [kHashParams]
    void *features;                       // [n][32]
    unsigned char *bin;                   // [n], or null
    int n, rowsType, featType;
    float eps;
};

struct HashBwdArgs {
    const unsigned char *bin;             // [n]
    const void *gradFeatures;             // [n][32]
    const float *params;
    float *workspace;                     // [kHashMaxGridBwd + 1][kHashSlice]: the workgroups' sums, then G
    float *gradParams;                    // [kHashParams]
    int n, gradType;
    float eps;
};

// the wave's LDS traffic has landed, and the compiler moves no memory access across this point
HSD void hash_wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }

template <int kCtrl> HSD float hash_dpp(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xF, 0xF, false)); }

// One step of the folded butterfly: N sums in, N / 2 out.  A lane whose bit `m` is clear keeps the even ones and hands
// over the odd ones, its partner l xor m the other way round; what is kept is own + partner's, as in the plain butterfly.
template <int N, typename X> HSD void hash_fold(const float (&y)[N], bool upper, X exchange, float (&z)[N / 2]) {
    _Pragma("unroll") for (int k = 0; k < N / 2; ++k) {
        const float keep = upper ? y[2 * k + 1] : y[2 * k], send = upper ? y[2 * k] : y[2 * k + 1];
        z[k] = keep + exchange(send);
    }
}

// The sums of 8 partial sums over the wave's 64 lanes: lane l ends with bit (l & 7)'s, the butterfly's value bit for bit.
HSD float hash_reduce(const float (&y)[kHashBits], int lane) {
    float z4[4], z2[2], z1[1];
    hash_fold<8>(y, lane & 1, [](float v) { return hash_dpp<0xB1>(v); }, z4);                  // quad_perm [1,0,3,2]: l xor 1
    hash_fold<4>(z4, lane & 2, [](float v) { return hash_dpp<0x4E>(v); }, z2);                 // quad_perm [2,3,0,1]: l xor 2
    hash_fold<2>(z2, lane & 4, [](float v) { return __shfl_xor(v, 4, 64); }, z1);
    float s = z1[0];
    _Pragma("unroll") for (int m = 8; m < 64; m <<= 1) s = s + __shfl_xor(s, m, 64);
    return s;
}

// T[b][c] = the LayerNorm of table row b: half-wave h of the workgroup takes the rows h, h + 8, ...
HSD void hash_norm_table(const float *params, float eps, float *T) {
    const int half = threadIdx.x / kHashFeat, c = threadIdx.x % kHashFeat;
    const float gamma = params[kHashGammaAt + c], beta = params[kHashBetaAt + c];
    for (int b = half; b < kHashBins; b += kHashHalves) {
        const float t[1] = {params[kHashTableAt + b * kHashFeat + c]};
        float that[1];
        row_norm<1, kHashFeat>(t, eps, that);
        T[b * kHashFeat + c] = fmaf(that[0], gamma, beta);
    }
}

template <int kThreads = kRowsThreads>
__global__ __launch_bounds__(kThreads) void k_hash_fwd(HashArgs a) {
    __shared__ float T[kHashSlice];
    __shared__ alignas(16) float X[kRowsWaves][kHashSub * kPackRow];
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64, sub = lane / kHashFeat, cl = lane % kHashFeat;
    float P[kHashBits][kHashCols];
    _Pragma("unroll") for (int i = 0; i < kHashBits; ++i)
        _Pragma("unroll") for (int j = 0; j < kHashCols; ++j)
            P[i][j] = (j < kHashCols - 1 || lane < kHashTail) ? a.params[i * kPackRow + lane + 64 * j] : 0.f;
    hash_norm_table(a.params, a.eps, T);
    const int nrounds = (a.n + kHashRows - 1) / kHashRows;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row0 = round * kHashRows + wave * kHashSub;                  // the wave's first row
        const int left = a.n - row0, nrow = left < 0 ? 0 : left < kHashSub ? left : kHashSub;
        __syncthreads();                                                       // the previous round's readers are done (first: none)
        const size_t first = (size_t)row0 * kPackRow;
        if (a.rowsType == kElemF32) emb_stage_rows((const float *)a.rows, first, nrow * kPackRow, true, X[wave], lane);
        else if (a.rowsType == kElemBf16) emb_stage_rows((const SampleBf16 *)a.rows, first, nrow * kPackRow, true, X[wave], lane);
        else emb_stage_rows((const SampleF16 *)a.rows, first, nrow * kPackRow, true, X[wave], lane);
        __syncthreads();                                                       // the rows (and in the first round the table) are there
        if (nrow > 0) {                                                        // wave-uniform
            int bins[kHashSub];
            _Pragma("unroll") for (int s = 0; s < kHashSub; ++s) {
                const float *x = X[wave] + (s < nrow ? s : 0) * kPackRow;      // a wave with one row works it twice
                float y[kHashBits];
                _Pragma("unroll") for (int i = 0; i < kHashBits; ++i) y[i] = 0.f;
                _Pragma("unroll") for (int j = 0; j < kHashCols - 1; ++j) {
                    const float xv = x[lane + 64 * j];
                    _Pragma("unroll") for (int i = 0; i < kHashBits; ++i) y[i] = fmaf(xv, P[i][j], y[i]);
                }
                if (lane < kHashTail) {
                    const float xv = x[lane + 64 * (kHashCols - 1)];
                    _Pragma("unroll") for (int i = 0; i < kHashBits; ++i) y[i] = fmaf(xv, P[i][kHashCols - 1], y[i]);
                }
                bins[s] = (int)(__ballot(hash_reduce(y, lane) > 0.f) & 0xFFull);   // lanes 0 .. 7 hold bits 0 .. 7
            }
            if (sub < nrow) {
                const int row = row0 + sub, b = sub ? bins[1] : bins[0];
                elem_store(a.features, a.featType, (size_t)row * kHashFeat + cl, T[b * kHashFeat + cl]);
                if (a.bin && cl == 0) a.bin[row] = (unsigned char)b;
            }
        }
    }
}

// The gradient and the bin of this lane's row in `round`; bin -1 past n.
HSD void hash_bwd_load(const HashBwdArgs &a, int round, int wave, int sub, int cl, float &g, int &b) {
    const int row = round * kHashRows + wave * kHashSub + sub;
    g = 0.f; b = -1;
    if (row < a.n) {
        g = elem_load(a.gradFeatures, a.gradType, (size_t)row * kHashFeat + cl);
        b = (int)a.bin[row];
    }
}

template <int kThreads = kRowsThreads>
__global__ __launch_bounds__(kThreads) void k_hash_bwd_bins(HashBwdArgs a) {
    __shared__ float S[kRowsWaves][kHashSlice];
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64, sub = lane / kHashFeat, cl = lane % kHashFeat;
    float *mine = S[wave];
    for (int i = lane; i < kHashSlice; i += 64) mine[i] = 0.f;
    hash_wave_sync();
    const int nrounds = (a.n + kHashRows - 1) / kHashRows;
    float g; int b;
    hash_bwd_load(a, blockIdx.x, wave, sub, cl, g, b);
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        float gn = 0.f; int bn = -1;
        if (round + (int)gridDim.x < nrounds) hash_bwd_load(a, round + gridDim.x, wave, sub, cl, gn, bn);
        if (b != __shfl_xor(b, kHashFeat, 64)) {                               // wave-uniform: the halves hold different bins
            if (b >= 0) mine[b * kHashFeat + cl] = mine[b * kHashFeat + cl] + g;
            hash_wave_sync();
        } else {                                                               // one bin: the first row's half, then the second's
            _Pragma("unroll") for (int s = 0; s < kHashSub; ++s) {
                if (sub == s && b >= 0) mine[b * kHashFeat + cl] = mine[b * kHashFeat + cl] + g;
                hash_wave_sync();
            }
        }
        g = gn; b = bn;
    }
    __syncthreads();
    float *out = a.workspace + (size_t)blockIdx.x * kHashSlice;
    for (int i = tid; i < kHashSlice; i += kThreads) out[i] = ((S[0][i] + S[1][i]) + S[2][i]) + S[3][i];
}

// G: the bins' sums [256][32] (the last slice of the workspace).
template <int kThreads = kRowsThreads>
__global__ __launch_bounds__(kThreads) void k_hash_bwd_table(HashBwdArgs a, const float *G) {
    __shared__ float seg[2][kHashHalves][kHashFeat];
    const int tid = threadIdx.x, half = tid / kHashFeat, c = tid % kHashFeat;
    for (int i = tid; i < kHashProj; i += kThreads) a.gradParams[i] = 0.f;
    const float gamma = a.params[kHashGammaAt + c];
    float dgamma = 0.f, dbeta = 0.f;
    for (int i = 0; i < kHashBins / kHashHalves; ++i) {
        const int at = (half * (kHashBins / kHashHalves) + i) * kHashFeat + c;
        const float t[1] = {a.params[kHashTableAt + at]}, g = G[at];
        float that[1], dt[1];
        const float rstd = row_norm<1, kHashFeat>(t, a.eps, that);
        const float h[1] = {gamma * g};
        row_norm_bwd<1, kHashFeat>(h, that, rstd, dt);
        const unsigned long long nz = __ballot(g != 0.f);                      // both halves of the wave; this one's 32 bits
        const bool any = ((nz >> (kHashFeat * (half & 1))) & 0xFFFFFFFFull) != 0ull;
        a.gradParams[kHashTableAt + at] = any ? dt[0] : 0.f;
        dgamma = fmaf(g, that[0], dgamma);
        dbeta = dbeta + g;
    }
    seg[0][half][c] = dgamma; seg[1][half][c] = dbeta;
    __syncthreads();
    if (half < 2) {                                                            // half 0: d gamma, half 1: d beta
        float s = seg[half][0][c];
        for (int k = 1; k < kHashHalves; ++k) s = s + seg[half][k][c];
        a.gradParams[(half == 0 ? kHashGammaAt : kHashBetaAt) + c] = s;
    }
}

}  // namespace hs
