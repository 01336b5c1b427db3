// The entity encoder (hs_entity_encode, hs_entity_encode_backward): the first layer of the reference's SimpleNet
// (scripts/jax_policy.py:113-161) over k_pack's rows.  Every entity of the four tables self [45], agents [5][14],
// boxes [9][17] and ramps [2][14] goes through its table's Dense(E), a LayerNorm and a leaky ReLU; agents, boxes and ramps
// are max-pooled over their entities; the four results make a row of 4 E features.  include/hideseek.h states the
// arithmetic.
//
// It moves 296 elements in and 4 E out per row, and evaluates 296 fmaf per channel and 17 LayerNorms per row.
//   lanes     lane = channel.  kLanes = min(E, 64) lanes hold an entity's channels, kCh = E / kLanes channels each (lane cl
//             holds cl and, at E = 128, cl + 64); at E = 32 the two halves of a wave work on two rows (kSub = 2).  A wave
//             takes kSub consecutive rows per round and a workgroup of four waves kRows = 4 kSub: grid-stride over rounds.
//             Every entity of a row is worked by the same lanes one after the other, so the maximum over the entities and
//             the index of the first entity that attains it stay in registers.
//   stage     the 102 E parameters go to LDS once per workgroup (26 KB at E = 64, 52 KB at E = 128).  Each wave stages its
//             own rows, widened to f32, into its own [kSub][296] piece of LDS: from a 16-byte aligned base lane i loads
//             the i-th 16 bytes of them (a row is 37 or 74 such pieces), else by element; widening is exact, so both paths
//             leave the same image.
//   dot       W_g[k][c] is read once per k and used for every entity of the table (up to 9 accumulators per channel):
//             the 64 lanes read 64 consecutive dwords, one per bank of either half, so without a conflict.  x_k is one
//             address for all lanes of a row: a broadcast, at E = 32 two addresses in two different 32-lane groups.
//   reduce    the sums of the LayerNorm over the channels are hs_rows.h's row_sum over kLanes lanes (StridedMap).
//   store     a wave stores E consecutive features (and E argmax bytes) per table.
// Nothing in a row's features depends on the grid, on the row's position or on the path its bytes took.
//
// The backward recomputes z, mu and rstd from the rows and produces the gradient of the parameters alone.  It works
// table by table: inside a table's pass a lane keeps the table's (K + 3) kCh sums (dW, db, dgamma, dbeta of its
// channels; at most 48 kCh registers) over all the rows its wave takes, in round order.  After the pass the two halves
// of a wave are added at E = 32 (half 0 + half 1), and the sums leave as the table's part of the workgroup's slice
// [blockIdx.x][102 E] of a workspace, as hs_rows.h describes.  Rows past n are staged as zeros and take part with
// dy = 0: they add +-0.  No scratch.
#pragma once
#include "hs_k_pack.h"                     // the row's layout
#include "hs_rows.h"

namespace hs {

constexpr int kEmbTables = 4;
constexpr int kEmbParamRows = 102;                                      // sum over the tables of K + 3, in rows of E floats
constexpr int kEmbMaxE = 128;

__host__ __device__ constexpr int emb_K(int g) { return g == 0 ? kPackColAgents : g == 1 ? kPackAgentW : g == 2 ? kPackBoxW : kPackRampW; }
__host__ __device__ constexpr int emb_N(int g) { return g == 0 ? 1 : g == 1 ? kPackAgentN : g == 2 ? kPackBoxN : kPackRampN; }
__host__ __device__ constexpr int emb_col(int g) { return g == 0 ? 0 : g == 1 ? kPackColAgents : g == 2 ? kPackColBoxes : kPackColRamps; }
// the first row of table g's block W [K][E] | b [E] | gamma [E] | beta [E] in the parameters
__host__ __device__ constexpr int emb_prow(int g) { return g == 0 ? 0 : emb_prow(g - 1) + emb_K(g - 1) + 3; }
static_assert(emb_prow(kEmbTables) == kEmbParamRows && emb_col(3) + emb_N(3) * emb_K(3) == kPackRow, "the four tables tile the row and the parameters");
static_assert(emb_K(0) == 45 && emb_K(0) + 3 == 48, "self is the widest table: 48 rows of sums at the most");

template <int E> struct EmbCfg {
    static_assert(E == 32 || E == 64 || E == 128, "embed_dim");
    static constexpr int kLanes = E < 64 ? E : 64;      // lanes that hold an entity's channels
    static constexpr int kCh = E / kLanes;              // channels per lane
    static constexpr int kSub = 64 / kLanes;            // rows a wave works side by side
    static constexpr int kRows = kRowsWaves * kSub;     // rows per workgroup and round
};
__host__ __device__ constexpr int emb_rows(int E) { return E == 32 ? EmbCfg<32>::kRows : EmbCfg<64>::kRows; }

struct EmbedArgs {
    const void *rows;                     // [n][kPackRow]
    const float *params;                  // [kEmbParamRows * E]
    void *features;                       // [n][4 E], or null
    unsigned char *argmax;                // [n][3][E], or null
    int n, rowsType, featType;
    float eps, slope;
};

struct EmbedBwdArgs {
    const void *rows;
    const float *params;
    const void *gradFeatures;             // [n][4 E]
    const unsigned char *argmax;          // [n][3][E]
    float *workspace;                     // [gridDim.x][kEmbParamRows * E]
    int n, rowsType, gradType;
    float eps, slope;
};

// `nel` consecutive elements from src + first, widened, to dst[0 .. nel): the wave's 64 lanes, 16 bytes each where `vec`
template <typename T> HSD void emb_stage_rows(const T *src, size_t first, int nel, bool vec, float *dst, int lane) {
    constexpr int kPer = 16 / (int)sizeof(T);
    if (vec) {                                                     // first is a multiple of kPackRow, which is one of kPer
        const ElemVec<T, kPer> *s = (const ElemVec<T, kPer> *)(src + first);
        for (int i = lane; i < nel / kPer; i += 64) {
            const ElemVec<T, kPer> v = s[i];
            for (int k = 0; k < kPer; ++k) dst[i * kPer + k] = (float)v.v[k];
        }
    } else {
        for (int i = lane; i < nel; i += 64) dst[i] = (float)src[first + i];
    }
}
static_assert(kPackRow % 8 == 0, "a row is a whole number of 16-byte pieces in every element type");

// z[j][q] = b[c_q] then fmaf(x_k(j), W[k][c_q], .) for ascending k: entity j < NE of a table with K inputs, channel
// c_q = cl + 64 q.  P: the table's block of the parameters, x: the row's first column of the table.
template <int E, int K, int NE>
HSD void emb_dot(const float *P, const float *x, int cl, float (&z)[NE][EmbCfg<E>::kCh]) {
    constexpr int kCh = EmbCfg<E>::kCh;
    _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
        const float b = P[K * E + cl + 64 * q];
        _Pragma("unroll") for (int j = 0; j < NE; ++j) z[j][q] = b;
    }
    _Pragma("unroll") for (int k = 0; k < K; ++k) {
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
            const float w = P[k * E + cl + 64 * q];
            _Pragma("unroll") for (int j = 0; j < NE; ++j) z[j][q] = fmaf(x[j * K + k], w, z[j][q]);
        }
    }
}

// LayerNorm of one entity: zhat, y and rstd from z
template <int E>
HSD float emb_norm(const float (&z)[EmbCfg<E>::kCh], const float (&gamma)[EmbCfg<E>::kCh], const float (&beta)[EmbCfg<E>::kCh], float eps,
                   float (&zhat)[EmbCfg<E>::kCh], float (&y)[EmbCfg<E>::kCh]) {
    const float rstd = row_norm<EmbCfg<E>::kCh, EmbCfg<E>::kLanes>(z, eps, zhat);
    _Pragma("unroll") for (int q = 0; q < EmbCfg<E>::kCh; ++q) y[q] = fmaf(zhat[q], gamma[q], beta[q]);
    return rstd;
}

// One table of one row, forward: the pooled features of this lane's channels and the first entity that attains them.
template <int E, int G>
HSD void emb_fwd_table(const EmbedArgs &a, const float *params, const float *xrow, int cl, int row, bool on) {
    constexpr int kCh = EmbCfg<E>::kCh, K = emb_K(G), NE = emb_N(G);
    const float *P = params + emb_prow(G) * E;
    float z[NE][kCh], gamma[kCh], beta[kCh], best[kCh];
    int arg[kCh];
    emb_dot<E, K, NE>(P, xrow + emb_col(G), cl, z);
    _Pragma("unroll") for (int q = 0; q < kCh; ++q) { gamma[q] = P[(K + 1) * E + cl + 64 * q]; beta[q] = P[(K + 2) * E + cl + 64 * q]; }
    _Pragma("unroll") for (int j = 0; j < NE; ++j) {
        float zhat[kCh], y[kCh];
        emb_norm<E>(z[j], gamma, beta, a.eps, zhat, y);
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
            const float v = y[q] >= 0.f ? y[q] : a.slope * y[q];
            if (j == 0 || v > best[q]) { best[q] = v; arg[q] = j; }           // a tie stays with the lower j
        }
    }
    if (on) {
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
            const int c = cl + 64 * q;
            if (a.features) elem_store(a.features, a.featType, (size_t)row * (4 * E) + G * E + c, best[q]);
            if (G > 0 && a.argmax) a.argmax[((size_t)row * 3 + (G - 1)) * E + c] = (unsigned char)arg[q];
        }
    }
}

template <int E>
__global__ __launch_bounds__(kRowsThreads) void k_embed_fwd(EmbedArgs a) {
    using Cfg = EmbCfg<E>;
    __shared__ float params[kEmbParamRows * E];
    __shared__ alignas(16) float X[kRowsWaves][Cfg::kSub * kPackRow];
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64, sub = lane / Cfg::kLanes, cl = lane % Cfg::kLanes;
    for (int i = tid; i < kEmbParamRows * E; i += kRowsThreads) params[i] = a.params[i];
    const bool vec = ((uintptr_t)a.rows & 15u) == 0;
    const int nrounds = (a.n + Cfg::kRows - 1) / Cfg::kRows;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row0 = round * Cfg::kRows + wave * Cfg::kSub;                // the wave's first row
        const int left = a.n - row0, nrow = left < 0 ? 0 : left < Cfg::kSub ? left : Cfg::kSub;
        __syncthreads();                                                       // the previous round's readers are done (first: none)
        const size_t first = (size_t)row0 * kPackRow;
        if (a.rowsType == kElemF32) emb_stage_rows((const float *)a.rows, first, nrow * kPackRow, vec, X[wave], lane);
        else if (a.rowsType == kElemBf16) emb_stage_rows((const SampleBf16 *)a.rows, first, nrow * kPackRow, vec, X[wave], lane);
        else emb_stage_rows((const SampleF16 *)a.rows, first, nrow * kPackRow, vec, X[wave], lane);
        __syncthreads();                                                       // the rows (and in the first round the parameters) are there
        if (nrow > 0) {                                                        // wave-uniform; a half without a row computes and stores nothing
            const int row = row0 + sub;
            const bool on = sub < nrow;
            const float *xrow = X[wave] + (on ? sub : 0) * kPackRow;
            emb_fwd_table<E, 0>(a, params, xrow, cl, row, on);
            emb_fwd_table<E, 1>(a, params, xrow, cl, row, on);
            emb_fwd_table<E, 2>(a, params, xrow, cl, row, on);
            emb_fwd_table<E, 3>(a, params, xrow, cl, row, on);
        }
    }
}

// One table's pass of the backward over all the rows of the workgroup; leaves the workgroup's sums in its workspace slice.
// P: LDS for the table's parameters [(K + 3) E], then reused for the waves' sums; X: [kRowsWaves][kSub][NE K].
// acc: this lane's sums in the rows of the table's block, dW [K] | db | dgamma | dbeta.
template <int E, int G>
HSD void emb_bwd_table(const EmbedBwdArgs &a, float *P, float *Xall) {
    using Cfg = EmbCfg<E>;
    constexpr int kCh = Cfg::kCh, K = emb_K(G), NE = emb_N(G), W = NE * K, kP = (K + 3) * E;
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64, sub = lane / Cfg::kLanes, cl = lane % Cfg::kLanes;
    float *X = Xall + wave * (Cfg::kSub * W);
    __syncthreads();                                                           // the previous table's sums have left P
    for (int i = tid; i < kP; i += kRowsThreads) P[i] = a.params[emb_prow(G) * E + i];
    float acc[K + 3][kCh], gamma[kCh], beta[kCh];
    _Pragma("unroll") for (int j = 0; j < K + 3; ++j)
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) acc[j][q] = 0.f;
    const int nrounds = (a.n + Cfg::kRows - 1) / Cfg::kRows;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row0 = round * Cfg::kRows + wave * Cfg::kSub;
        const int left = a.n - row0, nrow = left < 0 ? 0 : left < Cfg::kSub ? left : Cfg::kSub;
        __syncthreads();
        for (int i = lane; i < Cfg::kSub * W; i += 64) {                       // the table's columns of the wave's rows; zeros past n
            const int s = i / W, c = i - s * W;
            X[i] = s < nrow ? elem_load(a.rows, a.rowsType, (size_t)(row0 + s) * kPackRow + emb_col(G) + c) : 0.f;
        }
        __syncthreads();
        if (nrow > 0) {
            const int row = row0 + sub;
            const bool on = sub < nrow;
            const float *x = X + sub * W;
            float z[NE][kCh], gf[kCh];
            int am[kCh];
            _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
                const int c = cl + 64 * q;
                gamma[q] = P[(K + 1) * E + c]; beta[q] = P[(K + 2) * E + c];
                gf[q] = on ? elem_load(a.gradFeatures, a.gradType, (size_t)row * (4 * E) + G * E + c) : 0.f;
                am[q] = (G > 0 && on) ? (int)a.argmax[((size_t)row * 3 + (G - 1)) * E + c] : 0;
            }
            emb_dot<E, K, NE>(P, x, cl, z);
            _Pragma("unroll") for (int j = 0; j < NE; ++j) {
                bool sel = false;
                _Pragma("unroll") for (int q = 0; q < kCh; ++q) sel = sel || (on && am[q] == j);
                if (!__any(sel)) continue;                                     // wave-uniform: no channel of these rows chose entity j
                float zhat[kCh], y[kCh], dy[kCh], h[kCh], dz[kCh];
                const float rstd = emb_norm<E>(z[j], gamma, beta, a.eps, zhat, y);
                _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
                    dy[q] = (on && am[q] == j) ? gf[q] * (y[q] >= 0.f ? 1.0f : a.slope) : 0.f;
                    h[q] = gamma[q] * dy[q];
                }
                row_norm_bwd<kCh, Cfg::kLanes>(h, zhat, rstd, dz);
                _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
                    _Pragma("unroll") for (int k = 0; k < K; ++k) acc[k][q] = fmaf(x[j * K + k], dz[q], acc[k][q]);
                    acc[K][q] = acc[K][q] + dz[q];
                    acc[K + 1][q] = fmaf(dy[q], zhat[q], acc[K + 1][q]);
                    acc[K + 2][q] = acc[K + 2][q] + dy[q];
                }
            }
        }
    }
    if (Cfg::kSub == 2) {                                                      // the halves of a wave (E = 32)
        _Pragma("unroll") for (int q = 0; q < kCh; ++q)
            _Pragma("unroll") for (int j = 0; j < K + 3; ++j) acc[j][q] = __shfl(acc[j][q], cl, 64) + __shfl(acc[j][q], cl + 32, 64);
    }
    __syncthreads();                                                           // every wave is done with the parameters
    wave_sums_to_slice<StridedMap<kCh, Cfg::kLanes>>(acc, P, a.workspace + (size_t)blockIdx.x * (kEmbParamRows * E) + emb_prow(G) * E);
}

template <int E>
__global__ __launch_bounds__(kRowsThreads) void k_embed_bwd(EmbedBwdArgs a) {
    __shared__ float P[(emb_K(0) + 3) * E];
    __shared__ float X[kRowsWaves * EmbCfg<E>::kSub * emb_N(2) * emb_K(2)];
    emb_bwd_table<E, 0>(a, P, X);
    emb_bwd_table<E, 1>(a, P, X);
    emb_bwd_table<E, 2>(a, P, X);
    emb_bwd_table<E, 3>(a, P, X);
}

}  // namespace hs
