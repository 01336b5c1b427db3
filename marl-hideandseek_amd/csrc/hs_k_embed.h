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
//   reduce    the two sums of the LayerNorm over the channels: a lane adds its kCh channels in ascending order, then
//             log2(kLanes) xor shuffles (1, 2, 4, ...): float addition commutes, so every lane holds the same bits.
//   store     a wave stores E consecutive features (and E argmax bytes) per table.
// Nothing in a row's features depends on the grid, on the row's position or on the path its bytes took.
//
// The backward recomputes z, mu and rstd from the rows and produces the gradient of the parameters alone.  It works
// table by table: inside a table's pass a lane keeps the table's (K + 3) kCh sums (dW, db, dgamma, dbeta of its
// channels; at most 48 kCh registers) over all the rows its wave takes, in round order.  After the pass the waves of a
// workgroup add their sums in LDS in the order ((w0 + w1) + w2) + w3 (at E = 32 the two halves of a wave first, half 0 +
// half 1), and the workgroup writes them to its slice [blockIdx.x][102 E] of a workspace.  The grid is capped at
// kEmbMaxGridBwd so that the workspace has a fixed size; k_embed_grad_sum adds the slices in a fixed order
// (k_twohot_stats_sum's pattern).  Rows past n are staged as zeros and take part with dy = 0: they add +-0.
// No atomics, no scratch: the same inputs give the same bits on every call.
#pragma once
#include "hs_k_pack.h"                     // the row's layout
#include "hs_k_sample.h"                   // SampleBf16 / SampleF16: the narrow types and their exact widening

namespace hs {

constexpr int kEmbTables = 4;
constexpr int kEmbThreads = 256, kEmbWaves = kEmbThreads / 64;
constexpr int kEmbParamRows = 102;                                      // sum over the tables of K + 3, in rows of E floats
constexpr int kEmbMaxGrid = 2048;                                       // forward: 256 CUs x 8 workgroups
constexpr int kEmbMaxGridBwd = 512;                                     // backward: the slices of the workspace
constexpr int kEmbMaxE = 128;
constexpr int kEmbSumSegs = 8;
constexpr int kEmbSumCols = 32;

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
    static constexpr int kRows = kEmbWaves * kSub;      // rows per workgroup and round
};
__host__ __device__ constexpr int emb_rows(int E) { return E == 32 ? EmbCfg<32>::kRows : EmbCfg<64>::kRows; }
__host__ __device__ constexpr int emb_grid(int n, int E, int cap) {
    const int nb = (n + emb_rows(E) - 1) / emb_rows(E);
    return nb < cap ? nb : cap;
}

enum { kEmbF32 = 0, kEmbBf16 = 1, kEmbF16 = 2 };       // element types, chosen at run time: a wave-uniform branch per access

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

HSD float emb_load(const void *p, int type, size_t i) {
    if (type == kEmbF32) return ((const float *)p)[i];
    if (type == kEmbBf16) return (float)((const SampleBf16 *)p)[i];
    return (float)((const SampleF16 *)p)[i];
}
HSD void emb_store(void *p, int type, size_t i, float v) {
    if (type == kEmbF32) ((float *)p)[i] = v;
    else if (type == kEmbBf16) ((SampleBf16 *)p)[i] = (SampleBf16)v;
    else ((SampleF16 *)p)[i] = (SampleF16)v;
}

template <typename T> struct alignas(16) EmbVec { T v[16 / sizeof(T)]; };

// `nel` consecutive elements from src + first, widened, to dst[0 .. nel): the wave's 64 lanes, 16 bytes each where `vec`
template <typename T> HSD void emb_stage_rows(const T *src, size_t first, int nel, bool vec, float *dst, int lane) {
    constexpr int kPer = 16 / (int)sizeof(T);
    if (vec) {                                                     // first is a multiple of kPackRow, which is one of kPer
        const EmbVec<T> *s = (const EmbVec<T> *)(src + first);
        for (int i = lane; i < nel / kPer; i += 64) {
            const EmbVec<T> v = s[i];
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

// the sum over an entity's E channels of p[q] (this lane's channels): ascending q, then the xor butterfly 1, 2, 4, ...
template <int E> HSD float emb_sum(const float (&p)[EmbCfg<E>::kCh]) {
    float s = p[0];
    _Pragma("unroll") for (int q = 1; q < EmbCfg<E>::kCh; ++q) s = s + p[q];
    _Pragma("unroll") for (int m = 1; m < EmbCfg<E>::kLanes; m <<= 1) s = s + __shfl_xor(s, m, EmbCfg<E>::kLanes);
    return s;
}

// LayerNorm of one entity: zhat, y and rstd from z
template <int E>
HSD float emb_norm(const float (&z)[EmbCfg<E>::kCh], const float (&gamma)[EmbCfg<E>::kCh], const float (&beta)[EmbCfg<E>::kCh], float eps,
                   float (&zhat)[EmbCfg<E>::kCh], float (&y)[EmbCfg<E>::kCh]) {
    constexpr int kCh = EmbCfg<E>::kCh;
    const float mu = emb_sum<E>(z) / (float)E;
    float d[kCh], dd[kCh];
    _Pragma("unroll") for (int q = 0; q < kCh; ++q) { d[q] = z[q] - mu; dd[q] = d[q] * d[q]; }
    const float var = emb_sum<E>(dd) / (float)E;
    const float rstd = 1.0f / sqrtf(var + eps);
    _Pragma("unroll") for (int q = 0; q < kCh; ++q) { zhat[q] = d[q] * rstd; y[q] = fmaf(zhat[q], gamma[q], beta[q]); }
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
            if (a.features) emb_store(a.features, a.featType, (size_t)row * (4 * E) + G * E + c, best[q]);
            if (G > 0 && a.argmax) a.argmax[((size_t)row * 3 + (G - 1)) * E + c] = (unsigned char)arg[q];
        }
    }
}

template <int E>
__global__ __launch_bounds__(kEmbThreads) void k_embed_fwd(EmbedArgs a) {
    using Cfg = EmbCfg<E>;
    __shared__ float params[kEmbParamRows * E];
    __shared__ alignas(16) float X[kEmbWaves][Cfg::kSub * kPackRow];
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64, sub = lane / Cfg::kLanes, cl = lane % Cfg::kLanes;
    for (int i = tid; i < kEmbParamRows * E; i += kEmbThreads) params[i] = a.params[i];
    const bool vec = ((uintptr_t)a.rows & 15u) == 0;
    const int nrounds = (a.n + Cfg::kRows - 1) / Cfg::kRows;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row0 = round * Cfg::kRows + wave * Cfg::kSub;                // the wave's first row
        const int left = a.n - row0, nrow = left < 0 ? 0 : left < Cfg::kSub ? left : Cfg::kSub;
        __syncthreads();                                                       // the previous round's readers are done (first: none)
        const size_t first = (size_t)row0 * kPackRow;
        if (a.rowsType == kEmbF32) emb_stage_rows((const float *)a.rows, first, nrow * kPackRow, vec, X[wave], lane);
        else if (a.rowsType == kEmbBf16) emb_stage_rows((const SampleBf16 *)a.rows, first, nrow * kPackRow, vec, X[wave], lane);
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
// P: LDS for the table's parameters [(K + 3) E], then reused for the waves' sums; X: [kEmbWaves][kSub][NE K].
template <int E, int G>
HSD void emb_bwd_table(const EmbedBwdArgs &a, float *P, float *Xall) {
    using Cfg = EmbCfg<E>;
    constexpr int kCh = Cfg::kCh, K = emb_K(G), NE = emb_N(G), W = NE * K, kP = (K + 3) * E;
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64, sub = lane / Cfg::kLanes, cl = lane % Cfg::kLanes;
    float *X = Xall + wave * (Cfg::kSub * W);
    __syncthreads();                                                           // the previous table's sums have left P
    for (int i = tid; i < kP; i += kEmbThreads) P[i] = a.params[emb_prow(G) * E + i];
    float dW[K][kCh], db[kCh], dg[kCh], dbt[kCh], gamma[kCh], beta[kCh];
    _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
        db[q] = dg[q] = dbt[q] = 0.f;
        _Pragma("unroll") for (int k = 0; k < K; ++k) dW[k][q] = 0.f;
    }
    const int nrounds = (a.n + Cfg::kRows - 1) / Cfg::kRows;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row0 = round * Cfg::kRows + wave * Cfg::kSub;
        const int left = a.n - row0, nrow = left < 0 ? 0 : left < Cfg::kSub ? left : Cfg::kSub;
        __syncthreads();
        for (int i = lane; i < Cfg::kSub * W; i += 64) {                       // the table's columns of the wave's rows; zeros past n
            const int s = i / W, c = i - s * W;
            X[i] = s < nrow ? emb_load(a.rows, a.rowsType, (size_t)(row0 + s) * kPackRow + emb_col(G) + c) : 0.f;
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
                gf[q] = on ? emb_load(a.gradFeatures, a.gradType, (size_t)row * (4 * E) + G * E + c) : 0.f;
                am[q] = (G > 0 && on) ? (int)a.argmax[((size_t)row * 3 + (G - 1)) * E + c] : 0;
            }
            emb_dot<E, K, NE>(P, x, cl, z);
            _Pragma("unroll") for (int j = 0; j < NE; ++j) {
                bool sel = false;
                _Pragma("unroll") for (int q = 0; q < kCh; ++q) sel = sel || (on && am[q] == j);
                if (!__any(sel)) continue;                                     // wave-uniform: no channel of these rows chose entity j
                float zhat[kCh], y[kCh], dy[kCh], h[kCh], hz[kCh];
                const float rstd = emb_norm<E>(z[j], gamma, beta, a.eps, zhat, y);
                _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
                    dy[q] = (on && am[q] == j) ? gf[q] * (y[q] >= 0.f ? 1.0f : a.slope) : 0.f;
                    h[q] = gamma[q] * dy[q];
                    hz[q] = h[q] * zhat[q];
                }
                const float mh = emb_sum<E>(h) / (float)E, mhz = emb_sum<E>(hz) / (float)E;
                _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
                    const float dz = rstd * ((h[q] - mh) - zhat[q] * mhz);
                    _Pragma("unroll") for (int k = 0; k < K; ++k) dW[k][q] = fmaf(x[j * K + k], dz, dW[k][q]);
                    db[q] = db[q] + dz;
                    dg[q] = fmaf(dy[q], zhat[q], dg[q]);
                    dbt[q] = dbt[q] + dy[q];
                }
            }
        }
    }
    // the halves of a wave (E = 32), then the waves in the order ((w0 + w1) + w2) + w3, through P
    if (Cfg::kSub == 2) {
        _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
            _Pragma("unroll") for (int k = 0; k < K; ++k) dW[k][q] = __shfl(dW[k][q], cl, 64) + __shfl(dW[k][q], cl + 32, 64);
            db[q] = __shfl(db[q], cl, 64) + __shfl(db[q], cl + 32, 64);
            dg[q] = __shfl(dg[q], cl, 64) + __shfl(dg[q], cl + 32, 64);
            dbt[q] = __shfl(dbt[q], cl, 64) + __shfl(dbt[q], cl + 32, 64);
        }
    }
    for (int w = 0; w < kEmbWaves; ++w) {
        __syncthreads();                                                       // w = 0: every wave is done with the parameters
        if (wave == w && sub == 0) {
            _Pragma("unroll") for (int q = 0; q < kCh; ++q) {
                const int c = cl + 64 * q;
                _Pragma("unroll") for (int k = 0; k < K; ++k) P[k * E + c] = w == 0 ? dW[k][q] : P[k * E + c] + dW[k][q];
                P[K * E + c] = w == 0 ? db[q] : P[K * E + c] + db[q];
                P[(K + 1) * E + c] = w == 0 ? dg[q] : P[(K + 1) * E + c] + dg[q];
                P[(K + 2) * E + c] = w == 0 ? dbt[q] : P[(K + 2) * E + c] + dbt[q];
            }
        }
    }
    __syncthreads();
    float *out = a.workspace + (size_t)blockIdx.x * (kEmbParamRows * E) + emb_prow(G) * E;
    for (int i = tid; i < kP; i += kEmbThreads) out[i] = P[i];
}

template <int E>
__global__ __launch_bounds__(kEmbThreads) void k_embed_bwd(EmbedBwdArgs a) {
    __shared__ float P[(emb_K(0) + 3) * E];
    __shared__ float X[kEmbWaves * EmbCfg<E>::kSub * emb_N(2) * emb_K(2)];
    emb_bwd_table<E, 0>(a, P, X);
    emb_bwd_table<E, 1>(a, P, X);
    emb_bwd_table<E, 2>(a, P, X);
    emb_bwd_table<E, 3>(a, P, X);
}

// out[i] = sum of workspace[0 .. nparts)[i], i < len, always in the same order: segment sg of kEmbSumSegs adds its slices
// in ascending order onto 0, the segments are added in ascending order (k_twohot_stats_sum's pattern).
template <int kSegs = kEmbSumSegs>
__global__ __launch_bounds__(kEmbSumCols * kSegs) void k_embed_grad_sum(const float *__restrict__ workspace, int nparts, int len, float *__restrict__ out) {
    __shared__ float seg[kSegs][kEmbSumCols];
    const int c = threadIdx.x % kEmbSumCols, sg = threadIdx.x / kEmbSumCols;
    const int i = blockIdx.x * kEmbSumCols + c;
    const int per = (nparts + kSegs - 1) / kSegs;
    const int b0 = sg * per, b1 = b0 + per < nparts ? b0 + per : nparts;
    float s = 0.f;
    if (i < len)
        for (int b = b0; b < b1; ++b) s = s + workspace[(size_t)b * len + i];
    seg[sg][c] = s;
    __syncthreads();
    if (sg == 0 && i < len) {
        float t = seg[0][c];
        for (int k = 1; k < kSegs; ++k) t = t + seg[k][c];
        out[i] = t;
    }
}

}  // namespace hs
