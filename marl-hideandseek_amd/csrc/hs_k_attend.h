// The attention core of the entity self-attention encoder (hs_entity_attend, hs_entity_attend_backward): what sits
// between the QKV GEMM and the output GEMM of EntitySelfAttentionNet(num_embed_channels, num_out_channels, num_heads = 4)
// (the reference's scripts/jax_policy.py builds its ActorNet and CriticNet from it for hide-and-seek).  A row is S = 17
// tokens (self, 5 agents, 9 boxes, 2 ramps) of E = 4 D channels, D = 16 or 32: per head and query a softmax over at most
// 17 keys.  include/hideseek.h states the arithmetic.  The GEMMs stay with the BLAS library.
//
// A row moves 3 S E values in and S E out (backward: 4 S E in, 3 S E out) and costs about 4 S S E multiply-adds forward and
// 10 S S E backward, all VALU f32: MFMA's order of summation is not ours to state.
//   rows      a wave takes one row per round and a workgroup of four waves four rows, grid-stride, as k_dense does.
//   tasks     a (token, head) pair is a task, t = 4 token + head, 68 per row.  FOUR lanes share a task: lane l works task
//             16 pass + l / 4 and, of the head's D channels, the P = D / 4 adjacent ones from P (l % 4) on.  A row is 5
//             passes: four full ones and one of 4 tasks on 16 lanes, 272 of 320 lane slots (85 %).  One lane per task
//             would take 2 passes for 68 of 128 slots (53 %) and D accumulators per lane; two lanes per task 3 passes
//             (71 %).  With four, a dot product over D is a lane's P terms and two butterfly steps, a lane's piece of a
//             token is 16 or 32 bytes, and the 16 tasks of a pass read one whole token's K (or V) row between them.
//             On the query side the task's token is the query i; on the key side (backward, dK and dV) it is the key j.
//   LDS       K and V of a row in f32 are 17 KB at E = 128, so four rows of both do not fit 64 KB.  A wave has ONE buffer
//             B [17][E] f32 (8.5 KB at E = 128) and stages one operand at a time in it, widened once: K for the scores,
//             then V for the weighted sum.  The probabilities wait in a second buffer M [4][17][17] f32 (4.5 KB), not in
//             registers: 5 passes x 17 of them, with the passes unrolled, took the kernel past 256 VGPRs and to one wave
//             per SIMD; with M the passes are a rolled loop.  The backward goes K, grad_out, V, K, q through B; M holds
//             p for dv, is overwritten in place by ds (a task reads and writes only its own row) for dq and dk, and is
//             what turns both from (query, key) at the query's lanes to the key's lanes.
//             52 KB per workgroup at E = 128 and 35 KB at E = 64: three or four workgroups per CU by LDS.  No scratch.
//   mask      key_mask's 17 bytes become one wave-uniform word by a ballot (bit 0 forced on): a masked key is skipped
//             by a uniform branch, or deselected by the compiler, never multiplied by zero.
// Every round has the same barriers for all four waves; a wave whose row lies past n does nothing between them.
// Nothing in a row's outputs depends on the grid, on n or on the row's position, and there is no cross-row sum.
#pragma once
#include "hs_k_dense.h"                    // dense_load / dense_store: pieces of adjacent elements of run-time type

namespace hs {

constexpr int kAttendTokens = 17, kAttendHeads = 4;
constexpr int kAttendTasks = kAttendTokens * kAttendHeads;                         // 68
constexpr int kAttendTaskLanes = 4, kAttendPassTasks = 64 / kAttendTaskLanes;      // 16 tasks per pass
constexpr int kAttendPasses = (kAttendTasks + kAttendPassTasks - 1) / kAttendPassTasks;      // 5
constexpr int kAttendProbs = kAttendHeads * kAttendTokens * kAttendTokens;         // M: [head][query][key]

struct AttendArgs {
    const void *qkv;                      // [n][17][3][4][D]
    const unsigned char *mask;            // [n][17], or null
    void *out;                            // [n][17][E]
    int n, qkvType, outType;
};

struct AttendBwdArgs {
    const void *qkv;
    const unsigned char *mask;
    const void *gradOut;                  // [n][17][E] of gradType
    void *gradQkv;                        // [n][17][3][4][D] of gradType
    int n, qkvType, gradType;
};

// What a lane works in pass `pass`: the task's token and head, and its first channel within a token's E.
template <int E> struct AttendTask {
    int token, head, c0;
    bool active;
    HSD AttendTask(int pass, int lane) {
        constexpr int D = E / kAttendHeads, P = D / kAttendTaskLanes;
        const int t = pass * kAttendPassTasks + lane / kAttendTaskLanes;
        active = t < kAttendTasks;                                             // false only in the last pass
        const int tt = active ? t : 0;                                         // an idle lane repeats task 0 and stores nothing
        token = tt / kAttendHeads;
        head = tt % kAttendHeads;
        c0 = head * D + P * (lane % kAttendTaskLanes);
    }
};

template <int P> HSD void attend_load(const void *p, int type, size_t i, float (&v)[P]) {
    _Pragma("unroll") for (int k = 0; k < P; k += 4) {
        float t[4];
        dense_load<4>(p, type, i + k, t);
        _Pragma("unroll") for (int c = 0; c < 4; ++c) v[k + c] = t[c];
    }
}
template <int P> HSD void attend_store(void *p, int type, size_t i, const float (&v)[P]) {
    _Pragma("unroll") for (int k = 0; k < P; k += 4) {
        float t[4];
        _Pragma("unroll") for (int c = 0; c < 4; ++c) t[c] = v[k + c];
        dense_store<4>(p, type, i + k, t);
    }
}
template <int P> HSD void attend_lds(const float *B, int i, float (&v)[P]) {
    _Pragma("unroll") for (int k = 0; k < P; k += 4) {
        const ElemVec<float, 4> t = *(const ElemVec<float, 4> *)(B + i + k);
        _Pragma("unroll") for (int c = 0; c < 4; ++c) v[k + c] = t.v[c];
    }
}

// B[token][c] = src[base + token stride + c], widened: the wave's 64 lanes copy 4-element pieces, contiguous per token.
template <int E> HSD void attend_stage(float *B, const void *src, int type, size_t base, int stride, int lane) {
    constexpr int kPieces = kAttendTokens * E / 4, kPerToken = E / 4;
    _Pragma("unroll") for (int k = 0; k < (kPieces + 63) / 64; ++k) {
        const int idx = lane + 64 * k;
        if (idx < kPieces) {
            const int token = idx / kPerToken, c = 4 * (idx % kPerToken);
            float t[4];
            dense_load<4>(src, type, base + (size_t)token * stride + c, t);
            ElemVec<float, 4> o;
            _Pragma("unroll") for (int q = 0; q < 4; ++q) o.v[q] = t[q];
            *(ElemVec<float, 4> *)(B + token * E + c) = o;
        }
    }
}

// the dot product over a head's D channels of this lane's P terms a and b: the lane's terms in ascending order, then the
// butterfly 1, 2 over the task's four lanes (row_sum's order with kLanes = 4)
template <int P> HSD float attend_dot(const float (&a)[P], const float (&b)[P]) {
    float p[P];
    _Pragma("unroll") for (int c = 0; c < P; ++c) p[c] = a[c] * b[c];
    return row_sum<P, kAttendTaskLanes>(p);
}

// The wave-uniform word of the valid keys of `row`: bit j set where key j counts; bit 0 always.
HSD unsigned attend_valid(const unsigned char *mask, int row, int lane) {
    constexpr unsigned all = (1u << kAttendTokens) - 1u;
    if (!mask) return all;
    const bool on = lane < kAttendTokens && mask[(size_t)row * kAttendTokens + lane] != 0;
    return ((unsigned)__ballot(on) & all) | 1u;
}

// M's row of (head, query): its 17 keys
HSD int attend_m(int head, int query) { return (head * kAttendTokens + query) * kAttendTokens; }

// The softmax rows of the wave's row, from K staged in B, into M: M[head][i][j] = p_ij, 0 for a masked key.  The four
// lanes of a task hold the same bits; the first of them writes.  Forward and backward run exactly this.
template <int E>
HSD void attend_probs(const float *B, float *M, const void *qkv, int type, size_t rowBase, unsigned valid, int lane) {
    constexpr int D = E / kAttendHeads, P = D / kAttendTaskLanes, S = kAttendTokens;
    const float scale = 1.0f / sqrtf((float)D);
    _Pragma("unroll 1") for (int pass = 0; pass < kAttendPasses; ++pass) {
        const AttendTask<E> t(pass, lane);
        float q[P], s[S];
        attend_load<P>(qkv, type, rowBase + (size_t)t.token * (3 * E) + t.c0, q);
        _Pragma("unroll") for (int j = 0; j < S; ++j) {
            s[j] = 0.f;
            if (valid >> j & 1u) {
                float k[P];
                attend_lds<P>(B, j * E + t.c0, k);
                s[j] = attend_dot<P>(q, k) * scale;
            }
        }
        float m = s[0];
        _Pragma("unroll") for (int j = 1; j < S; ++j)
            if (valid >> j & 1u) m = fmaxf(m, s[j]);
        float l = 0.f;
        _Pragma("unroll") for (int j = 0; j < S; ++j)
            if (valid >> j & 1u) {
                s[j] = expf(s[j] - m);
                l = j == 0 ? s[j] : l + s[j];
            }
        _Pragma("unroll") for (int j = 0; j < S; ++j)
            if (valid >> j & 1u) s[j] = s[j] / l;
        if (t.active && lane % kAttendTaskLanes == 0) {
            float *Mrow = M + attend_m(t.head, t.token);
            _Pragma("unroll") for (int j = 0; j < S; ++j) Mrow[j] = s[j];
        }
    }
}

// acc[c] = ((+0 + w_0 x_0[c]) + w_1 x_1[c]) + ... over the tokens whose bit is set in `take`, x_r = B[r][c0 + c] and
// w_r = W[r wstride]: the weighted sums of both sides (out and dq with the valid keys, dv and dk with every query).
template <int E, int P> HSD void attend_weighted(const float *B, const float *W, int wstride, unsigned take, int c0, float (&acc)[P]) {
    _Pragma("unroll") for (int c = 0; c < P; ++c) acc[c] = 0.f;
    _Pragma("unroll") for (int r = 0; r < kAttendTokens; ++r)
        if (take >> r & 1u) {
            const float w = W[r * wstride];
            float x[P];
            attend_lds<P>(B, r * E + c0, x);
            _Pragma("unroll") for (int c = 0; c < P; ++c) acc[c] = acc[c] + w * x[c];
        }
}

template <int E>
__global__ __launch_bounds__(kRowsThreads) void k_attend_fwd(AttendArgs a) {
    constexpr int D = E / kAttendHeads, P = D / kAttendTaskLanes, S = kAttendTokens;
    __shared__ __attribute__((aligned(16))) float Bs[kRowsWaves][S * E];
    __shared__ float Ms[kRowsWaves][kAttendProbs];
    const int wave = threadIdx.x / 64, lane = hs_lane() % 64;
    float *B = Bs[wave], *M = Ms[wave];
    const int nrounds = (a.n + kRowsWaves - 1) / kRowsWaves;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {      // the same rounds, and barriers, for all four waves
        const int row = round * kRowsWaves + wave;
        const bool live = row < a.n;                                           // wave-uniform
        const size_t rowBase = (size_t)row * (S * 3 * E);
        unsigned valid = 0;
        __syncthreads();                                                       // the previous round's readers of B and M are done
        if (live) {
            valid = attend_valid(a.mask, row, lane);
            attend_stage<E>(B, a.qkv, a.qkvType, rowBase + E, 3 * E, lane);    // K
        }
        __syncthreads();
        if (live) attend_probs<E>(B, M, a.qkv, a.qkvType, rowBase, valid, lane);
        __syncthreads();
        if (live) attend_stage<E>(B, a.qkv, a.qkvType, rowBase + 2 * E, 3 * E, lane);      // V
        __syncthreads();
        if (live) {
            _Pragma("unroll 1") for (int pass = 0; pass < kAttendPasses; ++pass) {
                const AttendTask<E> t(pass, lane);
                float acc[P];
                attend_weighted<E, P>(B, M + attend_m(t.head, t.token), 1, valid, t.c0, acc);
                if (t.active) attend_store<P>(a.out, a.outType, (size_t)row * (S * E) + t.token * E + t.c0, acc);
            }
        }
    }
}

template <int E>
__global__ __launch_bounds__(kRowsThreads) void k_attend_bwd(AttendBwdArgs a) {
    constexpr int D = E / kAttendHeads, P = D / kAttendTaskLanes, S = kAttendTokens;
    constexpr unsigned all = (1u << S) - 1u;
    __shared__ __attribute__((aligned(16))) float Bs[kRowsWaves][S * E];
    __shared__ float Ms[kRowsWaves][kAttendProbs];
    const int wave = threadIdx.x / 64, lane = hs_lane() % 64;
    float *B = Bs[wave], *M = Ms[wave];
    const float scale = 1.0f / sqrtf((float)D);
    const int nrounds = (a.n + kRowsWaves - 1) / kRowsWaves;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row = round * kRowsWaves + wave;
        const bool live = row < a.n;
        const size_t rowBase = (size_t)row * (S * 3 * E), outBase = (size_t)row * (S * E);
        unsigned valid = 0;
        __syncthreads();                                                       // the previous round's readers of B and M are done
        if (live) {
            valid = attend_valid(a.mask, row, lane);
            attend_stage<E>(B, a.qkv, a.qkvType, rowBase + E, 3 * E, lane);    // K
        }
        __syncthreads();
        if (live) attend_probs<E>(B, M, a.qkv, a.qkvType, rowBase, valid, lane);           // M = p
        __syncthreads();
        if (live) attend_stage<E>(B, a.gradOut, a.gradType, outBase, E, lane);             // grad_out
        __syncthreads();
        if (live) {                                                            // key side: dv_j = sum_i p_ij dout_i
            _Pragma("unroll 1") for (int pass = 0; pass < kAttendPasses; ++pass) {
                const AttendTask<E> t(pass, lane);
                float acc[P];
                attend_weighted<E, P>(B, M + attend_m(t.head, 0) + t.token, S, all, t.c0, acc);
                const bool on = valid >> t.token & 1u;
                _Pragma("unroll") for (int c = 0; c < P; ++c) acc[c] = on ? acc[c] : 0.f;
                if (t.active) attend_store<P>(a.gradQkv, a.gradType, rowBase + (size_t)t.token * (3 * E) + 2 * E + t.c0, acc);
            }
        }
        __syncthreads();
        if (live) attend_stage<E>(B, a.qkv, a.qkvType, rowBase + 2 * E, 3 * E, lane);      // V
        __syncthreads();
        if (live) {                                                            // query side: dp, then ds over p in M, a task its own row
            _Pragma("unroll 1") for (int pass = 0; pass < kAttendPasses; ++pass) {
                const AttendTask<E> t(pass, lane);
                float *Mrow = M + attend_m(t.head, t.token);
                float g[P], p[S], dp[S], dot = 0.f;
                attend_load<P>(a.gradOut, a.gradType, outBase + t.token * E + t.c0, g);
                _Pragma("unroll") for (int j = 0; j < S; ++j) {
                    p[j] = Mrow[j];
                    dp[j] = 0.f;
                    if (valid >> j & 1u) {
                        float v[P];
                        attend_lds<P>(B, j * E + t.c0, v);
                        dp[j] = attend_dot<P>(g, v);
                        dot = dot + p[j] * dp[j];
                    }
                }
                if (t.active && lane % kAttendTaskLanes == 0) {                // after the four lanes' reads: one wave, in order
                    _Pragma("unroll") for (int j = 0; j < S; ++j) Mrow[j] = (valid >> j & 1u) ? p[j] * (dp[j] - dot) : 0.f;
                }
            }
        }
        __syncthreads();                                                       // M = ds
        if (live) attend_stage<E>(B, a.qkv, a.qkvType, rowBase + E, 3 * E, lane);          // K again
        __syncthreads();
        if (live) {                                                            // query side: dq_i = (sum_j ds_ij k_j) scale
            _Pragma("unroll 1") for (int pass = 0; pass < kAttendPasses; ++pass) {
                const AttendTask<E> t(pass, lane);
                float acc[P];
                attend_weighted<E, P>(B, M + attend_m(t.head, t.token), 1, valid, t.c0, acc);
                _Pragma("unroll") for (int c = 0; c < P; ++c) acc[c] = acc[c] * scale;
                if (t.active) attend_store<P>(a.gradQkv, a.gradType, rowBase + (size_t)t.token * (3 * E) + t.c0, acc);
            }
        }
        __syncthreads();
        if (live) attend_stage<E>(B, a.qkv, a.qkvType, rowBase, 3 * E, lane);              // q
        __syncthreads();
        if (live) {                                                            // key side: dk_j = (sum_i ds_ij q_i) scale
            _Pragma("unroll 1") for (int pass = 0; pass < kAttendPasses; ++pass) {
                const AttendTask<E> t(pass, lane);
                float acc[P];
                attend_weighted<E, P>(B, M + attend_m(t.head, 0) + t.token, S, all, t.c0, acc);
                const bool on = valid >> t.token & 1u;
                _Pragma("unroll") for (int c = 0; c < P; ++c) acc[c] = on ? acc[c] * scale : 0.f;
                if (t.active) attend_store<P>(a.gradQkv, a.gradType, rowBase + (size_t)t.token * (3 * E) + E + t.c0, acc);
            }
        }
    }
}

}  // namespace hs
