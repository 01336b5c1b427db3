// Action sampling: the actor's logits of every agent row turned into the [rows][5] i32 action quintuple the next step
// reads, with the log-probability and entropy a PPO learner stores (hs_sample_actions) — what the reference's learner
// does with a multi-discrete actor head (scripts/jax_train.py:146-148, actions_num_buckets = [5, 5, 5, 2, 2]).
//
// Row `world * A + slot` has L = sum of buckets[h] logits, head after head, at logits + row * stride (elements of f32,
// bf16 or f16, widened to f32 exactly; all arithmetic is f32).  Head h with K logits l_0 .. l_{K-1}:
//     m = max l_i;  e_i = expf(l_i - m);  c_i = (e_0 + e_1) + ... + e_i in index order;  S = c_{K-1}
//     log_prob_h = (l_a - m) - logf(S)
//     entropy_h  = logf(S) - (sum_i e_i (l_i - m)) / S       in index order; a term with e_i == 0 is exactly 0
// with a = DRAW: the smallest index with u S < c_a, else the last index with e_i > 0 (a bucket with e_i == 0, such as
// one masked with -inf, is never drawn);  GREEDY: the first index of the maximum;  EVALUATE: the stored action, clamped
// into [0, K).  The uniform of (row, head): g = (worldOffset + world) * A + slot, k = threefry2x32(seed, g, counter),
// u = RNG{k, h}.sampleUniform() (hs_core.h), so a draw depends on the global agent row alone and not on how the worlds
// are dealt to handles.  Row sums: (((x_0 + x_1) + x_2) + x_3) + x_4.  A head needs one finite logit; +inf and NaN
// logits are not supported.
//
// It moves little (about 10 MB at 96 000 rows) and is bound by launch and latency.  A workgroup takes kSampleRows
// consecutive rows at a time (grid-stride over row blocks): lane i reads element i of the block's logits, row after row
// (with stride == L one contiguous range), into an LDS image [kSampleRows][L | 1] f32 (the odd pitch spreads the rows
// over the banks).  Then eight lanes per row, five of them at work: lane (row, head) makes its head's action, log_prob and
// entropy and leaves them in LDS.  The block's actions, head_log_prob, log_prob and entropy are contiguous ranges again:
// lane q stores element q, and the lane of a row adds its five head values in the fixed order.  No atomics, no scratch;
// nothing depends on the grid or on the block of rows a row falls into.
#pragma once
#include "hs_core.h"

namespace hs {

constexpr int kSampleHeads = 5, kSampleMaxBuckets = 16, kSampleMaxLogits = 64;
constexpr int kSampleDraw = 0, kSampleGreedy = 1, kSampleEvaluate = 2;
constexpr int kSampleThreads = 256;
constexpr int kSampleLanesPerRow = 8;                                   // five heads, three idle lanes: a row never straddles a wave
constexpr int kSampleRows = kSampleThreads / kSampleLanesPerRow;        // 32 agent rows per block
constexpr int kSampleMaxGrid = 2048;                                    // 256 CUs x the 8 workgroups of 4 waves a CU holds
static_assert(kSampleHeads <= kSampleLanesPerRow && kSampleRows * kSampleHeads <= kSampleThreads, "a lane per (row, head) and per stored element");

typedef __bf16 SampleBf16;
typedef _Float16 SampleF16;

struct SampleArgs {
    const void *logits;
    const int32_t *actionIn;              // EVALUATE: the actions to score
    int32_t *action;                      // DRAW / GREEDY: where the actions go
    const float *selfMask;                // HS_SAMPLE_ZERO_INACTIVE: the self_mask export, else null
    float *logProb, *entropy, *headLogProb;
    uint64_t bucketK, bucketOff;          // byte h: buckets[h] and the row's first logit of head h
    int rows, stride, L, mode;
    uint32_t seed0, seed1, counter, row0Global;      // row0Global = worldOffset * A
};

__host__ __device__ constexpr int sample_grid(int rows) {
    const int nb = (rows + kSampleRows - 1) / kSampleRows;
    return nb < kSampleMaxGrid ? nb : kSampleMaxGrid;
}

struct SampleImage {
    float logit[kSampleRows * (kSampleMaxLogits | 1)];
    int32_t action[kSampleRows * kSampleHeads];
    float logProb[kSampleRows * kSampleHeads], entropy[kSampleRows * kSampleHeads];
};

// One head: K logits at l.  `a` comes in as the stored action (EVALUATE) and goes out as the head's action.
HSD void sample_head(const float *l, int K, int mode, float u, int &a, float &logProb, float &entropy) {
    float m = l[0];
    int amax = 0;
    for (int i = 1; i < K; ++i)
        if (l[i] > m) { m = l[i]; amax = i; }
    float S = 0.f, T = 0.f;
    for (int i = 0; i < K; ++i) {
        const float d = l[i] - m, e = expf(d);
        S = i ? S + e : e;
        const float t = e == 0.f ? 0.f : e * d;
        T = i ? T + t : t;
    }
    if (mode == kSampleGreedy) a = amax;
    else if (mode == kSampleEvaluate) a = a < 0 ? 0 : (a < K ? a : K - 1);
    else {
        const float t = u * S;
        float c = 0.f;
        int last = 0;
        a = -1;
        for (int i = 0; i < K; ++i) {                 // the same e_i and the same sums as above
            const float e = expf(l[i] - m);
            c = i ? c + e : e;
            if (e > 0.f) last = i;
            if (t < c) { a = i; break; }
        }
        if (a < 0) a = last;
    }
    const float logS = logf(S);
    logProb = (l[a] - m) - logS;
    entropy = logS - T / S;
}

template <typename T>
__global__ __launch_bounds__(kSampleThreads) void k_sample(SampleArgs a) {
    __shared__ SampleImage im;
    const T *logits = (const T *)a.logits;
    const int tid = threadIdx.x, L = a.L, pitch = L | 1;
    const int r = tid / kSampleLanesPerRow, h = tid % kSampleLanesPerRow;
    const int K = h < kSampleHeads ? (int)((a.bucketK >> (8 * h)) & 0xffu) : 0, off = (int)((a.bucketOff >> (8 * h)) & 0xffu);

    const int nblocks = (a.rows + kSampleRows - 1) / kSampleRows;
    for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int row0 = b * kSampleRows;
        const int nrows = a.rows - row0 < kSampleRows ? a.rows - row0 : kSampleRows;
        if (b != blockIdx.x) __syncthreads();             // the previous block's readers are done with the image
        for (int i = tid; i < nrows * L; i += kSampleThreads) {
            const int ri = i / L, c = i - ri * L;
            im.logit[ri * pitch + c] = (float)logits[(size_t)(row0 + ri) * (size_t)a.stride + c];
        }
        __syncthreads();
        if (r < nrows && h < kSampleHeads) {
            const int row = row0 + r, q = r * kSampleHeads + h;
            int act = 0;
            float lp = 0.f, ent = 0.f;
            if (!a.selfMask || a.selfMask[row] != 0.f) {
                float u = 0.f;
                if (a.mode == kSampleDraw) {
                    const RandKey k = threefry2x32({a.seed0, a.seed1}, a.row0Global + (uint32_t)row, a.counter);
                    RNG rng{k, (uint32_t)h};
                    u = rng.sampleUniform();
                } else if (a.mode == kSampleEvaluate) act = a.actionIn[(size_t)row * kSampleHeads + h];
                sample_head(im.logit + r * pitch + off, K, a.mode, u, act, lp, ent);
            }
            im.action[q] = act; im.logProb[q] = lp; im.entropy[q] = ent;
        }
        __syncthreads();
        const size_t q0 = (size_t)row0 * kSampleHeads;
        if (tid < nrows * kSampleHeads) {
            if (a.mode != kSampleEvaluate) a.action[q0 + tid] = im.action[tid];
            if (a.headLogProb) a.headLogProb[q0 + tid] = im.logProb[tid];
        }
        if (tid < nrows) {
            const float *p = im.logProb + tid * kSampleHeads, *e = im.entropy + tid * kSampleHeads;
            if (a.logProb) a.logProb[row0 + tid] = (((p[0] + p[1]) + p[2]) + p[3]) + p[4];
            if (a.entropy) a.entropy[row0 + tid] = (((e[0] + e[1]) + e[2]) + e[3]) + e[4];
        }
    }
}

}  // namespace hs
