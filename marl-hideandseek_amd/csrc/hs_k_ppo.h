// The PPO update's loss and its gradients (hs_ppo_loss): a minibatch of n samples — new logits and value, stored action,
// old log-probability, advantage, return — turned into d loss / d logits, d loss / d value and the sums behind the loss
// statistics, as the reference's learner defines the objective (scripts/jax_train.py:41-45: clipped surrogate, clipped
// value loss, entropy bonus).  include/hideseek.h states the arithmetic; every term has a closed-form gradient, so the
// learner needs no autograd graph of the loss.
//
// It moves about 120 bytes per sample (the logits in, the gradients out, eight scalars) and is bound by HBM traffic, so
// every global access of a wave is a contiguous range.  A workgroup takes kPpoRows consecutive samples at a time
// (grid-stride over row blocks, the grid capped at kPpoMaxGrid so that the workspace of partial sums has a fixed size):
//   stage   lane i reads element i of the block's logits (with stride == L one contiguous range) into an LDS image
//           [kPpoRows][L | 1] f32 (k_sample's odd pitch); lane q reads element q of the block's actions; lanes
//           32 k .. 32 k + 31 read the block's range of the k-th per-sample array (old_log_prob, advantage, mask, value,
//           returns, old_value), so the six ranges are in flight in different waves at once.
//   heads   eight lanes per sample, five at work: lane (sample, head) runs sample_head (hs_k_sample.h) in EVALUATE mode,
//           which makes log_prob_h and entropy_h the bits hs_sample_actions returns, and leaves them in LDS.
//   grads   the same lane adds the sample's five head values in k_sample's order, makes ratio, the clipped surrogate and
//           g_lp (each of the five lanes for itself: no broadcast, no further barrier), and overwrites its head's logits
//           in the image with their gradients; e_i is recomputed by the same expf of the same argument.  The lane of
//           head 0 also makes the value term and adds the sample's terms to its f64 statistics.
//   store   lane q stores element q of the block's gradients, rounded to grad_dtype, and lane r the r-th grad_value.
// The statistics of a workgroup's samples are added in lane order and left in partials[blockIdx.x]; k_partials_sum
// (hs_rows.h) adds the workgroups in its fixed order.  No atomics, no scratch, no register array indexed
// dynamically; nothing in a sample's results depends on the grid or on the block it falls into.
//
// The number of active samples, which every gradient is divided by, is counted before: k_ppo_count leaves one integer
// per workgroup (at most kPpoCountGrid of them) and every workgroup of k_ppo adds those itself — integers, so the order
// does not matter.  Without a mask the count is n.
#pragma once
#include <type_traits>
#include "hs_k_gae.h"                     // kGaeMoments (adv_moments), and through it hs_k_sample.h: sample_head, the narrow types

namespace hs {

constexpr int kPpoStats = 7;              // sum pg, sum vl, sum ent, sum kl, policy-clipped, value-clipped, count
constexpr int kPpoThreads = 256;
constexpr int kPpoLanesPerRow = kSampleLanesPerRow;                     // five heads, three idle lanes
constexpr int kPpoRows = kPpoThreads / kPpoLanesPerRow;                 // 32 samples per block
constexpr int kPpoMaxGrid = 2048;                                       // 256 CUs x the 8 workgroups of 4 waves a CU holds
constexpr int kPpoCountGrid = kPpoThreads;                              // k_ppo_count: one partial per lane of k_ppo
constexpr int kPpoSumSegs = 32;                                         // k_partials_sum: segments summed side by side
constexpr int kPpoRowArrays = 6;                                        // old_log_prob, advantage, mask, value, returns, old_value
static_assert(kPpoRows * kSampleHeads <= kPpoThreads && kPpoRowArrays * kPpoRows <= kPpoThreads, "a lane per staged element");
static_assert(kPpoRows == 32, "the lanes of a per-sample array are half a wave");

struct PpoAbsent {};                      // element type of an array that was not given (value, grad_logits)

struct PpoArgs {
    const void *logits;
    const int32_t *action;
    const float *oldLogProb, *advantage;
    const double *advMoments;             // or null
    const float *mask;                    // or null
    const void *value;                    // or null
    const float *returns, *oldValue;      // oldValue: or null
    void *gradLogits, *gradValue;         // either may be null
    double *partials;                     // [gridDim.x][kPpoStats], or null: no stats
    const int32_t *counts;                // [countParts] of k_ppo_count (with a mask)
    uint64_t bucketK, bucketOff;          // byte h: buckets[h] and the sample's first logit of head h
    int n, stride, gradStride, L, countParts;
    float clip, valueCoef, entropyCoef, gradScale;
};

__host__ __device__ constexpr int ppo_grid(int n) {
    const int nb = (n + kPpoRows - 1) / kPpoRows;
    return nb < kPpoMaxGrid ? nb : kPpoMaxGrid;
}
__host__ __device__ constexpr int ppo_count_grid(int n) {
    const int nb = (n + kPpoThreads - 1) / kPpoThreads;
    return nb < kPpoCountGrid ? nb : kPpoCountGrid;
}

// counts[b] = the number of mask[i] != 0 among the samples workgroup b strides over.  (A template, as the other
// kernels of this file: emitted where hideseek.hip first launches it.)
template <int kThreads = kPpoThreads>
__global__ __launch_bounds__(kThreads) void k_ppo_count(const float *__restrict__ mask, int n, int32_t *__restrict__ counts) {
    __shared__ int32_t red[kThreads];
    int32_t c = 0;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * kThreads) c += mask[i] != 0.f;
    red[threadIdx.x] = c;
    __syncthreads();
    for (int k = kThreads / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = red[0];
}

struct PpoImage {
    float logit[kPpoRows * (kSampleMaxLogits | 1)];       // the logits, then their gradients
    int32_t action[kPpoRows * kSampleHeads];
    float logProb[kPpoRows * kSampleHeads], entropy[kPpoRows * kSampleHeads];
    float row[kPpoRowArrays][kPpoRows];                   // old_log_prob, advantage, mask, value, returns, old_value
    float gradValue[kPpoRows];
    int32_t count[kPpoThreads];
    double stat[kPpoStats][kPpoRows];
};

// mean and std + 1e-8f of the advantage normaliser from the moments of hs_compute_gae (both 0 / 1e-8f without a sample).
HSD void ppo_normaliser(const double *m, float &mean, float &stdEps) {
    const double cnt = m[4], mu = cnt == 0.0 ? 0.0 : m[0] / cnt, var = cnt == 0.0 ? 0.0 : m[1] / cnt - mu * mu;
    mean = (float)mu;
    stdEps = (float)sqrt(var > 0.0 ? var : 0.0) + 1e-8f;
}

// A gradient as it is stored: +0 for an inactive sample and for a zero of either sign.
HSD float ppo_stored(bool on, float y) { return on && y != 0.f ? y : 0.f; }

// TL, TG, TV: the element types of logits, grad_logits (PpoAbsent: none) and value / grad_value (PpoAbsent: no value term):
// what changes the instructions of a block of samples is decided at compile time.  The mask, old_value, adv_moments and
// the statistics are each a wave-uniform branch around one load or a handful of additions.
// (The kernel's work with scale() where the header has grad_scale: k_ppo_scaled, hs_k_loss_scale.h, gives grad_scale * S.)
template <typename TL, typename TG, typename TV, typename Scale>
HSD void ppo_samples(const PpoArgs &a, const Scale scale) {
    __shared__ PpoImage im;
    constexpr bool kGrad = !std::is_same<TG, PpoAbsent>::value, kValue = !std::is_same<TV, PpoAbsent>::value;
    const TL *logits = (const TL *)a.logits;
    const int tid = threadIdx.x, L = a.L, pitch = L | 1;
    const int r = tid / kPpoLanesPerRow, h = tid % kPpoLanesPerRow;
    const int K = h < kSampleHeads ? (int)((a.bucketK >> (8 * h)) & 0xffu) : 0, off = (int)((a.bucketOff >> (8 * h)) & 0xffu);
    const int which = tid / kPpoRows, lane = tid % kPpoRows;      // stage: array `which`, sample `lane` of the block

    const bool MASK = a.mask != nullptr, STATS = a.partials != nullptr;
    int32_t cnt = a.n;
    if (MASK) {                                                   // the partial counts of k_ppo_count, added by every workgroup
        im.count[tid] = tid < a.countParts ? a.counts[tid] : 0;
        __syncthreads();
        for (int k = kPpoThreads / 2; k > 0; k >>= 1) {
            if (tid < k) im.count[tid] += im.count[tid + k];
            __syncthreads();
        }
        cnt = im.count[0];
    }
    const float w = scale() / (float)cnt;
    float mean = 0.f, stdEps = 1.f;
    if (a.advMoments) ppo_normaliser(a.advMoments, mean, stdEps);
    const float lo = 1.f - a.clip, hi = 1.f + a.clip;
    double sPg = 0.0, sVl = 0.0, sEnt = 0.0, sKl = 0.0, sPc = 0.0, sVc = 0.0, sN = 0.0;

    const int nblocks = (a.n + kPpoRows - 1) / kPpoRows;
    for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int row0 = b * kPpoRows;
        const int nrows = a.n - row0 < kPpoRows ? a.n - row0 : kPpoRows;
        if (b != blockIdx.x) __syncthreads();             // the previous block's readers are done with the image
        for (int i = tid; i < nrows * L; i += kPpoThreads) {
            const int ri = i / L, c = i - ri * L;
            im.logit[ri * pitch + c] = (float)logits[(size_t)(row0 + ri) * (size_t)a.stride + c];
        }
        if (tid < nrows * kSampleHeads) im.action[tid] = a.action[(size_t)row0 * kSampleHeads + tid];
        if (lane < nrows) {
            const size_t at = (size_t)row0 + lane;
            if (which == 0) im.row[0][lane] = a.oldLogProb[at];
            else if (which == 1) im.row[1][lane] = a.advantage[at];
            else if (which == 2) im.row[2][lane] = MASK ? a.mask[at] : 1.f;
            else if (which == 3) { if constexpr (kValue) im.row[3][lane] = (float)((const TV *)a.value)[at]; }
            else if (which == 4) { if constexpr (kValue) im.row[4][lane] = a.returns[at]; }
            else if (which == 5) { if constexpr (kValue) if (a.oldValue) im.row[5][lane] = a.oldValue[at]; }
        }
        __syncthreads();
        const bool mine = r < nrows && h < kSampleHeads;
        const float *l = im.logit + r * pitch + off;
        int act = 0;
        float lpH = 0.f, entH = 0.f;
        if (mine) {
            act = im.action[r * kSampleHeads + h];
            sample_head(l, K, kSampleEvaluate, 0.f, act, lpH, entH);
            im.logProb[r * kSampleHeads + h] = lpH; im.entropy[r * kSampleHeads + h] = entH;
        }
        __syncthreads();
        if (mine) {
            const float *p = im.logProb + r * kSampleHeads, *e = im.entropy + r * kSampleHeads;
            const float lp = (((p[0] + p[1]) + p[2]) + p[3]) + p[4], ent = (((e[0] + e[1]) + e[2]) + e[3]) + e[4];
            const bool on = im.row[2][r] != 0.f;
            const float oldLp = im.row[0][r], adv = im.row[1][r];
            const float A = a.advMoments ? (adv - mean) / stdEps : adv;
            const float dlp = lp - oldLp, ratio = expf(dlp);
            const float s1 = ratio * A, s2 = fminf(fmaxf(ratio, lo), hi) * A;
            const bool unclipped = s1 <= s2;
            const float gLp = unclipped ? -s1 : 0.f;
            // The head's m, S and log S for p_i and t_i.  log_prob_h and entropy_h, the values that share their bits with
            // hs_sample_actions, are sample_head's own; these three only enter the gradients, which the tests hold to
            // the restatement of the header, so a change of sample_head cannot silently change what they check.
            if (kGrad) {
                float m = l[0];
                for (int i = 1; i < K; ++i)
                    if (l[i] > m) m = l[i];
                float S = 0.f;
                for (int i = 0; i < K; ++i) {
                    const float ei = expf(l[i] - m);
                    S = i ? S + ei : ei;
                }
                const float logS = logf(S);
                float *g = im.logit + r * pitch + off;
                for (int i = 0; i < K; ++i) {
                    const float d = g[i] - m, ei = expf(d), pi = ei / S;
                    const float t = pi * ((d - logS) + entH);
                    const float x = gLp * ((i == act ? 1.f : 0.f) - pi) + a.entropyCoef * t;
                    g[i] = ppo_stored(on && ei > 0.f, w * x);
                }
            }
            if (h == 0) {
                float vl = 0.f;
                bool vclip = false;
                if constexpr (kValue) {
                    const float v = im.row[3][r], R = im.row[4][r], dv = v - R;
                    float gV = dv;
                    if (a.oldValue) {
                        const float vo = im.row[5][r], dvo = v - vo;              // inside the clip range vc is v itself
                        const float dvc = fabsf(dvo) <= a.clip ? dv : (vo + (dvo < 0.f ? -a.clip : a.clip)) - R;
                        const float u1 = dv * dv, u2 = dvc * dvc;
                        vl = 0.5f * (u1 >= u2 ? u1 : u2);
                        gV = u1 >= u2 ? dv : 0.f;
                        vclip = u2 > u1;
                    } else vl = 0.5f * (dv * dv);
                    im.gradValue[r] = ppo_stored(on, w * (a.valueCoef * gV));
                }
                if (STATS && on) {
                    sPg += (double)(unclipped ? -s1 : -s2); sVl += (double)vl; sEnt += (double)ent;
                    sKl += (double)((ratio - 1.f) - dlp);
                    sPc += s2 < s1 ? 1.0 : 0.0; sVc += vclip ? 1.0 : 0.0; sN += 1.0;
                }
            }
        }
        __syncthreads();
        if constexpr (kGrad) {
            TG *out = (TG *)a.gradLogits;
            for (int i = tid; i < nrows * L; i += kPpoThreads) {
                const int ri = i / L, c = i - ri * L;
                out[(size_t)(row0 + ri) * (size_t)a.gradStride + c] = (TG)im.logit[ri * pitch + c];
            }
        }
        if constexpr (kValue)
            if (a.gradValue && tid < nrows) ((TV *)a.gradValue)[(size_t)row0 + tid] = (TV)im.gradValue[tid];
    }
    if (STATS) {                                          // lane q < kPpoStats adds statistic q of the 32 sample lanes in order
        __syncthreads();
        if (h == 0) {
            im.stat[0][r] = sPg; im.stat[1][r] = sVl; im.stat[2][r] = sEnt; im.stat[3][r] = sKl;
            im.stat[4][r] = sPc; im.stat[5][r] = sVc; im.stat[6][r] = sN;
        }
        __syncthreads();
        if (tid < kPpoStats) {
            double s = im.stat[tid][0];
            for (int k = 1; k < kPpoRows; ++k) s += im.stat[tid][k];
            a.partials[(size_t)blockIdx.x * kPpoStats + tid] = s;
        }
    }
}

template <typename TL, typename TG, typename TV>
__global__ __launch_bounds__(kPpoThreads) void k_ppo(PpoArgs a) {
    ppo_samples<TL, TG, TV>(a, [&] { return a.gradScale; });
}

}  // namespace hs
