// The two-hot symlog critic head (hs_twohot_value): a sample's B logits over bins in symlog space turned into the decoded
// value and, with returns, into the cross-entropy against the two-hot target, d loss / d logits and the sums behind the
// value statistics (Hafner et al. 2023, DreamerV3; the critic the reference trains, scripts/jax_policy.py:369).
// include/hideseek.h states the arithmetic.
//
// It moves B logits in and B gradients out per sample (255 x 2 x 2 bytes with bf16) and evaluates one expf per logit.
// A workgroup takes kTwRows consecutive samples at a time (grid-stride over row blocks, the grid capped at kTwMaxGrid so
// that the workspace of partial sums has a fixed size):
//   stage   with stride == B a block's logits are one contiguous byte range whose length is a multiple of 16 for a whole
//           block; from a 16-byte aligned base lane i loads the i-th 16 bytes of it (one global_load_dwordx4) and
//           scatters the 4 or 8 elements into an LDS image [kTwRows][kTwPitch] f32.  Strided logits, an unaligned base
//           and the last bytes of a partial block are loaded by element.
//   sample  eight lanes per sample, lane h taking bins h, h + 8, h + 16, ...: the 64 reads of a wave fall on rows
//           8 w .. 8 w + 7 and columns 8 j + h, dwords (8 r + h) mod 64 apart with kTwPitch = 8 mod 64, so on 64 different
//           banks.  Pass 1 the maximum; pass 2 e_i = expf(l_i - m), left in the image, with S and Y added per lane in
//           ascending order and across the eight lanes as ((0+1)+(2+3)) + ((4+5)+(6+7)) by three xor shuffles (float
//           addition commutes, so every lane holds the same bits); d_k and d_{k+1} of the two target bins are kept by the
//           lanes that pass them and fetched by a shuffle.  Pass 3 overwrites e_i with grad_i: no expf is evaluated twice.
//   store   lane i stores the i-th 16 bytes of the block's gradients where grad_stride == B and the base is aligned,
//           else by element; lane r stores the r-th value.
// The statistics of a workgroup's samples are added in lane order and left in partials[blockIdx.x];
// k_partials_sum (hs_rows.h) adds the workgroups in its fixed order.  No atomics, no scratch; nothing
// in a sample's results depends on the grid, on the block it falls into or on the path its bytes took.
//
// The number of active samples comes from k_ppo_count (hs_k_ppo.h) into a counts buffer of this call's own.
#pragma once
#include "hs_k_ppo.h"                      // k_ppo_count, ppo_count_grid, PpoAbsent, the narrow types

namespace hs {

constexpr int kTwStats = 6;                // sum ce, sum (v - R)^2, sum v, sum R, sum R^2, count
constexpr int kTwThreads = 256;
constexpr int kTwLanesPerRow = 8;
constexpr int kTwRows = kTwThreads / kTwLanesPerRow;                    // 32 samples per block
constexpr int kTwMaxBins = 256;
constexpr int kTwPitch = kTwMaxBins + 8;                                // = 8 mod 64: see `sample` above
constexpr int kTwMaxGrid = 2048;                                        // 256 CUs x 8 workgroups
constexpr int kTwSumSegs = 32;
static_assert(kTwRows == 32 && kTwPitch % 64 == 8 && kTwPitch >= kTwMaxBins, "the image's rows start eight banks apart");
static_assert(kTwThreads == kPpoCountGrid, "one partial count of k_ppo_count per lane");

struct TwohotArgs {
    const void *logits;
    const float *returns, *mask;          // either may be null
    void *value, *gradLogits;             // either may be null
    double *partials;                     // [gridDim.x][kTwStats], or null: no stats
    const int32_t *counts;                // [countParts] of k_ppo_count (with a mask)
    int n, stride, gradStride, B, countParts;
    float lo, hi, lossCoef, gradScale;
};

__host__ __device__ constexpr int twohot_grid(int n) {
    const int nb = (n + kTwRows - 1) / kTwRows;
    return nb < kTwMaxGrid ? nb : kTwMaxGrid;
}

template <typename T> struct alignas(16) TwVec { T v[16 / sizeof(T)]; };

struct TwImage {
    float x[kTwRows * kTwPitch];          // the logits, then e_i, then the gradients
    float value[kTwRows];
    int32_t count[kTwThreads];
    double stat[kTwStats][kTwRows];
};

// a + the value of lane (lane ^ k) of the same eight
HSD float tw_add_xor(float a, int k) { return a + __shfl_xor(a, k, kTwLanesPerRow); }

// TL, TG, TV: the element types of logits, grad_logits (PpoAbsent: none) and value (PpoAbsent: none).  returns, mask and
// the statistics are wave-uniform branches.
// (The kernel's work with scale() where the header has grad_scale: k_twohot_scaled, hs_k_loss_scale.h, gives grad_scale * S.)
template <typename TL, typename TG, typename TV, typename Scale>
HSD void twohot_samples(const TwohotArgs &a, const Scale scale) {
    __shared__ TwImage im;
    constexpr bool kGrad = !std::is_same<TG, PpoAbsent>::value, kValue = !std::is_same<TV, PpoAbsent>::value;
    constexpr int kPerL = 16 / (int)sizeof(TL);
    const TL *logits = (const TL *)a.logits;
    const int tid = threadIdx.x, B = a.B;
    const int r = tid / kTwLanesPerRow, h = tid % kTwLanesPerRow;
    const bool MASK = a.mask != nullptr, STATS = a.partials != nullptr, RET = a.returns != nullptr;
    const bool vecIn = a.stride == B && ((uintptr_t)a.logits & 15u) == 0;

    int32_t cnt = a.n;
    if (MASK) {                                                   // the partial counts of k_ppo_count, added by every workgroup
        im.count[tid] = tid < a.countParts ? a.counts[tid] : 0;
        __syncthreads();
        for (int k = kTwThreads / 2; k > 0; k >>= 1) {
            if (tid < k) im.count[tid] += im.count[tid + k];
            __syncthreads();
        }
        cnt = im.count[0];
    }
    const float w = scale() / (float)cnt;
    const float lo = a.lo, hi = a.hi, step = (hi - lo) / (float)(B - 1);
    double sCe = 0.0, sSq = 0.0, sV = 0.0, sR = 0.0, sR2 = 0.0, sN = 0.0;

    const int nblocks = (a.n + kTwRows - 1) / kTwRows;
    for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const int row0 = b * kTwRows;
        const int nrows = a.n - row0 < kTwRows ? a.n - row0 : kTwRows;
        const int nel = nrows * B;
        float R = 0.f;
        bool on = r < nrows;
        if (on) {                                                 // the eight lanes of a sample read the same address
            if (RET) R = a.returns[(size_t)row0 + r];
            if (MASK) on = a.mask[(size_t)row0 + r] != 0.f;
        }
        if (b != blockIdx.x) __syncthreads();                     // the previous block's readers are done with the image
        int done = 0;                                             // elements the 16-byte loads cover
        if (vecIn) {
            const TwVec<TL> *src = (const TwVec<TL> *)(logits + (size_t)row0 * (size_t)B);
            const int nvec = nel / kPerL;
            for (int i0 = 0; i0 < nvec; i0 += kTwThreads) {
                const int i = i0 + tid;
                if (i < nvec) {
                    const TwVec<TL> v = src[i];
                    int ri = i * kPerL / B, c = i * kPerL - ri * B;
                    for (int k = 0; k < kPerL; ++k) {
                        im.x[ri * kTwPitch + c] = (float)v.v[k];
                        if (++c == B) { c = 0; ++ri; }
                    }
                }
            }
            done = nvec * kPerL;
        }
        _Pragma("unroll 1") for (int i0 = done; i0 < nel; i0 += kTwThreads) {
            const int i = i0 + tid;
            if (i < nel) {
                const int ri = i / B, c = i - ri * B;
                im.x[ri * kTwPitch + c] = (float)logits[(size_t)(row0 + ri) * (size_t)a.stride + c];
            }
        }
        // columns B .. B + 7 hold -inf: e = 0 there, which adds +0 to S and to Y, so every lane runs the same number of
        // rounds over a row whatever B is (rows past nrows hold what the last block left: computed, never stored)
        float *x = im.x + r * kTwPitch;
        x[B + h] = -INFINITY;
        __syncthreads();
        float m = -INFINITY;
        _Pragma("unroll 1") for (int j = h; j < B + h; j += kTwLanesPerRow) m = fmaxf(m, x[j]);
        for (int k = 1; k < kTwLanesPerRow; k <<= 1) m = fmaxf(m, __shfl_xor(m, k, kTwLanesPerRow));
        // the two target bins, before the pass that meets their d
        int kb = 0;
        float f = 0.f;
        if (RET) {
            const float z = copysignf(log1pf(fabsf(R)), R), zc = fminf(fmaxf(z, lo), hi);
            const float u = (zc - lo) / step;
            kb = (int)floorf(u);
            kb = kb < 0 ? 0 : kb;
            kb = kb > B - 2 ? B - 2 : kb;
            f = fminf(fmaxf(u - (float)kb, 0.f), 1.f);
        }
        float S = 0.f, Y = 0.f, dk = 0.f, dk1 = 0.f;
        _Pragma("unroll 1") for (int j = h; j < B + h; j += kTwLanesPerRow) {
            const float d = x[j] - m, e = expf(d), bj = lo + (float)j * step;
            x[j] = e;
            S = S + e;
            Y = Y + e * bj;
            dk = j == kb ? d : dk;
            dk1 = j == kb + 1 ? d : dk1;
        }
        S = tw_add_xor(tw_add_xor(tw_add_xor(S, 1), 2), 4);
        Y = tw_add_xor(tw_add_xor(tw_add_xor(Y, 1), 2), 4);
        const float rS = 1.0f / S, y = Y * rS;
        const float v = copysignf(expm1f(fabsf(y)), y);
        if (kValue && h == 0) im.value[r] = on && v != 0.f ? v : 0.f;
        if (RET) {
            if (kGrad)
                _Pragma("unroll 1") for (int j = h; j < B + h; j += kTwLanesPerRow) {
                    const float p = x[j] * rS, t = j == kb ? 1.0f - f : j == kb + 1 ? f : 0.f;
                    const float g = w * (a.lossCoef * (p - t));
                    x[j] = on && g != 0.f ? g : 0.f;
                }
            if (STATS) {
                dk = __shfl(dk, kb % kTwLanesPerRow, kTwLanesPerRow);
                dk1 = __shfl(dk1, (kb + 1) % kTwLanesPerRow, kTwLanesPerRow);
                const float logS = logf(S), lpk = dk - logS, lpk1 = dk1 - logS;
                const float ce = -((1.0f - f) * lpk + f * lpk1);
                const double dv = (double)v - (double)R;
                const bool add = h == 0 && on;                    // selects: what an inactive sample holds reaches no sum
                sCe += add ? (double)ce : 0.0; sSq += add ? dv * dv : 0.0; sV += add ? (double)v : 0.0;
                sR += add ? (double)R : 0.0; sR2 += add ? (double)R * (double)R : 0.0; sN += add ? 1.0 : 0.0;
            }
        }
        __syncthreads();
        if constexpr (kGrad) {
            constexpr int kPerG = 16 / (int)sizeof(TG);
            TG *out = (TG *)a.gradLogits;
            int stored = 0;
            if (a.gradStride == B && ((uintptr_t)a.gradLogits & 15u) == 0) {
                TwVec<TG> *dst = (TwVec<TG> *)(out + (size_t)row0 * (size_t)B);
                const int nvec = nel / kPerG;
                for (int i0 = 0; i0 < nvec; i0 += kTwThreads) {
                    const int i = i0 + tid;
                    if (i < nvec) {
                        TwVec<TG> v;
                        int ri = i * kPerG / B, c = i * kPerG - ri * B;
                        for (int k = 0; k < kPerG; ++k) {
                            v.v[k] = (TG)im.x[ri * kTwPitch + c];
                            if (++c == B) { c = 0; ++ri; }
                        }
                        dst[i] = v;
                    }
                }
                stored = nvec * kPerG;
            }
            _Pragma("unroll 1") for (int i0 = stored; i0 < nel; i0 += kTwThreads) {
                const int i = i0 + tid;
                if (i < nel) {
                    const int ri = i / B, c = i - ri * B;
                    out[(size_t)(row0 + ri) * (size_t)a.gradStride + c] = (TG)im.x[ri * kTwPitch + c];
                }
            }
        }
        if constexpr (kValue)
            if (tid < nrows) ((TV *)a.value)[(size_t)row0 + tid] = (TV)im.value[tid];
    }
    if (STATS) {                                          // lane q < kTwStats adds statistic q of the 32 sample lanes in order
        __syncthreads();
        if (h == 0) {
            im.stat[0][r] = sCe; im.stat[1][r] = sSq; im.stat[2][r] = sV; im.stat[3][r] = sR; im.stat[4][r] = sR2; im.stat[5][r] = sN;
        }
        __syncthreads();
        if (tid < kTwStats) {
            double s = im.stat[tid][0];
            for (int k = 1; k < kTwRows; ++k) s += im.stat[tid][k];
            a.partials[(size_t)blockIdx.x * kTwStats + tid] = s;
        }
    }
}

template <typename TL, typename TG, typename TV>
__global__ __launch_bounds__(kTwThreads) void k_twohot(TwohotArgs a) {
    twohot_samples<TL, TG, TV>(a, [&] { return a.gradScale; });
}

}  // namespace hs
