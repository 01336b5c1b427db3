// Observation normaliser: the exponential moving average of the reference's policy wrapper
// (scripts/jax_policy.py:372-390, ObservationsEMANormalizer.create(decay = 0.99999, ...)) kept on the device.
// k_norm_update folds the moments that k_pack emits into a caller-owned state and rewrites the table
// mu[kPackRow] | inv[kPackRow] from it; k_pack_norm is k_pack (hs_k_pack.h) with y = (x - mu[c]) * inv[c] applied to every
// element on its way out of the LDS image, before the actor's mask and the cast.  The arithmetic of both is the contract
// of include/hideseek.h (hs_obs_norm_request, hs_pack_policy_inputs_normalized); madrona_learn itself is on no machine, so
// the update rule is this project's, not pinned to the reference.
//
// Included after the other kernel headers, and every kernel here is a template, so that the compiler numbers the
// functions of the existing kernels, and with them their branch labels, as before.
#pragma once
#include "hs_k_pack.h"

namespace hs {

constexpr int kNormState = 2 * kPackRow + 1;      // m1[kPackRow], m2[kPackRow], N
constexpr int kNormTable = 2 * kPackRow;          // mu[kPackRow], inv[kPackRow]
constexpr int kNormThreads = 320;                 // a lane per column, five waves, one workgroup
constexpr int kNormMaxMoments = 4096;
static_assert(kNormThreads >= kPackRow && kNormState == kPackMoments, "a lane per column; the state has the layout of the moments");

// prep_counter and self_type are not normalised (jax_policy.py:382-389); the masks are not columns of the row
__host__ __device__ constexpr bool norm_skipped(int c) { return c == 0 || c == kPackColType; }

struct NormArgs {
    const double *moments;                // [numMoments][kPackMoments]
    int numMoments;
    double decay, eps;
    double *state;                        // [kNormState]
    float *table;                         // [kNormTable]
};

// One workgroup.  Lane c adds column c's numMoments terms of sum m x and sum m x x in index order; every lane adds the
// counts in the same order, so n (and with it the branch) has one bit pattern in all of them.  No atomics.
template <int kThreads = kNormThreads>
__global__ __launch_bounds__(kThreads) void k_norm_update(NormArgs a) {
    const int c = threadIdx.x;
    const bool col = c < kPackRow;
    double n = a.moments[2 * kPackRow];
    for (int k = 1; k < a.numMoments; ++k) n += a.moments[(size_t)k * kPackMoments + 2 * kPackRow];
    const bool fold = n > 0.0;
    double N = a.state[2 * kPackRow], m1 = 0.0, m2 = 0.0;
    if (col) {
        m1 = a.state[c];
        m2 = a.state[kPackRow + c];
        if (fold) {
            double s1 = a.moments[c], s2 = a.moments[kPackRow + c];
            for (int k = 1; k < a.numMoments; ++k) {
                s1 += a.moments[(size_t)k * kPackMoments + c];
                s2 += a.moments[(size_t)k * kPackMoments + kPackRow + c];
            }
            const double w = 1.0 - a.decay;
            m1 = a.decay * m1 + w * (s1 / n);
            m2 = a.decay * m2 + w * (s2 / n);
        }
    }
    if (fold) N = a.decay * N + (1.0 - a.decay);
    __syncthreads();                      // every lane has read the old N
    if (col) {
        if (fold) { a.state[c] = m1; a.state[kPackRow + c] = m2; }
        float mu = 0.f, inv = 1.f;
        if (!norm_skipped(c) && N > 0.0) {
            const double mean = m1 / N;
            double v = m2 / N - mean * mean;
            v = v < 0.0 ? 0.0 : v;
            mu = (float)mean;
            inv = (float)(1.0 / sqrt(v + a.eps));
        }
        a.table[c] = mu;
        a.table[kPackRow + c] = inv;
    }
    if (c == 0 && fold) a.state[2 * kPackRow] = N;
}

// k_pack with the normaliser's table: same image, same grid, same moments (of the raw image).
template <typename TA, typename TC, bool MOM>
__global__ __launch_bounds__(kPackThreads) void k_pack_norm(PackArgs a, const float *__restrict__ table) {
    pack_blocks<TA, TC, MOM, true>(a, table);
}

}  // namespace hs
