// Advantages and value targets of a rollout (hs_compute_gae): generalised advantage estimation as the reference trains
// with it (scripts/jax_train.py:45,152-153: gamma 0.998, gae_lambda 0.95, 40 steps per update), over rewards, dones and
// critic values stored [T][rows], rows = agent rows (world * A + slot), contiguous.
//
// Per row, with gl = gamma * lambda (an f32 product) and carry = 0, for t = T-1 down to 0, all IEEE f32 without contraction:
//     v = value[t];  vn = t == T-1 ? bootstrap : value[t+1]             (narrow values widened exactly)
//     active = no mask || mask[t] != 0;   ended = done[t] != 0
//     inactive:  adv = ret = carry = +0.0                                (selects: a NaN of this step reaches no output)
//     active:    delta = ended ? reward[t] - v : (reward[t] + gamma * vn) - v
//                adv   = ended ? delta : delta + gl * carry;   ret = adv + v;   carry = adv
// Moments (optional), over the active (t, row) pairs, in f64: sum adv, sum adv^2, sum ret, sum ret^2, count.  Every lane
// adds its own terms from t = T-1 down, the workgroup's lanes are added in lane order, the workgroups' partials are added
// by k_partials_sum (hs_rows.h) in its fixed order: no atomics, and an order that depends on (rows, T) alone.
//
// The recurrence is serial in t and independent across rows: one lane per row, so that a wave's access to time slice t
// of an array is one contiguous 256-byte range (128 for bf16 / f16 values).  The chain is two to three dependent f32
// operations per step and the loads do not depend on it: a lane holds the slices of kGaeBlock time steps in registers,
// and two such blocks alternate (A is consumed while B's loads are in flight and the other way round), so a wave has
// between one and two blocks of loads outstanding and never waits for its own stores.  Every loop over a block is
// unrolled at compile time: no register array is indexed dynamically, nothing goes to scratch.  value[t+1] is the v of
// the iteration before, kept in a register.  Nothing depends on the grid: a row's results are those of its own chain.
#pragma once
#include "hs_k_sample.h"                  // SampleBf16 / SampleF16: the narrow types and their exact widening

namespace hs {

constexpr int kGaeMaxSteps = 4096, kGaeMoments = 5;
constexpr int kGaeThreads = 64;           // one wave per workgroup: 96 000 rows are 1 500 workgroups over 256 CUs
constexpr int kGaeBlock = 8;              // time steps a lane holds in registers per block; two blocks alternate
constexpr int kGaeSumSegs = 32;           // k_partials_sum: segments of the partials summed side by side

struct GaeArgs {
    const float *reward;
    const int32_t *done;
    const void *value, *bootstrap;
    const float *mask;                    // or null
    float *advantage, *returns;           // either may be null
    double *partials;                     // [gridDim.x][kGaeMoments], or null: no moments
    int rows, steps;
    float gamma, lambda;
};

__host__ __device__ constexpr int gae_grid(int rows) { return (rows + kGaeThreads - 1) / kGaeThreads; }

template <typename T> struct GaeSlices {  // kGaeBlock consecutive time steps of one row
    float r[kGaeBlock], m[kGaeBlock];
    int32_t d[kGaeBlock];
    T v[kGaeBlock];
};
struct GaeSums { double adv, adv2, ret, ret2, n; };

// Steps t0 .. t0 + n of row `row` into s.  FULL: n == kGaeBlock.  A slice's address is a wave-uniform base (array +
// t * rows) plus the lane's row.  MASK: there is a mask.
template <typename T, bool MASK, bool FULL> HSD void gae_load(const GaeArgs &a, int t0, uint32_t row, int n, GaeSlices<T> &s) {
#pragma unroll
    for (int j = 0; j < kGaeBlock; ++j) {
        const size_t at = (size_t)(t0 + j) * (size_t)a.rows;
        if (FULL || j < n) {
            s.r[j] = (a.reward + at)[row]; s.d[j] = (a.done + at)[row]; s.v[j] = ((const T *)a.value + at)[row];
            s.m[j] = MASK ? (a.mask + at)[row] : 1.f;
        } else {
            s.r[j] = 0.f; s.d[j] = 0; s.v[j] = (T)0.f; s.m[j] = 0.f;
        }
    }
}

// The chain over the block's steps, last first, and their stores.  MOM: with moments.  BOTH: advantage and returns are
// both there (otherwise each is looked at).
template <typename T, bool MOM, bool BOTH, bool FULL>
HSD void gae_chain(const GaeArgs &a, int t0, uint32_t row, int n, const GaeSlices<T> &s, float gl, float &vn, float &carry, GaeSums &sum) {
#pragma unroll
    for (int j = kGaeBlock - 1; j >= 0; --j) {
        if (FULL || j < n) {
            const size_t at = (size_t)(t0 + j) * (size_t)a.rows;
            const float v = (float)s.v[j], r = s.r[j];
            const bool active = s.m[j] != 0.f, ended = s.d[j] != 0;
            const float delta = ended ? r - v : (r + a.gamma * vn) - v;
            const float run = ended ? delta : delta + gl * carry;
            const float adv = active ? run : 0.f, ret = active ? run + v : 0.f;
            carry = adv; vn = v;
            if (BOTH || a.advantage) (a.advantage + at)[row] = adv;
            if (BOTH || a.returns) (a.returns + at)[row] = ret;
            if (MOM) {                                    // an inactive step adds +0.0
                const double da = (double)adv, dr = (double)ret;
                sum.adv += da; sum.adv2 += da * da; sum.ret += dr; sum.ret2 += dr * dr; sum.n += active ? 1.0 : 0.0;
            }
        }
    }
}

// One row's chain from t = steps - 1 down.  What the request leaves out is decided once, here, and not inside the
// blocks: a block of loads and a block of the chain are straight-line code, so the loads of a block issue back to back
// and the chain waits for each slice as it needs it.
template <typename T, bool MASK, bool MOM, bool BOTH> HSD void gae_row(const GaeArgs &a, uint32_t row, GaeSums &sum) {
    const float gl = a.gamma * a.lambda;
    float vn = (float)((const T *)a.bootstrap)[row], carry = 0.f;
    int t0 = (a.steps - 1) / kGaeBlock * kGaeBlock;       // the last block: steps - t0 of its kGaeBlock steps exist
    GaeSlices<T> A, B;
    gae_load<T, MASK, false>(a, t0, row, a.steps - t0, A);
    if (t0 > 0) gae_load<T, MASK, true>(a, t0 - kGaeBlock, row, kGaeBlock, B);
    gae_chain<T, MOM, BOTH, false>(a, t0, row, a.steps - t0, A, gl, vn, carry, sum);
    for (t0 -= kGaeBlock; t0 >= 0; t0 -= kGaeBlock) {
        if (t0 > 0) gae_load<T, MASK, true>(a, t0 - kGaeBlock, row, kGaeBlock, A);
        gae_chain<T, MOM, BOTH, true>(a, t0, row, kGaeBlock, B, gl, vn, carry, sum);
        if ((t0 -= kGaeBlock) < 0) break;
        if (t0 > 0) gae_load<T, MASK, true>(a, t0 - kGaeBlock, row, kGaeBlock, B);
        gae_chain<T, MOM, BOTH, true>(a, t0, row, kGaeBlock, A, gl, vn, carry, sum);
    }
}

template <typename T>
__global__ __launch_bounds__(kGaeThreads) void k_gae(GaeArgs a) {
    const uint32_t row = blockIdx.x * kGaeThreads + threadIdx.x;
    GaeSums sum = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (row < (uint32_t)a.rows) {
        const bool both = a.advantage && a.returns;
        if (a.mask) {
            if (a.partials) { if (both) gae_row<T, true, true, true>(a, row, sum); else gae_row<T, true, true, false>(a, row, sum); }
            else { if (both) gae_row<T, true, false, true>(a, row, sum); else gae_row<T, true, false, false>(a, row, sum); }
        } else {
            if (a.partials) { if (both) gae_row<T, false, true, true>(a, row, sum); else gae_row<T, false, true, false>(a, row, sum); }
            else { if (both) gae_row<T, false, false, true>(a, row, sum); else gae_row<T, false, false, false>(a, row, sum); }
        }
    }
    if (a.partials) {                                     // lane q < kGaeMoments adds moment q of the lanes in lane order
        __shared__ double red[kGaeMoments][kGaeThreads];
        const int tid = threadIdx.x;
        red[0][tid] = sum.adv; red[1][tid] = sum.adv2; red[2][tid] = sum.ret; red[3][tid] = sum.ret2; red[4][tid] = sum.n;
        __syncthreads();
        if (tid < kGaeMoments) {
            double s = red[tid][0];
            for (int k = 1; k < kGaeThreads; ++k) s += red[tid][k];
            a.partials[(size_t)blockIdx.x * kGaeMoments + tid] = s;
        }
    }
}

// The grouped form (hs_compute_gae_grouped): the rows are G groups of m = rows / G consecutive rows (the slots of a
// population's policies), the chains are k_gae's, and the moments are one vector per group.  The grid is cut per group:
// blockIdx.y is the group and has gae_grid(m) workgroups, workgroup x of group g takes the rows g m + 64 x .. and a lane
// past m is idle, so the lanes a workgroup adds, and the gae_grid(m) partials k_partials_sum adds per group, are those of
// k_gae on a handle of m rows that is given the group's columns: the moments of a group have that call's bits.  The
// partials are [G][gae_grid(m)][kGaeMoments].  The body repeats k_gae's text around gae_row, which stays as it is there
// so that k_gae compiles to the code it had.
struct GaeGroupedArgs {
    GaeArgs a;                            // rows = all rows
    int perGroup;                         // m
};

template <typename T>
__global__ __launch_bounds__(kGaeThreads) void k_gae_grouped(GaeGroupedArgs g) {
    GaeArgs a = g.a;                                      // the group's view: its first row is row 0, a time slice is still a.rows long
    const size_t first = (size_t)blockIdx.y * (size_t)g.perGroup;
    a.reward += first; a.done += first;
    a.value = (const T *)a.value + first; a.bootstrap = (const T *)a.bootstrap + first;
    if (a.mask) a.mask += first;
    if (a.advantage) a.advantage += first;
    if (a.returns) a.returns += first;
    const uint32_t row = blockIdx.x * kGaeThreads + threadIdx.x;
    GaeSums sum = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (row < (uint32_t)g.perGroup) {
        const bool both = a.advantage && a.returns;
        if (a.mask) {
            if (a.partials) { if (both) gae_row<T, true, true, true>(a, row, sum); else gae_row<T, true, true, false>(a, row, sum); }
            else { if (both) gae_row<T, true, false, true>(a, row, sum); else gae_row<T, true, false, false>(a, row, sum); }
        } else {
            if (a.partials) { if (both) gae_row<T, false, true, true>(a, row, sum); else gae_row<T, false, true, false>(a, row, sum); }
            else { if (both) gae_row<T, false, false, true>(a, row, sum); else gae_row<T, false, false, false>(a, row, sum); }
        }
    }
    if (a.partials) {                                     // lane q < kGaeMoments adds moment q of the lanes in lane order
        __shared__ double red[kGaeMoments][kGaeThreads];
        const int tid = threadIdx.x;
        red[0][tid] = sum.adv; red[1][tid] = sum.adv2; red[2][tid] = sum.ret; red[3][tid] = sum.ret2; red[4][tid] = sum.n;
        __syncthreads();
        if (tid < kGaeMoments) {
            double s = red[tid][0];
            for (int k = 1; k < kGaeThreads; ++k) s += red[tid][k];
            a.partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kGaeMoments + tid] = s;
        }
    }
}

}  // namespace hs
