// The gradient reduction of data-parallel training (hs_reduce_gradients): dst = the mean of up to kReduceMaxShards flat
// f32 gradient buffers, each weighted by its shard's share of the active samples, in ONE launch and in a fixed order, so
// that every replica that reduces the same buffers holds the same bits.  include/hideseek.h states the arithmetic.
//
//   k_reduce   every wave reads the counts and makes the weights itself, in f64 (C = the sum of the counts that are not 0,
//              in index order; w_g = (float)(c_g / C)): all waves hold the same bits, and nothing goes through memory.  A
//              shard whose count is 0 is left out by a uniform branch: its buffer is not read.  Then per quad, the loads of
//              every remaining source in flight before the first add, acc = w_a * x_a, acc = acc + w_g * x_g in index
//              order in IEEE f32, unfused, and one store.  Lane 0 of workgroup 0 writes C into `total`.
// The shape is k_adam_step's (hs_k_adam.h): quads of 4 floats as one 16-byte access, the short last quad by element
// (adam_load / adam_store), 256 lanes, a grid-stride loop over at most kAdamStepMaxGrid workgroups.  An element's result
// depends on nothing but its inputs and the counts.  dst may be one of the sources: a lane has read its quad from every
// source before it writes it, and no other lane touches that quad.  No atomics, no LDS, no scratch: the loop over the
// shards is unrolled, so the quads and the weights stay in registers.
//
// Included ahead of hs_k_adam.h in hideseek.hip, as hs_k_loss_scale.h: the kernel is a template, emitted where
// launch_reduce (at the end of hideseek.hip, behind every other kernel) names it.
#pragma once
#include "hs_k_adam.h"                    // adam_load, adam_store, adam_grid

namespace hs {

constexpr int kReduceMaxShards = 16;

struct ReduceArgs {
    const float *src[kReduceMaxShards];   // [n] each; the first `shards` are read
    const double *count;                  // [shards]
    float *dst;                           // [n]
    double *total;                        // [1] or null
    int n, shards;
};

template <int kThreads = kAdamThreads>
__global__ __launch_bounds__(kThreads) void k_reduce(ReduceArgs a) {
    // the weights: uniform over the grid
    double c[kReduceMaxShards], C = 0.0;
    unsigned live = 0;                                                         // bit g: shard g counts
    _Pragma("unroll") for (int g = 0; g < kReduceMaxShards; ++g) {
        c[g] = 0.0;
        if (g < a.shards) {
            c[g] = a.count[g];
            if (c[g] != 0.0) { live |= 1u << g; C = C + c[g]; }                // a NaN count counts: it is not 0
        }
    }
    float w[kReduceMaxShards];
    _Pragma("unroll") for (int g = 0; g < kReduceMaxShards; ++g) w[g] = (live >> g & 1u) ? (float)(c[g] / C) : 0.f;

    const int tid = threadIdx.x;
    const int64_t quads = ((int64_t)a.n + kAdamVec - 1) / kAdamVec, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + tid; q < quads; q += stride) {
        const int64_t i = kAdamVec * q;
        float x[kReduceMaxShards][kAdamVec];
        _Pragma("unroll") for (int g = 0; g < kReduceMaxShards; ++g)
            if (live >> g & 1u) adam_load(a.src[g], i, a.n, x[g]);
        float acc[kAdamVec] = {0.f, 0.f, 0.f, 0.f};                            // every count 0: +0
        bool first = true;
        _Pragma("unroll") for (int g = 0; g < kReduceMaxShards; ++g) {
            if (live >> g & 1u) {
                _Pragma("unroll") for (int k = 0; k < kAdamVec; ++k) {
                    const float p = w[g] * x[g][k];
                    acc[k] = first ? p : acc[k] + p;                           // the first product is taken as it is, not added to +0
                }
                first = false;
            }
        }
        adam_store(a.dst, i, a.n, acc);
    }
    if (a.total && blockIdx.x == 0 && tid == 0) a.total[0] = C;
}

}  // namespace hs
