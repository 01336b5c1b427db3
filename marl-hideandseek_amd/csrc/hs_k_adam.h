// The optimiser (hs_adam_step): the clip by the global gradient norm and the Adam step that end every update of the
// reference's learner (scripts/jax_train.py: lr = 1e-4, max_grad_norm = 5), over ONE flat f32 buffer each of parameters,
// gradients and the two moments.  include/hideseek.h states the arithmetic; madrona_learn's optimiser is on no machine, so
// the rule is this project's (optax's clip_by_global_norm followed by Adam / AdamW), not pinned to the reference.
//
// Two launches, in the shape of k_ppo_count -> k_ppo:
//   k_adam_norm   one f64 partial per workgroup: the sum of (double)g * (double)g over the workgroup's elements (a product
//                 of two f32 is exact in f64).  Workgroup 0 also copies the caller's state into the workspace, behind the
//                 partials: the snapshot k_adam_step reads.
//   k_adam_step   every workgroup adds the partials itself, in index order (all hold the same bits), makes the norm, the
//                 clip factor and the bias corrections in f64, then updates its elements in f32.  Lane 0 of workgroup 0
//                 writes the new state and the statistics.
// Which element falls to whom (the contract of k_adam_norm; the tests restate it): the buffer is cut into quads of 4
// adjacent floats, quad q = elements 4 q .. 4 q + 3, Q = ceil(n / 4) of them, the last one short when n is no multiple of
// 4.  With G = min(ceil(Q / 256), kAdamMaxGrid) workgroups of 256 lanes, quad q = (trip * G + b) * 256 + lane belongs to
// lane `lane` of workgroup b in its trip `trip`.  A lane adds the squares of its quads in trip order and inside a quad in
// index order onto +0; lane 0 then adds the 256 lane sums in lane order.  A full quad is one 16-byte access; the short
// quad goes by element, and elements past n are never touched.  (The norm kernel has the loads of kAdamUnroll trips in
// flight before it adds them; a trip past the end adds +0, which changes no bit of a sum that is +0 or above.)
// k_adam_step's grid is its own (up to kAdamStepMaxGrid workgroups): nothing in an element's result depends on it.
//
// The state is race-free without any order among workgroups: k_adam_step reads the snapshot, which only k_adam_norm
// writes, and writes the caller's state, which only k_adam_norm reads; the two launches are ordered by the stream.
// No atomics, no scratch.
//
// Included after the other kernel headers, and every kernel here is a template, as hs_k_norm.h explains.
#pragma once
#include "hs_rows.h"                      // ElemVec

namespace hs {

constexpr int kAdamThreads = 256;
constexpr int kAdamVec = 4;                                             // floats per quad: one 16-byte access
constexpr int kAdamMaxGrid = 256;                                       // k_adam_norm: workgroups, and partials, at the most
constexpr int kAdamStepMaxGrid = 2048;                                  // k_adam_step: 256 CUs x 8 workgroups of 4 waves
constexpr int kAdamUnroll = 4;                                          // k_adam_norm: trips whose loads are in flight together
constexpr int kAdamState = 4;                                           // beta1^t, beta2^t, t, skipped steps
constexpr int kAdamStats = 4;                                           // gnorm, clip, skipped, t after the call
constexpr int kAdamWorkspace = kAdamMaxGrid + kAdamState;               // f64: the partials, then the snapshot of the state
static_assert(kAdamThreads >= kAdamMaxGrid && kAdamThreads >= kAdamState, "a lane per partial and per state word");

__host__ __device__ constexpr int adam_grid(int n, int cap) {
    const int quads = (int)(((int64_t)n + kAdamVec - 1) / kAdamVec), nb = (quads + kAdamThreads - 1) / kAdamThreads;
    return nb < cap ? nb : cap;
}

struct AdamArgs {
    float *p, *g, *m, *v;                 // [n]
    const double *ws;                     // [kAdamWorkspace]: k_adam_norm's partials and its snapshot of the state
    double *state, *stats;                // [kAdamState]; [kAdamStats] or null
    int n, nparts, zeroGrad;
    float lr, b1, b2, omb1, omb2, eps, wd;
    double gradScale, maxNorm;
};

// elements i .. i + 3 of p (i a multiple of 4): one piece when they all lie below n, else those that do, and +0 for the rest
HSD void adam_load(const float *p, int64_t i, int n, float (&x)[kAdamVec]) {
    if (i + kAdamVec <= (int64_t)n) {
        const ElemVec<float, kAdamVec> t = *(const ElemVec<float, kAdamVec> *)(p + i);
        _Pragma("unroll") for (int k = 0; k < kAdamVec; ++k) x[k] = t.v[k];
    } else {
        _Pragma("unroll") for (int k = 0; k < kAdamVec; ++k) x[k] = i + k < (int64_t)n ? p[i + k] : 0.f;
    }
}
HSD void adam_store(float *p, int64_t i, int n, const float (&x)[kAdamVec]) {
    if (i + kAdamVec <= (int64_t)n) {
        ElemVec<float, kAdamVec> t;
        _Pragma("unroll") for (int k = 0; k < kAdamVec; ++k) t.v[k] = x[k];
        *(ElemVec<float, kAdamVec> *)(p + i) = t;
    } else {
        _Pragma("unroll") for (int k = 0; k < kAdamVec; ++k)
            if (i + k < (int64_t)n) p[i + k] = x[k];
    }
}

// k_adam_norm's work: the workgroup's partial into ws[blockIdx.x], then snapshot(lane) in workgroup 0.  (A function of its
// own so that the loss-scaled step, hs_k_loss_scale.h, takes a second snapshot beside the same sum.)
template <int kThreads, typename Snapshot>
HSD void adam_norm(const float *g, int n, double *ws, const Snapshot snapshot) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    const int64_t quads = ((int64_t)n + kAdamVec - 1) / kAdamVec, stride = (int64_t)gridDim.x * kThreads;
    double acc = 0.0;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + tid; q < quads; q += kAdamUnroll * stride) {
        float x[kAdamUnroll][kAdamVec];
        _Pragma("unroll") for (int u = 0; u < kAdamUnroll; ++u) adam_load(g, kAdamVec * (q + u * stride), n, x[u]);
        _Pragma("unroll") for (int u = 0; u < kAdamUnroll; ++u)
            _Pragma("unroll") for (int k = 0; k < kAdamVec; ++k) acc = acc + (double)x[u][k] * (double)x[u][k];
    }
    red[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = red[0];
        for (int l = 1; l < kThreads; ++l) s = s + red[l];
        ws[blockIdx.x] = s;
    }
    if (blockIdx.x == 0) snapshot(tid);
}

template <int kThreads = kAdamThreads>
__global__ __launch_bounds__(kThreads) void k_adam_norm(const float *__restrict__ g, int n, const double *__restrict__ state, double *__restrict__ ws) {
    adam_norm<kThreads>(g, n, ws, [=](int tid) { if (tid < kAdamState) ws[kAdamMaxGrid + tid] = state[tid]; });
}

// k_adam_step's work with scale() where the header has grad_scale: the norm from the partials, the update of the
// workgroup's elements, and by lane 0 of workgroup 0 the new state, the statistics and then after(skipped).  (The
// loss-scaled step, hs_k_loss_scale.h, gives grad_scale / S and the update of the loss-scale state.)
template <int kThreads, typename Scale, typename After>
HSD void adam_update(const AdamArgs &a, const Scale scale, const After after) {
    __shared__ double part[kAdamMaxGrid];
    const int tid = threadIdx.x;
    if (tid < a.nparts) part[tid] = a.ws[tid];
    __syncthreads();
    double sum = part[0];                                                      // every lane reads the same word: a broadcast
    for (int k = 1; k < a.nparts; ++k) sum = sum + part[k];
    const double p1 = a.ws[kAdamMaxGrid], p2 = a.ws[kAdamMaxGrid + 1], t = a.ws[kAdamMaxGrid + 2], skips = a.ws[kAdamMaxGrid + 3];
    const double gradScale = scale();
    const double gnorm = gradScale * sqrt(sum);
    const bool skipped = !__builtin_isfinite(gnorm);
    const double clip = skipped ? 0.0 : (a.maxNorm > 0.0 && gnorm > a.maxNorm) ? a.maxNorm / gnorm : 1.0;
    const float s = (float)(gradScale * clip);
    const double p1n = p1 * (double)a.b1, p2n = p2 * (double)a.b2;
    const float bc1 = (float)(1.0 - p1n), bc2 = (float)(1.0 - p2n);
    const bool decay = a.wd != 0.f;

    const int64_t quads = ((int64_t)a.n + kAdamVec - 1) / kAdamVec, stride = (int64_t)gridDim.x * kThreads;
    const float zero[kAdamVec] = {0.f, 0.f, 0.f, 0.f};
    if (skipped) {                                                             // uniform over the grid
        if (a.zeroGrad)
            for (int64_t q = (int64_t)blockIdx.x * kThreads + tid; q < quads; q += stride) adam_store(a.g, kAdamVec * q, a.n, zero);
    } else {
        for (int64_t q = (int64_t)blockIdx.x * kThreads + tid; q < quads; q += stride) {
            const int64_t i = kAdamVec * q;
            float g[kAdamVec], p[kAdamVec], m[kAdamVec], v[kAdamVec];
            adam_load(a.g, i, a.n, g); adam_load(a.p, i, a.n, p); adam_load(a.m, i, a.n, m); adam_load(a.v, i, a.n, v);
            _Pragma("unroll") for (int k = 0; k < kAdamVec; ++k) {
                const float gk = g[k] * s;
                m[k] = a.b1 * m[k] + a.omb1 * gk;
                v[k] = a.b2 * v[k] + a.omb2 * (gk * gk);
                const float u = (m[k] / bc1) / (sqrtf(v[k] / bc2) + a.eps);
                p[k] = p[k] - a.lr * (decay ? u + a.wd * p[k] : u);
            }
            adam_store(a.p, i, a.n, p); adam_store(a.m, i, a.n, m); adam_store(a.v, i, a.n, v);
            if (a.zeroGrad) adam_store(a.g, i, a.n, zero);
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        if (skipped) a.state[3] = skips + 1.0;
        else { a.state[0] = p1n; a.state[1] = p2n; a.state[2] = t + 1.0; }
        if (a.stats) { a.stats[0] = gnorm; a.stats[1] = clip; a.stats[2] = skipped ? 1.0 : 0.0; a.stats[3] = skipped ? t : t + 1.0; }
        after(skipped);
    }
}

template <int kThreads = kAdamThreads>
__global__ __launch_bounds__(kThreads) void k_adam_step(AdamArgs a) {
    adam_update<kThreads>(a, [&] { return a.gradScale; }, [](bool) {});
}

}  // namespace hs
