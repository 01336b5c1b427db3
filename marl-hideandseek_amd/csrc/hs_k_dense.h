// A dense layer after its GEMM (hs_dense_norm_act, hs_dense_norm_act_backward): the bias, the LayerNorm over the C
// channels and the leaky ReLU of one layer of the reference's MLP(num_channels=256, num_layers=3) at the end of SimpleNet
// (scripts/jax_policy.py:163-167), forward and backward.  include/hideseek.h states the arithmetic.  The GEMM z = x W
// stays with the BLAS library: this file starts at its result.
//
// A row moves C values in and C out, and costs one LayerNorm: the kernel is bound by its memory accesses.
//   lanes     lane l holds the V = C / 64 ADJACENT channels V l .. V l + V - 1 (1, 2, 4 or 8), not k_lstm's l + 64 q: a
//             lane's access to a row is one piece of V elements (at C = 256 8 bytes in bf16 / f16 and 16 bytes in f32; at
//             C = 512 in f32 two pieces of 16 bytes), and a wave's access is the whole row, contiguous.  At C = 64 it is
//             one element per lane as in k_lstm.  z, y, grad_y and grad_z are 16-byte aligned for that; there is no
//             by-element path.  A wave takes one row per round and a workgroup of four waves four rows: grid-stride.
//   params    the 3 V values of bias | gamma | beta that a lane needs stay in its registers for the whole kernel.
//   reduce    hs_rows.h's row_sum over this map (AdjacentMap): the terms a lane adds first are other channels than
//             k_lstm's, so the order of a row's sum is this kernel's own.
// The forward uses no LDS and has no barrier.  Nothing in a row's outputs depends on the grid or on the row's position.
//
// The backward recomputes the forward from z and the parameters, writes grad_z of its row and keeps the 3 V sums of
// grad_params of its channels in registers over all the rows its wave takes, in round order; they leave as the
// workgroup's slice [blockIdx.x][3 C] of a workspace of its own, as hs_rows.h describes.  A wave whose row lies past n
// adds nothing.  No scratch.
#pragma once
#include "hs_rows.h"

namespace hs {

constexpr int kDenseParamRows = 3;                                      // bias | gamma | beta, rows of C floats
constexpr int kDenseMaxC = 512;

struct DenseArgs {
    const void *z;                        // [n][C]
    const float *params;                  // [3 C]
    void *y;                              // [n][C]
    int n, zType, yType;
    float eps, slope;
};

struct DenseBwdArgs {
    const void *z;
    const float *params;
    const void *gradY;                    // [n][C] of yType
    void *gradZ;                          // [n][C] of zType, or null
    float *workspace;                     // [gridDim.x][3 C], or null
    int n, zType, yType;
    float eps, slope;
};

template <typename T, int V> HSD void dense_load_as(const void *p, size_t i, float (&v)[V]) {
    const ElemVec<T, V> t = *(const ElemVec<T, V> *)((const T *)p + i);
    _Pragma("unroll") for (int k = 0; k < V; ++k) v[k] = (float)t.v[k];
}
template <typename T, int V> HSD void dense_store_as(void *p, size_t i, const float (&v)[V]) {
    ElemVec<T, V> t;
    _Pragma("unroll") for (int k = 0; k < V; ++k) t.v[k] = (T)v[k];
    *(ElemVec<T, V> *)((T *)p + i) = t;
}
// elements i .. i + V - 1 (i a multiple of V) of an array of run-time type, widened exactly / rounded to nearest even
template <int V> HSD void dense_load(const void *p, int type, size_t i, float (&v)[V]) {
    if (type == kElemF32) dense_load_as<float, V>(p, i, v);
    else if (type == kElemBf16) dense_load_as<SampleBf16, V>(p, i, v);
    else dense_load_as<SampleF16, V>(p, i, v);
}
template <int V> HSD void dense_store(void *p, int type, size_t i, const float (&v)[V]) {
    if (type == kElemF32) dense_store_as<float, V>(p, i, v);
    else if (type == kElemBf16) dense_store_as<SampleBf16, V>(p, i, v);
    else dense_store_as<SampleF16, V>(p, i, v);
}

// What forward and backward both compute of one row, per channel of this lane.
template <int C> struct DenseRow {
    float h[C / 64], u[C / 64];
    float rstd;
};

// P: this lane's parameters [3][V] (bias, gamma, beta)
template <int C>
HSD void dense_row(const void *z, int zType, const float (&P)[kDenseParamRows][C / 64], float eps, int row, int lane, DenseRow<C> &r) {
    constexpr int V = C / 64;
    float a[V];
    dense_load<V>(z, zType, (size_t)row * C + V * lane, a);
    _Pragma("unroll") for (int k = 0; k < V; ++k) a[k] = a[k] + P[0][k];
    r.rstd = row_norm<V>(a, eps, r.h);
    _Pragma("unroll") for (int k = 0; k < V; ++k) r.u[k] = fmaf(P[1][k], r.h[k], P[2][k]);
}

template <int C>
__global__ __launch_bounds__(kRowsThreads) void k_dense_fwd(DenseArgs a) {
    constexpr int V = C / 64;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    float P[kDenseParamRows][V];
    lane_params<AdjacentMap<V>>(a.params, lane, P);
    const int nrounds = (a.n + kRowsWaves - 1) / kRowsWaves;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row = round * kRowsWaves + wave;
        if (row >= a.n) break;                                                 // wave-uniform; the later rounds lie further past n
        DenseRow<C> r;
        dense_row<C>(a.z, a.zType, P, a.eps, row, lane, r);
        float y[V];
        _Pragma("unroll") for (int k = 0; k < V; ++k) y[k] = r.u[k] > 0.f ? r.u[k] : a.slope * r.u[k];
        dense_store<V>(a.y, a.yType, (size_t)row * C + V * lane, y);
    }
}

template <int C>
__global__ __launch_bounds__(kRowsThreads) void k_dense_bwd(DenseBwdArgs a) {
    constexpr int V = C / 64;
    __shared__ float S[kDenseParamRows * C];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    float P[kDenseParamRows][V], acc[kDenseParamRows][V];
    lane_params<AdjacentMap<V>>(a.params, lane, P);
    _Pragma("unroll") for (int j = 0; j < kDenseParamRows; ++j)
        _Pragma("unroll") for (int k = 0; k < V; ++k) acc[j][k] = 0.f;
    const int nrounds = (a.n + kRowsWaves - 1) / kRowsWaves;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row = round * kRowsWaves + wave;
        if (row >= a.n) break;                                                 // wave-uniform; no barrier inside the loop
        DenseRow<C> r;
        dense_row<C>(a.z, a.zType, P, a.eps, row, lane, r);
        const size_t i0 = (size_t)row * C + V * lane;
        float g[V], du[V], dh[V], da[V];
        dense_load<V>(a.gradY, a.yType, i0, g);
        _Pragma("unroll") for (int k = 0; k < V; ++k) {
            du[k] = r.u[k] > 0.f ? g[k] : a.slope * g[k];
            dh[k] = du[k] * P[1][k];
        }
        row_norm_bwd<V>(dh, r.h, r.rstd, da);
        _Pragma("unroll") for (int k = 0; k < V; ++k) {
            acc[0][k] = acc[0][k] + da[k];
            acc[1][k] = fmaf(du[k], r.h[k], acc[1][k]);
            acc[2][k] = acc[2][k] + du[k];
        }
        if (a.gradZ) dense_store<V>(a.gradZ, a.zType, i0, da);
    }
    if (!a.workspace) return;                                                  // uniform over the grid
    wave_sums_to_slice<AdjacentMap<V>>(acc, S, a.workspace + (size_t)blockIdx.x * (kDenseParamRows * C));
}

}  // namespace hs
