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
//   reduce    dense_sum: the lane's own V terms in ascending order, then the xor butterfly 1, 2, ..., 32.  The order is
//             this kernel's own (the lanes hold other channels than lstm_sum's).
// The forward uses no LDS and has no barrier.  Nothing in a row's outputs depends on the grid or on the row's position.
//
// The backward recomputes the forward from z and the parameters, writes grad_z of its row and keeps the 3 V sums of
// grad_params of its channels in registers over all the rows its wave takes, in round order.  The waves then add in LDS as
// ((w0 + w1) + w2) + w3 and the workgroup writes its slice [blockIdx.x][3 C] of a workspace of its own; the grid is capped
// at kDenseMaxGridBwd, and k_embed_grad_sum (hs_k_embed.h) adds the slices in its fixed order.  A wave whose row lies past
// n adds nothing.  No atomics, no scratch: the same inputs give the same bits.
#pragma once
#include "hs_k_embed.h"                    // the element types and their codes, k_embed_grad_sum

namespace hs {

constexpr int kDenseThreads = 256, kDenseWaves = kDenseThreads / 64;    // a workgroup takes kDenseWaves rows per round
constexpr int kDenseParamRows = 3;                                      // bias | gamma | beta, rows of C floats
constexpr int kDenseMaxGrid = kEmbMaxGrid;                              // forward
constexpr int kDenseMaxGridBwd = kEmbMaxGridBwd;                        // backward: the slices of the workspace
constexpr int kDenseMaxC = 512;

__host__ __device__ constexpr int dense_grid(int n, int cap) {
    const int nb = (n + kDenseWaves - 1) / kDenseWaves;
    return nb < cap ? nb : cap;
}

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

// V adjacent elements as one piece: 16 bytes at the most per access, aligned to its size
template <typename T, int V> struct alignas(sizeof(T) * V < 16 ? sizeof(T) * V : 16) DenseVec { T v[V]; };

template <typename T, int V> HSD void dense_load_as(const void *p, size_t i, float (&v)[V]) {
    const DenseVec<T, V> t = *(const DenseVec<T, V> *)((const T *)p + i);
    _Pragma("unroll") for (int k = 0; k < V; ++k) v[k] = (float)t.v[k];
}
template <typename T, int V> HSD void dense_store_as(void *p, size_t i, const float (&v)[V]) {
    DenseVec<T, V> t;
    _Pragma("unroll") for (int k = 0; k < V; ++k) t.v[k] = (T)v[k];
    *(DenseVec<T, V> *)((T *)p + i) = t;
}
// elements i .. i + V - 1 (i a multiple of V) of an array of run-time type, widened exactly / rounded to nearest even
template <int V> HSD void dense_load(const void *p, int type, size_t i, float (&v)[V]) {
    if (type == kEmbF32) dense_load_as<float, V>(p, i, v);
    else if (type == kEmbBf16) dense_load_as<SampleBf16, V>(p, i, v);
    else dense_load_as<SampleF16, V>(p, i, v);
}
template <int V> HSD void dense_store(void *p, int type, size_t i, const float (&v)[V]) {
    if (type == kEmbF32) dense_store_as<float, V>(p, i, v);
    else if (type == kEmbBf16) dense_store_as<SampleBf16, V>(p, i, v);
    else dense_store_as<SampleF16, V>(p, i, v);
}

// the sum over a row's C channels of p[k] (this lane's channels V l + k): ascending k, then the xor butterfly 1, 2, ..., 32
template <int C> HSD float dense_sum(const float (&p)[C / 64]) {
    float s = p[0];
    _Pragma("unroll") for (int k = 1; k < C / 64; ++k) s = s + p[k];
    _Pragma("unroll") for (int m = 1; m < 64; m <<= 1) s = s + __shfl_xor(s, m, 64);
    return s;
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
    float a[V], d[V], dd[V];
    dense_load<V>(z, zType, (size_t)row * C + V * lane, a);
    _Pragma("unroll") for (int k = 0; k < V; ++k) a[k] = a[k] + P[0][k];
    const float mu = dense_sum<C>(a) / (float)C;
    _Pragma("unroll") for (int k = 0; k < V; ++k) { d[k] = a[k] - mu; dd[k] = d[k] * d[k]; }
    const float var = dense_sum<C>(dd) / (float)C;
    r.rstd = 1.0f / sqrtf(var + eps);
    _Pragma("unroll") for (int k = 0; k < V; ++k) { r.h[k] = d[k] * r.rstd; r.u[k] = fmaf(P[1][k], r.h[k], P[2][k]); }
}

template <int C> HSD void dense_params(const float *params, int lane, float (&P)[kDenseParamRows][C / 64]) {
    _Pragma("unroll") for (int j = 0; j < kDenseParamRows; ++j)
        _Pragma("unroll") for (int k = 0; k < C / 64; ++k) P[j][k] = params[j * C + (C / 64) * lane + k];
}

template <int C>
__global__ __launch_bounds__(kDenseThreads) void k_dense_fwd(DenseArgs a) {
    constexpr int V = C / 64;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    float P[kDenseParamRows][V];
    dense_params<C>(a.params, lane, P);
    const int nrounds = (a.n + kDenseWaves - 1) / kDenseWaves;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row = round * kDenseWaves + wave;
        if (row >= a.n) break;                                                 // wave-uniform; the later rounds lie further past n
        DenseRow<C> r;
        dense_row<C>(a.z, a.zType, P, a.eps, row, lane, r);
        float y[V];
        _Pragma("unroll") for (int k = 0; k < V; ++k) y[k] = r.u[k] > 0.f ? r.u[k] : a.slope * r.u[k];
        dense_store<V>(a.y, a.yType, (size_t)row * C + V * lane, y);
    }
}

template <int C>
__global__ __launch_bounds__(kDenseThreads) void k_dense_bwd(DenseBwdArgs a) {
    constexpr int V = C / 64;
    __shared__ float S[kDenseParamRows * C];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    float P[kDenseParamRows][V], acc[kDenseParamRows][V];
    dense_params<C>(a.params, lane, P);
    _Pragma("unroll") for (int j = 0; j < kDenseParamRows; ++j)
        _Pragma("unroll") for (int k = 0; k < V; ++k) acc[j][k] = 0.f;
    const int nrounds = (a.n + kDenseWaves - 1) / kDenseWaves;
    for (int round = blockIdx.x; round < nrounds; round += gridDim.x) {
        const int row = round * kDenseWaves + wave;
        if (row >= a.n) break;                                                 // wave-uniform; no barrier inside the loop
        DenseRow<C> r;
        dense_row<C>(a.z, a.zType, P, a.eps, row, lane, r);
        const size_t i0 = (size_t)row * C + V * lane;
        float g[V], du[V], dh[V], hz[V], da[V];
        dense_load<V>(a.gradY, a.yType, i0, g);
        _Pragma("unroll") for (int k = 0; k < V; ++k) {
            du[k] = r.u[k] > 0.f ? g[k] : a.slope * g[k];
            dh[k] = du[k] * P[1][k];
            hz[k] = dh[k] * r.h[k];
        }
        const float m1 = dense_sum<C>(dh) / (float)C, m2 = dense_sum<C>(hz) / (float)C;
        _Pragma("unroll") for (int k = 0; k < V; ++k) {
            da[k] = r.rstd * ((dh[k] - m1) - r.h[k] * m2);
            acc[0][k] = acc[0][k] + da[k];
            acc[1][k] = fmaf(du[k], r.h[k], acc[1][k]);
            acc[2][k] = acc[2][k] + du[k];
        }
        if (a.gradZ) dense_store<V>(a.gradZ, a.zType, i0, da);
    }
    if (!a.workspace) return;                                                  // uniform over the grid
    for (int w = 0; w < kDenseWaves; ++w) {                                    // ((w0 + w1) + w2) + w3
        if (w) __syncthreads();
        if (wave == w) {
            _Pragma("unroll") for (int j = 0; j < kDenseParamRows; ++j)
                _Pragma("unroll") for (int k = 0; k < V; ++k) {
                    const int i = j * C + V * lane + k;
                    S[i] = w == 0 ? acc[j][k] : S[i] + acc[j][k];
                }
        }
    }
    __syncthreads();
    float *out = a.workspace + (size_t)blockIdx.x * (kDenseParamRows * C);
    for (int i = threadIdx.x; i < kDenseParamRows * C; i += kDenseThreads) out[i] = S[i];
}

}  // namespace hs
