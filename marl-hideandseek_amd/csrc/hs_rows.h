// What the row-wise learner kernels (k_embed, k_lstm, k_dense) share: a wave works a row of N channels, a workgroup of
// four waves takes its rows grid-stride in rounds, and every sum has one fixed order.  include/hideseek.h states the
// arithmetic per entry point; the orders it states are written here, once.
//   elements  arrays of f32, bf16 or f16 chosen at run time by a code (a wave-uniform branch per access), read by
//             element or as one ElemVec piece of up to 16 bytes; widening is exact, narrowing rounds to nearest even.
//   channels  a lane holds kPer of a row's N = kLanes kPer channels.  StridedMap: c = lane + kLanes q, a wave's access is
//             kLanes consecutive elements.  AdjacentMap: c = kPer lane + q, a lane's access is one piece of kPer elements.
//   row_sum   a lane's own kPer terms in ascending order, then the xor butterfly 1, 2, 4, ... over the kLanes lanes: float
//             addition commutes, so every lane ends with the same bits.
//   LayerNorm row_norm and row_norm_bwd are the statistics and their gradient with exactly the expression trees written
//             below; the affine part and the activation differ in operand order and stay with each kernel.
//   gradients a backward keeps its parameter sums in registers over all the rows its wave takes, in round order;
//             wave_sums_to_slice adds the waves in LDS as ((w0 + w1) + w2) + w3 and writes the workgroup's slice of a
//             workspace, whose size the backward grid cap fixes; k_partials_sum adds the slices: kSegs segments each add a
//             contiguous run of slices in ascending order onto 0, then segment 0 adds the segments in ascending order.
// No atomics anywhere: the same inputs give the same bits on every call.
#pragma once
#include "hs_dev.h"
#include "hs_k_sample.h"                   // SampleBf16 / SampleF16 only: the narrow types of every learner kernel are declared
                                           // there, and moving them would change what hs_k_sample.h and hs_k_gae.h include

namespace hs {

constexpr int kRowsThreads = 256, kRowsWaves = kRowsThreads / 64;       // a workgroup: four waves, each at rows of its own
constexpr int kRowsMaxGrid = 2048;                                      // forward: 256 CUs x 8 workgroups
constexpr int kRowsMaxGridBwd = 512;                                    // backward: the slices of a workspace
constexpr int kRowsSumSegs = 8, kRowsSumCols = 32;                      // k_partials_sum over a backward's workspace

__host__ __device__ constexpr int rows_grid(int n, int rowsPerRound, int cap) {
    const int nb = (n + rowsPerRound - 1) / rowsPerRound;
    return nb < cap ? nb : cap;
}

enum { kElemF32 = 0, kElemBf16 = 1, kElemF16 = 2 };    // element types, chosen at run time

HSD float elem_load(const void *p, int type, size_t i) {
    if (type == kElemF32) return ((const float *)p)[i];
    if (type == kElemBf16) return (float)((const SampleBf16 *)p)[i];
    return (float)((const SampleF16 *)p)[i];
}
HSD void elem_store(void *p, int type, size_t i, float v) {
    if (type == kElemF32) ((float *)p)[i] = v;
    else if (type == kElemBf16) ((SampleBf16 *)p)[i] = (SampleBf16)v;
    else ((SampleF16 *)p)[i] = (SampleF16)v;
}

// V adjacent elements as one piece: 16 bytes at the most per access, aligned to its size
template <typename T, int V> struct alignas(sizeof(T) * V < 16 ? sizeof(T) * V : 16) ElemVec { T v[V]; };

// A lane-to-channel map: kLanes lanes hold a row's kN = kLanes kPer channels, kPer each; ch is the index, counted from
// `base`, of the q-th of this lane's.
template <int P, int L = 64> struct StridedMap {
    static constexpr int kPer = P, kLanes = L, kN = L * P;
    HSD static int ch(int base, int lane, int q) { return base + lane + L * q; }
};
template <int P> struct AdjacentMap {
    static constexpr int kPer = P, kLanes = 64, kN = 64 * P;
    HSD static int ch(int base, int lane, int q) { return base + P * lane + q; }
};

// the sum over a row's channels of p[q] (this lane's)
template <int kPer, int kLanes = 64> HSD float row_sum(const float (&p)[kPer]) {
    float s = p[0];
    _Pragma("unroll") for (int q = 1; q < kPer; ++q) s = s + p[q];
    _Pragma("unroll") for (int m = 1; m < kLanes; m <<= 1) s = s + __shfl_xor(s, m, kLanes);
    return s;
}

// LayerNorm statistics of a row: xhat from x; returns rstd
template <int kPer, int kLanes = 64> HSD float row_norm(const float (&x)[kPer], float eps, float (&xhat)[kPer]) {
    constexpr float N = (float)(kPer * kLanes);
    const float mu = row_sum<kPer, kLanes>(x) / N;
    float d[kPer], dd[kPer];
    _Pragma("unroll") for (int q = 0; q < kPer; ++q) { d[q] = x[q] - mu; dd[q] = d[q] * d[q]; }
    const float var = row_sum<kPer, kLanes>(dd) / N;
    const float rstd = 1.0f / sqrtf(var + eps);
    _Pragma("unroll") for (int q = 0; q < kPer; ++q) xhat[q] = d[q] * rstd;
    return rstd;
}

// its gradient: dx from h = gamma * dy (the gradient with respect to xhat)
template <int kPer, int kLanes = 64> HSD void row_norm_bwd(const float (&h)[kPer], const float (&xhat)[kPer], float rstd, float (&dx)[kPer]) {
    constexpr float N = (float)(kPer * kLanes);
    float hz[kPer];
    _Pragma("unroll") for (int q = 0; q < kPer; ++q) hz[q] = h[q] * xhat[q];
    const float mh = row_sum<kPer, kLanes>(h) / N, mhz = row_sum<kPer, kLanes>(hz) / N;
    _Pragma("unroll") for (int q = 0; q < kPer; ++q) dx[q] = rstd * ((h[q] - mh) - xhat[q] * mhz);
}

// this lane's values of kRows parameter rows of N floats each
template <typename Map, int kRows> HSD void lane_params(const float *params, int lane, float (&P)[kRows][Map::kPer]) {
    _Pragma("unroll") for (int j = 0; j < kRows; ++j)
        _Pragma("unroll") for (int q = 0; q < Map::kPer; ++q) P[j][q] = params[Map::ch(j * Map::kN, lane, q)];
}

// The waves' register sums acc, added through S (LDS, kRows N floats, free to be written once every wave has arrived) as
// ((w0 + w1) + w2) + w3, then to out[0 .. kRows N): the workgroup's slice.  The lane comes from hs_lane(): inside
// `wave == w` the compiler knows the range of threadIdx.x and rewrites a lane derived from it, in some of the addresses
// and not in others, after which it neither pairs the LDS accesses nor sees that they are distinct.
template <typename Map, int kRows> HSD void wave_sums_to_slice(const float (&acc)[kRows][Map::kPer], float *S, float *out) {
    constexpr int N = Map::kN;
    const int wave = threadIdx.x / 64, lane = hs_lane() % 64;
    for (int w = 0; w < kRowsWaves; ++w) {
        if (w) __syncthreads();
        if (wave == w && lane < Map::kLanes) {                                 // k_embed<32>: the upper half-wave's sums are folded already
            _Pragma("unroll") for (int j = 0; j < kRows; ++j)
                _Pragma("unroll") for (int q = 0; q < Map::kPer; ++q) {
                    const int i = Map::ch(j * N, lane, q);
                    S[i] = w == 0 ? acc[j][q] : S[i] + acc[j][q];
                }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kRows * N; i += kRowsThreads) out[i] = S[i];
}

// out[c] = sum of partials[0 .. nparts)[c], c < len, always in the same order: kSegs lanes per column each add a
// contiguous run of slices in ascending order onto 0, then the first of them adds the runs in ascending order.
template <typename T, int kCols, int kSegs>
__global__ __launch_bounds__(kCols * kSegs) void k_partials_sum(const T *__restrict__ partials, int nparts, int len, T *__restrict__ out) {
    __shared__ T seg[kSegs][kCols];
    const int cl = threadIdx.x % kCols, sg = threadIdx.x / kCols, c = blockIdx.x * kCols + cl;
    const int per = (nparts + kSegs - 1) / kSegs;
    const int b0 = sg * per, b1 = b0 + per < nparts ? b0 + per : nparts;
    T s = 0;
    if (c < len)
        for (int b = b0; b < b1; ++b) s = s + partials[(size_t)b * len + c];
    seg[sg][cl] = s;
    __syncthreads();
    if (sg == 0 && c < len) {
        T t = seg[0][cl];
        for (int k = 1; k < kSegs; ++k) t = t + seg[k][cl];
        out[c] = t;
    }
}

}  // namespace hs
