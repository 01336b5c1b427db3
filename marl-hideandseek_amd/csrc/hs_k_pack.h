// Policy-input rows: the exported observations of every agent packed into one row of kPackRow features, in the
// learner's element type (hs_pack_policy_inputs) — what the reference's policy does to the observation tensors before
// its network sees them (scripts/jax_policy.py:84-98 extract_self_obs, :262-280 the actor's masked entity tables,
// :372-390 the critic's unmasked ones).
//
// Row `world * A + slot`, columns:
//     0          (float)prep_counter / 96.0f
//     1 - 13     self_data
//     14         (float)self_type
//     15 - 44    lidar
//     45 - 114   agent_data   5 x 14, entity-major
//     115 - 267  box_data     9 x 17
//     268 - 295  ramp_data    2 x 14
// The critic row holds the data as exported; the actor row holds data * visibility mask of the entity in columns 45-295
// (an IEEE f32 multiplication, not a select).  Narrowing to bf16 / f16 rounds the f32 value to nearest even.
// Moments (optional): with m = self_mask of the row and x the f32 critic value, sum m x, sum m x x per column and sum m,
// in f64: each workgroup keeps its sums in registers over the row blocks it owns and stores them to its row of
// a workspace; k_partials_sum (hs_rows.h) adds the rows in its fixed order.  No atomics, so the result is the same on every run.
//
// It is a gather / convert / scatter kernel bound by HBM.  A workgroup takes kPackRows consecutive agent rows at a time
// (grid-stride over row blocks).  Every input table is ONE contiguous byte range over those rows, starting on a
// 128-byte boundary (kPackRows rows x 4 B), so it is read with 16-byte loads, lane i the i-th 16 bytes of the range
// (4-byte loads for what a partial last block leaves over), and its elements go to their columns of an LDS image
// [kPackRows][kPackRow] f32 of the critic rows.  The output rows of the block are again one contiguous range: lane i
// takes the i-th 16 bytes of it (4 f32 or 8 narrow values, never across a row: kPackRow is a multiple of 8), reads them
// from the image with ds_read_b128, multiplies by the masks for the actor, converts and stores 16 bytes.
#pragma once
#include <type_traits>
#include "hs_state.h"

namespace hs {

// widths of the packed tables (hideseek.hip asserts them against kExports and HS_PACK_ROW)
constexpr int kPackSelfW = 13, kPackLidarW = 30;
constexpr int kPackAgentN = 5, kPackAgentW = 14, kPackBoxN = 9, kPackBoxW = 17, kPackRampN = 2, kPackRampW = 14;
constexpr int kPackColSelf = 1, kPackColType = kPackColSelf + kPackSelfW, kPackColLidar = kPackColType + 1;
constexpr int kPackColAgents = kPackColLidar + kPackLidarW;                    // the "self" row ends here
constexpr int kPackColBoxes = kPackColAgents + kPackAgentN * kPackAgentW;
constexpr int kPackColRamps = kPackColBoxes + kPackBoxN * kPackBoxW;
constexpr int kPackRow = kPackColRamps + kPackRampN * kPackRampW;
constexpr int kPackMoments = 2 * kPackRow + 1;
constexpr int kPackEntities = kPackAgentN + kPackBoxN + kPackRampN;           // visibility masks per row
constexpr float kPackPrepScale = 96.f;                                         // jax_policy.py:86
static_assert(kPackRow % 8 == 0, "a 16-byte piece of a bf16 / f16 row must not cross rows");

constexpr int kPackThreads = 256;
constexpr int kPackRows = 32;             // agent rows per block: 37 KB of image, four workgroups per CU
constexpr int kPackMaxGrid = 1024;        // workgroups (and rows of the moments workspace): 256 CUs x 4
constexpr int kPackSumSegs = 16;          // k_partials_sum: segments of the workspace rows summed side by side

struct PackAbsent {};                     // element type of an output that was not requested
typedef __bf16 PackBf16;
typedef _Float16 PackF16;
typedef short PackShort8 __attribute__((ext_vector_type(8)));
typedef __bf16 PackBf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 PackF16x2 __attribute__((ext_vector_type(2)));
typedef float PackFloat2 __attribute__((ext_vector_type(2)));

struct PackArgs {
    const int32_t *prep, *selfType;
    const float *selfObs, *selfMask, *lidar, *agentObs, *boxObs, *rampObs, *visAgents, *visBoxes, *visRamps;
    void *actor, *critic;
    double *partials;                     // [gridDim.x][kPackMoments]
    int rows;
};

__host__ __device__ constexpr int pack_grid(int rows) {
    const int nb = (rows + kPackRows - 1) / kPackRows;
    return nb < kPackMaxGrid ? nb : kPackMaxGrid;
}

// The mask of column c >= kPackColAgents within a row's kPackEntities masks.
HSD int pack_mask_index(int c) {
    if (c < kPackColBoxes) return (c - kPackColAgents) / kPackAgentW;
    if (c < kPackColRamps) return kPackAgentN + (c - kPackColBoxes) / kPackBoxW;
    return kPackAgentN + kPackBoxN + (c - kPackColRamps) / kPackRampW;
}

// n consecutive elements of a table with W per row, from src (16-byte aligned), to dst[row * STRIDE + col] through f().
template <int W, int STRIDE, bool FULL, typename T, typename F>
HSD void pack_stage(const T *__restrict__ src, int nrows, float *dst, F f) {
    typedef T Vec4 __attribute__((ext_vector_type(4)));
    const int n = FULL ? kPackRows * W : nrows * W, n4 = n >> 2;
    const Vec4 *src4 = (const Vec4 *)src;
#pragma unroll
    for (int i = threadIdx.x; i < n4; i += kPackThreads) {
        const Vec4 v = src4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = i * 4 + k, r = e / W;
            dst[r * STRIDE + (e - r * W)] = f(v[k]);
        }
    }
    if (!FULL) {                          // a partial last block may end inside a 16-byte piece
        const int e = n4 * 4 + threadIdx.x;
        if (e < n) { const int r = e / W; dst[r * STRIDE + (e - r * W)] = f(src[e]); }
    }
}

struct PackImage {
    alignas(16) float row[kPackRows * kPackRow];          // the critic rows, f32
    float vis[kPackRows * kPackEntities];                 // visibility masks, agents | boxes | ramps
    float selfMask[kPackRows];
    unsigned char maskOf[kPackRow];                       // column -> its mask (pack_mask_index)
};

template <bool FULL> HSD void pack_load(const PackArgs &a, size_t row0, int nrows, PackImage &im, bool actor, bool moments) {
    auto same = [](float x) { return x; };
    float *img = im.row;
    pack_stage<1, kPackRow, FULL>(a.prep + row0, nrows, img, [](int32_t p) { return (float)p / kPackPrepScale; });
    pack_stage<kPackSelfW, kPackRow, FULL>(a.selfObs + row0 * kPackSelfW, nrows, img + kPackColSelf, same);
    pack_stage<1, kPackRow, FULL>(a.selfType + row0, nrows, img + kPackColType, [](int32_t t) { return (float)t; });
    pack_stage<kPackLidarW, kPackRow, FULL>(a.lidar + row0 * kPackLidarW, nrows, img + kPackColLidar, same);
    pack_stage<kPackAgentN * kPackAgentW, kPackRow, FULL>(a.agentObs + row0 * (kPackAgentN * kPackAgentW), nrows, img + kPackColAgents, same);
    pack_stage<kPackBoxN * kPackBoxW, kPackRow, FULL>(a.boxObs + row0 * (kPackBoxN * kPackBoxW), nrows, img + kPackColBoxes, same);
    pack_stage<kPackRampN * kPackRampW, kPackRow, FULL>(a.rampObs + row0 * (kPackRampN * kPackRampW), nrows, img + kPackColRamps, same);
    if (actor) {
        pack_stage<kPackAgentN, kPackEntities, FULL>(a.visAgents + row0 * kPackAgentN, nrows, im.vis, same);
        pack_stage<kPackBoxN, kPackEntities, FULL>(a.visBoxes + row0 * kPackBoxN, nrows, im.vis + kPackAgentN, same);
        pack_stage<kPackRampN, kPackEntities, FULL>(a.visRamps + row0 * kPackRampN, nrows, im.vis + kPackAgentN + kPackBoxN, same);
    }
    if (moments) pack_stage<1, 1, FULL>(a.selfMask + row0, nrows, im.selfMask, same);
}

// K f32 values -> 16 bytes of T at dst.
HSD void pack_store16(float *dst, const float (&v)[4]) { *(float4 *)dst = float4{v[0], v[1], v[2], v[3]}; }
HSD void pack_store16(PackBf16 *dst, const float (&v)[8]) {
    union { PackBf16x2 h[4]; PackShort8 s; } u;
#pragma unroll
    for (int k = 0; k < 4; ++k) u.h[k] = __builtin_convertvector(PackFloat2{v[2 * k], v[2 * k + 1]}, PackBf16x2);
    *(PackShort8 *)dst = u.s;
}
HSD void pack_store16(PackF16 *dst, const float (&v)[8]) {
    union { PackF16x2 h[4]; PackShort8 s; } u;
#pragma unroll
    for (int k = 0; k < 4; ++k) u.h[k] = __builtin_convertvector(PackFloat2{v[2 * k], v[2 * k + 1]}, PackF16x2);
    *(PackShort8 *)dst = u.s;
}

// The block's rows to out (rows of kPackRow T from row0 on), 16 bytes per lane and pass; MASKED: the actor's rows.
// NORM: y = (x - mu[c]) * inv[c] first, an f32 subtraction and an f32 multiplication, with mu | inv the two halves of
// `table` (hs_k_norm.h).  A piece starts at a column that is a multiple of K, so its mu and inv are aligned 16-byte
// vectors of the table, loaded from global memory (2.4 KB, cache-resident) ahead of the ds_read they meet.
template <typename T, bool MASKED, bool NORM> HSD void pack_write(T *out, size_t row0, int nrows, const PackImage &im, const float *__restrict__ table) {
    constexpr int K = 16 / (int)sizeof(T), kPerRow = kPackRow / K;
    T *dst = out + row0 * kPackRow;
    const int n = nrows * kPerRow;
    for (int q = threadIdx.x; q < n; q += kPackThreads) {
        float v[K];
        [[maybe_unused]] float4 mu[K / 4], inv[K / 4];
        if (NORM) {
            const int c0 = (q % kPerRow) * K;
#pragma unroll
            for (int k = 0; k < K / 4; ++k) {
                mu[k] = *(const float4 *)(table + c0 + 4 * k);
                inv[k] = *(const float4 *)(table + kPackRow + c0 + 4 * k);
            }
        }
#pragma unroll
        for (int k = 0; k < K; k += 4) {
            const float4 x = *(const float4 *)(im.row + q * K + k);
            v[k] = x.x; v[k + 1] = x.y; v[k + 2] = x.z; v[k + 3] = x.w;
        }
        if (NORM) {
#pragma unroll
            for (int k = 0; k < K; k += 4) {
                v[k] = (v[k] - mu[k / 4].x) * inv[k / 4].x;
                v[k + 1] = (v[k + 1] - mu[k / 4].y) * inv[k / 4].y;
                v[k + 2] = (v[k + 2] - mu[k / 4].z) * inv[k / 4].z;
                v[k + 3] = (v[k + 3] - mu[k / 4].w) * inv[k / 4].w;
            }
        }
        if (MASKED) {
            const int r = q / kPerRow, c0 = (q - r * kPerRow) * K;
            if (c0 + K > kPackColAgents) {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (c0 + k >= kPackColAgents) v[k] = v[k] * im.vis[r * kPackEntities + im.maskOf[c0 + k]];
            }
        }
        pack_store16(dst + (size_t)q * K, v);
    }
}

struct PackDirect {};                     // the staging of k_pack and k_pack_norm: row r of the output is agent row r (pack_load)

// The body of k_pack and of k_pack_norm (hs_k_norm.h), one instantiation per kernel, so the image is that kernel's LDS:
// the row blocks of one workgroup staged, written as the actor's and the critic's rows, and the moments of the raw image.
// With a Route other than PackDirect (k_pack_routed, hs_k_pack_routed.h) the image is staged by route.load() instead, and
// route.finish() runs after the rows are written; everything else is this body as it is.
template <typename TA, typename TC, bool MOM, bool NORM, typename Route = PackDirect>
HSD void pack_blocks(const PackArgs a, const float *__restrict__ table, Route route = Route{}) {
    constexpr bool kActor = !std::is_same<TA, PackAbsent>::value;
    constexpr bool kRouted = !std::is_same<Route, PackDirect>::value;
    __shared__ PackImage im;
    if (kActor)
        for (int c = kPackColAgents + threadIdx.x; c < kPackRow; c += kPackThreads) im.maskOf[c] = (unsigned char)pack_mask_index(c);
    // moments: lane t owns columns t and kPackThreads + t
    constexpr int kOwn = (kPackRow + kPackThreads - 1) / kPackThreads;
    double s1[kOwn], s2[kOwn], cnt = 0.0;
#pragma unroll
    for (int j = 0; j < kOwn; ++j) s1[j] = s2[j] = 0.0;

    const int nblocks = (a.rows + kPackRows - 1) / kPackRows;
    for (int b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const size_t row0 = (size_t)b * kPackRows;
        const int nrows = a.rows - (int)row0 < kPackRows ? a.rows - (int)row0 : kPackRows;
        if (b != blockIdx.x) __syncthreads();             // the previous block's readers are done with the image
        if constexpr (kRouted) route.load(a, row0, nrows, im, kActor, MOM);
        else if (nrows == kPackRows) pack_load<true>(a, row0, nrows, im, kActor, MOM);
        else pack_load<false>(a, row0, nrows, im, kActor, MOM);
        __syncthreads();
        if constexpr (kActor) pack_write<TA, true, NORM>((TA *)a.actor, row0, nrows, im, table);
        if constexpr (!std::is_same<TC, PackAbsent>::value) pack_write<TC, false, NORM>((TC *)a.critic, row0, nrows, im, table);
        if constexpr (kRouted) route.template finish<TA, TC>(a, row0, nrows);
        if (MOM) {
#pragma unroll
            for (int j = 0; j < kOwn; ++j) {
                const int c = j * kPackThreads + threadIdx.x;
                if (c < kPackRow)
                    for (int r = 0; r < nrows; ++r) {
                        const double x = (double)im.row[r * kPackRow + c], mx = (double)im.selfMask[r] * x;
                        s1[j] += mx;
                        s2[j] += mx * x;
                    }
            }
            if (threadIdx.x == 0)
                for (int r = 0; r < nrows; ++r) cnt += (double)im.selfMask[r];
        }
    }
    if (MOM) {
        double *p = a.partials + (size_t)blockIdx.x * kPackMoments;
#pragma unroll
        for (int j = 0; j < kOwn; ++j) {
            const int c = j * kPackThreads + threadIdx.x;
            if (c < kPackRow) { p[c] = s1[j]; p[kPackRow + c] = s2[j]; }
        }
        if (threadIdx.x == 0) p[2 * kPackRow] = cnt;
    }
}

template <typename TA, typename TC, bool MOM>
__global__ __launch_bounds__(kPackThreads) void k_pack(PackArgs a) {
    pack_blocks<TA, TC, MOM, false>(a, nullptr);
}

}  // namespace hs
