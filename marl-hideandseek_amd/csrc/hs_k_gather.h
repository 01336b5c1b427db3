// The minibatch gather (hs_gather_sequences): cutting m shuffled BPTT sequences out of a rollout of K chunks of L steps
// over n rows, every field of the rollout in ONE launch.  include/hideseek.h states the contract: sequence id s = k n + r,
// a per-step field copies dst[t][j] = src[k L + t][r] for t < L, a per-chunk field dst[j] = src[k][r]; a pure copy of bytes.
//
// A bandwidth kernel: no LDS, no arithmetic on the data, and the one atomic is the count of the ids out of range.
// How the work is dealt.  The host puts the WIDE fields first (row_bytes a multiple of 16 and both bases 16-byte aligned:
// the 592-byte rows of the policy inputs, the 512- and 1024-byte rows of the LSTM states, which carry almost all of the
// bytes) and the NARROW ones (everything else: 4- and 20-byte rows) behind them.  A unit of work belongs to one wave:
//   unit u = slot m + j,   slot < nWide:   the rows of sequence index[j] of wide field `slot`, a wave per row-copy: lane l
//                                           moves the 16-byte pieces l, l + 64, ... of a row, kGatherInFlight rows' loads
//                                           in flight before the first store;
//                          slot == nWide:  the rows of sequence index[j] of EVERY narrow field, dword by dword, field after
//                                           field: the narrow fields ride along in one wave per sequence.
// Neighbouring waves take neighbouring j of one field, so their stores fill neighbouring rows of dst[t].  The grid is
// capped at kGatherMaxGrid workgroups of four waves, which take their units grid-stride.  The wave index goes through
// readfirstlane: slot, j, the id and with them every row base are scalar, and a lane adds its piece's offset.
// Byte offsets are 64-bit throughout: the actor rows of the training size are 2.27 GB.
// An id outside [0, K n) reads nothing: its destination rows are written as zeros, and the wave of slot 0 counts it.
// (DESIGN.md section 5 has the measurement, and that of a second form which interleaved the slots of a sequence, took all
// per-chunk fields in one unit and had six loads in flight: it was slower.)
//
// The kernel is a template, as hs_k_norm.h explains.
#pragma once
#include "hs_dev.h"

namespace hs {

constexpr int kGatherThreads = 256;
constexpr int kGatherWaves = kGatherThreads / 64;
constexpr int kGatherMaxFields = 16;
constexpr int kGatherMaxGrid = 2048;                                    // 256 CUs x 8 workgroups of 4 waves
constexpr int kGatherInFlight = 4;                                      // rows of a wide field whose loads are in flight together
constexpr int kGatherVec = 16;                                          // bytes of a wide lane's piece

struct GatherField {
    const char *src;
    char *dst;
    int32_t rowBytes, perChunk;
};

struct GatherArgs {
    GatherField f[kGatherMaxFields];      // the wide fields, then the narrow ones
    const int32_t *index;                 // [m]
    int32_t *bad;                         // [1] or null: zero before the launch
    int32_t nWide, nFields;
    int32_t m, L, n;
    int32_t total;                        // K n
    uint32_t units;                       // (nWide + (nFields > nWide)) m
};

typedef uint32_t GatherPiece __attribute__((ext_vector_type(4)));

// the rows of one sequence of a wide field: src rows row0, row0 + n, ... (a per-chunk field has one), dst rows j, m + j, ...
HSD void gather_wide(const GatherField &f, int rows, int64_t row0, int n, int m, int j, bool ok, int lane) {
    const int pieces = f.rowBytes / kGatherVec;
    const int64_t rb = f.rowBytes;
    for (int t0 = 0; t0 < rows; t0 += kGatherInFlight) {
        for (int p = lane; p < pieces; p += 64) {
            GatherPiece v[kGatherInFlight];
            _Pragma("unroll") for (int q = 0; q < kGatherInFlight; ++q) {
                v[q] = GatherPiece{0u, 0u, 0u, 0u};
                if (ok && t0 + q < rows) v[q] = *(const GatherPiece *)(f.src + (row0 + (int64_t)(t0 + q) * n) * rb + (int64_t)p * kGatherVec);
            }
            _Pragma("unroll") for (int q = 0; q < kGatherInFlight; ++q)
                if (t0 + q < rows) *(GatherPiece *)(f.dst + ((int64_t)(t0 + q) * m + j) * rb + (int64_t)p * kGatherVec) = v[q];
        }
    }
}

// the same for a narrow field, a dword per lane: dword e of the sequence is word e % W of its row e / W
HSD void gather_narrow(const GatherField &f, int rows, int64_t row0, int n, int m, int j, bool ok, int lane) {
    const int W = f.rowBytes / 4, words = rows * W;
    for (int e = lane; e < words; e += 64) {
        const int t = e / W, w = e - t * W;
        uint32_t v = 0u;
        if (ok) v = ((const uint32_t *)f.src)[(row0 + (int64_t)t * n) * W + w];
        ((uint32_t *)f.dst)[((int64_t)t * m + j) * W + w] = v;
    }
}

template <int kThreads = kGatherThreads>
__global__ __launch_bounds__(kThreads) void k_gather(GatherArgs a) {
    const int lane = threadIdx.x % 64;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kGatherWaves + threadIdx.x / 64));
    const uint32_t stride = gridDim.x * kGatherWaves;                   // units < 2^31 and stride <= 8192: u + stride does not wrap
    for (uint32_t u = wave; u < a.units; u += stride) {
        const int slot = (int)(u / (uint32_t)a.m), j = (int)(u - (uint32_t)slot * (uint32_t)a.m);
        const int32_t s = a.index[j];
        const bool ok = (uint32_t)s < (uint32_t)a.total;
        const int k = ok ? s / a.n : 0, r = ok ? s - k * a.n : 0;
        if (!ok && slot == 0 && lane == 0 && a.bad) atomicAdd(a.bad, 1);
        if (slot < a.nWide) {
            const GatherField &f = a.f[slot];
            gather_wide(f, f.perChunk ? 1 : a.L, f.perChunk ? (int64_t)s : (int64_t)k * a.L * a.n + r, a.n, a.m, j, ok, lane);
        } else {
            for (int i = a.nWide; i < a.nFields; ++i) {
                const GatherField &f = a.f[i];
                gather_narrow(f, f.perChunk ? 1 : a.L, f.perChunk ? (int64_t)s : (int64_t)k * a.L * a.n + r, a.n, a.m, j, ok, lane);
            }
        }
    }
}

}  // namespace hs
