// Episode statistics (hs_episode_stats): after a step, one lane per agent row (row = world * A + slot) advances the row's
// tracker (undiscounted and discounted return, length, the latched agent type) and the lane of a world's first row the
// world's (the latched team order), and every episode that ended with the step is folded into a table of f64 sums.
// include/hideseek.h states the arithmetic, IEEE f32 without contraction in a fixed order, and the restart rule, which is
// rollout.state_zero_into's.
//
// A workgroup takes whole worlds, kEpiThreads / A of them, so that what a world needs of its rows (did one end, did one
// restart) crosses lanes through LDS and a barrier and never through memory another workgroup writes: the row state is
// updated in place, and a lane that read a sibling row's phase from memory would race with the lane that owns it.  The
// rows of a workgroup are contiguous: a wave's access to an input or a state array is one 256-byte range.  The last
// lanes of a workgroup (kEpiThreads % A, and those past the last world) hold no row.
// Sums: a lane holds the kEpiStats terms of its own row (and of its world); a wave adds them by the xor butterfly 1, 2,
// 4, ... (float addition commutes: every lane ends with the same bits), the workgroup's waves are added in wave order
// onto the first, and k_episode_fold adds the workgroups' partials as k_partials_sum (hs_rows.h) does, kSegs runs of
// slices in ascending order, then the runs in ascending order, and adds that sum to the table once.  No atomics, and an
// order that depends on (worlds, A) alone.  Episodes end every 240 steps: a workgroup none of whose rows ended writes
// +0.0 partials (what the sums would have given) without the butterfly.
#pragma once
#include "hs_state.h"

namespace hs {

constexpr int kEpiThreads = 256, kEpiStats = 14, kEpiSide = 5;
constexpr int kEpiHiderWins = 10, kEpiSeekerWins = 11, kEpiDraws = 12, kEpiWorldEpisodes = 13;
constexpr int kEpiOut = 0, kEpiTracked = 1, kEpiWaiting = 2;
constexpr int kEpiSumSegs = 32;           // k_episode_fold: segments of the partials summed side by side

struct EpisodeArgs {
    const float *reward;
    const int32_t *done, *selfType;
    const float *selfMask, *episodeResult;
    const int32_t *hiderTeam;             // or null: from counts
    const int *counts;                    // the handle's SimState::counts (cnt_seekers_first)
    float *ret, *disc, *gpow;
    int32_t *len, *type, *phase;
    int32_t *worldTeam, *worldPhase;
    double *partials;                     // [episode_grid][kEpiStats]
    int worlds, A;
    float gamma;
};

__host__ __device__ constexpr int episode_worlds_per_group(int A) { return kEpiThreads / A; }
__host__ __device__ constexpr int episode_grid(int worlds, int A) {
    return (worlds + episode_worlds_per_group(A) - 1) / episode_worlds_per_group(A);
}

// (A template, as the other kernels added after the first stages are: emitted where launch_episode names it.)
template <int kThreads = kEpiThreads>
__global__ __launch_bounds__(kThreads) void k_episode(EpisodeArgs a) {
    constexpr int kWaves = kThreads / 64;
    __shared__ int32_t flags[kThreads];                   // bit 0: the row ended, bit 1: it restarted
    __shared__ double waveSum[kWaves][kEpiStats];
    const int tid = threadIdx.x;
    const int perGroup = kThreads / a.A;
    const int w0 = blockIdx.x * perGroup;
    const int nw = a.worlds - w0 < perGroup ? a.worlds - w0 : perGroup;
    double s[kEpiStats];
#pragma unroll
    for (int q = 0; q < kEpiStats; ++q) s[q] = 0.0;
    int f = 0;
    if (tid < nw * a.A) {
        const size_t row = (size_t)w0 * (size_t)a.A + (size_t)tid;
        const int32_t phase = a.phase[row], done = a.done[row];
        const float m = a.selfMask[row];
        const bool was = phase == kEpiTracked;
        float ret = a.ret[row], disc = a.disc[row], gpow = a.gpow[row];
        int32_t len = a.len[row];
        const int32_t type = a.type[row];
        const float rw = a.reward[row];
        const float R = was ? rw : 0.f;                   // a select: what an untracked row carries reaches nothing
        if (was) { ret = ret + R; disc = disc + gpow * R; gpow = gpow * a.gamma; len = len + 1; }
        const bool ended = was && done != 0;
        if (ended) {
            const double dr = (double)ret;
            const int o = type != 0 ? kEpiSide : 0;       // hiders after seekers
#pragma unroll
            for (int side = 0; side < 2; ++side)          // (no register array is indexed dynamically)
                if (o == side * kEpiSide) {
                    s[side * kEpiSide + 0] = 1.0; s[side * kEpiSide + 1] = dr; s[side * kEpiSide + 2] = dr * dr;
                    s[side * kEpiSide + 3] = (double)disc; s[side * kEpiSide + 4] = (double)len;
                }
        }
        const bool restart = done != 0 || (phase != kEpiWaiting && (!was || m == 0.f));
        if (restart) {
            a.ret[row] = 0.f; a.disc[row] = 0.f; a.gpow[row] = 1.f; a.len[row] = 0;
            a.type[row] = a.selfType[row]; a.phase[row] = m != 0.f ? kEpiTracked : kEpiOut;
        } else if (was) {
            a.ret[row] = ret; a.disc[row] = disc; a.gpow[row] = gpow; a.len[row] = len;
        }
        f = (ended ? 1 : 0) | (restart ? 2 : 0);
    }
    flags[tid] = f;
    const int any = __syncthreads_or(f & 1);              // (the barrier flags[] needs as well)
    if (tid < nw) {                                       // lane tid: world w0 + tid, whose rows are lanes tid A .. tid A + A - 1
        const int w = w0 + tid;
        int e = 0;
        for (int k = 0; k < a.A; ++k) e |= flags[tid * a.A + k];
        if (e) {
            if (e & 1) {
                const int32_t h = a.worldTeam[w];
                s[kEpiWorldEpisodes] = 1.0;
                if (a.worldPhase[w] == 1 && (h == 0 || h == 1)) {
                    const float x = a.episodeResult[(size_t)w * 2 + h];
                    s[kEpiHiderWins] = x == 1.f ? 1.0 : 0.0; s[kEpiSeekerWins] = x == 0.f ? 1.0 : 0.0; s[kEpiDraws] = x == 0.5f ? 1.0 : 0.0;
                }
            }
            a.worldTeam[w] = a.hiderTeam ? a.hiderTeam[w] : (cnt_seekers_first(a.counts[w]) ? 1 : 0);
            a.worldPhase[w] = 1;
        }
    }
    double *out = a.partials + (size_t)blockIdx.x * kEpiStats;
    if (!any) {                                           // no episode ended here: every term is +0.0
        if (tid < kEpiStats) out[tid] = 0.0;
        return;
    }
#pragma unroll
    for (int q = 0; q < kEpiStats; ++q) {
        double v = s[q];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d, 64);
        s[q] = v;
    }
    if (tid % 64 == 0) {
#pragma unroll
        for (int q = 0; q < kEpiStats; ++q) waveSum[tid / 64][q] = s[q];
    }
    __syncthreads();
    if (tid < kEpiStats) {
        double t = waveSum[0][tid];
        for (int k = 1; k < kWaves; ++k) t = t + waveSum[k][tid];
        out[tid] = t;
    }
}

// table[c] = table[c] + (the sum of partials[0 .. nparts)[c] in k_partials_sum's order), c < kEpiStats: one workgroup.
template <int kSegs = kEpiSumSegs>
__global__ __launch_bounds__(kEpiStats * kSegs) void k_episode_fold(const double *__restrict__ partials, int nparts, double *__restrict__ table) {
    __shared__ double seg[kSegs][kEpiStats];
    const int c = threadIdx.x % kEpiStats, sg = threadIdx.x / kEpiStats;
    const int per = (nparts + kSegs - 1) / kSegs;
    const int b0 = sg * per, b1 = b0 + per < nparts ? b0 + per : nparts;
    double s = 0;
    for (int b = b0; b < b1; ++b) s = s + partials[(size_t)b * kEpiStats + c];
    seg[sg][c] = s;
    __syncthreads();
    if (sg == 0) {
        double t = seg[0][c];
        for (int k = 1; k < kSegs; ++k) t = t + seg[k][c];
        table[c] = table[c] + t;
    }
}

}  // namespace hs
