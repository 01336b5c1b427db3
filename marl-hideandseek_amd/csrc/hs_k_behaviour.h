// Behaviour statistics (hs_behaviour_stats): after a step, one lane per world advances the world's tracker (where its
// boxes and ramps stood at the episode's start, at the end of the preparation phase and now, who had locked them, how
// far each side has travelled, how often it grabbed) and every episode that ended with the step is folded into a table
// of f64 sums.  include/hideseek.h states the arithmetic, IEEE f32 without contraction in a fixed order, and which
// observation belongs to which episode.
//
// One lane per world: a world's state and inputs are its own, so nothing crosses lanes but the sums, and the ordered
// travel sum of a side is a loop of one lane.  A lane walks its world's 136 bytes of positions (and as many of
// last_pos) at a 136-byte stride; the 17 loads of a wave fall into the same 69 cache lines, so the lines come once from
// L2 and the rest from the vector L1.  A workgroup is one wave of 64 worlds: 16 000 worlds are 250 workgroups, about one
// per CU, and the kernel has no barrier and no LDS (DESIGN §8 has the measurement against a plain copy).
// Locks: with no array given the lane reads the 11 body metadata words of its world's slot (hs_state.h Col: 8 worlds of a
// row are adjacent), which is what the observation stage exports as the lock columns of box_data / ramp_data, once per
// world instead of once per agent row and without a search for the world's first active row.
// Sums: a lane holds the kBehStats terms of its world; the wave adds them by the xor butterfly 1, 2, 4, ... (float
// addition commutes: every lane ends with the same bits), and k_behaviour_fold adds the workgroups' partials as
// k_partials_sum (hs_rows.h) does, kSegs runs of slices in ascending order, then the runs in ascending order, and adds
// that sum to the table once.  No atomics, and an order that depends on the number of worlds alone.  Episodes end every
// 240 steps: a workgroup with nothing to book writes +0.0 partials (what the sums would have given) without the butterfly.
#pragma once
#include "hs_state.h"

namespace hs {

constexpr int kBehThreads = 64, kBehStats = 27, kBehKind = 9, kBehSide = 3;
constexpr int kBehWorldEpisodes = 0, kBehReachedMain = 1, kBehBad = 2, kBehBoxes = 3, kBehRamps = 12, kBehSeekers = 21, kBehHiders = 24;
constexpr int kBehUnarmed = 0, kBehPrep = 1, kBehMain = 2, kBehWaiting = 3;
constexpr int kBehObjects = kMaxBoxes + kMaxRamps;      // 11 entries of positions and locks, the boxes first
constexpr int kBehSumSegs = 32;           // k_behaviour_fold: segments of the partials summed side by side

struct BehaviourArgs {
    const float *positions;
    const int32_t *locks;                 // or null: from bmeta
    const int32_t *counts4;               // or null: from counts
    const int32_t *prep, *done, *selfType;
    const float *selfMask, *grabbing;
    int grabStride;
    float moveEps;
    const int *counts;                    // the handle's SimState::counts
    const int *slotOfWorld;
    Col<int, kNumDSlots> bmeta;
    int32_t *phase, *nObj, *nSide;
    float *startPos, *prepPos, *lastPos;
    int32_t *prepLocks, *lastLocks;
    float *travel;
    int32_t *grab, *agentSteps, *wasActive;
    double *partials;                     // [behaviour_grid][kBehStats]
    int worlds, A;
};

__host__ __device__ constexpr int behaviour_grid(int worlds) { return (worlds + kBehThreads - 1) / kBehThreads; }

// d(a, b) of the contract: every operation one f32 operation, the root correctly rounded
HSD float beh_dist(float ax, float ay, float bx, float by) {
    const float dx = ax - bx, dy = ay - by;
    const float xx = dx * dx, yy = dy * dy;
    return sqrtf(xx + yy);
}
HSD int beh_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The lock of object entry j (boxes 0-8, ramps 9-10) of world w as the lock columns export it; nb, nr: the world's counts.
HSD int32_t beh_lock(const BehaviourArgs &a, int w, int slot, int j, int nb, int nr) {
    if (a.locks) return a.locks[(size_t)w * kBehObjects + j];
    const bool present = j < kMaxBoxes ? j < nb : j - kMaxBoxes < nr;
    const int m = a.bmeta(j < kMaxBoxes ? kBoxSlot0 + j : kRampSlot0 + (j - kMaxBoxes), slot);
    if (!present || meta_resp(m) != RESP_STATIC) return 0;
    return meta_owner(m) == OWNER_HIDER ? 1 : 2;
}

// (A template, as the other kernels added after the first stages are: emitted where launch_behaviour names it.)
template <int kThreads = kBehThreads>
__global__ __launch_bounds__(kThreads) void k_behaviour(BehaviourArgs a) {
    static_assert(kThreads == 64, "a workgroup is one wave: the butterfly is the whole reduction");
    const int tid = threadIdx.x;
    const int w = blockIdx.x * kThreads + tid;
    double s[kBehStats];
#pragma unroll
    for (int q = 0; q < kBehStats; ++q) s[q] = 0.0;
    bool books = false;
    if (w < a.worlds) {
        const size_t row0 = (size_t)w * (size_t)a.A;
        // steps 1, 5 and 6 over the world's rows
        bool ended = false, restarted = false;
        int first = -1, stepsS = 0, stepsH = 0, grabS = 0, grabH = 0;
        for (int k = 0; k < a.A; ++k) {
            const size_t row = row0 + (size_t)k;
            const bool act = a.selfMask[row] != 0.f, was = a.wasActive[row] != 0, dn = a.done[row] != 0;
            ended = ended || (dn && was);
            restarted = restarted || (act && !was && !dn);
            if (act) {
                if (first < 0) first = k;
                const bool hider = a.selfType[row] != 0;
                const int g = a.grabbing[row * (size_t)a.grabStride] != 0.f ? 1 : 0;
                if (hider) { stepsH += 1; grabH += g; } else { stepsS += 1; grabS += g; }
            }
            a.wasActive[row] = act ? 1 : 0;
        }
        const int32_t phase = a.phase[w];
        const bool armed = phase == kBehPrep || phase == kBehMain;
        const float *pos = a.positions + (size_t)w * (2 * kNumDSlots);
        float *startPos = a.startPos + (size_t)w * (2 * kBehObjects), *prepPos = a.prepPos + (size_t)w * (2 * kBehObjects);
        float *lastPos = a.lastPos + (size_t)w * (2 * kNumDSlots);
        int32_t *prepLocks = a.prepLocks + (size_t)w * kBehObjects, *lastLocks = a.lastLocks + (size_t)w * kBehObjects;
        if (first < 0) { s[kBehBad] = 1.0; books = true; }
        // step 2: the episode that ended, from the state as the previous call left it
        if (ended && armed) {
            books = true;
            const bool main = phase == kBehMain;
            s[kBehWorldEpisodes] = 1.0; s[kBehReachedMain] = main ? 1.0 : 0.0;
#pragma unroll
            for (int kind = 0; kind < 2; ++kind) {        // (no register array is indexed dynamically)
                const int n = a.nObj[(size_t)w * 2 + kind], base = kind ? kMaxBoxes : 0, cap = kind ? kMaxRamps : kMaxBoxes;
                float maxPrep = 0.f, maxMain = 0.f;
                int movedPrep = 0, movedMain = 0, hidPrep = 0, seekPrep = 0, hidEnd = 0, seekEnd = 0, objects = 0;
                for (int j = 0; j < cap; ++j) {
                    if (j >= n) break;
                    const int e = base + j;
                    const float sx = startPos[2 * e], sy = startPos[2 * e + 1], px = prepPos[2 * e], py = prepPos[2 * e + 1];
                    const float lx = lastPos[2 * e], ly = lastPos[2 * e + 1];
                    const float movePrep = main ? beh_dist(px, py, sx, sy) : beh_dist(lx, ly, sx, sy);
                    const float moveMain = main ? beh_dist(lx, ly, px, py) : 0.f;
                    maxPrep = fmaxf(maxPrep, movePrep); maxMain = fmaxf(maxMain, moveMain);
                    movedPrep += movePrep > a.moveEps ? 1 : 0; movedMain += moveMain > a.moveEps ? 1 : 0;
                    const int32_t le = lastLocks[e], lp = main ? prepLocks[e] : le;
                    hidPrep += lp == 1 ? 1 : 0; seekPrep += lp == 2 ? 1 : 0; hidEnd += le == 1 ? 1 : 0; seekEnd += le == 2 ? 1 : 0;
                    objects += 1;
                }
                const int o = kind ? kBehRamps : kBehBoxes;
                s[o + 0] = (double)maxPrep; s[o + 1] = (double)maxMain; s[o + 2] = (double)movedPrep; s[o + 3] = (double)movedMain;
                s[o + 4] = (double)hidPrep; s[o + 5] = (double)seekPrep; s[o + 6] = (double)hidEnd; s[o + 7] = (double)seekEnd;
                s[o + 8] = (double)objects;
            }
            s[kBehSeekers + 0] = (double)a.travel[(size_t)w * 2]; s[kBehSeekers + 1] = (double)a.grab[(size_t)w * 2];
            s[kBehSeekers + 2] = (double)a.agentSteps[(size_t)w * 2];
            s[kBehHiders + 0] = (double)a.travel[(size_t)w * 2 + 1]; s[kBehHiders + 1] = (double)a.grab[(size_t)w * 2 + 1];
            s[kBehHiders + 2] = (double)a.agentSteps[(size_t)w * 2 + 1];
        }
        if (first >= 0) {
            const int32_t p = a.prep[row0 + (size_t)first];
            int nb, nr, nh, ns;
            if (a.counts4) {
                const int32_t *c = a.counts4 + (size_t)w * 4;
                nb = c[0]; nr = c[1]; nh = c[2]; ns = c[3];
            } else {
                const int c = a.counts[w];
                nb = cnt_boxes(c); nr = cnt_ramps(c); nh = cnt_hiders(c); ns = cnt_seekers(c);
            }
            nb = beh_clamp(nb, kMaxBoxes); nr = beh_clamp(nr, kMaxRamps); nh = beh_clamp(nh, kMaxAgents); ns = beh_clamp(ns, kMaxAgents - nh);
            const int slot = a.locks ? 0 : a.slotOfWorld[w];
            const bool start = ended || phase == kBehUnarmed || (phase != kBehWaiting && restarted);
            if (start) {                                  // step 3
                a.nObj[(size_t)w * 2] = nb; a.nObj[(size_t)w * 2 + 1] = nr;
                a.nSide[(size_t)w * 2] = ns; a.nSide[(size_t)w * 2 + 1] = nh;
                for (int e = 0; e < kNumDSlots; ++e) {
                    const float x = pos[2 * e], y = pos[2 * e + 1];
                    lastPos[2 * e] = x; lastPos[2 * e + 1] = y;
                    if (e < kBehObjects) { startPos[2 * e] = x; startPos[2 * e + 1] = y; prepPos[2 * e] = x; prepPos[2 * e + 1] = y; }
                }
                for (int j = 0; j < kBehObjects; ++j) {
                    const int32_t l = beh_lock(a, w, slot, j, nb, nr);
                    prepLocks[j] = l; lastLocks[j] = l;
                }
                a.travel[(size_t)w * 2] = 0.f; a.travel[(size_t)w * 2 + 1] = 0.f;
                a.grab[(size_t)w * 2] = grabS; a.grab[(size_t)w * 2 + 1] = grabH;
                a.agentSteps[(size_t)w * 2] = stepsS; a.agentSteps[(size_t)w * 2 + 1] = stepsH;
                a.phase[w] = p > 0 ? kBehPrep : kBehMain;
            } else if (armed) {                           // step 4
                const int lh = a.nSide[(size_t)w * 2 + 1], ls = a.nSide[(size_t)w * 2];
                float travelS = a.travel[(size_t)w * 2], travelH = a.travel[(size_t)w * 2 + 1];
                const bool release = phase == kBehPrep && p == 0;
                for (int e = 0; e < kNumDSlots; ++e) {
                    const float x = pos[2 * e], y = pos[2 * e + 1];
                    if (e >= kBehObjects) {
                        const int i = e - kBehObjects;
                        const float d = beh_dist(x, y, lastPos[2 * e], lastPos[2 * e + 1]);
                        if (i < lh) travelH = travelH + d;
                        else if (i - lh < ls) travelS = travelS + d;
                    } else if (release) {
                        prepPos[2 * e] = x; prepPos[2 * e + 1] = y;
                    }
                    lastPos[2 * e] = x; lastPos[2 * e + 1] = y;
                }
                for (int j = 0; j < kBehObjects; ++j) {
                    const int32_t l = beh_lock(a, w, slot, j, nb, nr);
                    lastLocks[j] = l;
                    if (release) prepLocks[j] = l;
                }
                a.travel[(size_t)w * 2] = travelS; a.travel[(size_t)w * 2 + 1] = travelH;
                a.grab[(size_t)w * 2] += grabS; a.grab[(size_t)w * 2 + 1] += grabH;
                a.agentSteps[(size_t)w * 2] += stepsS; a.agentSteps[(size_t)w * 2 + 1] += stepsH;
                if (release) a.phase[w] = kBehMain;
            }
        }
    }
    double *out = a.partials + (size_t)blockIdx.x * kBehStats;
    if (!__any(books ? 1 : 0)) {                          // nothing to book here: every term is +0.0
        if (tid < kBehStats) out[tid] = 0.0;
        return;
    }
#pragma unroll
    for (int q = 0; q < kBehStats; ++q) {
        double v = s[q];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d, 64);
        s[q] = v;
    }
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < kBehStats; ++q) out[q] = s[q];
    }
}

// table[c] = table[c] + (the sum of partials[0 .. nparts)[c] in k_partials_sum's order), c < kBehStats: one workgroup.
template <int kSegs = kBehSumSegs>
__global__ __launch_bounds__(kBehStats * kSegs) void k_behaviour_fold(const double *__restrict__ partials, int nparts, double *__restrict__ table) {
    __shared__ double seg[kSegs][kBehStats];
    const int c = threadIdx.x % kBehStats, sg = threadIdx.x / kBehStats;
    const int per = (nparts + kSegs - 1) / kSegs;
    const int b0 = sg * per, b1 = b0 + per < nparts ? b0 + per : nparts;
    double s = 0;
    for (int b = b0; b < b1; ++b) s = s + partials[(size_t)b * kBehStats + c];
    seg[sg][c] = s;
    __syncthreads();
    if (sg == 0) {
        double t = seg[0][c];
        for (int k = 1; k < kSegs; ++k) t = t + seg[k][c];
        table[c] = table[c] + t;
    }
}

}  // namespace hs
