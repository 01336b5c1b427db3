// The league (hs_league_step): P policies play each other on one simulator.  After a step, one lane per agent row (row =
// world * A + slot) routes the row to the policy of its side under the fixed schedule of include/hideseek.h (world w plays
// pair q = w mod P^2: policy q / P the hiders, policy q % P the seekers) and ranks it in the stable sort of all rows by
// (policy, row) by the closed form stated there: no scan across worlds and no sort.  The lane of a world's first row books
// the game that ended with the step under the hider team latched at its start, and latches the next.
// hs_league_step_scheduled is the same kernel body with the schedule read from a table of the handle (LeagueTable below):
// the two differ only in how a world finds its pair and the sides held before it.
//
// The shape is k_episode's: a workgroup takes whole worlds, kLeagueThreads / A of them, its rows are contiguous (a wave's
// access to an input is one 256-byte range), and what a world needs of its rows (how many are hiders, is one masked, the
// sides of the rows before a row) crosses lanes through LDS and one barrier.  The last lanes of a workgroup
// (kLeagueThreads % A, and those past the last world) hold no row.
// Counts: integers, so the order of addition cannot show.  A workgroup keeps a histogram of its finished games (and of its
// malformed worlds, the bin after the last outcome) in LDS and adds every nonzero bin to the handle's step table with one
// integer atomic; games end every 240 steps, and a workgroup in which nothing was booked adds nothing.  k_league_fold, one
// workgroup, adds the step table to the caller's counts, rates the step's games in f64 against the ratings as they stood
// (one lane per ordered pair, then one lane per policy that adds the pairs' terms in ascending (i, j): the additions a
// policy's rating sees are those of the serial loop, in its order), writes `bad`, and leaves the step table zero for the
// next call.
#pragma once
#include "hs_state.h"

namespace hs {

constexpr int kLeagueThreads = 256, kLeagueMaxPolicies = 16, kLeagueOutcomes = 4;
constexpr int kLeagueMaxGroup = kLeagueMaxPolicies * kLeagueMaxPolicies;                      // the pairs of a schedule table
constexpr int kLeagueMaxBins = kLeagueMaxPolicies * kLeagueMaxPolicies * kLeagueOutcomes;     // + 1: the malformed worlds
constexpr int kLeagueHidersWin = 0, kLeagueSeekersWin = 1, kLeagueDraw = 2, kLeagueNoOutcome = 3;

struct LeagueArgs {
    const int32_t *done, *selfType;
    const float *selfMask, *episodeResult;
    const int32_t *hiderTeam;             // or null: from counts
    const int *counts;                    // the handle's SimState::counts (cnt_seekers_first)
    int32_t *policy, *slot, *rowOfSlot, *clearSlot;       // slot, rowOfSlot and clearSlot may be null
    int32_t *worldTeam, *worldPhase;
    int32_t *step;                        // the handle's step table, [P * P * 4 + 1], zero between calls
    int worlds, A, P, k;
};

__host__ __device__ constexpr int league_worlds_per_group(int A) { return kLeagueThreads / A; }
__host__ __device__ constexpr int league_grid(int worlds, int A) {
    return (worlds + league_worlds_per_group(A) - 1) / league_worlds_per_group(A);
}

// How a world finds its game.  Both forms answer the same questions for world w's pair q = w mod group(): the two
// policies, the sides a policy holds in the pairs of the group before q, and the game's cell of the N x N table; a group
// gives every policy sides() sides, and a policy owns block() slots in all.
// The fixed schedule of hs_league_step, in closed form: pair q is (q / P, q % P).
struct LeagueAllPairs {
    int P;
    struct Game {
        int q, i, j, P;
        // as hiders in the pairs p P .. p P + P - 1, as seekers in every P-th
        __device__ int held(int p, bool) const {
            const int asHiders = q - p * P < 0 ? 0 : q - p * P > P ? P : q - p * P;
            const int asSeekers = i + (j > p ? 1 : 0);
            return asHiders + asSeekers;
        }
        __device__ int cell() const { return q; }
    };
    __device__ int group() const { return P * P; }
    __device__ int sides() const { return 2 * P; }
    __device__ int block(int worlds, int A) const { return worlds / P * A; }      // R / P: worlds is a multiple of P^2
    __device__ Game game(int q) const { const int i = q / P; return {q, i, q - i * P, P}; }
};
// A table (hs_league_set_schedule): entry q is (hider policy, seeker policy, the sides each holds in the pairs before q),
// 16 bytes, so the lanes of a world read one broadcast int4.  Indexed per world: a workgroup's worlds span groups.
struct LeagueTable {
    const int4 *pairs;
    int G, c, N;
    struct Game {
        int i, j, heldI, heldJ, N;
        __device__ int held(int, bool hider) const { return hider ? heldI : heldJ; }
        __device__ int cell() const { return i * N + j; }
    };
    __device__ int group() const { return G; }
    __device__ int sides() const { return c; }
    __device__ int block(int worlds, int A) const { return worlds / G * c * (A / 2); }    // R / N: worlds is a multiple of G
    __device__ Game game(int q) const { const int4 e = pairs[q]; return {e.x, e.y, e.z, e.w, N}; }
};

template <int kThreads, typename Schedule>
__device__ __forceinline__ void league_rows(const LeagueArgs &a, const Schedule sched) {
    __shared__ int32_t flags[kThreads];                   // bit 0: the row's self_type is nonzero, bit 1: its self_mask is 0
    __shared__ int32_t hist[kLeagueMaxBins + 1];
    const int tid = threadIdx.x;
    const int A = a.A, P = a.P, k = a.k, PP = P * P, bins = PP * kLeagueOutcomes;
    const int perGroup = kThreads / A;
    const int w0 = blockIdx.x * perGroup;
    const int nw = a.worlds - w0 < perGroup ? a.worlds - w0 : perGroup;
    const bool live = tid < nw * A;
    for (int b = tid; b <= bins; b += kThreads) hist[b] = 0;
    const size_t row = (size_t)w0 * (size_t)A + (size_t)tid;
    int32_t done = 0;
    int f = 0;
    if (live) {
        done = a.done[row];
        f = (a.selfType[row] != 0 ? 1 : 0) | (a.selfMask[row] == 0.f ? 2 : 0);
    }
    flags[tid] = f;
    __syncthreads();
    int booked = 0;
    if (live) {
        const int lw = tid / A, r = tid - lw * A;         // the world within the workgroup, the row within the world
        const int w = w0 + lw;
        int hiders = 0, masked = 0, hidersBefore = 0;
        for (int b = 0; b < A; ++b) {
            const int fb = flags[lw * A + b];
            hiders += fb & 1; masked |= fb & 2;
            hidersBefore += b < r ? fb & 1 : 0;
        }
        const bool malformed = hiders != k || masked != 0;
        const bool hider = malformed ? r < k : (f & 1) != 0;
        if (malformed) hidersBefore = r < k ? r : k;
        const int group = sched.group();
        const int g = w / group, q = w - g * group;
        const auto game = sched.game(q);
        const int i = game.i, j = game.j;                 // the hiders' policy, the seekers'
        const int p = hider ? i : j;
        const int held = game.held(p, hider);             // the sides p holds in the worlds before q of the group
        const int rank = i == j ? r : hider ? hidersBefore : r - hidersBefore;
        const int s = p * sched.block(a.worlds, A) + g * (sched.sides() * k) + k * held + rank;
        a.policy[row] = p;
        if (a.slot) a.slot[row] = s;
        if (a.rowOfSlot) a.rowOfSlot[s] = (int32_t)row;
        if (a.clearSlot) a.clearSlot[s] = done;
        if (r == 0) {                                     // the world: its rows carry one done
            const int32_t phase = a.worldPhase[w];
            if (malformed) { atomicAdd(&hist[bins], 1); booked = 1; }
            if (done != 0 && phase == 1) {
                const int32_t h = a.worldTeam[w];
                int o = kLeagueNoOutcome;
                if (h == 0 || h == 1) {
                    const float x = a.episodeResult[(size_t)w * 2 + h];
                    o = x == 1.f ? kLeagueHidersWin : x == 0.f ? kLeagueSeekersWin : x == 0.5f ? kLeagueDraw : kLeagueNoOutcome;
                }
                atomicAdd(&hist[game.cell() * kLeagueOutcomes + o], 1);
                booked = 1;
            }
            if (done != 0 || phase == 0) {
                a.worldTeam[w] = a.hiderTeam ? a.hiderTeam[w] : (cnt_seekers_first(a.counts[w]) ? 1 : 0);
                a.worldPhase[w] = 1;
            }
        }
    }
    if (!__syncthreads_or(booked)) return;                // (the barrier hist[] needs as well)
    for (int b = tid; b <= bins; b += kThreads) {
        const int32_t v = hist[b];
        if (v != 0) atomicAdd(&a.step[b], v);
    }
}

template <int kThreads = kLeagueThreads>
__global__ __launch_bounds__(kThreads) void k_league(LeagueArgs a) {
    league_rows<kThreads>(a, LeagueAllPairs{a.P});
}

// hs_league_step_scheduled: `a.P` is the table's N.
template <int kThreads = kLeagueThreads>
__global__ __launch_bounds__(kThreads) void k_league_scheduled(LeagueArgs a, const int4 *__restrict__ pairs, int G, int c) {
    league_rows<kThreads>(a, LeagueTable{pairs, G, c, a.P});
}

// counts += the step table; elo moved by the step's games, all rated against elo as it stood; *bad = the step's malformed
// worlds; the step table zeroed.  One workgroup of kLeagueMaxPolicies^2 lanes.
template <int kThreads = kLeagueMaxPolicies * kLeagueMaxPolicies>
__global__ __launch_bounds__(kThreads) void k_league_fold(int32_t *__restrict__ step, int P, double kFactor, long long *__restrict__ counts,
                                                          double *__restrict__ elo, int32_t *__restrict__ bad) {
    __shared__ double term[kThreads];                     // [i * P + j]: what the pair moves, +0.0 where it rated no game
    const int tid = threadIdx.x, PP = P * P;
    double d = 0.0;
    if (tid < PP) {
        const int i = tid / P, j = tid - i * P;
        int32_t D[kLeagueOutcomes];
#pragma unroll
        for (int o = 0; o < kLeagueOutcomes; ++o) {
            D[o] = step[tid * kLeagueOutcomes + o];
            if (D[o] != 0) { counts[tid * kLeagueOutcomes + o] += D[o]; step[tid * kLeagueOutcomes + o] = 0; }
        }
        const int32_t n = D[kLeagueHidersWin] + D[kLeagueSeekersWin] + D[kLeagueDraw];
        if (i != j && n != 0) {
            const double S = (double)D[kLeagueHidersWin] + 0.5 * (double)D[kLeagueDraw];
            const double E = 1.0 / (1.0 + pow(10.0, (elo[j] - elo[i]) / 400.0));
            d = kFactor * (S - (double)n * E);
        }
    }
    term[tid] = d;
    if (tid == 0) {
        const int32_t b = step[PP * kLeagueOutcomes];
        if (bad) *bad = b;
        if (b != 0) step[PP * kLeagueOutcomes] = 0;
    }
    const int any = __syncthreads_or(d != 0.0);           // every read of elo is before this barrier, every write after it
    if (!any || tid >= P) return;
    double e = elo[tid];
    for (int i = 0; i < P; ++i) {
        if (i == tid) {
            for (int j = 0; j < P; ++j)
                if (j != tid) e = e + term[tid * P + j];
        } else {
            e = e - term[i * P + tid];
        }
    }
    elo[tid] = e;
}

}  // namespace hs
