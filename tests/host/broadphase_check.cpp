// Host check of marl-hideandseek_amd/csrc/hs_broadphase.h (tests/test_broadphase_host.py builds and runs it).
// It walks the data flow of phase_detect (hs_k_physics.h) for ONE world on the CPU, the eight lanes of the world as a
// loop, and compares the candidate masks with the plain loops over every wall and every ordered pair.
//   broadphase_check walls   100 000 random (body AABB, wall set) cases
//   broadphase_check pairs   the pair schedule for 13 .. 17 slots
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "hs_broadphase.h"

using namespace hs;

constexpr int kLanes = 8, kStaged = 32, kWallsMax = 36;
static std::mt19937_64 rng(20240917);
static double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
static int pick(int n) { return (int)(rng() % (unsigned long long)n); }

static float special() {
    static const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    static const float v[] = {0.f, -0.f, inf, -inf, nan, -20.f, -15.f, -10.f, -5.f, 5.f, 10.f, 15.f, 20.f,
                              -15.000001f, 14.999999f, 1e6f, -1e6f, 3e5f, -7e4f};
    return v[pick(sizeof(v) / sizeof(v[0]))];
}
static float coord() { return pick(8) == 0 ? special() : (float)uni(-22.0, 22.0); }

struct Walls { int n; float cx[kWallsMax], cy[kWallsMax], hx[kWallsMax], hy[kWallsMax]; };
struct Box { float lox, hix, loy, hiy; bool zin; };

// the strip masks as wall_strip_masks builds them: lane l packs walls l, l + 8, l + 16, l + 24, then the lanes exchange
static void build_masks(const Walls &w, unsigned xm[kLanes], unsigned ym[kLanes]) {
    unsigned wx[kLanes], wy[kLanes];
    for (int l = 0; l < kLanes; ++l) {
        wx[l] = wy[l] = 0u;
        for (int r = 0; r < 4; ++r) {
            const int k = l + r * kLanes;
            if (k >= w.n) continue;
            const unsigned b = wall_strips(w.cx[k], w.cy[k], w.hx[k], w.hy[k]);
            wx[l] |= (b & 0xffu) << (8 * r);
            wy[l] |= (b >> 8) << (8 * r);
        }
    }
    for (int l = 0; l < kLanes; ++l) {
        xm[l] = ym[l] = 0u;
        for (int j = 0; j < kLanes; ++j) { xm[l] |= strip_mask_part(wx[j], l, j); ym[l] |= strip_mask_part(wy[j], l, j); }
    }
}
// the definition of the masks: bit k of xm[s] <=> strip s lies between the strips of wall k's two x ends
static bool masks_match_definition(const Walls &w, const unsigned xm[kLanes], const unsigned ym[kLanes]) {
    for (int s = 0; s < kLanes; ++s)
        for (int k = 0; k < kStaged; ++k) {
            bool inx = false, iny = false;
            if (k < w.n) {
                const WallBox b = wall_box(w.cx[k], w.cy[k], w.hx[k], w.hy[k]);
                const int a0 = strip_of(b.x0), a1 = strip_of(b.x1), c0 = strip_of(b.y0), c1 = strip_of(b.y1);
                inx = (a0 <= s && s <= a1) || (a1 <= s && s <= a0);
                iny = (c0 <= s && s <= c1) || (c1 <= s && s <= c0);
            }
            if (((xm[s] >> k) & 1u) != (unsigned)inx || ((ym[s] >> k) & 1u) != (unsigned)iny) return false;
        }
    return true;
}
static unsigned long long masked(const Walls &w, const unsigned xm[kLanes], const unsigned ym[kLanes], const Box &b, int *tested) {
    const unsigned sx = extent_strips(b.lox, b.hix), sy = extent_strips(b.loy, b.hiy);
    unsigned ax = 0u, ay = 0u;
    for (int s = 0; s < kStrips; ++s) { ax |= (sx >> s & 1u) ? xm[s] : 0u; ay |= (sy >> s & 1u) ? ym[s] : 0u; }
    unsigned cand = b.zin ? ax & ay : 0u;
    unsigned long long out = 0ull;
    while (cand) {
        const int k = __builtin_ctz(cand); cand &= cand - 1u;
        ++*tested;
        if (wall_hit(b.zin, b.lox, b.hix, b.loy, b.hiy, wall_box(w.cx[k], w.cy[k], w.hx[k], w.hy[k]))) out |= 1ull << k;
    }
    for (int k = kStaged; k < w.n; ++k)
        if (wall_hit(b.zin, b.lox, b.hix, b.loy, b.hiy, wall_box(w.cx[k], w.cy[k], w.hx[k], w.hy[k]))) out |= 1ull << k;
    return out;
}
static unsigned long long plain(const Walls &w, const Box &b) {
    unsigned long long out = 0ull;
    for (int k = 0; k < w.n; ++k)
        if (wall_hit(b.zin, b.lox, b.hix, b.loy, b.hiy, wall_box(w.cx[k], w.cy[k], w.hx[k], w.hy[k]))) out |= 1ull << k;
    return out;
}

static Walls random_walls(int n) {
    Walls w; std::memset(&w, 0, sizeof(w)); w.n = n;
    for (int k = 0; k < n; ++k) {
        const int kind = pick(16);
        if (kind == 0) {                              // anything at all, special values and negative half-extents included
            w.cx[k] = coord(); w.cy[k] = coord(); w.hx[k] = pick(2) ? special() : (float)uni(-3.0, 20.0); w.hy[k] = pick(2) ? special() : (float)uni(-3.0, 20.0);
        } else {                                      // a wall of a level: long and thin along x or y
            const float len = (float)uni(0.5, 20.0), thin = 0.25f;
            const bool alongX = pick(2) != 0;
            w.cx[k] = pick(6) == 0 ? special() : (float)(5.0 * pick(9) - 20.0 + (pick(2) ? 0.0 : uni(-2.5, 2.5)));
            w.cy[k] = pick(6) == 0 ? special() : (float)(5.0 * pick(9) - 20.0 + (pick(2) ? 0.0 : uni(-2.5, 2.5)));
            w.hx[k] = alongX ? len : thin; w.hy[k] = alongX ? thin : len;
        }
    }
    return w;
}
static Box random_box() {
    Box b; b.zin = pick(8) != 0;
    switch (pick(8)) {
    case 0: {                                         // wholly outside the outermost boundaries
        const float sgn = pick(2) ? 1.f : -1.f, x = sgn * (float)uni(20.0, 1e6), y = pick(2) ? (float)uni(-22.0, 22.0) : sgn * (float)uni(20.0, 1e6);
        b.lox = x - 1.f; b.hix = x + 1.f; b.loy = y - 1.f; b.hiy = y + 1.f; break;
    }
    case 1: b.lox = b.loy = (float)uni(-1e6, -20.0); b.hix = b.hiy = (float)uni(20.0, 1e6); break;      // spans every strip
    case 2: b.lox = b.hix = coord(); b.loy = b.hiy = coord(); break;                                   // degenerate
    case 3: b.lox = coord(); b.hix = coord(); b.loy = coord(); b.hiy = coord(); break;                   // anything, inverted included
    case 4: {                                         // centred exactly on a strip boundary
        const float x = 5.f * (float)(pick(7) - 3), y = 5.f * (float)(pick(7) - 3), h = (float)uni(0.0, 1.0);
        b.lox = x - h; b.hix = x + h; b.loy = y - h; b.hiy = y + h; break;
    }
    default: {                                        // a body of a level
        const float x = (float)uni(-21.0, 21.0), y = (float)uni(-21.0, 21.0), hx = (float)uni(0.2, 6.0), hy = (float)uni(0.2, 6.0);
        b.lox = x - hx; b.hix = x + hx; b.loy = y - hy; b.hiy = y + hy;
    }
    }
    return b;
}

static int check_walls() {
    static const int counts[] = {4, 32, 33, 36, 30, 17};
    long long cases = 0, hits = 0, tests = 0, allTests = 0, tailHits = 0;
    for (int set = 0; set < 12500; ++set) {
        const Walls w = random_walls(counts[set % 6]);
        unsigned xm[kLanes], ym[kLanes];
        build_masks(w, xm, ym);
        if (!masks_match_definition(w, xm, ym)) { std::printf("FAIL: strip masks of wall set %d\n", set); return 1; }
        for (int i = 0; i < 8; ++i, ++cases) {
            const Box b = random_box();
            int tested = 0;
            const unsigned long long a = masked(w, xm, ym, b, &tested), e = plain(w, b);
            if (a != e) {
                std::printf("FAIL: set %d (%d walls) box [%g, %g] x [%g, %g] zin %d: %016llx, exact %016llx\n", set, w.n,
                            b.lox, b.hix, b.loy, b.hiy, (int)b.zin, a, e);
                return 1;
            }
            hits += __builtin_popcountll(e); tailHits += __builtin_popcountll(e >> kStaged);
            tests += tested; allTests += w.n < kStaged ? w.n : kStaged;
        }
    }
    std::printf("walls OK: %lld cases, %lld hits (%lld on walls beyond the staged ones), %lld exact tests on staged walls instead of %lld\n",
                cases, hits, tailHits, tests, allTests);
    // not vacuous, and the strips do select
    return cases >= 100000 && hits > cases / 2 && tailHits > 100 && tests < allTests / 2 ? 0 : 1;
}

static int check_pairs() {
    long long hitsAll = 0, wrapped = 0;
    for (int ns = 13; ns <= 17; ++ns) {
        int seen[kNumDSlots][kNumDSlots] = {};
        for (int s = 0; s < ns; ++s) {
            int j = s;
            for (int d = 1; d <= pair_steps(ns); ++d) {
                j = pair_next(j, ns);
                if (j != (s + d) % ns) { std::printf("FAIL: partner of %d at distance %d of %d\n", s, d, ns); return 1; }
                if (pair_mine(s, d, ns)) ++seen[s < j ? s : j][s < j ? j : s];
            }
        }
        for (int a = 0; a < ns; ++a)
            for (int b = 0; b < ns; ++b)
                if (seen[a][b] != (a < b ? 1 : 0)) { std::printf("FAIL: pair (%d, %d) of %d slots visited %d times\n", a, b, ns, seen[a][b]); return 1; }
        for (int trial = 0; trial < 4000; ++trial) {
            bool have[kNumDSlots], dyn[kNumDSlots]; V3 lo[kNumDSlots], hi[kNumDSlots];
            const float spread = trial % 2 ? 3.f : 8.f;
            for (int s = 0; s < ns; ++s) {
                have[s] = pick(5) != 0; dyn[s] = have[s] && pick(3) != 0;
                const V3 c = {(float)uni(-spread, spread), (float)uni(-spread, spread), (float)uni(0.0, 2.0)};
                const V3 h = {(float)uni(0.0, 2.0), (float)uni(0.0, 2.0), (float)uni(0.0, 1.0)};
                lo[s] = c - h; hi[s] = c + h;
                if (pick(40) == 0) lo[s].x = special();
                if (pick(40) == 0) hi[s].y = special();
            }
            auto hit = [&](int a, int b) { return have[b] & have[a] & (dyn[a] | dyn[b]) & aabb_hit(lo[a], hi[a], lo[b], hi[b]); };
            unsigned expect[kNumDSlots] = {}, got[kNumDSlots] = {}, xch[kNumDSlots] = {}, hm[kNumDSlots] = {};
            for (int a = 0; a < ns; ++a)
                for (int b = a + 1; b < ns; ++b) if (hit(a, b)) expect[a] |= 1u << b;        // the double loop
            for (int s = 0; s < ns; ++s) {                                                    // the schedule, slot by slot
                int j = s;
                for (int d = 1; d <= pair_steps(ns); ++d) {
                    j = pair_next(j, ns);
                    if (pair_mine(s, d, ns) && hit(s, j)) hm[s] |= 1u << j;
                }
                for (unsigned below = hm[s] & ((1u << s) - 1u); below; below &= below - 1u) { xch[__builtin_ctz(below)] |= 1u << s; ++wrapped; }
            }
            for (int s = 0; s < ns; ++s) {
                got[s] = (hm[s] & ~((2u << s) - 1u)) | xch[s];
                if (got[s] != expect[s]) { std::printf("FAIL: %d slots, trial %d, slot %d: %05x, double loop %05x\n", ns, trial, s, got[s], expect[s]); return 1; }
                hitsAll += __builtin_popcount(expect[s]);
            }
        }
    }
    std::printf("pairs OK: 13 .. 17 slots, every pair once; %lld hits, %lld of them handed to the lower slot\n", hitsAll, wrapped);
    return hitsAll > 10000 && wrapped > 1000 ? 0 : 1;
}

int main(int argc, char **argv) {
    const bool walls = argc < 2 || !std::strcmp(argv[1], "walls"), pairs = argc < 2 || !std::strcmp(argv[1], "pairs");
    if (walls && check_walls()) return 1;
    if (pairs && check_pairs()) return 1;
    return 0;
}
