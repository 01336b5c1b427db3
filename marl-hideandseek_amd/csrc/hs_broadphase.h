// The pure parts of the k_physics broadphase (hs_k_physics.h phase_detect): the exact AABB predicates, the strips
// that pre-select a body's walls, and the schedule that visits each pair of body slots once.  Plain scalar functions
// like hs_core.h, so that a host program can compile them too (tests/host/broadphase_check.cpp).
//
// Walls.  The arena is cut into kStrips strips in x and again in y (strip_of).  Once per step a world's walls are
// turned into 2 x kStrips masks: bit k of xmask[s] says that wall k's x extent touches strip s.  A body then tests
// only the walls in (OR of xmask over its x strips) & (OR of ymask over its y strips), with the exact predicate
// (wall_hit).  That set holds every wall the exact predicate accepts: wall_hit needs lo.x <= wx1 and wx0 <= hi.x,
// strip_of is monotone, so strip_of(lo.x) <= strip_of(wx1) and strip_of(wx0) <= strip_of(hi.x) and the two strip
// ranges intersect (strip_range spans min..max of its ends, so this holds for inverted extents as well); the same in y.
// A NaN fails wall_hit whatever the strips say.  The masks therefore change which walls are tested, never the result.
#pragma once
#include "hs_core.h"

namespace hs {

constexpr int kStrips = 8;

// Strip of a coordinate: 5 m wide, boundaries at -15, -10, ... 15 (the arena's walls lie within +-20); everything
// beyond goes to the end strips.  Monotone non-decreasing in v: a product and a sum with constants, two clamps and
// a truncation are each monotone.  (NaN: fmax drops it, strip 0.)
HSD int strip_of(float v) {
    const float t = v * 0.2f + 4.f;
    return (int)__builtin_fminf(__builtin_fmaxf(t, 0.f), (float)(kStrips - 1));
}
// bits min(a, b) .. max(a, b)
HSD unsigned strip_range(int a, int b) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return (2u << hi) - (1u << lo);
}
HSD unsigned extent_strips(float v0, float v1) { return strip_range(strip_of(v0), strip_of(v1)); }

// The exact test of a body's AABB against a wall (cx, cy, hx, hy); `zin`: the body is dynamic and overlaps the walls' z range.
struct WallBox { float x0, x1, y0, y1; };
HSD WallBox wall_box(float cx, float cy, float hx, float hy) { return {cx - hx, cx + hx, cy - hy, cy + hy}; }
HSD bool wall_hit(bool zin, float lox, float hix, float loy, float hiy, WallBox w) {
    return zin & (lox <= w.x1) & (w.x0 <= hix) & (loy <= w.y1) & (w.y0 <= hiy);
}
// x strips of a wall in bits 0-7, y strips in bits 8-15
HSD unsigned wall_strips(float cx, float cy, float hx, float hy) {
    const WallBox w = wall_box(cx, cy, hx, hy);
    return extent_strips(w.x0, w.x1) | (extent_strips(w.y0, w.y1) << 8);
}
// Transposing strips-per-wall into walls-per-strip inside a world's 8 lanes: lane j holds, one byte each, the strips of
// walls j, j + 8, j + 16, j + 24 (word `w`); the lane of strip `s` takes its bit of every byte to the walls' places.
HSD unsigned strip_mask_part(unsigned w, int s, int j) { return ((w >> s) & 0x01010101u) << j; }

// The exact test of two bodies' AABBs; symmetric in the two bodies.
HSD bool aabb_hit(V3 loa, V3 hia, V3 lob, V3 hib) {
    return (loa.x <= hib.x) & (lob.x <= hia.x) & (loa.y <= hib.y) & (lob.y <= hia.y) & (loa.z <= hib.z) & (lob.z <= hia.z);
}
// Each unordered pair of the slots 0 .. ns-1 once: slot s is tested against the slots (s + d) % ns, d = 1 .. ns / 2,
// and when ns is even the distance ns / 2 is taken from the lower half only (the upper half would repeat the same pairs).
HSD int pair_steps(int ns) { return ns >> 1; }
HSD bool pair_mine(int s, int d, int ns) { return 2 * d != ns || s < d; }
HSD int pair_next(int j, int ns) { return j + 1 == ns ? 0 : j + 1; }      // the partner of the next distance

}  // namespace hs
