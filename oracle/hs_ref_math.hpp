// ORACLE — TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is shipped or called by the
// product path (marl-hideandseek_amd/); only tests/, __graft_entry__.smoke() and bench.py's
// cpu_baseline leg may build/load it.  The dependency runs one way: the oracle reads the product's
// scalar core, the product never includes anything from oracle/.
//
// PARITY UNPINNED: the reference's arithmetic for vectors/quaternions/AABBs lives in the
// Madrona engine (external/madrona, an empty submodule directory in the reference snapshot,
// pinned commit unknown).  The scalar core (csrc/hs_core.h: V3 / Q / M3 and their fused
// multiply-adds, the trigonometry, the RNG, the constants, enums and object tables, the
// ray-against-one-hull tests) is ONE file read by both compilers, so a leaf expression cannot
// differ between the two sides; it is pinned from first principles (known-answer vectors, libm,
// the reference's meshes), not by comparing the sides.  Everything above it — level generation,
// narrowphase, solver scheduling, observations, rendering — is restated here separately from the
// kernels, against the semantics visible at the call sites (src/sim.cpp, src/level_gen.cpp).
// All float code must be compiled with -ffp-contract=off: the HIP product evaluates the same
// expression trees in the same order so results agree bit for bit.  The fused multiply-adds are
// written out one by one (hs_fma) — as a CUDA build of the reference fuses by default (nvcc
// --fmad=true), though which of its operations that fuses is as unknowable as the rest of the
// engine's arithmetic.
#pragma once
#include "../marl-hideandseek_amd/csrc/hs_core.h"

namespace hsref {
using namespace hs;

// ---- helpers only the oracle uses ----
struct V2 { float x, y; };
static inline V3 operator*(float s, V3 a) { return {a.x * s, a.y * s, a.z * s}; }
static inline float getc(V3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }

// Real-Time Collision Detection 4.2.6 style transformed AABB: M = R * diag(scale).
static inline AABB aabb_apply_trs(AABB b, V3 t, Q r, V3 s) {
    M3 m = m3_from_quat(r);
    m.c0 = m.c0 * s.x; m.c1 = m.c1 * s.y; m.c2 = m.c2 * s.z;
    float lo[3] = {t.x, t.y, t.z}, hi[3] = {t.x, t.y, t.z};
    const V3 cols[3] = {m.c0, m.c1, m.c2};
    const float bl[3] = {b.lo.x, b.lo.y, b.lo.z}, bh[3] = {b.hi.x, b.hi.y, b.hi.z};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            float mij = getc(cols[j], i);
            float e = mij * bl[j], f = mij * bh[j];
            if (e < f) { lo[i] += e; hi[i] += f; } else { lo[i] += f; hi[i] += e; }
        }
    }
    return {{lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}};
}

}  // namespace hsref
