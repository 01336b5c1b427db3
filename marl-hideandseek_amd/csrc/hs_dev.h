// Device-only helpers for the HIP kernels (gfx950) on top of the scalar core (hs_core.h: math, RNG, constants and object
// tables, the one text the CPU oracle reads too).  What lives here knows about lanes, LDS capacities or the kernels' packing.
#pragma once
#include "hs_core.h"

// The lane index as the physics kernel reads it: an OPAQUE copy of threadIdx.x.  k_physics is one function of ~60 000
// instructions whose phases each derive a dozen lane constants (world = lane / 8, LDS offsets of its rows, ...).  Given
// the plain threadIdx.x the compiler computes them all once at the top of the kernel and keeps them alive through the
// substep loop — some forty registers of loop invariants in a kernel that sits at the 256-register budget of two waves
// per SIMD (12 spilled dwords, 52 B of scratch per lane).  An empty asm makes every call a value of its own: each phase
// re-derives its constants (a few integer instructions) and nothing lives across phases: 223 registers, no spill, no
// scratch.
__device__ __forceinline__ int hs_lane() { int x = threadIdx.x; asm volatile("" : "+v"(x)); return x; }

namespace hs {

// Candidate-pair capacities per world per substep (DESIGN.md "Engine decisions"); -DHS_MAX_DD_CAND / -DHS_MAX_S_CAND
// shrink them for the overflow test (tests/test_gpu_status.py), nothing else overrides them.
#ifndef HS_MAX_DD_CAND
#define HS_MAX_DD_CAND 16
#endif
#ifndef HS_MAX_S_CAND
#define HS_MAX_S_CAND 24
#endif
constexpr int kMaxDDCand = HS_MAX_DD_CAND;
constexpr int kGrabWords = 15;      // grab-joint record: r2 3, attach2 4, separation 1, r1 3, attach1 4
constexpr int kMaxSCand = HS_MAX_S_CAND;

// body meta word: (objType+1) | response<<8 | owner<<16 ; 0 == empty slot
HSD int meta_pack(int obj, int resp, int owner) { return (obj + 1) | (resp << 8) | (owner << 16); }
HSD int meta_obj(int m) { return (m & 0xff) - 1; }
HSD int meta_resp(int m) { return (m >> 8) & 0xff; }
HSD int meta_owner(int m) { return (m >> 16) & 0xff; }

// 1 / inverse inertia per axis (0 where the inverse is 0): the same IEEE quotients integrate would compute, folded
// at compile time
HSD V3 obj_inertia(int o) {
    if (o == OBJ_CUBE) return {1.f / 0.75f, 1.f / 0.75f, 1.f / 0.75f};
    if (o == OBJ_BOX) return {1.f / 0.96f, 1.f / 0.088235294f, 1.f / 0.090566038f};
    if (o == OBJ_RAMP) return {1.f / 0.692307692f, 1.f / 0.9f, 1.f / 0.6f};
    if (o == OBJ_HIDER || o == OBJ_SEEKER) return {0.f, 0.f, 1.f / 1.5f};
    return {0.f, 0.f, 0.f};
}

}  // namespace hs
