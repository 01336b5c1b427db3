// The probe table of the scalar core: ONE function that evaluates one core function on one case, read — like hs_core.h
// itself — by both compilers.  g++ compiles it into the CPU oracle (hsref_core_eval) and into tests/host/core_check.cpp;
// hipcc compiles it into k_core_eval (hs_debug_core_eval).  tests/test_core_float64.py pins the host compile to plain
// float64 references, tests/test_gpu_core_probe.py compares the device compile with the host compile bit for bit.
// Test infrastructure only: no kernel of the simulator or the learner calls anything here, and hs_core.h does not
// include this file.
//
// A case is 16 input words and 16 output words.  Integer operands and results travel as bit patterns; every output
// word an op does not name is written as +0.  V3 = x y z, Q = w x y z, in consecutive words.
//
//   op                     in                                            out
//    0 DOT                 a[0..2] b[3..5]                               [0]
//    1 DOT_ADD             a[0..2] b[3..5] c[6]                          [0]
//    2 CROSS               a[0..2] b[3..5]                               [0..2]
//    3 CROSS_ADD           a[0..2] b[3..5] c[6..8]                       [0..2]
//    4 MADD                a[0..2] b[3..5] s[6]                          [0..2]   a + b s
//    5 NMADD               a[0..2] b[3..5] s[6]                          [0..2]   a - b s
//    6 LEN                 a[0..2]                                       [0]
//    7 NORMALIZE           a[0..2]                                       [0..2]
//    8 QMUL                a[0..3] b[4..7]                               [0..3]
//    9 QINV                q[0..3]                                       [0..3]
//   10 QNORMALIZE          q[0..3]                                       [0..3]
//   11 QROT                q[0..3] v[4..6]                               [0..2]
//   12 M3_FROM_QUAT        q[0..3]                                       c0[0..2] c1[3..5] c2[6..8]
//   13 QUAT_ANGLE_AXIS_Z   angle[0]                                      [0..3]
//   14 QUAT_TO_EULER       q[0..3]                                       roll pitch yaw [0..2]
//   15 WORLD_INV_INERTIA   q[0..3] invI[4..6]                            xx xy xz yy yz zz [0..5]
//   16 SYM_MUL             xx xy xz yy yz zz [0..5] v[6..8]              [0..2]
//   17 QUAT_ADD_ROTATION   q[0..3] dth[4..6]                             [0..3]
//   18 SINCOS              x[0]                                          sin [0] cos [1]
//   19 ATAN                x[0]                                          [0]
//   20 ATAN2               y[0] x[1]                                     [0]
//   21 ASIN                x[0]                                          [0]
//   22 AABB_OVERLAPS       a.lo[0..2] a.hi[3..5] b.lo[6..8] b.hi[9..11]  int32 0 / 1 [0]
//   23 RNG_BITS32          key.a[0] key.b[1] count[2]  (uint32)          uint32 [0], count afterwards [1]
//   24 SAMPLE_I32          key.a[0] key.b[1] count[2] a[3] b[4] (int32)  int32 [0], count afterwards [1]
//   25 SAMPLE_UNIFORM      key.a[0] key.b[1] count[2]                    float [0], count afterwards [1]
//   26 RAY_BOX_LOCAL       o[0..2] d[3..5] e[6..8]                       t or -1 [0]
//   27 RAY_WEDGE_LOCAL     o[0..2] d[3..5]                               t or -1 [0]
//   28 QMUL_QINV           q[0..3]                                       qmul(q, qinv(q)) [0..3]
//   29 EULER_OF_YAW        yaw[0]                                        quat_to_euler(quat_angle_axis_z(yaw)) [0..2]
#pragma once
#include "hs_core.h"

namespace hs {

enum : int { CORE_DOT = 0, CORE_DOT_ADD, CORE_CROSS, CORE_CROSS_ADD, CORE_MADD, CORE_NMADD, CORE_LEN, CORE_NORMALIZE,
             CORE_QMUL, CORE_QINV, CORE_QNORMALIZE, CORE_QROT, CORE_M3_FROM_QUAT, CORE_QUAT_ANGLE_AXIS_Z, CORE_QUAT_TO_EULER,
             CORE_WORLD_INV_INERTIA, CORE_SYM_MUL, CORE_QUAT_ADD_ROTATION, CORE_SINCOS, CORE_ATAN, CORE_ATAN2, CORE_ASIN,
             CORE_AABB_OVERLAPS, CORE_RNG_BITS32, CORE_SAMPLE_I32, CORE_SAMPLE_UNIFORM, CORE_RAY_BOX_LOCAL, CORE_RAY_WEDGE_LOCAL,
             CORE_QMUL_QINV, CORE_EULER_OF_YAW, CORE_NUM_OPS };
constexpr int kCoreWords = 16;          // words per case, in and out

HSD uint32_t core_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
HSD float core_word(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
HSD void core_put(float *out, V3 v) { out[0] = v.x; out[1] = v.y; out[2] = v.z; }
HSD void core_put(float *out, Q q) { out[0] = q.w; out[1] = q.x; out[2] = q.y; out[3] = q.z; }

HSD void core_eval(int op, const float *in, float *out) {
    HS_UNROLL
    for (int i = 0; i < kCoreWords; ++i) out[i] = 0.f;
    const V3 a = {in[0], in[1], in[2]}, b = {in[3], in[4], in[5]}, c = {in[6], in[7], in[8]};
    const Q q = {in[0], in[1], in[2], in[3]};
    const V3 v = {in[4], in[5], in[6]};
    RNG rng = {RandKey{core_bits(in[0]), core_bits(in[1])}, core_bits(in[2])};
    switch (op) {
    case CORE_DOT: out[0] = dot(a, b); break;
    case CORE_DOT_ADD: out[0] = dot_add(a, b, in[6]); break;
    case CORE_CROSS: core_put(out, cross(a, b)); break;
    case CORE_CROSS_ADD: core_put(out, cross_add(a, b, c)); break;
    case CORE_MADD: core_put(out, madd(a, b, in[6])); break;
    case CORE_NMADD: core_put(out, nmadd(a, b, in[6])); break;
    case CORE_LEN: out[0] = len(a); break;
    case CORE_NORMALIZE: core_put(out, normalize(a)); break;
    case CORE_QMUL: core_put(out, qmul(q, Q{in[4], in[5], in[6], in[7]})); break;
    case CORE_QINV: core_put(out, qinv(q)); break;
    case CORE_QNORMALIZE: core_put(out, qnormalize(q)); break;
    case CORE_QROT: core_put(out, qrot(q, v)); break;
    case CORE_M3_FROM_QUAT: { const M3 m = m3_from_quat(q); core_put(out, m.c0); core_put(out + 3, m.c1); core_put(out + 6, m.c2); break; }
    case CORE_QUAT_ANGLE_AXIS_Z: core_put(out, quat_angle_axis_z(in[0])); break;
    case CORE_QUAT_TO_EULER: core_put(out, quat_to_euler(q)); break;
    case CORE_WORLD_INV_INERTIA: {
        const Sym3 s = world_inv_inertia(q, v);
        out[0] = s.xx; out[1] = s.xy; out[2] = s.xz; out[3] = s.yy; out[4] = s.yz; out[5] = s.zz;
        break;
    }
    case CORE_SYM_MUL: { const Sym3 s = {in[0], in[1], in[2], in[3], in[4], in[5]}; core_put(out, sym_mul(s, c)); break; }
    case CORE_QUAT_ADD_ROTATION: core_put(out, quat_add_rotation(q, v)); break;
    case CORE_SINCOS: hs_sincosf(in[0], &out[0], &out[1]); break;
    case CORE_ATAN: out[0] = hs_atanf(in[0]); break;
    case CORE_ATAN2: out[0] = hs_atan2f(in[0], in[1]); break;
    case CORE_ASIN: out[0] = hs_asinf(in[0]); break;
    case CORE_AABB_OVERLAPS: {
        const AABB x = {a, b}, y = {c, V3{in[9], in[10], in[11]}};
        out[0] = core_word(aabb_overlaps(x, y) ? 1u : 0u);
        break;
    }
    case CORE_RNG_BITS32: out[0] = core_word(rng.bits32()); out[1] = core_word(rng.count); break;
    case CORE_SAMPLE_I32:
        out[0] = core_word((uint32_t)rng.sampleI32((int32_t)core_bits(in[3]), (int32_t)core_bits(in[4])));
        out[1] = core_word(rng.count);
        break;
    case CORE_SAMPLE_UNIFORM: out[0] = rng.sampleUniform(); out[1] = core_word(rng.count); break;
    case CORE_RAY_BOX_LOCAL: out[0] = ray_box_local(a, b, c); break;
    case CORE_RAY_WEDGE_LOCAL: out[0] = ray_wedge_local(a, b); break;
    case CORE_QMUL_QINV: core_put(out, qmul(q, qinv(q))); break;
    case CORE_EULER_OF_YAW: core_put(out, quat_to_euler(quat_angle_axis_z(in[0]))); break;
    default: break;
    }
}

}  // namespace hs
