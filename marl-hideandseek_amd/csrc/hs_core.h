// The scalar core: vector / quaternion math, trigonometry, RNG, constants and object tables.  ONE text read by two
// compilers: hipcc for the HIP kernels (through hs_dev.h) and the host compiler for the CPU oracle (whose math header
// includes this file; nothing here includes anything of the oracle's).  Plain C++17: pure scalar functions and constants that
// know nothing of lanes, LDS or memory layout.  Everything above this layer is written twice, separately, and the parity
// tests compare the two; this layer is pinned from first principles (tests/test_oracle_rng_math.py,
// tests/test_oracle_first_principles.py, tests/golden/object_table.json, tests/golden/ray_hull_cases.npz), function by
// function through the probe table hs_core_probe.h: tests/test_core_float64.py holds the host compile to plain float64
// restatements (rounding-count bounds for the products and sums, exact known answers for the fused multiply-adds, the RNG
// and aabb_overlaps, the trigonometry on its callers' domain and at every range switch, both branches of
// quat_add_rotation, the rays against half-space clipping), tests/host/core_check.cpp runs the same table under the
// address and undefined-behaviour sanitizers, and tests/test_gpu_core_probe.py compares the device compile with the host
// compile word for word — the assumption that the two compilers make the same bits of this text.
//
// Float discipline: both sides compile this with -ffp-contract=off and without fast-math.  Every expression here is
// written in a fixed association order with its fused multiply-adds spelled out (hs_fma: one rounding, the same on both
// machines); the parity tests compare the kernels' results with the CPU oracle bit for bit, so do not "simplify" arithmetic.
//
// The engine pieces the reference takes from Madrona (vector/quaternion math, RNG) are absent
// from the reference snapshot; see DESIGN.md "Engine decisions" for what is chosen here.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define HSD __device__ __forceinline__
#define HS_UNROLL _Pragma("unroll")
#else
#include <cmath>
#include <cstdint>
#define HSD inline
#define HS_UNROLL
#endif

namespace hs {

// ---- capacities and constants: src/sim.hpp:39-41, src/sim.cpp:14-17 ----
constexpr int kMaxBoxes = 9;
constexpr int kMaxRamps = 2;
constexpr int kMaxAgents = 6;
constexpr int kBoxSlot0 = 0;
constexpr int kRampSlot0 = 9;
constexpr int kAgentSlot0 = 11;
constexpr int kNumDSlots = 17;
constexpr int kMaxWalls = 36;
constexpr int kMaxPlanes = 3;
constexpr int kNumPrepSteps = 96;
constexpr int kEpisodeLen = 240;
constexpr int kNumSubsteps = 4;          // setupPhysicsStepTasks(..., 4, XPBD)  src/sim.cpp:1162-1163
constexpr float kSubstepH = (1.f / 30.f) / 4.f;
constexpr float kInvSubstepH = 120.f;
constexpr float kGravityZ = -9.8f;
constexpr float kMaxDepenVel = 3.f;
constexpr float kCosFovHalf = 0.382683426f;
constexpr float kPi = 3.14159265358979323846f;
// body ids a ray cast returns: 0..16 movable slots, 100+k walls, 200+p planes, -1 miss
constexpr int kHitWallBase = 100;
constexpr int kHitPlaneBase = 200;

// SimObject (src/sim.hpp:78-88)
enum : int { OBJ_SPHERE = 0, OBJ_PLANE = 1, OBJ_CUBE = 2, OBJ_WALL = 3, OBJ_HIDER = 4, OBJ_SEEKER = 5,
             OBJ_RAMP = 6, OBJ_BOX = 7, OBJ_NONE = -1 };
enum : int { OWNER_NONE = 0, OWNER_SEEKER = 1, OWNER_HIDER = 2, OWNER_UNOWNABLE = 3 };
enum : int { RESP_DYNAMIC = 0, RESP_KINEMATIC = 1, RESP_STATIC = 2 };
enum : int { AGENT_SEEKER = 0, AGENT_HIDER = 1 };
enum : uint32_t { FLAG_DEFAULT = 0, FLAG_USE_FIXED_WORLD = 1, FLAG_IGNORE_EPISODE_LENGTH = 2, FLAG_RANDOM_FLIP_TEAMS = 4,
                  FLAG_ZERO_AGENT_VELOCITY = 8, FLAG_EXT_SKIP_OBSERVATIONS = 1u << 16, FLAG_EXT_RENDER = 1u << 17 };

struct V3 { float x, y, z; };
struct Q { float w, x, y, z; };

HSD V3 v3(float x, float y, float z) { return V3{x, y, z}; }
HSD V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
HSD V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
HSD V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
HSD V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
HSD V3 mulc(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
HSD V3 vsel(bool c, V3 a, V3 b) { return {c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }
// (fused multiply-adds, written out one by one: the kernels and the CPU oracle read the same ones in the same places)
HSD float hs_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
HSD float dot(V3 a, V3 b) { return hs_fma(a.z, b.z, hs_fma(a.y, b.y, a.x * b.x)); }
HSD V3 cross(V3 a, V3 b) { return {hs_fma(a.y, b.z, -(a.z * b.y)), hs_fma(a.z, b.x, -(a.x * b.z)), hs_fma(a.x, b.y, -(a.y * b.x))}; }
// a + b * s and a - b * s, each component one fused multiply-add
HSD V3 madd(V3 a, V3 b, float s) { return {hs_fma(b.x, s, a.x), hs_fma(b.y, s, a.y), hs_fma(b.z, s, a.z)}; }
HSD V3 nmadd(V3 a, V3 b, float s) { return {hs_fma(-b.x, s, a.x), hs_fma(-b.y, s, a.y), hs_fma(-b.z, s, a.z)}; }
// a . b + c and a x b + c with every product fused
HSD float dot_add(V3 a, V3 b, float c) { return hs_fma(a.z, b.z, hs_fma(a.y, b.y, hs_fma(a.x, b.x, c))); }
HSD V3 cross_add(V3 a, V3 b, V3 c) {
    return {hs_fma(a.y, b.z, hs_fma(-a.z, b.y, c.x)), hs_fma(a.z, b.x, hs_fma(-a.x, b.z, c.y)), hs_fma(a.x, b.y, hs_fma(-a.y, b.x, c.z))};
}
HSD float len2(V3 a) { return dot(a, a); }
HSD float len(V3 a) { return sqrtf(dot(a, a)); }
// (madrona Vector3::normalize, used at sim.cpp:591,733,786) — v * (1/len)
HSD V3 normalize(V3 a) { float inv = 1.f / len(a); return a * inv; }

// ---- quaternions (w,x,y,z), madrona::math::Quat call sites sim.cpp:225,350,408-409,469 ----
HSD Q qmul(Q a, Q b) {
    return {hs_fma(-a.z, b.z, hs_fma(-a.y, b.y, hs_fma(-a.x, b.x, a.w * b.w))),
            hs_fma(-a.z, b.y, hs_fma(a.y, b.z, hs_fma(a.x, b.w, a.w * b.x))),
            hs_fma(a.z, b.x, hs_fma(a.y, b.w, hs_fma(-a.x, b.z, a.w * b.y))),
            hs_fma(a.z, b.w, hs_fma(-a.y, b.x, hs_fma(a.x, b.y, a.w * b.z)))};
}
HSD Q qinv(Q q) { return {q.w, -q.x, -q.y, -q.z}; }  // unit quaternions: conjugate
HSD Q qnormalize(Q q) {
    float n2 = hs_fma(q.z, q.z, hs_fma(q.y, q.y, hs_fma(q.x, q.x, q.w * q.w)));
    float inv = 1.f / sqrtf(n2);
    return {q.w * inv, q.x * inv, q.y * inv, q.z * inv};
}
// v' = 2(p.v)p + (2w^2-1)v + 2w(p x v)
HSD V3 qrot(Q q, V3 v) {
    V3 p = {q.x, q.y, q.z};
    float s = q.w;
    float d2 = 2.f * dot(p, v);
    float s2 = 2.f * s;
    float k = hs_fma(s2, s, -1.f);
    V3 c = cross(p, v);
    return {hs_fma(s2, c.x, hs_fma(d2, p.x, k * v.x)), hs_fma(s2, c.y, hs_fma(d2, p.y, k * v.y)), hs_fma(s2, c.z, hs_fma(d2, p.z, k * v.z))};
}

// sin/cos by Cody-Waite pi/2 reduction + cephes single-precision minimax polynomials; atan2/asin likewise.  These replace
// libm/ocml so that host oracle and device agree exactly.
HSD void hs_sincosf(float x, float *s_out, float *c_out) {
    const float two_over_pi = 0.63661977236758134308f;
    const float pio2_hi = 1.5707962512969970703125f;     // pi/2 split: hi + lo
    const float pio2_lo = 7.54978995489188216e-8f;
    float kf = x * two_over_pi;
    int k = (int)(kf + (kf >= 0.f ? 0.5f : -0.5f));
    float fk = (float)k;
    float r = (x - fk * pio2_hi) - fk * pio2_lo;
    float z = r * r;
    float sp = ((-1.9515295891e-4f * z + 8.3321608736e-3f) * z - 1.6666654611e-1f) * z * r + r;
    float cp = ((2.443315711809948e-5f * z - 1.388731625493765e-3f) * z + 4.166664568298827e-2f) * z * z
               - 0.5f * z + 1.f;
    int q = k & 3;
    float s = (q == 0) ? sp : (q == 1) ? cp : (q == 2) ? -sp : -cp;
    float c = (q == 0) ? cp : (q == 1) ? -sp : (q == 2) ? -cp : sp;
    *s_out = s; *c_out = c;
}
HSD float hs_atanf(float xin) {
    float sign = xin < 0.f ? -1.f : 1.f;
    float x = fabsf(xin);
    float y;
    // ranges: x > tan(3pi/8): pi/2 + atan(-(1/x));  x > tan(pi/8): pi/4 + atan((x-1)/(x+1));  else atan(x).  One division
    // serves both reductions: (-1)/x is the same correctly rounded quotient as -(1/x).
    const bool big = x > 2.414213562373095f, mid = x > 0.4142135623730950f;
    y = big ? 1.5707963267948966f : (mid ? 0.7853981633974483f : 0.f);
    if (mid) { const float num = big ? -1.f : x - 1.f, den = big ? x : x + 1.f; x = num / den; }
    float z = x * x;
    y = y + ((((8.05374449538e-2f * z - 1.38776856032e-1f) * z + 1.99777106478e-1f) * z - 3.33329491539e-1f) * z * x + x);
    return sign * y;
}
HSD float hs_atan2f(float y, float x) {
    if (x == 0.f) {
        if (y > 0.f) return 0.5f * kPi;
        if (y < 0.f) return -0.5f * kPi;
        return 0.f;
    }
    float a = hs_atanf(y / x);
    if (x < 0.f) { a = (y >= 0.f) ? a + kPi : a - kPi; }
    return a;
}
HSD float hs_asinf(float xin) {
    float sign = xin < 0.f ? -1.f : 1.f;
    float a = fabsf(xin);
    float z, x;
    bool flag = a > 0.5f;
    if (flag) { z = 0.5f * (1.f - a); x = sqrtf(z); }
    else { x = a; z = x * x; }
    float p = ((((4.2163199048e-2f * z + 2.4181311049e-2f) * z + 4.5470025998e-2f) * z + 7.4953002686e-2f) * z
               + 1.6666752422e-1f) * z * x + x;
    if (flag) { p = p + p; p = 1.5707963267948966f - p; }
    return sign * p;
}
// Quat::angleAxis(angle, {0,0,1}) (level_gen.cpp:139,179,215,277)
HSD Q quat_angle_axis_z(float angle) {
    float s, c;
    hs_sincosf(angle * 0.5f, &s, &c);
    return {c, 0.f, 0.f, s};
}

// ---- 3x3 rotation (columns) from a unit quaternion ----
struct M3 { V3 c0, c1, c2; };
HSD M3 m3_from_quat(Q q) {
    float y2 = q.y * q.y, z2 = q.z * q.z;
    float xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z;
    M3 m;
    m.c0 = {hs_fma(-2.f, hs_fma(q.y, q.y, z2), 1.f), 2.f * hs_fma(q.w, q.z, xy), 2.f * hs_fma(-q.w, q.y, xz)};
    m.c1 = {2.f * hs_fma(-q.w, q.z, xy), hs_fma(-2.f, hs_fma(q.x, q.x, z2), 1.f), 2.f * hs_fma(q.w, q.x, yz)};
    m.c2 = {2.f * hs_fma(q.w, q.y, xz), 2.f * hs_fma(-q.w, q.x, yz), hs_fma(-2.f, hs_fma(q.x, q.x, y2), 1.f)};
    return m;
}

// quatToEuler (src/sim.cpp:372-399)
HSD V3 quat_to_euler(Q q) {
    float sinr = 2.f * (q.w * q.x + q.y * q.z);
    float cosr = 1.f - 2.f * (q.x * q.x + q.y * q.y);
    float roll = hs_atan2f(sinr, cosr);
    float sinp = 2.f * (q.w * q.y - q.z * q.x);
    float pitch = fabsf(sinp) >= 1.f ? copysignf(kPi / 2.f, sinp) : hs_asinf(sinp);
    float siny = 2.f * (q.w * q.z + q.x * q.y);
    float cosy = 1.f - 2.f * (q.y * q.y + q.z * q.z);
    float yaw = hs_atan2f(siny, cosy);
    return {roll, pitch, yaw};
}

// ---- AABB overlap (madrona::math::AABB call sites level_gen.cpp:104-121,142-143) ----
struct AABB { V3 lo, hi; };
HSD bool aabb_overlaps(const AABB &a, const AABB &b) {
    return a.lo.x < b.hi.x && b.lo.x < a.hi.x && a.lo.y < b.hi.y && b.lo.y < a.hi.y &&
           a.lo.z < b.hi.z && b.lo.z < a.hi.z;
}

// ---- counter-based RNG: Threefry-2x32-20 (Salmon et al., SC'11), integer-only sampling paths.  Stands in for
// madrona::RNG / madrona::rand (call sites src/sim.cpp:105-114,163,187-190). ----
struct RandKey { uint32_t a, b; };
HSD uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
HSD RandKey threefry2x32(RandKey key, uint32_t c0, uint32_t c1) {
    const uint32_t ks0 = key.a, ks1 = key.b, ks2 = 0x1BD11BDAu ^ key.a ^ key.b;
    uint32_t x0 = c0 + ks0, x1 = c1 + ks1;
#define HS_TF_R(r) { x0 += x1; x1 = rotl32(x1, r); x1 ^= x0; }
    HS_TF_R(13) HS_TF_R(15) HS_TF_R(26) HS_TF_R(6)
    x0 += ks1; x1 += ks2 + 1u;
    HS_TF_R(17) HS_TF_R(29) HS_TF_R(16) HS_TF_R(24)
    x0 += ks2; x1 += ks0 + 2u;
    HS_TF_R(13) HS_TF_R(15) HS_TF_R(26) HS_TF_R(6)
    x0 += ks0; x1 += ks1 + 3u;
    HS_TF_R(17) HS_TF_R(29) HS_TF_R(16) HS_TF_R(24)
    x0 += ks1; x1 += ks2 + 4u;
    HS_TF_R(13) HS_TF_R(15) HS_TF_R(26) HS_TF_R(6)
    x0 += ks2; x1 += ks0 + 5u;
#undef HS_TF_R
    return {x0, x1};
}
// madrona::RNG: a key plus a draw counter; every draw derives a fresh sub-key.  An aggregate {key, count}.
struct RNG {
    RandKey k; uint32_t count;
    HSD RandKey advance() { return threefry2x32(k, count++, 0u); }
    HSD uint32_t bits32() { RandKey s = advance(); return s.a ^ s.b; }
    // half-open [a, b); an empty range (level_gen.cpp:87-88 when total==3) returns a.
    HSD int32_t sampleI32(int32_t a, int32_t b) {
        uint32_t range = (uint32_t)(b - a);
        uint32_t v = (uint32_t)(((uint64_t)bits32() * (uint64_t)range) >> 32);
        return a + (int32_t)v;
    }
    // uniform in [0,1): top 24 bits * 2^-24 (exact in fp32)
    HSD float sampleUniform() { return (float)(bits32() >> 8) * (1.f / 16777216.f); }
    HSD RandKey randKey() { return advance(); }
};

// ---- object tables: src/mgr.cpp:476-559,577-584 ----
// inverse mass and friction per SimObject (no level ever makes a sphere; the table has it)
HSD float obj_inv_mass(int o) { return (o == OBJ_CUBE || o == OBJ_RAMP || o == OBJ_BOX) ? 0.5f : ((o == OBJ_HIDER || o == OBJ_SEEKER || o == OBJ_SPHERE) ? 1.f : 0.f); }
HSD float obj_mu_s(int o) { return o == OBJ_PLANE ? 2.f : 0.5f; }
HSD float obj_mu_d(int o) {
    return (o == OBJ_PLANE || o == OBJ_CUBE || o == OBJ_WALL) ? 2.f
         : (o == OBJ_HIDER || o == OBJ_SEEKER) ? 16.f : (o == OBJ_RAMP) ? 1.f : (o == OBJ_BOX) ? 4.f : 0.5f;
}
// Diagonal inverse inertia in the object frame (uniform density solids; the wedge's product of
// inertia and centre-of-mass offset are dropped — DESIGN.md).  Agents: x,y zeroed (mgr.cpp:577-584).
HSD V3 obj_inv_inertia(int o) {
    if (o == OBJ_CUBE) return {0.75f, 0.75f, 0.75f};                       // m=2, 2x2x2
    if (o == OBJ_BOX) return {0.96f, 0.088235294f, 0.090566038f};          // m=2, 8x1.5x2
    if (o == OBJ_RAMP) return {0.692307692f, 0.9f, 0.6f};                  // m=2 wedge
    if (o == OBJ_HIDER || o == OBJ_SEEKER) return {0.f, 0.f, 1.5f};        // m=1, 2x2x2, yaw only
    return {0.f, 0.f, 0.f};
}
HSD V3 obj_half_extents(int o) { return o == OBJ_BOX ? V3{4.f, 0.75f, 1.f} : V3{1.f, 1.f, 1.f}; }

// ---- solver leaves ----
// World-space inverse inertia R diag(invI) R^T (symmetric, 6 values): evaluated once per manifold / joint from the
// body's rotation at that moment and kept while the manifold's contact points are solved.
struct Sym3 { float xx, xy, xz, yy, yz, zz; };
HSD Sym3 world_inv_inertia(Q q, V3 invI) {
    M3 m = m3_from_quat(q);
    V3 r0 = m.c0 * invI.x, r1 = m.c1 * invI.y, r2 = m.c2 * invI.z;
    Sym3 s;
    s.xx = hs_fma(r2.x, m.c2.x, hs_fma(r1.x, m.c1.x, r0.x * m.c0.x));
    s.xy = hs_fma(r2.x, m.c2.y, hs_fma(r1.x, m.c1.y, r0.x * m.c0.y));
    s.xz = hs_fma(r2.x, m.c2.z, hs_fma(r1.x, m.c1.z, r0.x * m.c0.z));
    s.yy = hs_fma(r2.y, m.c2.y, hs_fma(r1.y, m.c1.y, r0.y * m.c0.y));
    s.yz = hs_fma(r2.y, m.c2.z, hs_fma(r1.y, m.c1.z, r0.y * m.c0.z));
    s.zz = hs_fma(r2.z, m.c2.z, hs_fma(r1.z, m.c1.z, r0.z * m.c0.z));
    return s;
}
HSD V3 sym_mul(const Sym3 &s, V3 v) {
    return {hs_fma(s.xz, v.z, hs_fma(s.xy, v.y, s.xx * v.x)), hs_fma(s.yz, v.z, hs_fma(s.yy, v.y, s.xy * v.x)),
            hs_fma(s.zz, v.z, hs_fma(s.yz, v.y, s.xz * v.x))};
}
// q += 0.5 * (0,dth) * q, then — for small updates — ONE Newton step of 1/sqrt(|q|^2) from 1 instead of an exact
// normalisation (DESIGN.md "Engine decisions"): |q|^2 = 1 + |dth|^2/4 after the update, so the step leaves a norm error
// of 3/8 (|dth|^2/4)^2 (< 2e-5 even for a body tumbling at 20 rad/s) that the next update corrects again; it costs 4
// multiplies instead of sqrt + divide in the innermost loop of the solver.
HSD Q quat_add_rotation(Q q, V3 dth) {
    Q dq = qmul(Q{0.f, dth.x, dth.y, dth.z}, q);
    Q r = {hs_fma(0.5f, dq.w, q.w), hs_fma(0.5f, dq.x, q.x), hs_fma(0.5f, dq.y, q.y), hs_fma(0.5f, dq.z, q.z)};
    const float n2 = hs_fma(r.z, r.z, hs_fma(r.y, r.y, hs_fma(r.x, r.x, r.w * r.w)));
    // small updates (|dth| < 0.2 rad: every contact correction, ordinary integration); a joint that snaps a badly
    // misaligned body round can turn it by radians in one go and gets the exact normalisation
    const float k = n2 < 1.01f ? hs_fma(-0.5f, n2, 1.5f) : 1.f / sqrtf(n2);
    return {r.w * k, r.x * k, r.y * k, r.z * k};
}

// ---- ray against one hull in the hull's own frame (origin o, direction d local): entry t, or -1 for a miss.  Closest
// front-face entry; a ray that starts inside the hull does not hit it. ----
HSD float ray_box_local(V3 o, V3 d, V3 e) {
    float tn = -3.0e38f, tf = 3.0e38f;
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, ee[3] = {e.x, e.y, e.z};
    bool miss = false;
    HS_UNROLL
    for (int k = 0; k < 3; ++k) {
        if (dd[k] == 0.f) { if (oo[k] < -ee[k] || oo[k] > ee[k]) miss = true; continue; }
        // slab in centre / extent form: entry = -o/d - e/|d|, exit = -o/d + e/|d| (no near/far swap)
        float inv = 1.f / dd[k];
        const float r = ee[k] * fabsf(inv);                 // entry = -o/d - e/|d|, exit = -o/d + e/|d|, each one fused multiply-add
        tn = fmaxf(tn, hs_fma(-oo[k], inv, -r)); tf = fminf(tf, hs_fma(-oo[k], inv, r));
    }
    if (miss || tn > tf || tn < 0.f) return -1.f;
    return tn;
}
HSD float ray_wedge_local(V3 o, V3 d) {
    float tn = -3.0e38f, tf = 3.0e38f;
    // face normals and plane offsets of the wedge in its own frame: n.p = off
    const float fn[5][3] = {{0, 0, -1}, {0, 1, 0}, {0, -0.554700196f, 0.832050294f}, {1, 0, 0}, {-1, 0, 0}};
    const float off[5] = {1.f, 1.f, 0.277350098f, 1.f, 1.f};
    bool miss = false;
    HS_UNROLL
    for (int f = 0; f < 5; ++f) {
        V3 n = {fn[f][0], fn[f][1], fn[f][2]};
        float dist = dot(n, o) - off[f];
        float dn = dot(n, d);
        if (dn == 0.f) { if (dist > 0.f) miss = true; continue; }
        float t = -dist / dn;
        if (dn < 0.f) tn = fmaxf(tn, t); else tf = fminf(tf, t);
    }
    if (miss || tn > tf || tn < 0.f) return -1.f;
    return tn;
}

}  // namespace hs
