// Host check of marl-hideandseek_amd/csrc/hs_sat_box.h (tests/test_sat_box_host.py builds and runs it).
// For every case it runs the two halves of the box-only axis search one after the other, as the two lanes of a pair run
// them side by side, combines them, and compares the result code and the three words of the axis, as bit patterns, with
//   (a) the plain sequential search — all of A's faces, all of B's, the nine edge pairs in order, leaving at the first
//       separating axis — written here with per-axis helpers that take any normal;
//   (b) the oracle's collide_hulls (oracle/hs_ref_phys.hpp).
//   sat_box_check random        240 000 random box pairs; every result class must hold at least 1 % of them
//   sat_box_check special       yaw-only pairs, bodies against walls, exact ties across the lane split, +-0 components
//   sat_box_check file PATH     pairs from a text file: 20 floats per line (e, c, q of A, then of B)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "hs_ref_phys.hpp"
#include "hs_sat_box.h"

using namespace hs;

struct Box { V3 e, c; Q q; };
enum { SEP_FACE = 0, SEP_EDGE, EDGE_CONTACT, FACE_A, FACE_B, NCLASS };
static const char *const kClassName[NCLASS] = {"separated on a face", "separated on an edge", "edge contact",
                                               "face contact, reference A", "face contact, reference B"};

static unsigned bits(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
static bool same(V3 a, V3 b) { return bits(a.x) == bits(b.x) && bits(a.y) == bits(b.y) && bits(a.z) == bits(b.z); }

// ---- (a) the sequential search
static V3 axis_of(const BoxRef &h, int k) { const V3 a[3] = {h.ax, h.ay, h.az}; return a[k]; }
static float extent_of(const BoxRef &h, int k) { const float e[3] = {h.e.x, h.e.y, h.e.z}; return e[k]; }
static V3 face_normal(const BoxRef &h, int f) { const V3 a = axis_of(h, f >> 1); return (f & 1) ? a : -a; }
static float face_offset(const BoxRef &h, int f, V3 fn) { return dot(fn, h.c) + extent_of(h, f >> 1); }
static float sup_min(const BoxRef &h, V3 n) { return dot(n, h.c) - box_radius(h, n); }
static float sup_max(const BoxRef &h, V3 n) { return dot(n, h.c) + box_radius(h, n); }
struct Seq { AxisResult res; int cls; };
static bool faces_of(const BoxRef &X, const BoxRef &Y, float *best, int *fx) {
    *best = 0.f; *fx = -1;
    for (int f = 0; f < 6; ++f) {
        const V3 fn = face_normal(X, f);
        const float s = sup_min(Y, fn) - face_offset(X, f, fn);
        if (s > 0.f) return false;
        if (*fx < 0 || s > *best) { *best = s; *fx = f; }
    }
    return true;
}
static Seq sequential(const BoxRef &A, const BoxRef &B) {
    Seq r = {{0, {0.f, 0.f, 0.f}}, SEP_FACE};
    float bestA, bestB; int fa, fb;
    if (!faces_of(A, B, &bestA, &fa)) return r;
    if (!faces_of(B, A, &bestB, &fb)) return r;
    r.cls = SEP_EDGE;
    float bestE = 0.f; int ea = -1, eb = -1; V3 axE = {0.f, 0.f, 0.f};
    const V3 ab = B.c - A.c;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            V3 ax = cross(axis_of(A, i), axis_of(B, j));
            const float l2 = len2(ax);
            if (l2 < 1e-6f) continue;
            ax = ax * (1.f / sqrtf(l2));
            if (dot(ax, ab) < 0.f) ax = -ax;
            const float s = sup_min(B, ax) - sup_max(A, ax);
            if (s > 0.f) return r;
            if (ea < 0 || s > bestE) { bestE = s; ea = i; eb = j; axE = ax; }
        }
    const float bestF = fmaxf(bestA, bestB);
    if (ea >= 0 && bestE > 0.9f * bestF + 0.0025f) { r.res.code = 1 | (ea << 4) | (eb << 8); r.res.ax = axE; r.cls = EDGE_CONTACT; return r; }
    const bool refB = bestB > 0.98f * bestA + 0.00125f;
    r.res.code = 2 | ((refB ? fb : fa) << 4) | ((refB ? 1 : 0) << 8);
    r.cls = refB ? FACE_B : FACE_A;
    return r;
}

// ---- the code under test, the two lanes of a pair one after the other: the low lane has X = A, its partner X = B
static AxisResult two_halves(const BoxRef &A, const BoxRef &B) {
    const BoxFaceHalf fl = sat_box_faces(A, B), fh = sat_box_faces(B, A);
    const BoxEdgeHalf el = sat_box_edges(A, B, false), eh = sat_box_edges(B, A, true);
    return sat_box_combine(fl, fh, el, eh);
}

static long long g_cases = 0, g_clipless = 0, g_class[NCLASS];
static int g_fail = 0;
static void fail(const char *what, const Box &a, const Box &b, const AxisResult &got) {
    if (++g_fail > 10) return;
    std::printf("FAIL %s: code %#x ax %08x %08x %08x\n  A e %a %a %a  c %a %a %a  q %a %a %a %a\n  B e %a %a %a  c %a %a %a  q %a %a %a %a\n",
                what, got.code, bits(got.ax.x), bits(got.ax.y), bits(got.ax.z),
                a.e.x, a.e.y, a.e.z, a.c.x, a.c.y, a.c.z, a.q.w, a.q.x, a.q.y, a.q.z,
                b.e.x, b.e.y, b.e.z, b.c.x, b.c.y, b.c.z, b.q.w, b.q.x, b.q.y, b.q.z);
}
static void check(const Box &a, const Box &b) {
    const BoxRef A = box_ref(a.c, a.q, a.e), B = box_ref(b.c, b.q, b.e);
    const AxisResult got = two_halves(A, B);
    ++g_cases;
    // (a)
    const Seq seq = sequential(A, B);
    ++g_class[seq.cls];
    if (got.code != seq.res.code || !same(got.ax, seq.res.ax)) fail("against the sequential search", a, b, got);
    // (b)
    hsref::Hull HA, HB;
    hsref::hull_box(HA, A.c, A.ax, A.ay, A.az, A.e);
    hsref::hull_box(HB, B.c, B.ax, B.ay, B.az, B.e);
    hsref::RawManifold m;
    const bool hit = hsref::collide_hulls(HA, HB, m);
    const int kind = got.code & 3, lo = (got.code >> 4) & 15, up = (got.code >> 8) & 15;
    if (kind == 0) {
        if (hit) fail("code 0 but the oracle collides", a, b, got);
    } else if (kind == 1) {
        if (!hit || m.np != 1 || !same(m.n, got.ax)) fail("edge code against the oracle's manifold", a, b, got);
    } else {
        const hsref::Hull &R = up ? HB : HA, &I = up ? HA : HB;
        if (hit) {
            const V3 want = up ? -R.fn[lo] : R.fn[lo];
            if (!same(m.n, want)) fail("face code against the oracle's normal", a, b, got);
        } else {
            // the oracle's clip of the coded face returns no point: (a) has settled the code, this confirms the reason
            V3 p[4]; float d[4];
            ++g_clipless;
            if (hsref::clip_face_contact(R, lo, I, p, d) != 0) fail("face code but the oracle does not collide", a, b, got);
        }
    }
}

// ---- cases
static std::mt19937_64 rng(20250311);
static double uni(double a, double b) { return a + (b - a) * (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }
static int pick(int n) { return (int)(rng() % (unsigned long long)n); }
static Q quat(double w, double x, double y, double z) {
    const double n = std::sqrt(w * w + x * x + y * y + z * z);
    return {(float)(w / n), (float)(x / n), (float)(y / n), (float)(z / n)};
}
static Q any_rotation() {
    for (;;) {
        const double w = uni(-1, 1), x = uni(-1, 1), y = uni(-1, 1), z = uni(-1, 1), n = w * w + x * x + y * y + z * z;
        if (n > 1e-3 && n <= 1.0) return quat(w, x, y, z);
    }
}
static Q yaw(double a) { return quat(std::cos(0.5 * a), 0, 0, std::sin(0.5 * a)); }
static const Q kIdentity = {1.f, 0.f, 0.f, 0.f};
// the shapes of the game: cube, long box, agent (a cube that only yaws), wall (axis-aligned, 2.5 m high, standing on the floor)
enum { CUBE, LONG, AGENT, WALL, NSHAPE };
static Box shape(int s) {
    Box b;
    b.c = {(float)uni(-15, 15), (float)uni(-15, 15), 0.f};
    if (s == WALL) {
        const bool alongx = pick(2) == 0;
        const float l = (float)uni(0.5, 12), t = (float)uni(0.05, 0.6);
        b.e = {alongx ? l : t, alongx ? t : l, 1.25f}; b.q = kIdentity; b.c.z = 1.25f;
    } else {
        b.e = s == LONG ? V3{4.f, 0.75f, 1.f} : V3{1.f, 1.f, 1.f};
        const bool flat = s == AGENT || pick(3) == 0;
        b.q = flat ? yaw(uni(-3.2, 3.2)) : any_rotation();
        b.c.z = flat ? b.e.z + (float)uni(-0.05, 0.05) : (float)uni(0.5, 4);
    }
    return b;
}
// b's centre within `reach` x the sum of the half diagonals of a's; a wall keeps its height
static void place_near(const Box &a, Box &b, double reach, bool keep_z) {
    const double r = reach * (std::sqrt((double)len2(a.e)) + std::sqrt((double)len2(b.e)));
    for (;;) {
        const double x = uni(-1, 1), y = uni(-1, 1), z = uni(-1, 1);
        if (x * x + y * y + z * z > 1.0) continue;
        b.c.x = a.c.x + (float)(r * x); b.c.y = a.c.y + (float)(r * y);
        if (!keep_z) b.c.z = a.c.z + (float)(r * z);
        return;
    }
}

static int finish(const char *name, bool floors) {
    std::printf("%s: %lld cases, %lld with a face code whose clip is empty\n", name, g_cases, g_clipless);
    for (int k = 0; k < NCLASS; ++k) {
        std::printf("  %-28s %8lld  (%.2f %%)\n", kClassName[k], g_class[k], 100.0 * (double)g_class[k] / (double)g_cases);
        if (floors && g_class[k] * 100 < g_cases) { std::printf("FAIL: class '%s' holds under 1 %% of the cases\n", kClassName[k]); ++g_fail; }
    }
    if (g_fail) { std::printf("%d failures\n", g_fail); return 1; }
    std::printf("%s OK\n", name);
    return 0;
}

static int run_random() {
    for (int n = 0; n < 240000; ++n) {
        Box a = shape(pick(NSHAPE - 1)), b = shape(pick(NSHAPE));           // (A is a body; B a body or a wall, as in the kernel)
        // Half of the pairs anywhere within 1.2 x the sum of the half diagonals; the other half close to touching, where
        // the edge axes decide (a ball of that radius is mostly empty space around two long boxes)
        place_near(a, b, n & 1 ? 1.2 : 0.75, b.e.z == 1.25f);
        check(a, b);
    }
    return finish("random", true);
}

static float special_value(int k) {
    static const float v[] = {0.f, -0.f, 1.f, -1.f, 0.5f, -0.5f, 0.70710678f, -0.70710678f};
    return v[k % 8];
}
static int run_special() {
    // yaw-only pairs: the z axes are parallel (cross(z, z) = 0 is skipped) and the z faces of both boxes tie
    for (int n = 0; n < 20000; ++n) {
        Box a = shape(pick(2) ? AGENT : CUBE), b = shape(pick(3));
        a.q = yaw(uni(-3.2, 3.2)); b.q = pick(4) == 0 ? a.q : yaw(uni(-3.2, 3.2));
        a.c.z = a.e.z; b.c.z = pick(2) ? b.e.z : a.c.z + (float)uni(-2.2, 2.2);
        place_near(a, b, 0.9, true);
        check(a, b);
    }
    // bodies against walls, the quarter turns included (axes with exact zeros and ones, parallel to the wall's)
    for (int n = 0; n < 20000; ++n) {
        Box a = shape(pick(3)), b = shape(WALL);
        const int how = pick(4);
        if (how == 0) a.q = yaw(uni(-3.2, 3.2));
        if (how == 1) a.q = yaw(1.5707963267948966 * pick(4));
        if (how == 2) a.q = kIdentity;
        if (how != 3) a.c.z = a.e.z;
        place_near(a, b, 0.8, true);
        check(a, b);
    }
    // exact ties across the lane split: axis-aligned boxes whose overlaps along x and y are the same dyadic number, so that
    // faces of A tie with each other and with faces of B (the low lane's best against its partner's)
    for (int n = 0; n < 20000; ++n) {
        Box a, b;
        a.e = pick(2) ? V3{1.f, 1.f, 1.f} : V3{4.f, 0.75f, 1.f}; a.q = kIdentity;
        a.c = {(float)pick(17) - 8.f, (float)pick(17) - 8.f, a.e.z};
        const bool wall = pick(2) == 0;
        b.q = kIdentity;
        b.e = wall ? V3{0.25f * (float)(1 + pick(16)), 0.25f * (float)(1 + pick(16)), 1.25f} : V3{1.f, 1.f, 1.f};
        const float d = 0.0625f * (float)pick(9), d2 = pick(3) ? d : 0.0625f * (float)pick(9);      // overlap, 0 = touching
        const float sx = pick(2) ? 1.f : -1.f, sy = pick(2) ? 1.f : -1.f;
        b.c = {a.c.x + sx * (a.e.x + b.e.x - d), a.c.y + sy * (a.e.y + b.e.y - d2), wall ? 1.25f : a.c.z + (pick(2) ? 0.f : 2.f - d)};
        if (pick(4) == 0) { a.q = yaw(1.5707963267948966 * pick(4)); }
        check(a, b); check(b, a);
    }
    // +-0 and other special components in centres and quaternions, equal centres included
    for (int n = 0; n < 20000; ++n) {
        Box a = shape(pick(3)), b = shape(pick(NSHAPE));
        a.c = {special_value(pick(8)), special_value(pick(8)), pick(2) ? 1.f : special_value(pick(8))};
        b.c = {special_value(pick(8)), special_value(pick(8)), pick(2) ? b.e.z : special_value(pick(8))};
        for (Box *p : {&a, &b}) {
            if (p->e.z == 1.25f && p == &b) continue;            // (a wall keeps the identity)
            for (;;) {
                const Q q = {special_value(pick(8)), special_value(pick(8)), special_value(pick(8)), special_value(pick(8))};
                const float n2 = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
                if (n2 > 0.9f && n2 < 1.1f) { p->q = q; break; }
            }
        }
        check(a, b);
    }
    return finish("special", false);
}

static int run_file(const char *path) {
    std::FILE *f = std::fopen(path, "r");
    if (!f) { std::printf("cannot open %s\n", path); return 1; }
    float v[20];
    for (;;) {
        int k = 0;
        while (k < 20 && std::fscanf(f, "%f", &v[k]) == 1) ++k;
        if (k == 0) break;
        if (k != 20) { std::printf("short line in %s\n", path); std::fclose(f); return 1; }
        const Box a = {{v[0], v[1], v[2]}, {v[3], v[4], v[5]}, {v[6], v[7], v[8], v[9]}};
        const Box b = {{v[10], v[11], v[12]}, {v[13], v[14], v[15]}, {v[16], v[17], v[18], v[19]}};
        check(a, b);
    }
    std::fclose(f);
    return finish("file", false);
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "random")) return run_random();
    if (argc >= 2 && !std::strcmp(argv[1], "special")) return run_special();
    if (argc >= 3 && !std::strcmp(argv[1], "file")) return run_file(argv[2]);
    std::printf("usage: sat_box_check random | special | file PATH\n");
    return 2;
}
