// The separating-axis search for TWO BOXES, straight-line: what sat_axes (hs_collide.h) computes when both hulls are
// boxes, bit for bit, written as the two halves of its lane split and their combination.  Plain scalar functions like
// hs_broadphase.h, so that a host program can compile them too (tests/host/sat_box_check.cpp); the device wrapper
// (hs_collide.h sat_axes_box) adds only the exchange between the two lanes of a pair.
//
// Why a form of its own.  In sat_axes the face loop and the edge loop stay rolled (their trip counts and exits depend on
// the lane), so the face and edge indices are per-lane variables and every trip selects its axis and extent through
// masks, divides the pair index, and branches over the wedge's code.  With the hull kind known and the loops written
// out, every axis is a named field: the only selects left are the ones between the two lanes' roles.
//
// The half of a lane (role `hi` = the second lane of the pair):
//   faces   the lane's own box X against the other box Y: faces 0 .. 5 of X (A on the low lane, B on its partner);
//   edges   pairs p = 3 i + j of cross(A.axis[i], B.axis[j]): p = 0 .. 3 on the low lane, p = 4 .. 8 on its partner.
// Both halves are functions of (X, Y, role): X is the lane's own box (A on the low lane, B on its partner), Y the other.
// sat_axes leaves a loop at the first separating axis; here every axis is evaluated and the flags are ORed.  The result is
// the same: any separating axis gives code 0, and the running best is not read then.
#pragma once
#include "hs_core.h"

namespace hs {

// code 0 = separated;  1 | ea << 4 | eb << 8 = edge contact along `ax`;  2 | face << 4 | refB << 8 = face contact with
// reference face `face` of B (refB) or A;  3 = an extra plane (hs_k_physics.h phase_sat)
struct AxisResult { int code; V3 ax; };

struct BoxRef { V3 c, ax, ay, az, e; };      // centre, rotation columns, half extents
HSD BoxRef box_ref(V3 c, Q q, V3 e) { const M3 m = m3_from_quat(q); return {c, m.c0, m.c1, m.c2, e}; }
// (the expression of box_radius(HullRef), hs_collide.h)
HSD float box_radius(const BoxRef &h, V3 n) {
    return hs_fma(fabsf(dot(n, h.az)), h.e.z, hs_fma(fabsf(dot(n, h.ay)), h.e.y, fabsf(dot(n, h.ax)) * h.e.x));
}

// ---- faces of X against Y.  best / f: the first maximum of the six separations; sep: one of them is positive.
struct BoxFaceHalf { float best; int f; int sep; };
// Faces 2k and 2k + 1 of a box have the normals -axis_k and +axis_k.  sat_axes evaluates, for the normal n,
//     s = (dot(n, Y.c) - box_radius(Y, n)) - (dot(n, X.c) + e_k).
// Both faces share dY = dot(axis_k, Y.c), dX = dot(axis_k, X.c) and r = box_radius(Y, axis_k):
//   - a product and a fused multiply-add are odd functions under round-to-nearest (negating every input negates the
//     rounded result), so dot(-a, c) is -dot(a, c) — except that a sum which cancels exactly is +0 either way, so the
//     two can differ in the SIGN OF A ZERO;
//   - box_radius takes fabsf of its three dots, so it is the same for n and -n, and it is positive (a unit axis has a
//     non-zero dot with one of Y's axes, the extents are positive); e_k is positive too.  A zero of either sign minus r,
//     or plus e_k, is the same number: the sign of such a zero never reaches s.
// So (-dY - r) - (-dX + e_k) and (dY - r) - (dX + e_k) have the bits of the two evaluations of sat_axes.
HSD void box_face_pair(float dY, float dX, float r, float ek, int k, BoxFaceHalf &h) {
    const float s0 = (-dY - r) - (-dX + ek), s1 = (dY - r) - (dX + ek);
    h.sep |= (s0 > 0.f) | (s1 > 0.f);
    if (k == 0 || s0 > h.best) { h.best = s0; h.f = 2 * k; }        // "first or strictly greater", in face order
    if (s1 > h.best) { h.best = s1; h.f = 2 * k + 1; }
}
HSD BoxFaceHalf sat_box_faces(const BoxRef &X, const BoxRef &Y) {
    BoxFaceHalf h = {0.f, -1, 0};
    box_face_pair(dot(X.ax, Y.c), dot(X.ax, X.c), box_radius(Y, X.ax), X.e.x, 0, h);
    box_face_pair(dot(X.ay, Y.c), dot(X.ay, X.c), box_radius(Y, X.ay), X.e.y, 1, h);
    box_face_pair(dot(X.az, Y.c), dot(X.az, X.c), box_radius(Y, X.az), X.e.z, 2, h);
    return h;
}

// ---- edge-direction crosses of A and B, on the lane's own X and Y (A = X, B = Y on the low lane; A = Y, B = X on its
// partner).  best / ea / eb / ax: the first maximum over the lane's pairs (ea < 0: every pair of the lane was skipped as
// parallel); sep: one of them separates.
struct BoxEdgeHalf { float best; int ea, eb; V3 ax; int sep; };
// One pair, exactly the loop body of sat_axes: the skip of (nearly) parallel directions, 1.f / sqrtf(l2), the flip
// towards B, support_min(B) - support_max(A), the update.  `da`, `db`: the directions A.axis[i], B.axis[j]; `on`: the
// lane has a pair in this slot.  Both boxes' centre projections and radii are needed whatever the role, so the role
// only picks which pair of them is subtracted from which.
HSD void box_edge_slot(const BoxRef &X, const BoxRef &Y, bool hi, V3 ab, V3 da, V3 db, int i, int j, bool on, BoxEdgeHalf &h) {
    V3 ax = cross(da, db);
    const float l2 = len2(ax);
    on = on && !(l2 < 1e-6f);
    ax = ax * (1.f / sqrtf(l2));
    if (dot(ax, ab) < 0.f) ax = -ax;
    const float dX = dot(ax, X.c), dY = dot(ax, Y.c), rX = box_radius(X, ax), rY = box_radius(Y, ax);
    const float s = hi ? (dX - rX) - (dY + rY) : (dY - rY) - (dX + rX);
    h.sep |= on && s > 0.f;
    if (on && (h.ea < 0 || s > h.best)) { h.best = s; h.ea = i; h.eb = j; h.ax = ax; }
}
// Five slots: slot t is pair t on the low lane (t < 4) and pair 4 + t on its partner, so that both directions of a slot
// are named fields on either side of one select on `hi`.
//   (i, j):   low lane   (0,0) (0,1) (0,2) (1,0)  -        partner   (1,1) (1,2) (2,0) (2,1) (2,2)
HSD BoxEdgeHalf sat_box_edges(const BoxRef &X, const BoxRef &Y, bool hi) {
    BoxEdgeHalf h = {0.f, -1, -1, {0.f, 0.f, 0.f}, 0};
    const V3 ab = vsel(hi, X.c - Y.c, Y.c - X.c);                    // B.c - A.c
    //                                A.axis[i]: partner, low lane   B.axis[j]: partner, low lane
    box_edge_slot(X, Y, hi, ab, vsel(hi, Y.ay, X.ax), vsel(hi, X.ay, Y.ax), hi ? 1 : 0, hi ? 1 : 0, true, h);
    box_edge_slot(X, Y, hi, ab, vsel(hi, Y.ay, X.ax), vsel(hi, X.az, Y.ay), hi ? 1 : 0, hi ? 2 : 1, true, h);
    box_edge_slot(X, Y, hi, ab, vsel(hi, Y.az, X.ax), vsel(hi, X.ax, Y.az), hi ? 2 : 0, hi ? 0 : 2, true, h);
    box_edge_slot(X, Y, hi, ab, vsel(hi, Y.az, X.ay), vsel(hi, X.ay, Y.ax), hi ? 2 : 1, hi ? 1 : 0, true, h);
    box_edge_slot(X, Y, hi, ab, Y.az, X.az, 2, 2, hi, h);
    return h;
}

// ---- the two halves into the result, as the sequential search would leave it (lo: A's faces and pairs 0 .. 3, hi: B's
// faces and pairs 4 .. 8): a separating axis anywhere gives code 0; the second half of the edge pairs replaces the first
// half's best only if strictly greater; then the thresholds of sat_axes.
HSD AxisResult sat_box_combine(const BoxFaceHalf &fl, const BoxFaceHalf &fh, const BoxEdgeHalf &el, const BoxEdgeHalf &eh) {
    AxisResult res = {0, {0.f, 0.f, 0.f}};
    if (fl.sep | fh.sep | el.sep | eh.sep) return res;
    const float bestA = fl.best, bestB = fh.best;
    const int fa = fl.f, fb = fh.f;
    float bestE = el.best; int ea = el.ea, eb = el.eb; V3 axE = el.ax;
    if (eh.ea >= 0 && (ea < 0 || eh.best > bestE)) { bestE = eh.best; ea = eh.ea; eb = eh.eb; axE = eh.ax; }
    const float bestF = fmaxf(bestA, bestB);
    if (ea >= 0 && bestE > 0.9f * bestF + 0.0025f) { res.code = 1 | (ea << 4) | (eb << 8); res.ax = axE; return res; }
    const bool refB = bestB > 0.98f * bestA + 0.00125f;
    res.code = 2 | ((refB ? fb : fa) << 4) | ((refB ? 1 : 0) << 8);
    return res;
}

}  // namespace hs
