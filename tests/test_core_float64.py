"""The scalar core (marl-hideandseek_amd/csrc/hs_core.h) as the HOST compiler reads it, against plain float64.

hs_core.h is the one layer the kernels and the CPU oracle share, so no lock-step test can see a mistake in it.  Here every
function of it is evaluated through the probe table (csrc/hs_core_probe.h, hsref_core_eval) and compared with NumPy float64
restatements of the documented mathematics, written in this file with no code of the project's.  u = 2^-24 throughout.
tests/test_gpu_core_probe.py imports the inputs of this file and compares the device compile with the host compile bit for bit.

Bounds of the products and sums: |result - reference| <= k u M, M the sum of the absolute values of the terms of the
reference expression, k the number of roundings on the longest path of the expression as hs_core.h writes it (derived
beside each K entry below; none exceeds 16).  Everything else states its bound where it is used.

Domain of the trigonometry = the callers' domain:
  hs_sincosf   level-generation yaws theta = U[0,1) * pi and their halves (hs_k_reset.h sample_placement ->
               quat_angle_axis_z, oracle/hs_ref_level.hpp likewise) and the lidar angles (hs_k_reset.h k_lidar_table,
               oracle/hs_ref_sim.hpp): |x| <= 2 pi on the dense grid.  The 30 lidar angles 2 pi k / 30 + pi / 2 reach
               7.65 > 2 pi, so they are added one by one under the same tolerance.
  hs_atan2f    quat_to_euler's (sinr, cosr) and (siny, cosy) (hs_k_observe.h, oracle/hs_ref_sim.hpp): any direction,
               radius about 1 and below; hs_atanf sees their quotient, any real number.
  hs_asinf     quat_to_euler's sinp with |sinp| < 1 (the gimbal branch takes the rest): [-1, 1].
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20250607

# op numbers of csrc/hs_core_probe.h
OPS = {n: i for i, n in enumerate(
    ["DOT", "DOT_ADD", "CROSS", "CROSS_ADD", "MADD", "NMADD", "LEN", "NORMALIZE", "QMUL", "QINV", "QNORMALIZE", "QROT",
     "M3_FROM_QUAT", "QUAT_ANGLE_AXIS_Z", "QUAT_TO_EULER", "WORLD_INV_INERTIA", "SYM_MUL", "QUAT_ADD_ROTATION", "SINCOS",
     "ATAN", "ATAN2", "ASIN", "AABB_OVERLAPS", "RNG_BITS32", "SAMPLE_I32", "SAMPLE_UNIFORM", "RAY_BOX_LOCAL",
     "RAY_WEDGE_LOCAL", "QMUL_QINV", "EULER_OF_YAW"])}

# k = roundings on the longest path, as hs_core.h writes the expression (x2, x0.5 and negations are exact)
K = {
    "DOT": 3,                # a.x*b.x (1) -> fma with a.y*b.y (2) -> fma with a.z*b.z (3)
    "DOT_ADD": 3,            # three nested fmas, c inside the innermost
    "CROSS": 2,              # a.z*b.y (1) -> fma(a.y, b.z, -that) (2)
    "CROSS_ADD": 2,          # fma(-a.z, b.y, c.x) (1) -> fma(a.y, b.z, that) (2)
    "MADD": 1,               # one fma per component
    "NMADD": 1,
    "QMUL": 4,               # a.w*b.w (1) -> three nested fmas (4)
    "SYM_MUL": 3,            # s.xx*v.x (1) -> two nested fmas (3)
    "M3_DIAG": 3,            # z2 = q.z*q.z (1) -> fma(q.y, q.y, z2) (2) -> fma(-2, that, 1) (3)
    "M3_OFF": 2,             # xy = q.x*q.y (1) -> fma(q.w, q.z, xy) (2) -> x2 exact
    "QROT": 5,               # dot(p, v) (3) -> d2 exact -> fma(d2, p.x, k*v.x) (4) -> fma(s2, c.x, that) (5);
                             # the other operands arrive earlier: k = fma(s2, s, -1) (1) -> k*v.x (2), cross (2)
    "WORLD_INV_INERTIA": 7,  # diagonal entry of m3_from_quat (3) -> r0 = c0 * invI.x (4) -> r0.x*m.c0.x (5) -> two fmas (7)
}

PI32 = np.float32(3.14159265358979323846)        # kPi as a float: 0x40490FDB


# --------------------------------------------------------------------------------------------------------------------
# inputs: one seeded generator, drawn once, in a fixed order; shared with tests/test_gpu_core_probe.py
# --------------------------------------------------------------------------------------------------------------------
def pack(n, *parts):
    """[n, 16] float32 words from column blocks (float32 values; use words() for integers)."""
    x = np.zeros((n, 16), np.float32)
    c = 0
    for p in parts:
        p = np.asarray(p, np.float32).reshape(n, -1)
        x[:, c:c + p.shape[1]] = p
        c += p.shape[1]
    return x


def words(n, *cols):
    """[n, 16] words from integer columns, as bit patterns."""
    x = np.zeros((n, 16), np.uint32)
    for c, col in enumerate(cols):
        x[:, c] = np.asarray(col).astype(np.int64) & 0xFFFFFFFF
    return x.view(np.float32)


def comps(g, *shape):
    """+-[1e-3, 1e3] log-uniform, or exactly 0 (one in twenty): nothing underflows in a product of two or three."""
    x = g.choice([-1.0, 1.0], shape) * 10.0 ** g.uniform(-3.0, 3.0, shape)
    x[g.random(shape) < 0.05] = 0.0
    return x.astype(np.float32)


def unit_quats(g, n):
    """float32 roundings of unit quaternions; the first rows are the identity, pure yaws and axis half-turns."""
    q = g.normal(size=(n, 4))
    yaw = g.uniform(-np.pi, np.pi, n // 8)
    q[:n // 8] = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], 1)
    q[:5] = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [np.sqrt(0.5), 0, 0, np.sqrt(0.5)]]
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def directions(g, n, dim=3):
    d = g.normal(size=(n, dim))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def ulp_neighbours(centres, width=8, inside=None):
    """Every float32 within `width` ulps on either side of each centre (itself included); `inside` = (lo, hi) clips."""
    out = []
    for c in centres:
        x = np.float32(c)
        up, dn = [x], []
        for _ in range(width):
            up.append(np.nextafter(up[-1], np.float32(np.inf)))
            dn.append(np.nextafter((dn or [x])[-1], np.float32(-np.inf)))
        out += dn[::-1] + up
    out = np.array(out, np.float32)
    if inside is not None:
        out = out[(out >= inside[0]) & (out <= inside[1])]
    return out


def inexact_pairs(g, n):
    """float32 a, b whose float32 product is inexact; p = fl32(a b) and e = a b - p (exact in float64, and a float32)."""
    a = g.uniform(1.0, 2.0, 4 * n).astype(np.float32) * g.choice([-1.0, 1.0], 4 * n).astype(np.float32)
    b = g.uniform(1.0, 2.0, 4 * n).astype(np.float32)
    exact = a.astype(np.float64) * b.astype(np.float64)           # 48 bits: exact in float64
    p = exact.astype(np.float32)
    keep = np.flatnonzero(exact != p.astype(np.float64))[:n]
    assert len(keep) == n
    a, b, p = a[keep], b[keep], p[keep]
    e = a.astype(np.float64) * b.astype(np.float64) - p.astype(np.float64)
    assert np.all(e != 0) and np.array_equal(e, e.astype(np.float32).astype(np.float64))
    return a, b, p, e


# ---- Threefry-2x32-20 (Salmon et al., SC'11) and the sampling paths in integers.  The same text serves Python integers
# (the known-answer vectors) and NumPy uint64 arrays (the bulk): only + ^ & << >> on values kept below 2^32.
M32 = 0xFFFFFFFF
ROT = (13, 15, 26, 6, 17, 29, 16, 24)


def threefry2x32(k0, k1, c0, c1):
    ks = (k0, k1, (k0 ^ k1) ^ 0x1BD11BDA)
    x0, x1 = (c0 + ks[0]) & M32, (c1 + ks[1]) & M32
    for block in range(5):
        for r in ROT[:4] if block % 2 == 0 else ROT[4:]:
            x0 = (x0 + x1) & M32
            x1 = ((x1 << r) & M32) | (x1 >> (32 - r))
            x1 = x1 ^ x0
        x0 = (x0 + ks[(block + 1) % 3]) & M32
        x1 = (x1 + ks[(block + 2) % 3] + (block + 1)) & M32
    return x0, x1


def rng_bits32(k0, k1, count):
    a, b = threefry2x32(k0, k1, count, 0 * count)
    return a ^ b


def rng_sample_i32(bits, a, b):
    """half-open [a, b): a + floor(bits * (b - a) / 2^32), as a signed 32-bit value (bits, a, b: integer arrays)."""
    lo = (bits & 0xFFFF) * ((b - a) & M32)                        # 64-bit product in two halves: no overflow of uint64
    hi = (bits >> 16) * ((b - a) & M32)
    v = (hi + (lo >> 16)) >> 16
    return a + v


@functools.lru_cache(maxsize=None)
def all_inputs():
    """name -> dict(x = [n, 16] float32 words, ...what the references need).  Special cases come first in every table."""
    g = np.random.default_rng(SEED)
    N = 65536
    T = {}
    for name in ("DOT", "CROSS"):
        T[name] = dict(x=pack(N, comps(g, N, 3), comps(g, N, 3)))
    T["DOT_ADD"] = dict(x=pack(N, comps(g, N, 3), comps(g, N, 3), comps(g, N)))
    T["CROSS_ADD"] = dict(x=pack(N, comps(g, N, 3), comps(g, N, 3), comps(g, N, 3)))
    for name in ("MADD", "NMADD"):
        T[name] = dict(x=pack(N, comps(g, N, 3), comps(g, N, 3), comps(g, N)))
    T["QMUL"] = dict(x=pack(N, unit_quats(g, N), unit_quats(g, N)))
    T["QMUL_GENERAL"] = dict(op="QMUL", x=pack(N, comps(g, N, 4), comps(g, N, 4)))
    T["SYM_MUL"] = dict(x=pack(N, comps(g, N, 6), comps(g, N, 3)))
    q = unit_quats(g, N)
    T["QINV"] = dict(x=pack(N, q))
    T["QMUL_QINV"] = dict(x=pack(N, q))
    T["M3_FROM_QUAT"] = dict(x=pack(N, q))
    T["QROT"] = dict(x=pack(N, q, comps(g, N, 3)))
    T["WORLD_INV_INERTIA"] = dict(x=pack(N, q, comps(g, N, 3)))
    T["QUAT_TO_EULER"] = dict(x=pack(N, unit_quats(g, N)))

    # lengths log-uniform in [1e-3, 1e3]
    for name, dim in (("LEN", 3), ("NORMALIZE", 3), ("QNORMALIZE", 4)):
        T[name] = dict(x=pack(N, directions(g, N, dim) * 10.0 ** g.uniform(-3.0, 3.0, (N, 1))))

    # quat_add_rotation: |dth| across [0, 3] rad, and 1500 cases on each side of the switch |dth|^2 / 4 = 0.01, within 1e-4
    n_wide, n_side = N - 3000, 1500
    mag = np.concatenate([2.0 * np.sqrt(0.01 - g.uniform(0.0, 1e-4, n_side)), 2.0 * np.sqrt(0.01 + g.uniform(0.0, 1e-4, n_side)),
                          g.uniform(0.0, 3.0, n_wide)])
    mag[2 * n_side] = 0.0
    T["QUAT_ADD_ROTATION"] = dict(x=pack(N, unit_quats(g, N), directions(g, N) * mag[:, None]), n_side=n_side)

    # trigonometry: branch points first, then 2^20 evenly spaced inputs
    D = 1 << 20
    half_pi = [k * np.pi / 2 for k in range(-4, 5)]
    round_switch = [(m + 0.5) * np.pi / 2 for m in range(-5, 5)]          # kf +- 0.5 crosses an integer
    lidar = np.array([np.float32(2) * PI32 * (np.float32(k) / np.float32(30)) + PI32 / np.float32(2) for k in range(30)], np.float32)
    x = np.concatenate([ulp_neighbours(half_pi), ulp_neighbours(round_switch), lidar, np.linspace(-2 * np.pi, 2 * np.pi, D).astype(np.float32)])
    T["SINCOS"] = dict(x=pack(len(x), x), n_special=len(x) - D)
    t1, t3 = np.tan(np.pi / 8), np.tan(3 * np.pi / 8)
    big = 10.0 ** np.linspace(1.0, 6.0, 2048)
    x = np.concatenate([ulp_neighbours([-t3, -t1, 0.0, t1, t3]), np.float32([-0.0]), big.astype(np.float32), -big.astype(np.float32),
                        np.linspace(-8.0, 8.0, D).astype(np.float32)])
    T["ATAN"] = dict(x=pack(len(x), x))
    x = np.concatenate([ulp_neighbours([-0.5, 0.0, 0.5]), ulp_neighbours([-1.0, 1.0], inside=(-1.0, 1.0)), np.float32([-0.0]),
                        np.linspace(-1.0, 1.0, D).astype(np.float32)])
    T["ASIN"] = dict(x=pack(len(x), x))
    phi = np.linspace(-np.pi, np.pi, D)
    rad = np.array([1.0, 0.37, 1e-2])[np.arange(D) % 3]
    T["ATAN2"] = dict(x=pack(D, (rad * np.sin(phi)).astype(np.float32), (rad * np.cos(phi)).astype(np.float32)))
    # the axes and the signed zeros, as hs_atan2f is written: (y, x, expected bit pattern)
    half = np.float32(0.5) * PI32
    axes = [(2.0, 0.0, half), (2.0, -0.0, half), (-2.0, 0.0, -half), (-2.0, -0.0, -half),
            (0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (0.0, -0.0, 0.0), (-0.0, -0.0, 0.0),       # x == 0, y neither > 0 nor < 0: +0
            (0.0, 1.0, 0.0), (-0.0, 1.0, 0.0),        # atanf(-0) = sign(+1) * (0 + (+0)) = +0, where libm returns -0
            (0.0, -1.0, PI32),
            (-0.0, -1.0, PI32)]                       # `y >= 0.f` holds for -0: +pi, where libm returns -pi
    a = np.array(axes, np.float32)
    T["ATAN2_AXES"] = dict(op="ATAN2", x=pack(len(a), a[:, 0], a[:, 1]), expect=a[:, 2].copy())
    yaw = np.linspace(-np.pi, np.pi, N + 2)[1:-1].astype(np.float32)
    T["EULER_OF_YAW"] = dict(x=pack(N, yaw))
    T["QUAT_ANGLE_AXIS_Z"] = dict(x=pack(N, yaw))

    # RNG: 65 536 (key, count) pairs; count 0xFFFFFFFF, all-zero and all-one keys first
    k0, k1, cnt = (g.integers(0, 1 << 32, N, dtype=np.uint64) for _ in range(3))
    k0[:4], k1[:4], cnt[:4] = [0, M32, 0x13198A2E, 7], [0, M32, 0x03707344, 9], [0, M32, M32, M32]
    lo = g.integers(-(1 << 30), 1 << 30, N, dtype=np.int64)
    rng = np.minimum(g.integers(0, 1 << 31, N, dtype=np.int64), (1 << 31) - 1 - np.maximum(lo, 0))
    rng[g.random(N) < 0.25] %= 16                    # the small ranges the level generator draws from
    hi = lo + rng
    lo[:8], hi[:8] = [3, -5, -(1 << 31), -(1 << 30), 0, -7, 3, (1 << 31) - 2], [3, -5, -1, (1 << 30) - 1, 2, 0, 10, (1 << 31) - 1]
    assert np.all(hi >= lo) and np.all(hi - lo <= (1 << 31) - 1) and hi.max() < 1 << 31 and lo.min() >= -(1 << 31)
    assert (hi - lo).max() == (1 << 31) - 1 and np.any(hi == lo) and lo.min() < 0
    T["RNG_BITS32"] = dict(x=words(N, k0, k1, cnt), key=(k0, k1), count=cnt)
    T["SAMPLE_UNIFORM"] = dict(x=words(N, k0, k1, cnt), key=(k0, k1), count=cnt)
    T["SAMPLE_I32"] = dict(x=words(N, k0, k1, cnt, lo, hi), key=(k0, k1), count=cnt, a=lo, b=hi)

    # aabb_overlaps: integer boxes; the hand-written cases first (name, a.lo, a.hi, b.lo, b.hi, overlap)
    A = ((0, 0, 0), (2, 3, 4))
    hand = [("face", A, ((2, 0, 0), (4, 3, 4)), 0), ("edge", A, ((2, 3, 0), (4, 5, 4)), 0), ("corner", A, ((2, 3, 4), (3, 4, 5)), 0),
            ("b inside a", A, ((1, 1, 1), (1.5, 2, 3)), 1), ("a inside b", A, ((-1, -1, -1), (3, 4, 5)), 1), ("equal", A, A, 1),
            ("shifted", A, ((1, 1, 1), (3, 4, 5)), 1)]
    for k in range(3):                               # each of the six inequalities as the only one that fails
        for side in (0, 1):
            for gap in (0, 1):                       # touching, and apart
                lo_b, hi_b = [1, 1, 1], [3, 4, 5]
                if side == 0:
                    hi_b[k] = A[0][k] - gap; lo_b[k] = hi_b[k] - 2
                else:
                    lo_b[k] = A[1][k] + gap; hi_b[k] = lo_b[k] + 2
                hand.append((f"only axis {k} side {side} gap {gap}", A, (tuple(lo_b), tuple(hi_b)), 0))
    hb = np.array([[*a[0], *a[1], *b[0], *b[1]] for _, a, b, _ in hand], np.float64)
    lo_a, lo_b = g.integers(-4, 4, (4096, 3)), g.integers(-4, 4, (4096, 3))
    rb = np.concatenate([lo_a, lo_a + g.integers(1, 5, (4096, 3)), lo_b, lo_b + g.integers(1, 5, (4096, 3))], 1).astype(np.float64)
    T["AABB_OVERLAPS"] = dict(x=pack(len(hb) + 4096, np.concatenate([hb, rb])), n_hand=len(hand),
                              hand_expect=np.array([h[3] for h in hand]), hand_names=[h[0] for h in hand])

    # rays: aim from outside (sometimes inside) at a point of the hull's bounding box scaled by 1.4
    R = 32768
    for name, centre in (("RAY_BOX_LOCAL", None), ("RAY_WEDGE_LOCAL", np.array([0.0, -0.5, 0.0]))):
        if centre is None:
            e = np.where(g.random((R, 1)) < 0.5, np.array([[1.0, 1.0, 1.0], [4.0, 0.75, 1.0]])[g.integers(0, 2, R)], g.uniform(0.25, 4.0, (R, 3)))
            half_box, c = e, 0.0
        else:
            e, half_box, c = None, np.array([1.0, 1.5, 1.0]), centre
        p = c + g.uniform(-1.4, 1.4, (R, 3)) * half_box
        o = p + directions(g, R) * g.uniform(0.1, 12.0, (R, 1))
        d = (p - o) * g.uniform(0.05, 3.0, (R, 1))
        zero = g.random((R, 3)) < 0.06               # +-0 components: parallel to a pair of faces
        d = np.where(zero, np.where(g.random((R, 3)) < 0.5, -0.0, 0.0), d)
        d[np.all(d == 0, axis=1)] = [1.0, 0.0, -0.0]
        o, d = o.astype(np.float32), d.astype(np.float32)
        T[name] = dict(x=pack(R, o, d, e.astype(np.float32)) if e is not None else pack(R, o, d))
    return T


def table(name):
    return all_inputs()[name]


def op_of(name):
    return OPS[all_inputs()[name].get("op", name)]


def subset(x, n):
    """At most n rows of a table: the first n / 2 (the special cases lead every table) and an even sample of all of it."""
    if len(x) <= n:
        return x
    head = np.arange((n + 1) // 2)
    idx = np.unique(np.concatenate([head, np.linspace(0, len(x) - 1, n - len(head)).astype(np.int64)]))
    return x[idx]


@functools.lru_cache(maxsize=None)
def host(name):
    """The host compile's outputs for a whole table: (float32 [n, 16], the same as float64)."""
    import hs_ref
    hs_ref.build()
    out = hs_ref.core_eval(op_of(name), table(name)["x"])
    out.setflags(write=False)
    with np.errstate(invalid="ignore"):                           # (integer results that happen to be NaN patterns)
        return out, out.astype(np.float64)


def f64(name):
    return table(name)["x"].astype(np.float64)


def within(res, ref, bound, what):
    err = np.abs(res - ref)
    bad = ~(err <= bound)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: {res.size} values, worst error / bound = {worst:.3f}")
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), worst)
    assert np.all(res[(bound == 0) & np.isfinite(ref)] == ref[(bound == 0) & np.isfinite(ref)])


# --------------------------------------------------------------------------------------------------------------------
# products and sums
# --------------------------------------------------------------------------------------------------------------------
def test_no_k_exceeds_16_and_the_probe_table_has_every_op():
    assert max(K.values()) <= 16
    assert len(OPS) == 30 and all(op_of(n) in OPS.values() for n in all_inputs())
    assert set(OPS) <= {all_inputs()[n].get("op", n) for n in all_inputs()}, "an op without inputs"


def rot_matrix(q):
    """Rotation by q / |q| (float64), R[..., i, j], and the sum of the absolute values of each entry's terms."""
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = (q[..., i] for i in range(4))
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                  np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                  np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    a = np.abs
    MR = np.stack([np.stack([1 + 2 * (y * y + z * z), 2 * (a(x * y) + a(w * z)), 2 * (a(x * z) + a(w * y))], -1),
                   np.stack([2 * (a(x * y) + a(w * z)), 1 + 2 * (x * x + z * z), 2 * (a(y * z) + a(w * x))], -1),
                   np.stack([2 * (a(x * z) + a(w * y)), 2 * (a(y * z) + a(w * x)), 1 + 2 * (x * x + y * y)], -1)], -2)
    return R, MR


def off_unit(q):
    """| |q|^2 - 1 | of the float32 input: its own distance from unit length."""
    return np.abs(np.sum(q * q, axis=-1) - 1.0)


def test_dot_dot_add_cross_cross_add_madd_nmadd():
    for name in ("DOT", "DOT_ADD"):
        x, (_, r) = f64(name), host(name)
        terms = np.concatenate([x[:, 0:3] * x[:, 3:6], x[:, 6:7] if name == "DOT_ADD" else np.zeros((len(x), 1))], 1)
        within(r[:, 0], terms.sum(1), K[name] * U * np.abs(terms).sum(1), name)
    for name in ("CROSS", "CROSS_ADD"):
        x, (_, r) = f64(name), host(name)
        a, b, c = x[:, 0:3], x[:, 3:6], (x[:, 6:9] if name == "CROSS_ADD" else 0 * x[:, 6:9])
        i, j = [1, 2, 0], [2, 0, 1]
        ref = a[:, i] * b[:, j] - a[:, j] * b[:, i] + c
        M = np.abs(a[:, i] * b[:, j]) + np.abs(a[:, j] * b[:, i]) + np.abs(c)
        within(r[:, :3], ref, K[name] * U * M, name)
    for name, sgn in (("MADD", 1.0), ("NMADD", -1.0)):
        x, (_, r) = f64(name), host(name)
        a, b, s = x[:, 0:3], x[:, 3:6], x[:, 6:7]
        within(r[:, :3], a + sgn * b * s, K[name] * U * (np.abs(a) + np.abs(b * s)), name)
    for name in ("DOT", "DOT_ADD", "CROSS", "CROSS_ADD", "MADD", "NMADD"):
        assert np.all(host(name)[0][:, 3 if name not in ("DOT", "DOT_ADD") else 1:].view(np.uint32) == 0), "unnamed output words are +0"


def qmul64(a, b):
    aw, ax, ay, az = (a[:, i] for i in range(4))
    bw, bx, by, bz = (b[:, i] for i in range(4))
    terms = np.stack([np.stack([aw * bw, -ax * bx, -ay * by, -az * bz], -1), np.stack([aw * bx, ax * bw, ay * bz, -az * by], -1),
                      np.stack([aw * by, -ax * bz, ay * bw, az * bx], -1), np.stack([aw * bz, ax * by, -ay * bx, az * bw], -1)], 1)
    return terms.sum(-1), np.abs(terms).sum(-1)


def test_qmul_unit_and_general_operands():
    for name in ("QMUL", "QMUL_GENERAL"):
        x, (_, r) = f64(name), host(name)
        ref, M = qmul64(x[:, 0:4], x[:, 4:8])
        within(r[:, :4], ref, K["QMUL"] * U * M, name)


def test_qinv_is_the_conjugate_and_q_times_its_inverse_is_one():
    x, (r32, _) = table("QINV")["x"], host("QINV")
    assert np.array_equal(r32[:, :4].view(np.uint32), (x[:, :4] * np.float32([1, -1, -1, -1])).view(np.uint32))
    x, (_, r) = f64("QMUL_QINV"), host("QMUL_QINV")
    q = x[:, :4]
    _, M = qmul64(q, q * [1, -1, -1, -1])
    # q q* = (|q|^2, 0, 0, 0) exactly; the input is a float32 rounding of a unit quaternion, | |q|^2 - 1 | <= 2u + u^2 of it
    assert off_unit(q).max() <= 2 * U * (1 + U) + 1e-15           # (1e-15: the float64 normalisation before the rounding)
    one = np.zeros((len(q), 4)); one[:, 0] = 1.0
    bound = K["QMUL"] * U * M
    bound[:, 0] += off_unit(q)
    within(r[:, :4], one, bound, "qmul(q, qinv(q))")


def test_sym_mul():
    x, (_, r) = f64("SYM_MUL"), host("SYM_MUL")
    xx, xy, xz, yy, yz, zz = (x[:, i] for i in range(6))
    S = np.stack([np.stack([xx, xy, xz], -1), np.stack([xy, yy, yz], -1), np.stack([xz, yz, zz], -1)], 1)
    terms = S * x[:, None, 6:9]
    within(r[:, :3], terms.sum(-1), K["SYM_MUL"] * U * np.abs(terms).sum(-1), "sym_mul")


def m3_bound(q):
    R, MR = rot_matrix(q)
    k = np.where(np.eye(3, dtype=bool), K["M3_DIAG"], K["M3_OFF"])
    return R, MR, k * U * MR + 2 * off_unit(q)[:, None, None] * MR


def test_m3_from_quat_stores_columns():
    x, (r32, r) = f64("M3_FROM_QUAT"), host("M3_FROM_QUAT")
    R, _, bound = m3_bound(x[:, :4])
    cols = r[:, :9].reshape(-1, 3, 3)                         # [case, column k, row i]
    within(cols.transpose(0, 2, 1), R, bound, "m3_from_quat")
    # row 4 of the table is a yaw of +90 degrees: it takes x^ to y^, and x^'s image is c0
    assert np.allclose(x[4, :4], [np.sqrt(0.5), 0, 0, np.sqrt(0.5)], atol=1e-7)
    assert np.allclose(r[4, 0:3], [0, 1, 0], atol=1e-6) and np.allclose(r[4, 3:6], [-1, 0, 0], atol=1e-6), r[4, :9]
    assert np.all(r32[:, 9:].view(np.uint32) == 0)


def qrot_terms(q, v):
    """v' = 2 (p.v) p + (2 w^2 - 1) v + 2 w (p x v), the expression hs_core.h documents: sum of |terms| per component."""
    w, p = q[:, 0:1], q[:, 1:4]
    i, j = [1, 2, 0], [2, 0, 1]
    return (2 * np.abs(p) * np.abs(p * v).sum(1, keepdims=True) + (2 * w * w + 1) * np.abs(v)
            + 2 * np.abs(w) * (np.abs(p[:, i] * v[:, j]) + np.abs(p[:, j] * v[:, i])))


def test_qrot_and_its_agreement_with_the_matrix():
    x, (_, r) = f64("QROT"), host("QROT")
    q, v = x[:, :4], x[:, 4:7]
    R, MR, m3b = m3_bound(q)
    ref = np.einsum("nij,nj->ni", R, v)
    bound = (K["QROT"] * U + 2 * off_unit(q)[:, None]) * qrot_terms(q, v)
    within(r[:, :3], ref, bound, "qrot")
    # sum_k c_k v_k of the same quaternions (M3_FROM_QUAT shares them), in float64, against qrot: within the two bounds
    assert np.array_equal(table("M3_FROM_QUAT")["x"][:, :4], table("QROT")["x"][:, :4])
    cols = host("M3_FROM_QUAT")[1][:, :9].reshape(-1, 3, 3)
    by_matrix = np.einsum("nki,nk->ni", cols, v)
    within(r[:, :3], by_matrix, bound + np.einsum("nij,nj->ni", m3b, np.abs(v)), "qrot against sum c_k v_k")


def test_world_inv_inertia():
    x, (_, r) = f64("WORLD_INV_INERTIA"), host("WORLD_INV_INERTIA")
    q, I = x[:, :4], x[:, 4:7]
    R, MR = rot_matrix(q)
    ref = np.einsum("nik,nk,njk->nij", R, I, R)
    M = np.einsum("nik,nk,njk->nij", MR, np.abs(I), MR)
    got = np.stack([r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5]], 1)
    idx = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])            # xx xy xz yy yz zz
    within(got, ref[:, idx[0], idx[1]], (K["WORLD_INV_INERTIA"] * U + 2 * off_unit(q)[:, None]) * M[:, idx[0], idx[1]], "world_inv_inertia")


# --------------------------------------------------------------------------------------------------------------------
# the fused multiply-adds are fused: exact known answers
# --------------------------------------------------------------------------------------------------------------------
def test_fused_multiply_adds_are_fused(oracle):
    """fma(a, b, -fl(a b)) = a b - fl(a b) exactly, the rounding error of the product: non-zero here, and zero from a
    separate multiply and add.  4 096 pairs per case; each case puts one fused multiply-add of one function on the spot."""
    n = 4096
    a, b, p, e = inexact_pairs(np.random.default_rng(SEED + 1), n)
    z = np.zeros(n, np.float32)
    e32 = e.astype(np.float32)

    def run(op, *parts):
        return oracle.core_eval(OPS[op], pack(n, *parts))

    def exact(got, want, what):
        assert np.all(want != 0)
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), what

    # cross: each component is fma(u, v, -(u' v'))
    exact(run("CROSS", z, a, a, z, b, b)[:, 0], e32, "cross.x")
    exact(run("CROSS", a, z, a, b, z, b)[:, 1], e32, "cross.y")
    exact(run("CROSS", a, a, z, b, b, z)[:, 2], e32, "cross.z")
    # dot = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)): the product p, then -a b from either fused multiply-add
    exact(run("DOT", a, -a, z, b, b, z)[:, 0], -e32, "dot, inner")
    exact(run("DOT", a, z, -a, b, z, b)[:, 0], -e32, "dot, outer")
    # dot_add: c = -p inside the innermost; the axis says which of the three carries a b
    for k in range(3):
        va, vb = [z, z, z], [z, z, z]
        va[k], vb[k] = a, b
        exact(run("DOT_ADD", *va, *vb, -p)[:, 0], e32, f"dot_add, axis {k}")
    # madd = fma(b, s, a), nmadd = fma(-b, s, a), per component
    exact(run("MADD", -p, -p, -p, a, a, a, b)[:, :3], np.stack([e32] * 3, 1), "madd")
    exact(run("NMADD", p, p, p, a, a, a, b)[:, :3], np.stack([-e32] * 3, 1), "nmadd")
    # cross_add.x = fma(a.y, b.z, fma(-a.z, b.y, c.x))
    exact(run("CROSS_ADD", z, z, a, z, b, z, p, z, z)[:, 0], -e32, "cross_add, inner")
    exact(run("CROSS_ADD", z, a, z, z, z, b, -p, z, z)[:, 0], e32, "cross_add, outer")
    # qmul.w = a.w b.w - a.x b.x - a.y b.y - a.z b.z: the product, then each of the three fused multiply-adds
    for k in (1, 2, 3):
        qa, qb = [a, z, z, z], [b, z, z, z]
        qa[k], qb[k] = a, b
        exact(run("QMUL", *qa, *qb)[:, 0], -e32, f"qmul.w, fma {k}")
    # qmul.x / .y / .z: a.w * b.k is the product, a.k * b.w (with a.k = -a) the fused multiply-add that cancels it
    for k in (1, 2, 3):
        qa, qb = [a, z, z, z], [b, z, z, z]
        qa[k], qb[k] = -a, b
        exact(run("QMUL", *qa, *qb)[:, k], -e32, f"qmul component {k}")


# --------------------------------------------------------------------------------------------------------------------
# quat_add_rotation, normalize, qnormalize, len
# --------------------------------------------------------------------------------------------------------------------
def test_quat_add_rotation_both_branches():
    x, (_, r) = f64("QUAT_ADD_ROTATION"), host("QUAT_ADD_ROTATION")
    q, d = x[:, :4], x[:, 4:7]
    w, v = q[:, 0:1], q[:, 1:4]
    # q + (0, dth) q / 2 with (0, d)(w, v) = (-d.v, w d + d x v)
    ref = q + 0.5 * np.concatenate([-(d * v).sum(1, keepdims=True), w * d + np.cross(d, v)], 1)
    n2 = (ref * ref).sum(1)
    res = r[:, :4]
    norm = np.sqrt((res * res).sum(1))
    within(res / norm[:, None], ref / np.sqrt(n2)[:, None], np.full(res.shape, 8 * U), "quat_add_rotation, direction")
    # The switch is n2 < 1.01f on a float32 n2 (four roundings): within 1e-6 of it either branch may run, and there only
    # the looser bound is asked.
    xs = n2 - 1.0
    small, exact = n2 < 1.01 - 1e-6, n2 > 1.01 + 1e-6
    side = table("QUAT_ADD_ROTATION")["n_side"]
    dth2 = (d * d).sum(1) / 4
    assert np.sum((dth2 < 0.01) & (dth2 > 0.01 - 1.01e-4) & small) >= 1000 and np.sum((dth2 > 0.01) & (dth2 < 0.01 + 1.01e-4) & exact) >= 1000
    assert side >= 1000 and np.sum(exact) > 20000 and np.sum(small) > 1000 and np.sqrt(dth2.max()) * 2 > 2.9
    loose = ~exact
    within(norm[loose], np.ones(loose.sum()), 0.375 * xs[loose] ** 2 + 8 * U, "quat_add_rotation, Newton step: | |q| - 1 |")
    within(norm[exact], np.ones(exact.sum()), np.full(exact.sum(), 4 * U), "quat_add_rotation, exact normalisation: | |q| - 1 |")
    # and below the switch it IS the Newton step, sqrt(1 + x)(1 - x / 2) = 1 - 3/8 x^2 + O(x^3): short by more than x^2 / 4
    # (x^2 / 4 >= 1e-6 > 8u from x = 0.002 on)
    newton = small & (xs > 0.002)
    assert newton.sum() > 1000 and np.all(norm[newton] < 1.0 - 0.25 * xs[newton] ** 2)


def test_len_normalize_qnormalize():
    x, (_, r) = f64("LEN"), host("LEN")
    ref = np.sqrt((x[:, :3] ** 2).sum(1))
    assert ref.min() > 0.99e-3 and ref.max() < 1.01e3
    within(r[:, 0], ref, 4 * U * ref, "len")
    for name, dim in (("NORMALIZE", 3), ("QNORMALIZE", 4)):
        x, (_, r) = f64(name), host(name)
        ref = x[:, :dim] / np.sqrt((x[:, :dim] ** 2).sum(1, keepdims=True))
        within(r[:, :dim], ref, 4 * U * np.abs(ref), name.lower())


# --------------------------------------------------------------------------------------------------------------------
# trigonometry (tolerances of tests/test_oracle_rng_math.py: 5e-7 for sin and cos, 1e-6 for atan, atan2 and asin)
# --------------------------------------------------------------------------------------------------------------------
def test_sincos_on_the_callers_domain_and_at_the_range_switches():
    x, (_, r) = f64("SINCOS")[:, 0], host("SINCOS")
    assert len(x) >= (1 << 20) + 17 * 19 and np.abs(x).max() < 7.7
    err_s, err_c = np.abs(r[:, 0] - np.sin(x)), np.abs(r[:, 1] - np.cos(x))
    print(f"sincos: {len(x)} inputs, worst sin error {err_s.max():.3e}, cos {err_c.max():.3e}")
    assert err_s.max() < 5e-7 and err_c.max() < 5e-7, (x[err_s.argmax()], x[err_c.argmax()])
    assert np.abs(r[:, 0] ** 2 + r[:, 1] ** 2 - 1.0).max() <= 4 * 5e-7


def test_atan_atan2_asin():
    x, (_, r) = f64("ATAN")[:, 0], host("ATAN")
    err = np.abs(r[:, 0] - np.arctan(x))
    print(f"atan: {len(x)} inputs, worst error {err.max():.3e}")
    assert err.max() < 1e-6, x[err.argmax()]
    x, (_, r) = f64("ASIN")[:, 0], host("ASIN")
    assert np.abs(x).max() == 1.0
    err = np.abs(r[:, 0] - np.arcsin(x))
    print(f"asin: {len(x)} inputs, worst error {err.max():.3e}")
    assert err.max() < 1e-6, x[err.argmax()]
    x, (_, r) = f64("ATAN2"), host("ATAN2")
    err = np.abs(r[:, 0] - np.arctan2(x[:, 0], x[:, 1]))
    print(f"atan2: {len(x)} inputs, worst error {err.max():.3e}")
    assert err.max() < 1e-6, x[err.argmax()]


def test_atan2_on_the_axes_and_at_signed_zeros():
    """hs_atan2f as written.  (-0, x < 0) returns +pi — `y >= 0.f` holds for -0 — where libm's atan2 returns -pi; and
    (-0, x > 0) returns +0 where libm returns -0.  The project's behaviour, on both compilers; no caller can tell: yaws
    of exactly +-pi are one pose."""
    t = table("ATAN2_AXES")
    got = host("ATAN2_AXES")[0][:, 0]
    assert np.array_equal(got.view(np.uint32), t["expect"].view(np.uint32)), list(zip(t["x"][:, 0], t["x"][:, 1], got))
    assert got[-1] == PI32 and np.arctan2(np.float32(-0.0), np.float32(-1.0)) < 0       # ours +pi, libm's -pi
    assert PI32.view(np.uint32) == 0x40490FDB


def test_quat_to_euler_of_a_yaw_and_the_gimbal_branch(oracle):
    yaw = f64("EULER_OF_YAW")[:, 0]
    assert len(yaw) == 65536 and np.abs(yaw).max() < np.pi
    r = host("EULER_OF_YAW")[1]
    err = np.abs(r[:, :3] - np.stack([0 * yaw, 0 * yaw, yaw], 1))
    print(f"quat_to_euler(quat_angle_axis_z(yaw)): worst error {err.max():.3e}")
    assert err.max() <= 2e-6, yaw[err.max(1).argmax()]
    # the two steps one by one give the same words as the composition
    q = host("QUAT_ANGLE_AXIS_Z")[0]
    assert np.array_equal(oracle.core_eval(OPS["QUAT_TO_EULER"], q).view(np.uint32), host("EULER_OF_YAW")[0].view(np.uint32))
    assert np.all(q[:, 1:3].view(np.uint32) == 0)
    half = yaw / 2
    assert np.abs(q[:, 0] - np.cos(half)).max() < 5e-7 and np.abs(q[:, 3] - np.sin(half)).max() < 5e-7
    # gimbal: |sinp| = |2 (w y - z x)| >= 1 returns exactly +-kPi/2.  h = the float above sqrt(1/2): 2 fl(h h) >= 1.
    h = np.nextafter(np.float32(np.sqrt(0.5)), np.float32(1))
    assert 2 * np.float32(h * h) >= 1
    g = oracle.core_eval(OPS["QUAT_TO_EULER"], pack(4, [[h, 0, h, 0], [h, 0, -h, 0], [-h, 0, h, 0], [0.8, 0, 0.8, 0]]))
    want = PI32 / np.float32(2)
    assert want.view(np.uint32) == 0x3FC90FDB
    assert np.array_equal(g[:, 1].view(np.uint32), np.float32([want, -want, -want, want]).view(np.uint32)), g[:, 1]
    # general unit quaternions: roll, pitch, yaw rebuild the rotation (z-y-x order), away from the gimbal poles
    x, (_, r) = f64("QUAT_TO_EULER"), host("QUAT_TO_EULER")
    R, _ = rot_matrix(x[:, :4])
    keep = np.abs(R[:, 2, 0]) < 0.999
    ro, pi_, ya = (r[keep, i] for i in range(3))
    assert keep.sum() > 60000
    assert np.abs(np.sin(pi_) + R[keep, 2, 0]).max() < 2e-6                                  # sinp = -R[2][0]
    assert np.abs(np.cos(pi_) * np.cos(ya) - R[keep, 0, 0]).max() < 4e-6 and np.abs(np.cos(pi_) * np.sin(ya) - R[keep, 1, 0]).max() < 4e-6
    assert np.abs(np.cos(pi_) * np.sin(ro) - R[keep, 2, 1]).max() < 4e-6 and np.abs(np.cos(pi_) * np.cos(ro) - R[keep, 2, 2]).max() < 4e-6


# --------------------------------------------------------------------------------------------------------------------
# RNG: exact
# --------------------------------------------------------------------------------------------------------------------
KATS = [((0, 0), (0, 0), (0x6b200159, 0x99ba4efe)),
        ((0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x1cb996fc, 0xbb002be7)),
        ((0x13198a2e, 0x03707344), (0x243f6a88, 0x85a308d3), (0xc4923a9c, 0x483df7a0))]


def test_the_integer_restatement_passes_the_known_answer_vectors():
    for key, ctr, exp in KATS:                                    # Random123's vectors, as tests/test_oracle_rng_math.py
        assert threefry2x32(key[0], key[1], ctr[0], ctr[1]) == exp
        got = threefry2x32(*(np.array([v], np.uint64) for v in (*key, *ctr)))
        assert (int(got[0][0]), int(got[1][0])) == exp


def test_bits32_sample_i32_sample_uniform_are_exact():
    t = table("RNG_BITS32")
    bits = rng_bits32(*t["key"], t["count"])
    after = (t["count"] + 1) & M32
    assert int(t["count"][2]) == M32 and int(after[2]) == 0       # count 0xFFFFFFFF wraps
    out = host("RNG_BITS32")[0].view(np.uint32)
    assert np.array_equal(out[:, 0], bits.astype(np.uint32)) and np.array_equal(out[:, 1], after.astype(np.uint32))
    assert np.all(out[:, 2:] == 0)
    out = host("SAMPLE_UNIFORM")[0]
    want = ((bits >> 8).astype(np.float64) * 2.0 ** -24).astype(np.float32)          # 24 bits: exact
    assert np.array_equal(out[:, 0].view(np.uint32), want.view(np.uint32)) and np.all(out[:, 0] < 1) and np.all(out[:, 0] >= 0)
    assert np.array_equal(out[:, 1].view(np.uint32), after.astype(np.uint32))
    t = table("SAMPLE_I32")
    want = rng_sample_i32(bits.astype(np.int64), t["a"], t["b"])
    assert np.all((want >= t["a"]) & ((want < t["b"]) | (t["a"] == t["b"]))) and np.all(want[t["a"] == t["b"]] == t["a"][t["a"] == t["b"]])
    out = host("SAMPLE_I32")[0].view(np.int32)
    assert np.array_equal(out[:, 0].astype(np.int64), want)
    assert np.array_equal(out[:, 1].view(np.uint32), after.astype(np.uint32))
    wide = (t["b"] - t["a"]) == (1 << 31) - 1
    assert wide.sum() >= 2 and np.any(want[wide] != t["a"][wide])


def test_sample_uniform_stays_below_one_at_the_largest_draw(oracle):
    """A (key, count) whose draw has all of its top 24 bits set, found by search in the restatement: key (7, 9), counts
    from 0 on, 2^20 at a time (this key's first such count lies in the first chunk; one in 2^24 draws is one)."""
    found = None
    for chunk in range(64):
        cnt = np.arange(chunk << 20, (chunk + 1) << 20, dtype=np.uint64)
        bits = rng_bits32(np.array([7], np.uint64), np.array([9], np.uint64), cnt)
        hit = np.flatnonzero((bits >> 8) == 0xFFFFFF)
        if len(hit):
            found = int(cnt[hit[0]])
            break
    assert found is not None
    assert rng_bits32(7, 9, found) >> 8 == 0xFFFFFF               # in Python integers
    out = oracle.core_eval(OPS["SAMPLE_UNIFORM"], words(1, [7], [9], [found]))
    assert out[0, 0] == np.float32(1.0 - 2.0 ** -24) and out[0, 0] < 1
    top = oracle.core_eval(OPS["SAMPLE_I32"], words(1, [7], [9], [found], [-3], [11])).view(np.int32)
    assert top[0, 0] == 10                                        # the largest draw stays inside [a, b)


# --------------------------------------------------------------------------------------------------------------------
# aabb_overlaps: exact
# --------------------------------------------------------------------------------------------------------------------
def test_aabb_overlaps_open_boxes():
    t, x = table("AABB_OVERLAPS"), f64("AABB_OVERLAPS")
    got = host("AABB_OVERLAPS")[0].view(np.int32)[:, 0]
    n = t["n_hand"]
    assert n == 7 + 12
    for name, g, want in zip(t["hand_names"], got[:n], t["hand_expect"]):
        assert g == want, name
    # boxes overlap when their interiors meet: the intersection has a positive extent on every axis
    a_lo, a_hi, b_lo, b_hi = x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12]
    want = np.all(np.minimum(a_hi, b_hi) - np.maximum(a_lo, b_lo) > 0, axis=1)
    assert np.array_equal(got, want.astype(np.int32)) and 0.05 < want[n:].mean() < 0.95


# --------------------------------------------------------------------------------------------------------------------
# rays against one hull in its own frame
# --------------------------------------------------------------------------------------------------------------------
def box_planes(e):
    n = np.concatenate([np.eye(3), -np.eye(3)])[None].repeat(len(e), 0)         # [case, face, 3]
    return n, np.concatenate([e, e], 1)


def wedge_planes():
    """Outward unit normals and offsets of the ramp's five faces, from the reference's collision mesh (tests/golden/hulls.npz)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "hulls.npz"))
    v, faces = g["ramp_v"].astype(np.float64), g["ramp_f"]
    n, off = [], []
    for f in faces:
        p = v[[i for i in f if i >= 0]]
        m = np.cross(p[1] - p[0], p[2] - p[0])
        m /= np.linalg.norm(m)
        if m @ (p[0] - v.mean(0)) < 0:
            m = -m
        n.append(m); off.append(m @ p[0])
    return np.array(n), np.array(off)


def clip(o, d, n, off):
    """float64 half-space clipping with the header's conventions: the closest front-face entry; a start inside returns
    -1; a direction with n.d == 0 (+-0 components) is parallel, and then a start ON the plane counts as inside.
    Returns (t or -1, near): near marks the cases within 1e-4 (relative) of a decision — entry = exit, entry = 0, a start
    on a plane it runs parallel to — where rounding may flip either side; and the error scale (|o| + |e|) / min |n.d|."""
    dist = np.einsum("nfk,nk->nf", n, o) - off
    dn = np.einsum("nfk,nk->nf", n, d)
    par = dn == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(par, 0.0, -dist / dn)
    tn = np.where(~par & (dn < 0), t, -np.inf).max(1)
    tf = np.where(~par & (dn > 0), t, np.inf).min(1)
    miss = np.any(par & (dist > 0), axis=1)
    hit = ~miss & (tn <= tf) & (tn >= 0)
    return np.where(hit, tn, -1.0), tn, tf, dist, par


def ray_case(name):
    x, (_, r) = f64(name), host(name)
    o, d = x[:, 0:3], x[:, 3:6]
    if name == "RAY_BOX_LOCAL":
        e = x[:, 6:9]
        n, off = box_planes(e)
        size = np.linalg.norm(e, axis=1)
    else:
        wn, woff = wedge_planes()
        n, off = wn[None].repeat(len(x), 0), woff[None].repeat(len(x), 0)
        size = np.full(len(x), np.linalg.norm([1.0, 2.0, 1.0]))                 # the farthest vertex
    ref, tn, tf, dist, par = clip(o, d, n, off)
    # min |d_k| over the non-zero direction components, a component being taken along a face normal: t = -dist / (n.d),
    # and dist carries an error of a few u (|o| + |e|).  For the box, and for the wedge's four axis faces, n.d IS d_x,
    # d_y or d_z.  The wedge's slope has n = (0, -2, 3) / sqrt(13), which is no float: its n.d can be far smaller than
    # every d_k (a ray grazing the slope), and the float32 normal alone then moves t by 2^-25 |d| / |n.d| relative to
    # the mesh's exact plane.  With min |d_k| over x, y, z alone, 1 hit of the 14 656 here errs by 1.50 times the bound
    # (n.d = -0.044, d = (-14.5, -4.7, -3.2), |t - reference| = 2.8e-6 at t = 0.70), no fault of the arithmetic.
    ad = np.abs(np.einsum("nfk,nk->nf", n, d))
    scale = (np.linalg.norm(o, axis=1) + size) / np.where(ad > 0, ad, np.inf).min(1)
    reach = np.linalg.norm(o, axis=1) + size
    near = (np.abs(tn - tf) <= 1e-4 * scale) | (np.abs(tn) <= 1e-4 * scale) | np.any(par & (np.abs(dist) <= 1e-4 * reach[:, None]), axis=1)
    return r[:, 0], ref, near, scale


@pytest.mark.parametrize("name", ["RAY_BOX_LOCAL", "RAY_WEDGE_LOCAL"])
def test_rays_against_float64_clipping(name):
    got, ref, near, scale = ray_case(name)
    share = near.mean()
    hits = (ref >= 0) & ~near
    print(f"{name}: {len(ref)} rays, {hits.sum()} hits, left out {100 * share:.2f} %")
    assert share < 0.02 and hits.mean() > 0.2 and ((ref < 0) & ~near).mean() > 0.2
    keep = ~near
    assert np.array_equal(got[keep] >= 0, ref[keep] >= 0), np.flatnonzero(keep & ((got >= 0) != (ref >= 0)))[:8]
    assert np.all(got[keep & (ref < 0)] == -1.0)
    within(got[hits], ref[hits], 8 * U * scale[hits], name)


def test_rays_hand_written_exact_cases(oracle):
    one = (1, 1, 1)
    box = [  # o, d, e, t
        ((-3, 0, 0), (1, 0, 0), one, 2), ((-3, 0.5, -0.5), (2, 0, 0), one, 1), ((0, 0, 5), (0, 0, -1), one, 4),
        ((0, 4, 0), (-0.0, -0.5, 0), (4, 0.5, 1), 7),                             # axis-parallel, with a -0 component
        ((-3, 2, 0), (1, 0, 0), one, -1), ((-3, 0, -1.5), (1, 0, -0.0), one, -1),  # parallel, outside a slab
        ((1, 0, 0), (1, 0, 0), one, -1),                                          # starts on a face, points out
        ((1, 0, 0), (-1, 0, 0), one, 0), ((0.5, -1, 0.5), (0, 2, 0), one, 0),     # starts on a face, points in: hit at 0
        ((-3, 1, 1), (1, 0, 0), one, 2), ((4, -0.5, 5), (0, 0, -2), (4, 0.5, 1), 2),   # along an edge: on two faces = inside
        ((0, 0, 0), (1, 0, 0), one, -1), ((0.5, 0.5, -0.5), (1, 2, -1), one, -1),  # starts inside
        ((-3, -3, 0), (1, 1, 0), one, 2), ((-2, -3, -4), (1, 2, 4), (1, 1, 2), 1),  # diagonal, exact quotients
        ((3, 0, 0), (1, 0, 0), one, -1),                                          # behind the start
    ]
    x = pack(len(box), [[*o, *d, *e] for o, d, e, _ in box])
    got = oracle.core_eval(OPS["RAY_BOX_LOCAL"], x)[:, 0]
    assert np.array_equal(got, np.float32([t for *_, t in box])), got
    # the wedge: -1 <= x <= 1, y <= 1, z >= -1, and the slope 3 z - 2 y <= 1 from (y, z) = (-2, -1) up to (1, 1)
    wedge = [  # o, d, t, exact?
        ((-3, 0, -0.5), (1, 0, 0), 2, True), ((3, 0.5, 0), (-2, 0, 0), 1, True),  # the two sides
        ((0, 0, -4), (0, 0, 1), 3, True), ((0.5, -1, -3), (0, 0, 2), 1, True),    # from below
        ((0, 5, 0), (0, -1, 0), 4, True), ((0, 5, -0.5), (-0.0, -2, 0), 2, True),  # the back face y = 1
        ((0, 1, 0), (0, 1, 0), -1, True), ((0, 1, 0), (0, -1, 0), 0, True),       # on the back face: out, in
        ((1, 1, -3), (0, 0, 1), 2, True),                                         # along the edge x = 1, y = 1
        ((0, 0, 0), (0, 0, 1), -1, True), ((0, -3, 0), (0, 0, 1), -1, True),      # inside; beside the toe
        ((0, -0.5, 5), (0, 0, -1), 5, False), ((0, 1, 5), (0, 0, -1), 4, False),  # down onto the slope: z = (1 + 2 y) / 3
        ((0.5, -5, 0), (0, 1, 0), 4.5, False),                                    # level into the slope: y = (3 z - 1) / 2
        ((0, -5, 3), (0, 3, -2), 1.5, False),                                     # obliquely onto the slope at (0, -0.5, 0)
        ((0, -2, 1), (0, 3, 2), -1, True),                                        # along the slope (to a rounding of its normal), above it
    ]
    x = pack(len(wedge), [[*o, *d] for o, d, *_ in wedge])
    got = oracle.core_eval(OPS["RAY_WEDGE_LOCAL"], x)[:, 0].astype(np.float64)
    for (o, d, t, exact), g in zip(wedge, got):
        if exact:
            assert g == t, (o, d, t, g)
        else:   # the slope's normal (-2, 3) / sqrt(13) is no float: the bound of the random rays, with n.d for the component
            nd = abs(-2 * d[1] + 3 * d[2]) / np.sqrt(13.0)
            assert abs(g - t) <= 8 * U * (np.linalg.norm(o) + np.linalg.norm([1, 2, 1])) / nd, (o, d, t, g)


# --------------------------------------------------------------------------------------------------------------------
# tests/host/core_check.cpp: the same table in a stand-alone program, under the sanitizers where the toolchain has them
# --------------------------------------------------------------------------------------------------------------------
SRC = os.path.join(ROOT, "tests", "host", "core_check.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "marl-hideandseek_amd", "csrc"),
         "-I", os.path.join(ROOT, "oracle")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def checksum(out):
    w = out.view(np.uint32).astype(np.uint64).ravel()
    i = np.arange(len(w), dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(((w + np.uint64(0x9E3779B97F4A7C15)) * (np.uint64(2) * i + np.uint64(1))).sum(dtype=np.uint64))


def test_core_check_program_agrees_with_the_oracle_library(oracle, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("core_check")
    prog = str(d / "core_check")
    if subprocess.run([cxx] + FLAGS + SANITIZE + [SRC, "-o", prog], capture_output=True).returncode != 0:
        subprocess.run([cxx] + FLAGS + [SRC, "-o", prog], check=True)              # (no sanitizer runtimes here)
    want, recs = {}, []
    for name in all_inputs():
        op = op_of(name)
        x = subset(table(name)["x"], 8192)
        rec = np.empty((len(x), 17), np.uint32)
        rec[:, 0] = op
        rec[:, 1:] = x.view(np.uint32)
        recs.append(rec)
        want.setdefault(op, []).append(x)
    path = str(d / "cases.bin")
    np.concatenate(recs).tofile(path)
    r = subprocess.run([prog, "file", path], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0 and "file OK" in r.stdout, r.stdout + r.stderr
    lines = {int(l.split()[1]): l.split() for l in r.stdout.splitlines() if l.startswith("op ")}
    assert sorted(lines) == sorted(OPS.values())
    for op, xs in want.items():
        x = np.concatenate(xs)
        assert int(lines[op][3]) == len(x)
        assert int(lines[op][5], 16) == checksum(oracle.core_eval(op, x)), op
