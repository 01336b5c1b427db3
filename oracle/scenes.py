"""ORACLE — TEST INFRASTRUCTURE ONLY.

Crafted scenes through the Checkpoint record (src/sim.hpp:283-313): a record restores pos / rot / lin / ang / locked of
every box and ramp, and the pose of every agent, verbatim on both sides (oracle/hs_ref_ckpt.hpp load_checkpoint_system,
k_load_ckpt), so a test can put any hull in any pose in front of the kernels and of the oracle alike.  `inject` does
that for a lockstep.Pair, `inject_sim` for a HideAndSeekSimulator alone, `inject_ref` for a RefSim alone.

The float64 geometry below (numpy only) is the tests' own: half-spaces from the face loops of the reference's collision
meshes in tests/golden/hulls.npz, never from the oracle's or the device's hull tables.  No torch or gpu_hideseek import
at module level.
"""
import os

import numpy as np

BODY = [("pos", "<f4", 3), ("rot", "<f4", 4), ("lin", "<f4", 3), ("ang", "<f4", 3)]
OBJ = np.dtype(BODY + [("team", "<u4"), ("locked", "u1"), ("pad", "u1", 3)])
AGENT = np.dtype(BODY + [("grab_idx", "<i4"), ("r1", "<f4", 3), ("r2", "<f4", 3), ("att1", "<f4", 4), ("att2", "<f4", 4),
                         ("sep", "<f4")])
CKPT = np.dtype([("key", "<u4", 2), ("scores", "<i4", 2), ("step", "<i4"), ("agents", AGENT, 6), ("boxes", OBJ, 9),
                 ("ramps", OBJ, 2), ("nh", "<i4"), ("ns", "<i4"), ("nb", "<i4"), ("nr", "<i4")])
assert CKPT.itemsize == 1392

CUBE, RAMP, BOX, AGENT_OBJ = 2, 6, 7, 4      # SimObject (src/sim.hpp:78-88); hiders and seekers share the agent mesh
RAMP_SLOT0, AGENT_SLOT0, SLOTS = 9, 11, 17   # body slots of debug_bodies(): boxes 0-8, ramps 9-10, agents 11-16
WALL_TOP = 2.5                               # a wall is the box [cx +- hx] x [cy +- hy] x [0, 2.5]

_HULLS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "hulls.npz")
_MESH = {CUBE: "cube", RAMP: "ramp", BOX: "elongated", AGENT_OBJ: "agent", 5: "agent"}
_local = {}


# ------------------------------------------------------------------------------------------------ float64 geometry
def quat_to_matrix(q):
    """The rotation matrix of the quaternion (w, x, y, z), float64; q is used as given (not normalised)."""
    w, x, y, z = (float(c) for c in q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], np.float64)


def random_quats(rng, n):
    """n unit quaternions, uniform on the rotation group."""
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def yaw_quat(yaw):
    return np.array([np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)])


def local_hull(kind):
    """(vertices [nv, 3], face normals [nf, 3], face offsets [nf]) of a hull in its own frame, n . x <= d inside, from
    the vertex list and the face loops of tests/golden/hulls.npz (Newell normals; the loops are outward)."""
    if kind not in _local:
        g = np.load(_HULLS)
        name = _MESH[kind]
        v = g[f"{name}_v"].astype(np.float64)
        N, D = [], []
        for loop in g[f"{name}_f"].tolist():
            p = v[[i for i in loop if i >= 0]]
            n = sum(np.cross(p[i], p[(i + 1) % len(p)]) for i in range(len(p)))
            n = n / np.linalg.norm(n)
            assert (v @ n <= p[0] @ n + 1e-12).all(), "a face loop of a convex mesh, outward"
            N.append(n); D.append(float(p[0] @ n))
        _local[kind] = (v, np.array(N), np.array(D))
    return _local[kind]


def hull_vertices(kind, pos, rot):
    """World-space vertices [nv, 3] of a placed hull, float64."""
    return local_hull(kind)[0] @ quat_to_matrix(rot).T + np.asarray(pos, np.float64)


def half_spaces(kind, pos, rot):
    """World-space half-spaces N . x <= D of a placed cube, elongated box or ramp wedge, float64."""
    _, n, d = local_hull(kind)
    N = n @ quat_to_matrix(rot).T
    return N, d + N @ np.asarray(pos, np.float64)


def clip_ray(N, D, o, d):
    """The ray o + t d against the half-spaces N . x <= D, float64: (t, margin).  t is the closest front-face entry, or
    -1.0 for a miss and for a ray that starts inside; margin = min(|t_far - t_near|, |t_near|) tells how far the case is
    from grazing the hull or from starting on its surface (1.0 when one of the two does not exist)."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    den, num = N @ d, D - N @ o
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = num / den
    tn = np.max(np.where(den < -1e-12, tt, -np.inf))
    tf = np.min(np.where(den > 1e-12, tt, np.inf))
    inside_slabs = np.all(num[np.abs(den) <= 1e-12] >= 0)
    t = float(tn) if (inside_slabs and tn <= tf and tn >= 0) else -1.0
    margin = float(min(abs(tf - tn), abs(tn))) if np.isfinite(tn) and np.isfinite(tf) else 1.0
    return t, margin


def aabbs(bodies, meta):
    """World AABBs (lo, hi) [N, 17, 3] of the hulls in a debug_bodies() dump, float64; dead slots get an empty box."""
    lo = np.full(bodies.shape[:2] + (3,), np.inf)
    hi = np.full(bodies.shape[:2] + (3,), -np.inf)
    for w in range(bodies.shape[0]):
        for i in range(bodies.shape[1]):
            if meta[w, i, 0] in _MESH:
                v = hull_vertices(int(meta[w, i, 0]), bodies[w, i, :3], bodies[w, i, 3:7])
                lo[w, i], hi[w, i] = v.min(0), v.max(0)
    return lo, hi


def wall_clearance(walls, count, x, y):
    """Distance in the plane from (x, y) (arrays allowed) to the nearest of one world's first `count` wall boxes."""
    w = np.asarray(walls[:count], np.float64)
    dx = np.maximum(np.abs(np.asarray(x, np.float64)[..., None] - w[:, 0]) - w[:, 2], 0)
    dy = np.maximum(np.abs(np.asarray(y, np.float64)[..., None] - w[:, 1]) - w[:, 3], 0)
    return np.hypot(dx, dy).min(-1)


def open_spot(walls, count, reach=12.0, step=0.5):
    """The grid point (x, y) with |x|, |y| <= reach that is farthest from every wall of one world, and that distance."""
    g = np.arange(-reach, reach + step / 2, step)
    X, Y = np.meshgrid(g, g, indexing="ij")
    c = wall_clearance(walls, count, X, Y)
    k = np.unravel_index(np.argmax(c), c.shape)
    return float(X[k]), float(Y[k]), float(c[k])


def put(rec, pos, rot=(1, 0, 0, 0), lin=(0, 0, 0), ang=(0, 0, 0), locked=None):
    """Write one body of a record (an element of rec["boxes"], rec["ramps"] or rec["agents"])."""
    rec["pos"] = pos; rec["rot"] = rot; rec["lin"] = lin; rec["ang"] = ang
    if locked is not None:
        rec["locked"] = 1 if locked else 0


def slot_record(rec, slot):
    """The record element behind body slot `slot` (0-8 a box, 9-10 a ramp) of one world's record."""
    return rec["boxes"][slot] if slot < RAMP_SLOT0 else rec["ramps"][slot - RAMP_SLOT0]


# ------------------------------------------------------------------------------------------------ save, edit, load
def _records(raw):
    return np.ascontiguousarray(raw).copy().view(CKPT).reshape(-1)


def _raw(rec, n):
    return np.ascontiguousarray(rec).view(np.uint8).reshape(n, CKPT.itemsize)


def inject_ref(ref, edit):
    """The oracle alone: save every world, edit(records, meta) on a copy, load it, clear the control words."""
    ref.tensor("ckpt_ctrl")[:] = 1
    ref.save_checkpoints()
    rec = _records(ref.tensor("ckpt"))
    edit(rec, ref.bodies()[1])
    ref.tensor("ckpt")[:] = _raw(rec, ref.N)
    ref.tensor("ckpt_ctrl")[:] = 1
    ref.load_checkpoints()
    ref.tensor("ckpt_ctrl")[:] = 0
    return rec


def _sim_save(sim):
    import torch
    ctrl = sim.ckpt_ctrl_tensor().to_torch().view(torch.int32)
    ck = sim.ckpt_tensor().to_torch()
    ctrl[:] = 1
    sim.save_checkpoints()
    return ctrl, ck, ck.cpu().numpy()


def _sim_load(sim, ctrl, ck, raw):
    import torch
    ck.copy_(torch.from_numpy(raw).to(ck.device))
    ctrl[:] = 1
    sim.load_checkpoints()
    ctrl.zero_()


def inject_sim(sim, edit):
    """A HideAndSeekSimulator alone (no oracle): save every world, edit(records, meta) on a copy, load it."""
    ctrl, ck, raw = _sim_save(sim)
    rec = _records(raw)
    edit(rec, sim.debug_bodies()[1])
    _sim_load(sim, ctrl, ck, _raw(rec, sim.num_worlds))
    return rec


def inject(pair, edit):
    """Both sides of a lockstep.Pair: save every world and require byte-equal records; edit(records, meta) once on one
    copy (meta = debug_bodies()[1]: the hull kind of every slot); write the same bytes to both sides, load, clear the
    control words; then every exported tensor (the load re-runs the observations), bodies and walls must agree."""
    sim, ref = pair.sim, pair.ref
    ctrl, ck, raw = _sim_save(sim)
    ref.tensor("ckpt_ctrl")[:] = 1
    ref.save_checkpoints()
    assert np.array_equal(raw, ref.tensor("ckpt")), "saved records differ"
    rec = _records(raw)
    edit(rec, sim.debug_bodies()[1])
    raw = _raw(rec, ref.N)
    ref.tensor("ckpt")[:] = raw
    ref.tensor("ckpt_ctrl")[:] = 1
    ref.load_checkpoints()
    ref.tensor("ckpt_ctrl")[:] = 0
    _sim_load(sim, ctrl, ck, raw)
    pair.check("loaded")
    return rec
