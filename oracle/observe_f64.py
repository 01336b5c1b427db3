"""ORACLE — TEST INFRASTRUCTURE ONLY.

A float64 numpy restatement of the reference's observation stage, written from src/sim.cpp and from nothing of this
project's own observe code: euler angles, relative position / velocity and lock observations (sim.cpp:372-446),
collectObservationsSystem (:448-565), computeVisibilitySystem's CPU branch (:567-605, :663-708), lidarSystem (:712-745),
rewardsVisSystem / outputRewardsDonesSystem (:763-841) and globalPositionsDebugSystem (:895-941).  It is a pure function of
a dumped world state -- RefSim.bodies() / walls() or HideAndSeekSimulator.debug_bodies() / debug_walls(), the `self_type`
export and the agent count -- and knows nothing of lanes, culls or atomics: every ray is tested against every hull, wall
and plane of its world.  Float32 inputs are widened once; every operation after that is float64 with numpy's libm.  With
dtype=np.float32 the very same code runs in float32 (numpy's float32 arithmetic and trigonometry): the tests take their
tolerances from the difference between the two.

Layout of the inputs (the dumps' own): body slots 0-8 are boxes[0..8], 9-10 ramps[0..1], 11 + i the body of agent
interface i; meta = (objType, response, owner) with SimObject / ResponseType / OwnerTeam numbering (sim.hpp:78-88,
127-132; Static = 2); info = (numWalls, numPlanes, numActiveBoxes, numActiveRamps, numHiders, numSeekers, curEpisodeStep,
seekersFirst).  Agent rows are world * A + interface, as exported.

Geometry.  Hulls are the half-spaces of scenes.local_hull (the reference's collision meshes), which a
unit quaternion places as scenes.half_spaces does.  A wall is the box [cx +- hx] x [cy +- hy] x [0, 2.5].  Planes (level_gen.cpp:68-71):
every level has the floor, normal +z through the origin (:294-295, :346, :387, :402, :413, :455, :492); the debug levels 7
and 8 add x = -20 with normal +x and x = +20 with normal -x (:456-459, :493-496), the levels with info[1] == 3.  No debug
level other than 5 and 6 makes an agent (:336-499), so levels 2-4, 7 and 8 have no observation row to compute.

What the snapshot cannot settle, because Madrona itself is not part of it:
  * Madrona's vector algebra.  inv() is the conjugate, a * b the Hamilton product, fwd = +y, right = +x, up = +z, and
    q.rotateVec(v) = 2 (p . v) p + (2 w^2 - 1) v + 2 w (p x v) with p = (x, y, z), the form of Madrona's published
    math library.  For a unit quaternion every form of the rotation agrees; the simulator's quaternions are not exactly
    of unit length (|q|^2 - 1 reaches 7e-5 under the 240 N m torques of ZeroAgentVelocity), and there the forms differ by
    that much times the length of v -- millimetres at 50 m -- so the form is part of what is restated, and a ray is
    taken into a hull's frame by the same rotateVec (of the inverse rotation), as Madrona's ray tracer does, not by a
    matrix.
  * traceRay is Madrona's BVH.  ADOPTED, NOT PINNED, as DESIGN.md "Engine decisions" states them: the closest
    front-face entry with 0 <= t <= t_max in units of |d|; a ray that starts inside a hull does not hit it; ties keep
    the lower body id (a tie has a zero gap, so no test compares one).

What a single dump does not hold, and the caller therefore passes in:
  * who is grabbing (GrabData lives outside the body columns): `grabbing` [N * A], copied into self_data[12] and
    agent_data[.., 13];
  * the hider team's reward flag.  resetSystem sets it to 1 (:199), the observation pass that follows lowers it to -1 if a
    seeker sees a hider (:700-705), and the NEXT step's rewardsVisSystem lowers it again on the poses after physics
    (:799-801) before outputRewardsDonesSystem reads it.  So the reward of a dump depends on the visibility of the dump
    one step earlier: `prev` is this function's result for that dump.  Without it, and in the step of a reset
    (curEpisodeStep == 0), `reward_written` is False.

Not written by the reference, and marked so instead of guessed: prep_counter after step 96 (:462-464,
`prep_written`), the entries the double increment at :937-939 skips in global_positions (`global_written`), and every
row of an inactive agent (`active`).

Decision margins (out["margin"]): every discrete or ray-derived value comes with the distance by which float64 took the
decision -- |cos_angle - cos 67.5 deg|; along a ray the gap between the first and the second surface, the least
|min(t_far - t_near, t_near)| over the hulls that begin no later than the first hit (how far a hull is from being grazed,
or the origin from lying on it) and |t - t_max|, in metres; 1 - |sinp| for every euler triple; ||x| - 18| for the reward.
`robust` turns them into masks for given epsilons.
"""
import numpy as np

import scenes

PREP_STEPS, EPISODE_LEN = 96, 240                          # sim.cpp:16-17
MAX_BOXES, MAX_RAMPS, MAX_AGENTS = 9, 2, 6                   # sim.hpp:38-41
SEEKER, HIDER = 0, 1                                         # AgentType, sim.hpp:138-141
STATIC, OWNER_HIDER = 2, 2
LIDAR_RAYS, LIDAR_RANGE = 30, 200.0                          # sim.cpp:728, 738
COS_FOV = float(np.cos(np.radians(135.0 / 2.0)))             # sim.cpp:582, 767
WALL0, PLANE0 = scenes.SLOTS, scenes.SLOTS + 36              # ids of the surfaces a ray can hit: body slot, wall, plane
_SIZE = {scenes.BOX: (8.0, 1.5, 2.0), scenes.CUBE: (2.0, 2.0, 2.0)}   # level_gen.cpp:150, 191
_FACES = 6


# ---------------------------------------------------------------------------------------------- quaternions, in dtype
def _unit(q):
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def _matrix(q):
    """Rotation matrices [..., 3, 3] of quaternions (w, x, y, z) [..., 4]; scenes.quat_to_matrix, vectorised."""
    w, x, y, z = (q[..., i] for i in range(4))
    m = np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], -1)
    return m.reshape(q.shape[:-1] + (3, 3))


def _rot(q, v):
    """q.rotateVec(v) = 2 (p . v) p + (2 w^2 - 1) v + 2 w (p x v) with p = (x, y, z); q and v broadcast."""
    p, w = q[..., 1:], q[..., :1]
    return 2 * (p * v).sum(-1, keepdims=True) * p + (2 * w * w - 1) * v + 2 * w * np.cross(p, v)


def _conj(q):
    return q * np.array([1, -1, -1, -1], q.dtype)


def _qmul(a, b):
    aw, ax, ay, az = (a[..., i] for i in range(4))
    bw, bx, by, bz = (b[..., i] for i in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def _euler(q):
    """quatToEuler (sim.cpp:372-399) -> (roll, pitch, yaw) [..., 3] and 1 - |sinp|, the distance to the clamp."""
    w, x, y, z = (q[..., i] for i in range(4))
    roll = np.arctan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y))
    sinp = 2 * (w * y - z * x)
    half_pi = q.dtype.type(np.pi) / 2
    with np.errstate(invalid="ignore"):
        pitch = np.where(np.abs(sinp) >= 1, np.copysign(half_pi, sinp), np.arcsin(np.clip(sinp, -1, 1)))
    yaw = np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    return np.stack([roll, pitch, yaw], -1), 1 - np.abs(sinp)


def _relative(p0, q0, v0, w0, p, q, v, w):
    """computeRelativePosVelObs (sim.cpp:401-420) of bodies (p, q, v, w) [K, ..] in the frame of (p0, q0, v0, w0):
    [K, 12] and the euler margin [K]."""
    to_frame = _conj(q0)
    e, m = _euler(_unit(_qmul(to_frame, q)))
    return np.concatenate([_rot(to_frame, p - p0), e, _rot(to_frame, v - v0), _rot(to_frame, w - w0)], -1), m


# ------------------------------------------------------------------------------------------------------- ray casting
def _surfaces(b, meta, walls, info, dt):
    """Half-spaces n . x <= d of everything a ray can hit in one world, each in its own frame: (n [K, 6, 3], d [K, 6],
    pos [K, 3], rot [K, 4], ids [K]).  Walls and planes are given in the world frame (identity pose).  Unused face rows
    are 0 . x <= 1, which no ray ever leaves."""
    N, D, P, Q, ids = [], [], [], [], []
    origin, ident = np.zeros(3, dt), np.array([1, 0, 0, 0], dt)

    def add(n, d, i, pos=origin, rot=ident):
        pn = np.zeros((_FACES, 3), dt); pd = np.ones(_FACES, dt)
        pn[:len(d)] = n; pd[:len(d)] = d
        N.append(pn); D.append(pd); P.append(pos); Q.append(rot); ids.append(i)
    for s in range(scenes.SLOTS):
        kind = int(meta[s, 0])
        if kind in scenes._MESH:
            _, n, d = scenes.local_hull(kind)
            add(n.astype(dt), d.astype(dt), s, b[s, :3], b[s, 3:7])
    for k in range(int(info[0])):
        cx, cy, hx, hy = walls[k]
        n = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dt)
        add(n, np.array([cx + hx, -(cx - hx), cy + hy, -(cy - hy), scenes.WALL_TOP, 0], dt), WALL0 + k)
    planes = [((0, 0, 1), 0.0)] + ([((1, 0, 0), -20.0), ((-1, 0, 0), -20.0)] if int(info[1]) == 3 else [])
    assert int(info[1]) == len(planes), f"a level with {int(info[1])} planes is none of level_gen.cpp's"
    for p, (n, d) in enumerate(planes):       # the solid side of a plane is n . x <= d
        add(np.array([n], dt), np.array([d], dt), PLANE0 + p)
    return np.stack(N), np.stack(D), np.stack(P), np.stack(Q), np.array(ids)


def _trace(surfaces, o, d, t_max):
    """Rays o + t d [R, 3] against all surfaces: per ray the id of the closest front-face entry with 0 <= t <= t_max (-1:
    none) and its t, then the margins gap / graze / far in units of t (see the module docstring).  A ray is taken into
    a hull's frame as any vector is, by rotateVec of the inverse rotation; t is the same in both frames."""
    N, D, P, Q, ids = surfaces
    to_local = _conj(Q)[None]
    ol = _rot(to_local, o[:, None, :] - P[None])
    dl = _rot(to_local, np.broadcast_to(d[:, None, :], ol.shape))
    inf = np.inf
    den = np.einsum("kfc,rkc->rkf", N, dl)
    num = D[None] - np.einsum("kfc,rkc->rkf", N, ol)
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = num / den
        tn = np.where(den < 0, tt, -inf).max(-1)
        tf = np.where(den > 0, tt, inf).min(-1)
        m = np.minimum(tf - tn, tn)                           # >= 0: entered from outside, in front of the origin
    out = (den == 0) & (num < 0)                              # parallel to a face and outside it: never inside
    m = np.where(out.any(-1), -np.where(out, -num, inf).min(-1), m)
    hit = (m >= 0) & (tn <= t_max)
    th = np.where(hit, tn, inf)
    order = np.argsort(th, axis=1, kind="stable")             # stable: of equal t the lower id
    first = order[:, 0]
    r = np.arange(len(o))
    t1 = th[r, first]
    t2 = th[r, order[:, 1]] if th.shape[1] > 1 else np.full(len(o), inf)
    got = np.isfinite(t1)
    with np.errstate(invalid="ignore"):
        gap = np.where(got, t2 - t1, inf)
        graze = np.where(tn <= t1[:, None], np.abs(m), inf).min(-1)
        far = np.where(m >= 0, np.abs(tn - t_max), inf).min(-1)
    return np.where(got, ids[first], -1), np.where(got, t1, 0), gap, graze, far


# ---------------------------------------------------------------------------------------------------------- one world
def _world(w, A, b, meta, walls, info, team, grab, out, dt):
    mg = out["margin"]
    nb, nr, nh, ns, step = (int(info[i]) for i in (2, 3, 4, 5, 6))
    na = nh + ns
    row0 = w * A
    fwd, right = np.array([0, 1, 0], dt), np.array([1, 0, 0], dt)
    surfaces = _surfaces(b, meta, walls, info, dt)
    pos, rot, lin, ang = b[:, 0:3], b[:, 3:7], b[:, 7:10], b[:, 10:13]

    def locks(s):                                             # computeLockObservation, sim.cpp:422-446
        if meta[s, 1] != STATIC:
            return 0.0, 0.0
        return (1.0, 0.0) if meta[s, 2] == OWNER_HIDER else (0.0, 1.0)

    # globalPositionsDebugSystem, sim.cpp:895-941: hiders first, then seekers, whatever their interfaces
    gp, gw = out["global_positions"][w], out["global_written"][w]
    gw[:MAX_BOXES + MAX_RAMPS] = True
    gp[:nb] = pos[:nb, :2]
    gp[MAX_BOXES:MAX_BOXES + nr] = pos[scenes.RAMP_SLOT0:scenes.RAMP_SLOT0 + nr, :2]
    order = [i for i in range(na) if team[i] == HIDER] + [i for i in range(na) if team[i] == SEEKER]
    a0 = MAX_BOXES + MAX_RAMPS
    for k, i in enumerate(order):
        gp[a0 + k] = pos[scenes.AGENT_SLOT0 + i, :2]
    gw[a0:a0 + na] = True
    gw[a0 + na:a0 + MAX_AGENTS:2] = True                      # `out_offset++` twice per round: every other entry

    rays_o, rays_d, rays_max, spans = [], [], [], []
    for i in range(na):
        r, si = row0 + i, scenes.AGENT_SLOT0 + i
        out["active"][r] = True
        p0, q0, v0, w0 = pos[si], rot[si], lin[si], ang[si]
        to_frame = _conj(q0)
        if step <= PREP_STEPS:                                # sim.cpp:461-464
            out["prep_counter"][r, 0] = PREP_STEPS - step
            out["prep_written"][r] = True
        e, m = _euler(q0)                                     # sim.cpp:475-482: the agent's own rotation as it is
        out["self_data"][r] = np.concatenate([p0, e, _rot(to_frame, v0), _rot(to_frame, w0), [grab[i]]])
        mg["self_sinp"][r] = m

        if nb:                                                # sim.cpp:485-505
            rel, m = _relative(p0, q0, v0, w0, pos[:nb], rot[:nb], lin[:nb], ang[:nb])
            out["box_data"][r, :nb, :12] = rel
            out["box_data"][r, :nb, 12:15] = [_SIZE[int(meta[s, 0])] for s in range(nb)]
            out["box_data"][r, :nb, 15:17] = [locks(s) for s in range(nb)]
            mg["box_sinp"][r, :nb] = m
        if nr:                                                # sim.cpp:507-525
            s0 = scenes.RAMP_SLOT0
            rel, m = _relative(p0, q0, v0, w0, pos[s0:s0 + nr], rot[s0:s0 + nr], lin[s0:s0 + nr], ang[s0:s0 + nr])
            out["ramp_data"][r, :nr, :12] = rel
            out["ramp_data"][r, :nr, 12:14] = [locks(s0 + k) for k in range(nr)]
            mg["ramp_sinp"][r, :nr] = m
        others = [j for j in range(na) if j != i]             # sim.cpp:527-564: in interface order, self left out
        if others:
            so = [scenes.AGENT_SLOT0 + j for j in others]
            rel, m = _relative(p0, q0, v0, w0, pos[so], rot[so], lin[so], ang[so])
            k = len(others)
            out["agent_data"][r, :k, :12] = rel
            out["agent_data"][r, :k, 12] = [1.0 if team[j] == HIDER else 0.0 for j in others]
            out["agent_data"][r, :k, 13] = [grab[j] for j in others]
            mg["agent_sinp"][r, :k] = m

        # lidarSystem, sim.cpp:712-745
        theta = 2 * dt(np.pi) * (np.arange(LIDAR_RAYS, dtype=dt) / dt(LIDAR_RAYS)) + dt(np.pi) / 2
        d = np.cos(theta)[:, None] * _rot(q0, right) + np.sin(theta)[:, None] * _rot(q0, fwd)
        d = d / np.sqrt((d * d).sum(-1, keepdims=True))
        rays_o.append(np.broadcast_to(p0, d.shape)); rays_d.append(d); rays_max.append(np.full(len(d), LIDAR_RANGE, dt))
        # computeVisibilitySystem, sim.cpp:567-605, 663-708: boxes, ramps, the other agents
        targets = list(range(nb)) + [scenes.RAMP_SLOT0 + k for k in range(nr)] + [scenes.AGENT_SLOT0 + j for j in others]
        to = pos[targets] - p0 if targets else np.zeros((0, 3), dt)
        rays_o.append(np.broadcast_to(p0, to.shape)); rays_d.append(to); rays_max.append(np.ones(len(to), dt))
        spans.append((r, _rot(q0, fwd), np.array(targets, int), to, len(others)))

    if not na:
        return
    o, d, t_max = np.concatenate(rays_o), np.concatenate(rays_d), np.concatenate(rays_max)
    hit, t, gap, graze, far = _trace(surfaces, o, d, t_max[:, None])
    at = 0
    for r, f, targets, to, k in spans:
        sl = slice(at, at + LIDAR_RAYS); at += LIDAR_RAYS
        out["lidar"][r] = t[sl]                               # 0 where nothing was hit, sim.cpp:740-744
        mg["lidar_hit"][r], mg["lidar_gap"][r], mg["lidar_graze"][r], mg["lidar_far"][r] = hit[sl], gap[sl], graze[sl], far[sl]
        sl = slice(at, at + len(targets)); at += len(targets)
        if not len(targets):
            continue
        length = np.sqrt((to * to).sum(-1))
        cos_angle = (to / length[:, None]) @ f
        ahead = cos_angle >= COS_FOV                          # `cos_angle < threshold -> 0`
        vis = np.where(ahead & (hit[sl] == targets), 1.0, 0.0)
        big = np.full(len(targets), np.inf)
        vals = {"": vis, "_cos": np.abs(cos_angle - dt(COS_FOV)), "_cosv": cos_angle, "_len": length,
                "_gap": np.where(ahead, gap[sl] * length, big), "_graze": np.where(ahead, graze[sl] * length, big)}
        for name, a, z, cap in (("boxes", 0, nb, MAX_BOXES), ("ramps", nb, nb + nr, MAX_RAMPS),
                                ("agents", nb + nr, nb + nr + k, MAX_AGENTS - 1)):
            for suffix, v in vals.items():
                dst = out[f"visible_{name}_mask"][r, :, 0] if suffix == "" else mg[f"visible_{name}{suffix}"][r]
                dst[:z - a] = v[a:z]

    # rewardsVisSystem and outputRewardsDonesSystem, sim.cpp:763-841, run before resetSystem counts the step
    if step == 0:
        return
    for i in range(na):
        r = row0 + i
        x, y = (float(c) for c in pos[scenes.AGENT_SLOT0 + i, :2])
        mg["reward_bound"][r] = min(abs(abs(x) - 18.0), abs(abs(y) - 18.0))
        out["reward_penalty"][r] = abs(x) >= 18.0 or abs(y) >= 18.0


def seen(res, team, A):
    """Per world, the visibility bits that decide the hider team's reward: rows i and columns jj of
    visible_agents_mask where agent i is a seeker and the agent behind column jj a hider (sim.cpp:700-705, 779-803)."""
    team = np.asarray(team).reshape(-1)
    return (team == SEEKER)[:, None] & (res["agent_data"][:, :, 12] == 1) & res["active"][:, None]


def observe(bodies, meta, walls, info, self_type, A, grabbing=None, prev=None, dtype=np.float64):
    """The observation stage of every world of a dump; see the module docstring.  Returns a dict of arrays shaped as
    the exports (per-agent rows world * A + interface), the `*_written` / `active` masks, and "margin"."""
    dt = np.dtype(dtype).type
    n = len(bodies)
    rows = n * A
    b = np.asarray(bodies, np.float32).astype(dt)
    wl = np.asarray(walls, np.float32).astype(dt)
    team = np.asarray(self_type).reshape(n, A)
    grab = np.zeros((n, A), dt) if grabbing is None else np.asarray(grabbing, dt).reshape(n, A)
    z = lambda *s: np.zeros(s, dt)
    big = lambda *s: np.full(s, np.inf)
    out = {"self_data": z(rows, 13), "agent_data": z(rows, 5, 14), "box_data": z(rows, 9, 17), "ramp_data": z(rows, 2, 14),
           "visible_agents_mask": z(rows, 5, 1), "visible_boxes_mask": z(rows, 9, 1), "visible_ramps_mask": z(rows, 2, 1),
           "lidar": z(rows, LIDAR_RAYS), "reward": z(rows, 1), "prep_counter": np.zeros((rows, 1), np.int32),
           "global_positions": z(n, 17, 2), "global_written": np.zeros((n, 17), bool), "active": np.zeros(rows, bool),
           "prep_written": np.zeros(rows, bool), "reward_written": np.zeros(rows, bool),
           "reward_penalty": np.zeros(rows, bool)}
    mg = out["margin"] = {"self_sinp": big(rows), "agent_sinp": big(rows, 5), "box_sinp": big(rows, 9),
                          "ramp_sinp": big(rows, 2), "lidar_gap": big(rows, 30), "lidar_graze": big(rows, 30),
                          "lidar_far": big(rows, 30), "lidar_hit": np.full((rows, 30), -1), "reward_bound": big(rows)}
    for name, k in (("boxes", 9), ("ramps", 2), ("agents", 5)):
        for suffix in ("_cos", "_gap", "_graze"):
            mg[f"visible_{name}{suffix}"] = big(rows, k)
        mg[f"visible_{name}_cosv"] = z(rows, k)
        mg[f"visible_{name}_len"] = np.ones((rows, k), dt)
    for w in range(n):
        _world(w, A, b[w], np.asarray(meta[w]), wl[w], np.asarray(info[w]), team[w], grab[w], out, dt)

    # the reward (sim.cpp:806-841): the flag of the previous dump's observation pass, lowered again on these poses
    step = np.repeat(np.asarray(info)[:, 6], A)
    pairs = seen(out, team, A)
    now = (pairs & (out["visible_agents_mask"][:, :, 0] == 1)).reshape(n, -1).any(1)
    if prev is not None:
        before = (seen(prev, team, A) & (prev["visible_agents_mask"][:, :, 0] == 1)).reshape(n, -1).any(1)
        flag = np.repeat(np.where(now | before, -1.0, 1.0), A)
        value = np.where(team.reshape(-1) == SEEKER, -flag, flag) - 10.0 * out["reward_penalty"]
        early = step - 1 < PREP_STEPS - 1
        out["reward"][:, 0] = np.where(early, 0.0, value)
        out["reward_written"] = out["active"] & (step > 0)
    else:
        out["reward_written"] = out["active"] & (step > 0) & (step - 1 < PREP_STEPS - 1)
    return out


def robust(res, eps_cos, eps_t, eps_euler, prev=None, team=None, A=None):
    """Masks of the values whose float64 decision was taken by more than the epsilons: eps_cos on cos_angle, eps_t on
    ray parameters in metres per max(1, length), eps_euler on 1 - |sinp|.  Keys: the three visibility masks, "lidar",
    "self_euler" / "agent_euler" / "box_euler" / "ramp_euler", and "reward" (with `prev`, `team`, `A`): the team flag is
    robust when one robust bit of either dump says seen or every bit of both robustly says unseen, and the bound at
    |x|, |y| = 18 by eps_t."""
    mg = res["margin"]
    ok = {}
    for name in ("boxes", "ramps", "agents"):
        k = f"visible_{name}"
        e = eps_t * np.maximum(1.0, mg[k + "_len"])
        ok[k + "_mask"] = (mg[k + "_cos"] > eps_cos) & (mg[k + "_gap"] > e) & (mg[k + "_graze"] > e)
    e = eps_t * np.maximum(1.0, res["lidar"])
    ok["lidar"] = (mg["lidar_gap"] > e) & (mg["lidar_graze"] > e) & (mg["lidar_far"] > e)
    for name in ("self", "agent", "box", "ramp"):
        ok[name + "_euler"] = mg[name + "_sinp"] > eps_euler
    if prev is not None:
        n = len(res["active"]) // A
        flags = []
        for r in (res, prev):
            good = robust(r, eps_cos, eps_t, eps_euler)["visible_agents_mask"]
            pairs, vis = seen(r, team, A), r["visible_agents_mask"][:, :, 0] == 1
            flags.append(((pairs & vis & good).reshape(n, -1).any(1), (~pairs | (~vis & good)).reshape(n, -1).all(1)))
        team_ok = flags[0][0] | flags[1][0] | (flags[0][1] & flags[1][1])
        ok["reward"] = np.repeat(team_ok, A) & (mg["reward_bound"] > eps_t * 18)
    return ok


GROUPS = ("position", "euler", "velocity", "lidar")


def deviations(get, res, ok, lidar_ok=None):
    """Compare exported tensors (get(name) -> array shaped as the export) with a result of observe() on the rows and
    entries the reference writes.  Returns (err, wrong, share): err[group] the largest deviation per GROUPS (euler
    modulo 2 pi, lidar as |dt| / max(1, t)); wrong a list of (tensor, count) for values that must agree exactly and do
    not (flags, sizes, counters, zero fill, and the discrete values that `ok` calls robust); share[tensor] =
    (left out, all) for the entries `ok` leaves out."""
    act = res["active"]
    err = dict.fromkeys(GROUPS, 0.0)
    wrong, share = [], {}

    def upd(group, d):
        if d.size:
            err[group] = max(err[group], float(d.max()))

    def exact(name, x, y):
        bad = int((x != y).sum())
        if bad:
            wrong.append((name, bad))
    for name, euler, tail in (("self_data", "self_euler", 12), ("agent_data", "agent_euler", 12),
                              ("box_data", "box_euler", 12), ("ramp_data", "ramp_euler", 12)):
        x, y = np.asarray(get(name), np.float64)[act], np.asarray(res[name], np.float64)[act]
        d = np.abs(x - y)
        upd("position", d[..., 0:3])
        upd("velocity", d[..., 6:12])
        good = ok[euler][act]
        e = np.abs((d[..., 3:6] + np.pi) % (2 * np.pi) - np.pi)
        upd("euler", e[good])
        share[euler] = (int((~good).sum()), good.size)
        exact(name + "[12:]", x[..., tail:], y[..., tail:])
    gp = np.abs(np.asarray(get("global_positions"), np.float64) - res["global_positions"])
    upd("position", gp[res["global_written"]])
    good = ok["lidar"][act] if lidar_ok is None else lidar_ok[act]
    x, y = np.asarray(get("lidar"), np.float64)[act], np.asarray(res["lidar"], np.float64)[act]
    upd("lidar", (np.abs(x - y) / np.maximum(1.0, y))[good])
    exact("lidar hit or miss", (x != 0)[good], (y != 0)[good])
    share["lidar"] = (int((~good).sum()), good.size)
    for name in ("visible_agents_mask", "visible_boxes_mask", "visible_ramps_mask"):
        good = ok[name][act]
        exact(name, np.asarray(get(name))[act][..., 0][good], res[name][act][..., 0][good])
        share[name] = (int((~good).sum()), good.size)
    pw = res["prep_written"]
    exact("prep_counter", np.asarray(get("prep_counter"))[pw], res["prep_counter"][pw])
    rw = res["reward_written"]
    good = ok["reward"][rw] if "reward" in ok else np.ones(int(rw.sum()), bool)
    exact("reward", np.asarray(get("reward"), np.float64)[rw][good], np.asarray(res["reward"], np.float64)[rw][good])
    share["reward"] = (int((~good).sum()), good.size)
    return err, wrong, share
