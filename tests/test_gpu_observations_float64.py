"""k_observe and the reward path on the device against the float64 restatement of the reference
(oracle/observe_f64.py).  No oracle side takes part: the simulator's own exports are compared with the restatement of
the simulator's own debug_bodies() / debug_walls().  Tolerances, epsilons and the 2 % cap are those of
tests/test_observations_float64.py, which derives them from the restatement's float32-against-float64 deviation."""
import numpy as np
import pytest

import lockstep
import observe_f64 as O
import scenes
from scenes import BOX, CUBE
from test_observations_float64 import CAP, EPS_COS, EPS_T, TOLERANCE, drive, robust, snapshot

pytestmark = pytest.mark.gpu

FIXED = 3                # UseFixedWorld | IgnoreEpisodeLength
FAR = 100.0              # a crafted decision is taken by at least this many epsilons


class Device:
    """A HideAndSeekSimulator as the `side` of test_observations_float64.snapshot / drive."""

    def __init__(self, worlds, flags, seed, hiders, seekers):
        import gpu_hideseek
        self.sim = gpu_hideseek.HideAndSeekSimulator(
            exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=flags, rand_seed=seed,
            min_hiders=hiders[0], max_hiders=hiders[1], min_seekers=seekers[0], max_seekers=seekers[1], num_pbt_policies=1)
        self.sim.init()
        self.side = lockstep.GpuSide(self.sim)
        self.A = self.sim.agents_per_world
        self.rows = worlds * self.A

    def act(self, a):
        import torch
        dst = self.side.view("action")
        dst.copy_(torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dst.device))

    def step(self):
        self.sim.step()

    def inject(self, edit):
        return scenes.inject_sim(self.sim, edit)

    def close(self):
        self.sim.close()


def make(worlds, flags, seed, hiders, seekers):
    return Device(worlds, flags, seed, hiders, seekers)


def compare(x, r64, A, prev, tag, left):
    ok = robust(r64, x, A, prev)
    err, wrong, share = O.deviations(x.__getitem__, r64, ok)
    assert not wrong, (tag, wrong)
    for g in O.GROUPS:
        assert err[g] <= TOLERANCE[g], (tag, g, err[g], TOLERANCE[g])
    for k, (a, b) in share.items():
        left[k] = (left.get(k, (0, 0))[0] + a, left.get(k, (0, 0))[1] + b)
    return ok, err


def capped(left, label):
    print(f"{label}: left out as near an edge " + ", ".join(f"{k} {a}/{b}" for k, (a, b) in left.items()))
    for k, (a, b) in left.items():
        assert a <= CAP * b, (label, k, a, b)


# agents per world -> worlds, flags, seed, (min, max) hiders, (min, max) seekers.  k_observe has one instantiation per
# agent count (128, 128, 192, 320, 320 threads; the visibility rays start at lane 64, 128, 128, 192, 192); 13 worlds are
# one full octet and a partial one, so the octet / slot mapping and the empty-slot return run.
GENERATED = {2: (13, 0, 3, (1, 1), (1, 1)), 3: (13, 13, 5, (1, 1), (2, 2)), 4: (13, 0, 3, (2, 2), (2, 2)),
             5: (13, 13, 5, (1, 3), (1, 2)), 6: (13, 13, 5, (3, 3), (3, 3)), "4, one world": (1, 0, 3, (2, 2), (2, 2))}
_left = {}


@pytest.mark.parametrize("agents", list(GENERATED))
def test_generated_levels_on_the_device(agents):
    """Every instantiation of k_observe on generated levels with the "full" action stream, at init and after 40, 96 and
    130 steps: every exported observation, the masks, lidar, reward, counter and global positions."""
    dev = make(*GENERATED[agents])
    assert dev.A == (agents if isinstance(agents, int) else 4)
    worst = dict.fromkeys(O.GROUPS, 0.0)
    for s, x, (r64,), prev in drive(dev.side, dev.step, dev.act, dev.A, dev.rows, steps=(0, 40, 96, 130)):
        _, err = compare(x, r64, dev.A, prev, f"{agents} agents, step {s}", _left)
        worst = {g: max(worst[g], err[g]) for g in O.GROUPS}
    print(f"{agents} agents: largest errors " + ", ".join(f"{g} {worst[g]:.2e} (allowed {TOLERANCE[g]:.1e})" for g in O.GROUPS))
    dev.close()
    if agents == list(GENERATED)[-1]:
        capped(_left, "generated levels on the device")


def tilt(roll, pitch, yaw):
    """The quaternion of yaw about z after pitch about y after roll about x."""
    def q(angle, axis):
        out = np.zeros(4); out[0] = np.cos(angle / 2); out[1 + axis] = np.sin(angle / 2)
        return out
    return O._qmul(q(yaw, 2), O._qmul(q(pitch, 1), q(roll, 0)))


def test_crafted_scenes_on_the_device():
    """One hider (interface 0) and one seeker (interface 1) per world of the fixed level, written through the
    Checkpoint record at step 100 around the spot farthest from every wall; unused boxes and ramps hang in the sky.
    Each scene's expected bit comes from the restatement with its margin asserted to be at least FAR epsilons, so no
    scene can drift into the set that is left out; the device's exports are then compared as everywhere else, once
    after the load (which re-runs the observations) and once after a step (which computes the rewards)."""
    n = 12
    dev = make(n, FIXED, 3, (1, 1), (1, 1))
    A = dev.A
    walls, info = dev.side.walls()
    sx, sy, clear = scenes.open_spot(walls[0], info[0, 0])
    assert clear >= 9.0, clear
    thin = [k for k in range(info[0, 0]) if walls[0, k, 3] < 0.5 and walls[0, k, 2] >= 2.5 and abs(walls[0, k, 1]) < 15]
    others = lambda k, y: scenes.wall_clearance(np.delete(walls[0, :info[0, 0]], k, 0), info[0, 0] - 1, walls[0, k, 0], y)
    wk = max(thin, key=lambda k: min(others(k, walls[0, k, 1] - 2.5), others(k, walls[0, k, 1] + 2.5)))
    wx, wy = float(walls[0, wk, 0]), float(walls[0, wk, 1])
    used = {}

    def edit(rec, meta):
        cubes = np.flatnonzero(meta[0, :9, 0] == CUBE)
        boxes = np.flatnonzero(meta[0, :9, 0] == BOX)
        c0, c1, b0, r0 = int(cubes[0]), int(cubes[1]), int(boxes[0]), scenes.RAMP_SLOT0
        used.update(c0=c0, c1=c1, b0=b0)
        yq = scenes.yaw_quat

        def agents(w, hider, hyaw, seeker, syaw):
            scenes.put(rec[w]["agents"][0], (hider[0], hider[1], 1.0), (1, 0, 0, 0) if hyaw == 0 else yq(hyaw))
            scenes.put(rec[w]["agents"][1], (seeker[0], seeker[1], 1.0), (1, 0, 0, 0) if syaw == 0 else yq(syaw))

        def sky(w, keep=()):
            for s in range(scenes.AGENT_SLOT0):
                if s not in keep:
                    r = scenes.slot_record(rec[w], s)
                    scenes.put(r, (float(r["pos"][0]), float(r["pos"][1]), 40.0 + 4.0 * s), r["rot"])
        rec["step"] = 100
        # 0 (a): yaw exactly 0 (lidar directions with a zero component) beside a generic yaw, in the level as generated
        agents(0, (sx, sy), 0, (sx + 5, sy + 2), 0.7)
        # 1-3 (b): a cube exactly between, aside by more than its bounding radius (1.73), aside by less but clear of the hull
        for w, dx in ((1, 0.0), (2, 3.0), (3, 1.5)):
            sky(w, keep=(c0,))
            agents(w, (sx, sy + 8), np.pi, (sx, sy), 0)
            scenes.put(scenes.slot_record(rec[w], c0), (sx + dx, sy + 4, 1.0))
        # 4 (c): an elongated box yawed 45 degrees in front of the hider
        sky(4, keep=(b0,))
        agents(4, (sx, sy), 0.3, (sx - 6, sy - 4), 2.0)
        scenes.put(scenes.slot_record(rec[4], b0), (sx, sy + 6, 1.0), yq(np.pi / 4))
        # 5-6 (d): a ramp across the segment, which passes over its low end (local y = -1.5) or through its high end (0.5)
        for w, c in ((5, -1.5), (6, 0.5)):
            sky(w, keep=(r0,))
            agents(w, (sx, sy), 0, (sx, sy + 8), np.pi)
            scenes.put(scenes.slot_record(rec[w], r0), (sx + c, sy + 4, 1.0), yq(np.pi / 2))
        # 7 (e): cubes 60 and 75 degrees off the seeker's forward axis
        sky(7, keep=(c0, c1))
        agents(7, (sx, sy - 6), 0, (sx, sy), 0)
        scenes.put(scenes.slot_record(rec[7], c0), (sx + 6 * np.sin(np.pi / 3), sy + 6 * np.cos(np.pi / 3), 1.0))
        scenes.put(scenes.slot_record(rec[7], c1), (sx - 6 * np.sin(np.radians(75)), sy + 6 * np.cos(np.radians(75)), 1.0))
        # 8 (f): a box tilted about x and y
        sky(8, keep=(b0,))
        agents(8, (sx, sy), 0.4, (sx - 6, sy - 4), 2.0)
        scenes.put(scenes.slot_record(rec[8], b0), (sx, sy + 6, 5.0), tilt(0.5, 0.4, 0.3))
        # 9-10 (g): the seeker faces the hider with nothing between them, and across a wall
        sky(9); agents(9, (sx, sy + 6), np.pi, (sx, sy), 0)
        sky(10); agents(10, (wx, wy + 2.5), np.pi, (wx, wy - 2.5), 0)
        # 11 (h): the hider beyond x = 18, the seeker looking away
        sky(11); agents(11, (19.5, sy), 0, (sx, sy), np.pi / 2)
    dev.inject(edit)
    c0, c1, b0, r0 = used["c0"], used["c1"], used["b0"], scenes.RAMP_SLOT0
    left = {}
    x, (r64,) = snapshot(dev.side, A)
    ok, _ = compare(x, r64, A, None, "crafted scenes, loaded", left)
    mg = r64["margin"]
    H, S = (lambda w: w * A), (lambda w: w * A + 1)

    def decided(name, row, col, want):
        """The restatement says `want`, by FAR epsilons; the device's own value was compared by compare()."""
        assert r64[f"visible_{name}_mask"][row, col, 0] == want, (name, row, col)
        e = EPS_T * max(1.0, mg[f"visible_{name}_len"][row, col])
        assert mg[f"visible_{name}_cos"][row, col] > FAR * EPS_COS, (name, row, col, "cos")
        assert min(mg[f"visible_{name}_gap"][row, col], mg[f"visible_{name}_graze"][row, col]) > FAR * e, (name, row, col)
        assert x[f"visible_{name}_mask"][row, col, 0] == want, (name, row, col, "device")
    b = dev.side.bodies()[0]
    assert np.array_equal(b[0, scenes.AGENT_SLOT0, 3:7], [1, 0, 0, 0])                     # (a)
    assert (r64["lidar"][H(0)] > 0).sum() >= 10 and (r64["lidar"][S(0)] > 0).sum() >= 10
    assert ok["lidar"][[H(0), S(0)]].all()
    for w, want in ((1, 0.0), (2, 1.0), (3, 1.0)):                                         # (b)
        decided("agents", S(w), 0, want)
        decided("agents", H(w), 0, want)
    hit = mg["lidar_hit"][H(4)]                                                            # (c)
    th = 2 * np.pi * np.arange(30) / 30 + np.pi / 2 + 0.3
    d = np.stack([np.cos(th), np.sin(th)], 1)                                              # ray k of an agent yawed by 0.3
    to = np.array([0.0, 6.0])
    along, off = d @ to, np.abs(d[:, 0] * to[1] - d[:, 1] * to[0])
    near = (along > 0) & (off < np.hypot(4, 0.75))
    assert (hit[near] == b0).any() and (hit[near] != b0).any(), "rays inside the bounding sphere on both sides of the hull"
    assert ok["lidar"][H(4)][near].all()
    for w, want in ((5, 1.0), (6, 0.0)):                                                   # (d)
        decided("agents", H(w), 0, want)
        decided("agents", S(w), 0, want)
    decided("boxes", S(7), c0, 1.0)                                                        # (e)
    decided("boxes", S(7), c1, 0.0)
    assert abs(mg["visible_boxes_cosv"][S(7), c0] - 0.5) < 1e-6 and abs(mg["visible_boxes_cosv"][S(7), c1] - np.cos(np.radians(75))) < 1e-6
    e = r64["box_data"][H(8), b0, 3:6]                                                     # (f)
    assert abs(e[0]) > 0.2 and abs(e[1]) > 0.2 and ok["box_euler"][H(8), b0]
    decided("agents", S(9), 0, 1.0)                                                        # (g)
    decided("agents", S(10), 0, 0.0)
    assert mg["lidar_hit"][S(10), 0] == O.WALL0 + wk, "the wall is what the seeker's forward ray meets"

    dev.step()
    x1, (r1,) = snapshot(dev.side, A, prev=r64)
    ok1, _ = compare(x1, r1, A, r64, "crafted scenes, stepped", left)
    assert r1["reward_written"].all() and ok1["reward"].all(), "every crafted reward is decided far from an edge"
    for w, hider, seeker in ((9, -1.0, 1.0), (10, 1.0, -1.0), (11, 1.0 - 10.0, -1.0), (1, 1.0, -1.0), (2, -1.0, 1.0)):
        assert r1["reward"][H(w), 0] == hider and r1["reward"][S(w), 0] == seeker, (w, r1["reward"][H(w)], r1["reward"][S(w)])
        assert x1["reward"][H(w), 0] == hider and x1["reward"][S(w), 0] == seeker, (w, "device")
    assert r1["margin"]["reward_bound"][H(11)] > 1.0
    capped(left, "crafted scenes on the device")
    dev.close()
