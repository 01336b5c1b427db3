"""The stored ray cases on the device.  tests/golden/ray_hull_cases.npz holds random rays against randomly posed cubes,
elongated boxes and ramp wedges, which test_oracle_first_principles.py runs against the oracle's hull tests only.  Here
each hull is written into a world of its own through the Checkpoint record, 20 m up, and a 1 x 1 spectator camera
looks along the stored ray: k_spectate's hit id and depth against a float64 half-space clip (oracle/scenes.py), with the
bounding-sphere culls and without.  No oracle side takes part."""
import functools
import os

import numpy as np
import pytest

import scenes
from scenes import CUBE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "golden", "ray_hull_cases.npz")
SEED = 3
OFFSET = np.array([3.0, -2.0, 20.0])

# The largest error of the oracle's hull tests (hsref_ray_body, float32) against the float64 clip on these translated
# cases, as |t - t_clip| / max(1, t_clip): measured on the CPU by test_the_translated_cases_and_the_oracles_error
# below (6.787e-07 at t up to 8.5 and coordinates up to 30 m), which asserts that it stays below this figure.  The camera
# test allows four times as much, 2.72e-06: the camera's basis from a float32 quaternion and the pixel direction add a
# few roundings of their own.
ORACLE_ERROR = 6.8e-7
TOLERANCE = 4 * ORACLE_ERROR


@functools.lru_cache(maxsize=None)
def translated():
    """Per stored row: kind, float32 pose / origin / direction after the translation, the float64 clip's t of those
    float32 inputs, and `keep`: not grazing (margin >= 1e-3, as the stored test) and the floor not nearer than the hull."""
    g = np.load(CASES)["cases"]
    kind = g[:, 0].astype(int)
    pos = np.float32(g[:, 1:4] + OFFSET)
    rot = np.float32(g[:, 4:8])
    org = np.float32(g[:, 8:11] + OFFSET)
    dirn = np.float32(g[:, 11:14])
    t = np.zeros(len(g)); keep = np.zeros(len(g), bool)
    for i in range(len(g)):
        N, D = scenes.half_spaces(kind[i], pos[i], rot[i])
        t[i], margin = scenes.clip_ray(N, D, org[i], dirn[i])
        o, d = org[i].astype(np.float64), dirn[i].astype(np.float64)
        floor = -o[2] / d[2] if d[2] < 0 else np.inf
        keep[i] = margin >= 1e-3 and not (t[i] >= 0 and floor < t[i])
    return kind, pos, rot, org, dirn, t, keep


def test_the_translated_cases_and_the_oracles_error(oracle):
    """No GPU.  At most one stored case in six is left out after the translation (the stored test keeps more than 2 500
    of 3 000), hits and misses both remain in number, and the oracle's float32 hull tests on the translated cases stay
    within ORACLE_ERROR of the float64 clip: the figure the camera test's tolerance is four times of."""
    kind, pos, rot, org, dirn, t, keep = translated()
    assert (~keep).sum() * 6 <= len(keep), ((~keep).sum(), len(keep))
    assert (t[keep] >= 0).sum() > 500 and (t[keep] < 0).sum() > 500
    L = oracle.lib()
    f = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data
    worst = 0.0
    for i in np.flatnonzero(keep):
        got = L.hsref_ray_body(int(kind[i]), f(pos[i]), f(rot[i]), f(org[i]), f(dirn[i]))
        assert (got < 0) == (t[i] < 0), (i, got, t[i])
        if t[i] >= 0:
            worst = max(worst, abs(got - t[i]) / max(1.0, t[i]))
    print(f"skipped {(~keep).sum()} of {len(keep)}; oracle's largest error {worst:.3e}")
    assert worst <= ORACLE_ERROR, worst


@pytest.mark.gpu
def test_stored_rays_through_a_spectator_camera():
    """One world per stored case, all in one handle: hit == the slot the hull was written to exactly when the clip hits,
    and then depth / |d| == the clip's t within TOLERANCE * max(1, t); with the default culls and with exact=True, which
    must also agree bit for bit.  The bound is 2.72e-06 = 4 x 6.8e-07, the oracle's measured error against the same clip
    (ORACLE_ERROR above: measured against the reference clip, not against the kernel); k_spectate's largest error on an
    MI355X is 1.52e-06, all 2 998 cases kept, 838 of them hits."""
    import gpu_hideseek
    from gpu_hideseek.spectate import look_at
    kind, pos, rot, org, dirn, t, keep = translated()
    n = len(kind)
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=0, rand_seed=SEED, min_hiders=2,
        max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    sim.init()
    slot = np.full(n, -1)

    def edit(rec, meta):
        # the cases that need a cube get the worlds that have one
        kinds = meta[:, :scenes.AGENT_SLOT0, 0]
        worlds = np.argsort(-(kinds == CUBE).sum(1), kind="stable")
        order = np.argsort(kind != CUBE, kind="stable")
        for i, w in zip(order, worlds):
            have = np.flatnonzero(kinds[w] == kind[i])
            assert have.size, f"no world left with a hull of kind {kind[i]}"
            slot[i] = have[0]
            case_world[i] = w
            scenes.put(scenes.slot_record(rec[w], slot[i]), pos[i], rot[i])
    case_world = np.zeros(n, int)
    scenes.inject_sim(sim, edit)
    bodies = sim.debug_bodies()[0]
    assert np.array_equal(bodies[case_world, slot, :3], pos) and np.array_equal(bodies[case_world, slot, 3:7], rot)
    cams = [look_at(int(case_world[i]), org[i].astype(np.float64), org[i].astype(np.float64) + dirn[i].astype(np.float64),
                    fov_deg=60.0) for i in range(n)]
    res = {}
    for exact in (False, True):
        r = sim.spectate(cams, 1, 1, rgb=False, hit=True, exact=exact)
        res[exact] = (r["depth"].cpu().numpy().reshape(n), r["hit"].cpu().numpy().reshape(n))
    assert np.array_equal(res[False][0].view(np.int32), res[True][0].view(np.int32)), "culled depth != exact depth"
    assert np.array_equal(res[False][1], res[True][1]), "culled hit != exact hit"
    depth, hit = res[False]
    hits = t >= 0
    wrong = np.flatnonzero(keep & ((hit == slot) != hits))
    assert wrong.size == 0, [(int(i), int(kind[i]), int(hit[i]), int(slot[i]), float(t[i])) for i in wrong[:5]]
    sel = keep & hits
    got = depth[sel].astype(np.float64) / np.linalg.norm(dirn[sel].astype(np.float64), axis=1)
    err = np.abs(got - t[sel]) / np.maximum(1.0, t[sel])
    print(f"checked {int(keep.sum())} of {n} rays, {int(sel.sum())} hits; largest depth error {err.max():.3e} (allowed {TOLERANCE:.1e})")
    assert err.max() <= TOLERANCE, (int(np.flatnonzero(sel)[err.argmax()]), float(err.max()))
    assert (~keep).sum() * 6 <= n
    sim.close()
