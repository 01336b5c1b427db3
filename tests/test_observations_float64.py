"""The observation stage against a float64 restatement of the reference (oracle/observe_f64.py), on the CPU oracle.

The lock-step tests prove that k_observe equals the oracle bit for bit; this file proves that the oracle computes what
src/sim.cpp:372-941 computes: self / agent / box / ramp observations, the three visibility masks, lidar, the reward, the
preparation counter and the global positions, from nothing but the oracle's own dumped bodies and walls.

TOLERANCES are derived, not chosen.  The restatement is evaluated a second time with every array in float32 (numpy's
float32 arithmetic and trigonometry); its largest deviation from the float64 result over this file's own cases is
measured per group, printed, and required to stay below the figures recorded in F32_DEVIATION.  A group's tolerance is
four times its recorded figure -- the margin of test_action_sampling_host.py and test_gpu_crafted_rays.py, for the same
reason: the product's polynomials and fused order add a few roundings that a plain float32 evaluation does not have.
The measurement is against the float64 reference, never against the oracle or a kernel.

EPSILONS.  A discrete value (a visibility bit, which surface a lidar ray hit, the team reward that follows from
visibility) is compared only where float64 took the decision by more than four times the float32 deviation of the
quantity that decides: EPS_COS for cos_angle against cos 67.5 deg, EPS_T (per max(1, length) metres) for the gap between
the first two surfaces on a ray, for the hull that is nearly grazed and for |t - 200|.  Euler angles are compared where
1 - |sinp| >= EPS_EULER = 1e-3: asin and the two atan2 amplify the rounding of their arguments by 1 / sqrt(2 (1 - |sinp|)),
more than 22 times inside that band (pitch within 2.6 deg of the clamp at sim.cpp:382-387), and AT the clamp roll and yaw
are the atan2 of two roundings.  Bodies do lie there: with ZeroAgentVelocity agents knock ramps onto their sides, where
they rest with 1 - |sinp| < 1e-7 (63 of the 69 ramp triples left out at flags 13), so no smaller band would keep more.  What is left out is
counted, and at most 2 % of a tensor may be left out per scene set: a condition on the scene sets, checked on the
float64 reference alone before the seeds below were fixed.
"""
import functools

import numpy as np
import pytest

import lockstep
import observe_f64 as O

# Largest |float32 - float64| of the restatement over the cases below, as measured by
# test_float32_deviation_of_the_restatement (which asserts that the measurement stays below these): positions in metres,
# euler angles in radians modulo 2 pi, linear / angular velocities in m/s and rad/s, lidar as |dt| / max(1, t), cos_angle.
F32_DEVIATION = {"position": 9.4e-6, "euler": 3.6e-6, "velocity": 4.9e-6, "lidar": 1.8e-5, "cos": 1.7e-7}
TOLERANCE = {g: 4 * F32_DEVIATION[g] for g in O.GROUPS}
EPS_COS = 4 * F32_DEVIATION["cos"]
EPS_T = 4 * F32_DEVIATION["lidar"]
EPS_EULER = 1e-3
CAP = 0.02

WORLDS = 16
STEPS = (0, 40, 95, 96, 130)            # init, mid-preparation, the step before and the step at which rewards begin, later
# (min, max) hiders, (min, max) seekers: 1+1, 1+2, 2+1, 2+2, the variable teams (A = 5), 3+3
TEAMS = [((1, 1), (1, 1)), ((1, 1), (2, 2)), ((2, 2), (1, 1)), ((2, 2), (2, 2)), ((1, 3), (1, 2)), ((3, 3), (3, 3))]
SEEDS = {0: 3, 13: 5}


def snapshot(side, A, prev=None, dtypes=(np.float64,)):
    """A side's (RefSim or lockstep.GpuSide) exports, copied, and the restatement(s) of its dumped state."""
    b, m = side.bodies()
    w, info = side.walls()
    x = {n: np.array(side.tensor(n)) for n in lockstep.NAMES}
    res = [O.observe(b, m, w, info, x["self_type"], A, x["self_data"][:, 12], prev, dtype=t) for t in dtypes]
    return x, res


def robust(res, x, A, prev=None):
    return O.robust(res, EPS_COS, EPS_T, EPS_EULER, prev, x["self_type"], A)


def drive(side, step, act, A, rows, steps=STEPS, dtypes=(np.float64,), stream_seed=99):
    """Drive a side with the "full" stream; at each of `steps` yield (step, exports, restatements, previous float64
    restatement or None).  The restatement of the step before is made where the reward needs it (from step 96 on)."""
    draw, _ = lockstep.stream("full", stream_seed)
    prev = None
    for s in range(max(steps) + 1):
        if s:
            act(draw(s, rows))
            step()
        need = s + 1 in steps and s + 1 >= O.PREP_STEPS
        cur = None
        if s in steps:
            x, res = snapshot(side, A, prev, dtypes)
            yield s, x, res, prev
            cur = res[0]
        elif need:
            cur = snapshot(side, A)[1][0]
        prev = cur if need else None


@functools.lru_cache(maxsize=None)
def generated(flags):
    """Every checkpoint of every team configuration at one flag word: (tag, A, exports, r64, r32, prev)."""
    out = []
    for hiders, seekers in TEAMS:
        ref = lockstep.make_ref(WORLDS, flags, SEEDS[flags], hiders, seekers, threads=4)
        ref.init()
        A = ref.A

        def act(a):
            ref.tensor("action")[:] = a
        for s, x, (r64, r32), prev in drive(ref, ref.step, act, A, WORLDS * A, dtypes=(np.float64, np.float32)):
            out.append((f"teams {hiders} {seekers} flags {flags} step {s}", A, x, r64, r32, prev))
        ref.close()
    return out


@functools.lru_cache(maxsize=None)
def debug_levels():
    out = []
    for level in range(2, 9):
        ref = lockstep.make_ref(3, 2, 0, (1, 1), (1, 1), threads=1)
        ref.tensor("reset")[:] = level
        ref.init()
        for s in range(61):
            if s:
                ref.step()
            if s in (0, 20, 60):
                x, (r64, r32) = snapshot(ref, ref.A, dtypes=(np.float64, np.float32))
                out.append((f"level {level} step {s}", ref.A, x, r64, r32, None))
        ref.close()
    return out


SETS = {"generated, flags 0": lambda: generated(0), "generated, flags 13": lambda: generated(13),
        "debug levels 2-8": debug_levels}


def check_set(cases, label):
    """Every case of a scene set against its float64 restatement: groups within TOLERANCE, exact values exact, and at
    most CAP of each tensor left out as near an edge.  Returns the largest errors and the shares, printed."""
    worst = dict.fromkeys(O.GROUPS, 0.0)
    left = {}
    for tag, A, x, r64, _, prev in cases:
        ok = robust(r64, x, A, prev)
        err, wrong, share = O.deviations(x.__getitem__, r64, ok)
        assert not wrong, (tag, wrong)
        for g in O.GROUPS:
            assert err[g] <= TOLERANCE[g], (tag, g, err[g], TOLERANCE[g])
            worst[g] = max(worst[g], err[g])
        for k, (a, b) in share.items():
            left[k] = (left.get(k, (0, 0))[0] + a, left.get(k, (0, 0))[1] + b)
    print(f"{label}: largest errors " + ", ".join(f"{g} {worst[g]:.2e} (allowed {TOLERANCE[g]:.1e})" for g in O.GROUPS))
    print(f"{label}: left out as near an edge " + ", ".join(f"{k} {a}/{b}" for k, (a, b) in left.items()))
    for k, (a, b) in left.items():
        assert a <= CAP * b, (label, k, a, b)
    return worst, left


def test_float32_deviation_of_the_restatement(oracle):
    """The figures the tolerances come from: float32 against float64 evaluation of the restatement itself, over every
    case of this file.  Lidar is measured on the rays on which both evaluations hit the same surface."""
    worst = dict.fromkeys(F32_DEVIATION, 0.0)
    for label, cases in SETS.items():
        for tag, A, x, r64, r32, prev in cases():
            ok = O.robust(r64, 0.0, 0.0, EPS_EULER)
            same = r64["margin"]["lidar_hit"] == r32["margin"]["lidar_hit"]
            err, _, _ = O.deviations(r32.__getitem__, r64, ok, lidar_ok=same)
            for g in O.GROUPS:
                worst[g] = max(worst[g], err[g])
            for name in ("agents", "boxes", "ramps"):
                d = np.abs(r32["margin"][f"visible_{name}_cosv"].astype(np.float64) - r64["margin"][f"visible_{name}_cosv"])
                worst["cos"] = max(worst["cos"], float(d[r64["active"]].max(initial=0.0)))
    print("float32 against float64: " + ", ".join(f"{g} {v:.2e} (recorded {F32_DEVIATION[g]:.1e})" for g, v in worst.items()))
    for g, v in worst.items():
        assert v <= F32_DEVIATION[g], (g, v)
        assert v >= F32_DEVIATION[g] / 4, f"the recorded figure for {g} is no longer a measurement: {v}"


@pytest.mark.parametrize("flags", [0, 13])
def test_generated_levels_against_float64(oracle, flags):
    """Agent counts 2-6, fixed teams and the variable teams (1..3 hiders, 1..2 seekers: inactive interfaces, so the
    zero-fill branches at sim.cpp:489-492, 511-514, 530-533 run), 16 worlds each, the "full" action stream with grabs
    and locks, compared at init, step 40, 95, 96 and 130."""
    cases = generated(flags)
    check_set(cases, f"generated, flags {flags}")
    rows = sum(int(c[3]["active"].sum()) for c in cases)
    assert rows > 1500
    if flags == 13:
        assert any((~c[3]["active"]).any() for c in cases), "no inactive interface: the zero fill did not run"
    # the stream did make grabs and locks appear, and rewards of both signs
    if flags == 13:         # without ZeroAgentVelocity the random stream moves nobody up to a box in 130 steps
        assert any((c[2]["self_data"][:, 12] == 1).any() for c in cases)
    assert any((c[2]["box_data"][..., 15:17] == 1).any() for c in cases)
    assert any((c[2]["ramp_data"][..., 12:14] == 1).any() for c in cases)
    assert {-1.0, 1.0} <= set(np.concatenate([c[2]["reward"].ravel() for c in cases]).tolist())


def test_debug_levels_against_float64(oracle):
    """Debug levels 2-8 (level_gen.cpp:336-526).  Only 5 and 6 make agents; in the others nothing is observed, which
    the restatement and the oracle's self_mask must both say."""
    cases = debug_levels()
    check_set(cases, "debug levels 2-8")
    for tag, A, x, r64, _, _ in cases:
        level = int(tag.split()[1])
        assert np.array_equal(x["self_mask"][:, 0] == 1, r64["active"]), tag
        assert int(r64["active"].sum()) == {5: 3, 6: 6}.get(level, 0), tag


@pytest.mark.parametrize("flags", [0, 13])
def test_cross_checks_that_need_no_reference(oracle, flags):
    """agent_data[i, jj, 13] == self_data[j, 12] and agent_data[i, jj, 12] == (agent j is a hider) with j the jj-th
    interface other than i; box sizes follow the object type."""
    for tag, A, x, r64, _, _ in generated(flags):
        n = len(x["self_data"]) // A
        sd, ad = x["self_data"].reshape(n, A, 13), x["agent_data"].reshape(n, A, 5, 14)
        team, mask = x["self_type"].reshape(n, A), x["self_mask"].reshape(n, A) == 1
        for i in range(A):
            for jj in range(A - 1):
                j = jj if jj < i else jj + 1
                both = mask[:, i] & mask[:, j]
                assert np.array_equal(ad[both, i, jj, 13], sd[both, j, 12]), (tag, i, jj)
                assert np.array_equal(ad[both, i, jj, 12], (team[both, j] == O.HIDER).astype(np.float32)), (tag, i, jj)
                gone = mask[:, i] & ~mask[:, j]
                assert not ad[gone, i, jj].any(), (tag, i, jj, "an inactive interface is zero-filled")
        size = x["box_data"][r64["active"]][..., 12:15]
        ok = (size == (8, 1.5, 2)).all(-1) | (size == (2, 2, 2)).all(-1) | (size == 0).all(-1)
        assert ok.all(), tag


def test_rays_against_scenes_clip(oracle):
    """The restatement's vectorised ray cast against scenes.half_spaces / scenes.clip_ray, hull by hull, for the lidar
    rays of one world at init (unit quaternions up to float32 rounding, so the two placements agree to 1e-6)."""
    import scenes
    ref = lockstep.make_ref(1, 0, 3, (2, 2), (2, 2), threads=1)
    ref.init()
    (b, m), (w, info) = ref.bodies(), ref.walls()
    r = O.observe(b, m, w, info, ref.tensor("self_type"), ref.A)
    b = b.astype(np.float64)
    th = 2 * np.pi * np.arange(30) / 30 + np.pi / 2
    checked = 0
    for i in range(ref.A):
        p0, R = b[0, 11 + i, :3], scenes.quat_to_matrix(b[0, 11 + i, 3:7])
        for k in range(30):
            d = R @ np.array([np.cos(th[k]), np.sin(th[k]), 0.0])
            best = np.inf
            for s in range(scenes.SLOTS):
                if int(m[0, s, 0]) in scenes._MESH:
                    t, _ = scenes.clip_ray(*scenes.half_spaces(int(m[0, s, 0]), b[0, s, :3], b[0, s, 3:7]), p0, d)
                    best = min(best, t if t >= 0 else np.inf)
            hit, t = r["margin"]["lidar_hit"][i, k], r["lidar"][i, k]
            if 0 <= hit < scenes.SLOTS:       # the nearest hull is what the restatement hit, at the same t
                assert abs(best - t) <= 1e-5, (i, k, best, t)
                checked += 1
            elif hit >= 0:                    # a wall came first: no hull is nearer
                assert best >= t - 1e-5, (i, k, best, t)
            else:
                assert best == np.inf, (i, k, best)
    assert checked >= 10, checked
    ref.close()
