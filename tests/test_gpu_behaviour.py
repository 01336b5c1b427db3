"""Behaviour statistics on the GPU (sim.behaviour_stats, hs_behaviour_stats, csrc/hs_k_behaviour.h) against the numpy
restatement of tests/test_behaviour_host.py: synthetic inputs through explicit pointers, every state array bit for bit
after every call; the simulator's own state through null pointers next to the explicit form fed from its exports; an
independent float64 check on recorded exports; the refusals of the C ABI; the hooks of the four drivers; two shards."""
import ctypes as C

import numpy as np
import pytest

import test_behaviour_host as H
from test_behaviour_host import BOXES, EPS, F32_SUMS, HIDERS, INPUTS, ROW_KEYS, STATS, WORLD_KEYS

pytestmark = pytest.mark.gpu

# (worlds, A): (hiders, seekers, calls).  13 and 22 worlds: a partial workgroup and counts no lane layout divides; 130
# worlds of 2 rows: three workgroups of one lane per world, the last one partial
SHAPES = {(13, 5): (3, 2, 300), (22, 6): (3, 3, 300), (130, 2): (1, 1, 120)}
IDS = ["13x5", "22x6", "130x2"]
KEYS = WORLD_KEYS + ROW_KEYS


def _sim(worlds, hiders, seekers, flags=0, seed=0, min_each=None, **kw):
    import gpu_hideseek
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=flags, rand_seed=seed,
        min_hiders=hiders if min_each is None else min_each, max_hiders=hiders, min_seekers=seekers if min_each is None else min_each,
        max_seekers=seekers, num_pbt_policies=1, **kw)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x.view(np.int64) if x.dtype == np.float64 else x


def _state_np(state):
    return {k: t.cpu().numpy() for k, t in state.items()}


def _same_state(got, want, tag):
    for k in KEYS:
        ne = _bits(got[k]) != _bits(want[k]).reshape(got[k].shape)
        assert not ne.any(), (tag, k, int(ne.sum()), np.argwhere(ne)[:3].tolist())


def _check_table(got, want, booked, tag):
    """The sums of integers bit-equal (exact in any order); the sums of f32 values (maxima, travel) within
    (n - 1) 2^-53 sum |x| of the exact sum of the n values the restatement booked: the bound of a reordered f64 sum."""
    for i in range(STATS):
        if i in F32_SUMS:
            bound, exact = H.sum_bound(booked.get(i, []))
            print(f"{tag} [{i}]: |sum - exact| = {abs(got[i] - exact):.3e}, bound {bound:.3e}, n = {len(booked.get(i, []))}")
            assert abs(got[i] - exact) <= bound, (tag, i, got[i], exact, bound)
        else:
            assert got[i] == want[i], (tag, i, got[i], want[i])


def _device_inputs(calls):
    """{name: [calls, ...] tensor} on the device; grabbing at a stride of 3 elements inside a wider buffer."""
    import torch
    dev = {k: torch.from_numpy(np.stack([c[k] for c in calls])).cuda() for k in INPUTS if k != "grabbing"}
    wide = torch.full((len(calls), calls[0]["grabbing"].size, 3), float("nan"), device="cuda")
    wide[:, :, 1] = torch.from_numpy(np.stack([c["grabbing"] for c in calls])).cuda()
    dev["grabbing"] = wide[:, :, 1]
    return dev


_RUNS = {}


def _synthetic(worlds, A):
    """The synthetic calls through the kernel, every state array checked against the restatement after every call, once
    per shape."""
    import torch
    from gpu_hideseek import behaviour as B
    if (worlds, A) in _RUNS:
        return _RUNS[worlds, A]
    hiders, seekers, ncalls = SHAPES[worlds, A]
    calls = H.synthetic_calls(worlds, A, ncalls)
    dev = _device_inputs(calls)
    sim = _sim(worlds, hiders, seekers)
    sim.init()
    assert sim.agents_per_world == A and dev["grabbing"][0].stride(0) == 3
    st, table = B.new_state(worlds, A, "cuda"), torch.zeros(STATS, dtype=torch.float64, device="cuda")
    want_st, want_table, booked = H.new_state(worlds, A), np.zeros(STATS), {}
    for i, c in enumerate(calls):
        sim.behaviour_stats(st, table, move_eps=EPS, **{k: dev[k][i] for k in INPUTS})
        H.behaviour_step(want_st, want_table, A, **c, booked=booked)
        _same_state(_state_np(st), want_st, (worlds, A, i))
    got = table.cpu().numpy()
    assert np.isfinite(got).all() and got[0] > 50 and got[2] > 0
    _check_table(got, want_table, booked, f"{worlds}x{A}")
    _RUNS[worlds, A] = dict(sim=sim, dev=dev, ncalls=ncalls, state=_state_np(st), table=got)
    return _RUNS[worlds, A]


@pytest.fixture(scope="module", autouse=True)
def _close_sims():
    yield
    for r in _RUNS.values():
        r["sim"].close()
    _RUNS.clear()


@pytest.mark.parametrize("shape", list(SHAPES), ids=IDS)
def test_synthetic_calls_equal_the_restatement_after_every_call(shape):
    _synthetic(*shape)


@pytest.mark.parametrize("shape", list(SHAPES), ids=IDS)
def test_a_second_run_gives_the_same_bits_and_the_table_does_not_reach_the_state(shape):
    import torch
    from gpu_hideseek import behaviour as B
    worlds, A = shape
    r = _synthetic(worlds, A)
    sim, dev = r["sim"], r["dev"]
    st, table = B.new_state(worlds, A, "cuda"), torch.zeros(STATS, dtype=torch.float64, device="cuda")
    st2, table2 = B.new_state(worlds, A, "cuda"), torch.full((STATS,), 12345.678, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    for i in range(r["ncalls"]):
        kw = {k: dev[k][i] for k in INPUTS}
        sim.behaviour_stats(st, table, move_eps=EPS, **kw)
        with torch.cuda.stream(stream):                   # the stream form, and another table
            sim.behaviour_stats(st2, table2, move_eps=EPS, stream=stream, **kw)
        stream.synchronize()
    _same_state(_state_np(st), r["state"], "second run")
    assert np.array_equal(_bits(table.cpu().numpy()), _bits(r["table"]))
    _same_state(_state_np(st2), r["state"], "another table")
    assert not np.array_equal(table2.cpu().numpy(), r["table"])


def test_eager_step_on_the_device_follows_the_kernel():
    import torch
    from gpu_hideseek import behaviour as B
    worlds, A = 13, 5
    r = _synthetic(worlds, A)
    dev = r["dev"]
    st, table = B.new_state(worlds, A, "cuda"), torch.zeros(STATS, dtype=torch.float64, device="cuda")
    for i in range(r["ncalls"]):
        B.eager_step(st, table, A, *(dev[k][i] for k in INPUTS), move_eps=EPS)
    got, tb = _state_np(st), table.cpu().numpy()
    for k in KEYS:
        if k == "travel":                                 # up to the rounding of torch.sqrt (test_behaviour_host.SQRT_RTOL)
            assert np.allclose(got[k], r["state"][k], rtol=H.SQRT_RTOL, atol=0)
        else:
            assert np.array_equal(_bits(got[k]), _bits(r["state"][k])), k
    for i in range(STATS):
        assert abs(tb[i] - r["table"][i]) <= (H.SQRT_RTOL * r["table"][i] if i in F32_SUMS else 0), (i, tb[i], r["table"][i])


# ---- the C ABI ----
def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import behaviour as B
    from lockstep import EXT_SKIP_OBSERVATIONS
    INVALID, UNSUPPORTED = 1, 3
    worlds, A = 4, 4
    rows = worlds * A
    f32 = lambda n: torch.full((n + 8,), -7.0, device="cuda")                        # noqa: E731
    i32 = lambda n: torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")       # noqa: E731
    sizes = dict(phase=worlds, n_obj=2 * worlds, n_side=2 * worlds, start_pos=22 * worlds, prep_pos=22 * worlds, last_pos=34 * worlds, prep_locks=11 * worlds,
                 last_locks=11 * worlds, travel=2 * worlds, grab=2 * worlds, agent_steps=2 * worlds, was_active=rows)
    state = {k: (f32 if k in ("start_pos", "prep_pos", "last_pos", "travel") else i32)(n) for k, n in sizes.items()}
    assert tuple(state) == KEYS
    table = torch.full((STATS + 2,), -7.0, dtype=torch.float64, device="cuda")
    inputs = dict(positions=f32(34 * worlds), locks=i32(11 * worlds), counts=i32(4 * worlds), prep_counter=i32(rows), done=i32(rows), self_type=i32(rows),
                  self_mask=f32(rows), grabbing=f32(13 * rows))
    assert tuple(inputs) == INPUTS
    big = f32(80 * worlds)

    def req(move_eps=EPS, grab_stride=13, **kw):
        p = {k: t.data_ptr() for k, t in {**inputs, **state, "table": table}.items()}
        p.update(kw)
        return B.HsBehaviourRequest(*(p[k] for k in INPUTS), grab_stride, move_eps, *(p[k] for k in KEYS), p["table"])

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in (*state.values(), *inputs.values(), table, big))

    def call(sim, r, stream=False):
        p = C.byref(r) if r is not None else None
        if stream:
            return sim._L.hs_behaviour_stats_async(sim._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p)
        return sim._L.hs_behaviour_stats(sim._h, p)

    def message(sim):
        return sim._L.hs_last_error().decode()

    sim = _sim(worlds, 2, 2)
    for stream in (False, True):
        assert call(sim, req(), stream) == INVALID and "before hs_init" in message(sim)
    assert untouched()
    sim.init()
    nan, inf = float("nan"), float("inf")
    at = lambda t, off: t.data_ptr() + off           # noqa: E731
    bad = {"null request": (None, "null request"), "null table": (req(table=None), "null table"),
           "eps -0.5": (req(move_eps=-0.5), "move_eps"), "eps nan": (req(move_eps=nan), "move_eps"), "eps inf": (req(move_eps=inf), "move_eps"),
           "eps -inf": (req(move_eps=-inf), "move_eps"), "stride 0": (req(grab_stride=0), "grab_stride"), "stride -13": (req(grab_stride=-13), "grab_stride"),
           "positions +2": (req(positions=at(inputs["positions"], 2)), "aligned"), "locks +1": (req(locks=at(inputs["locks"], 1)), "aligned"),
           "counts +2": (req(counts=at(inputs["counts"], 2)), "aligned"), "done +1": (req(done=at(inputs["done"], 1)), "aligned"),
           "grabbing +2": (req(grabbing=at(inputs["grabbing"], 2)), "aligned"), "last_pos +2": (req(last_pos=at(state["last_pos"], 2)), "aligned"),
           "was_active +1": (req(was_active=at(state["was_active"], 1)), "aligned"), "table +4": (req(table=at(table, 4)), "8-byte"),
           "start = prep": (req(start_pos=big.data_ptr(), prep_pos=at(big, 4 * (22 * worlds - 1))), "prep_pos overlaps start_pos"),
           "grab in counts": (req(grab=at(inputs["counts"], 4 * (4 * worlds - 1))), "grab overlaps counts"),
           "last_pos in positions": (req(last_pos=inputs["positions"].data_ptr()), "last_pos overlaps positions"),
           "table in phase": (req(table=at(state["phase"], 8)), "table overlaps phase"),
           "was_active in the strided grabbing": (req(was_active=at(inputs["grabbing"], 4 * 13 * (rows - 1))), "was_active overlaps grabbing"),
           "the sim's own positions": (req(positions=None, prep_pos=sim.global_positions_tensor().to_torch().data_ptr()), "prep_pos overlaps positions"),
           "the sim's own self_data": (req(grabbing=None, travel=at(sim.self_data_tensor().to_torch(), 4 * 12)), "travel overlaps grabbing")}
    for k in KEYS:
        bad["null " + k] = (req(**{k: None}), "null state pointer")
    before = sim.global_positions_tensor().to_torch().clone()
    for stream in (False, True):
        for name, (r, what) in bad.items():
            assert call(sim, r, stream) == INVALID, (name, stream)
            assert what in message(sim) and message(sim).startswith("hs_behaviour_stats"), (name, message(sim))
    assert untouched() and torch.equal(before, sim.global_positions_tensor().to_torch())
    # a stride is not looked at where grabbing is the simulator's own
    st, tb = B.new_state(worlds, A, "cuda"), torch.zeros(STATS, dtype=torch.float64, device="cuda")
    ok = B.request(worlds, A, 0, st, tb)[1]
    ok.grab_stride = -1
    assert call(sim, ok) == 0 and bool((st["phase"] != 0).all())
    # inside an open step
    sim.step_begin()
    assert call(sim, req()) == INVALID and "open step" in message(sim)
    sim.step_end()
    assert untouched()
    sim.close()
    # no observations: a null observation-time input is refused, the explicit form works
    skip = _sim(worlds, 2, 2, flags=EXT_SKIP_OBSERVATIONS)
    skip.init()
    for k in ("positions", "prep_counter", "self_type", "self_mask", "grabbing"):
        assert call(skip, req(**{k: None})) == UNSUPPORTED and "HS_FLAG_EXT_SKIP_OBSERVATIONS" in message(skip)
    assert untouched()
    st, tb = B.new_state(worlds, A, "cuda"), torch.zeros(STATS, dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError, match="SKIP_OBSERVATIONS"):
        skip.behaviour_stats(st, tb)
    ones = torch.ones(rows, dtype=torch.int32, device="cuda")
    skip.behaviour_stats(st, tb, positions=torch.ones(worlds, 17, 2, device="cuda"), prep_counter=ones, self_type=ones, self_mask=torch.ones(rows, device="cuda"),
                         grabbing=torch.ones(rows, 13, device="cuda")[:, 12])
    assert st["phase"].cpu().tolist() == [1] * worlds and st["agent_steps"].cpu().tolist() == [[0, A]] * worlds and st["last_pos"].cpu().eq(1).all()
    skip.close()


# ---- the simulator's own state ----
REAL_WORLDS, REAL_STEPS, EPISODE, PREP = 64, 490, 240, 96


def _exports(sim, worlds):
    """What the explicit form is fed, from the exports alone, on the device, and the same on the host."""
    import torch
    from gpu_hideseek import replay
    A = sim.agents_per_world
    rows = worlds * A
    get = lambda n: getattr(sim, n + "_tensor")().to_torch()          # noqa: E731
    mask = get("self_mask").reshape(worlds, A)
    first = (mask != 0).to(torch.int32).argmax(1) + torch.arange(worlds, device=mask.device) * A      # each world's lowest active row
    box, ramp = get("box_data").reshape(rows, 9, 17)[first], get("ramp_data").reshape(rows, 2, 14)[first]
    lock = lambda x, c: (x[:, :, c] != 0).to(torch.int32) + 2 * (x[:, :, c + 1] != 0).to(torch.int32)    # noqa: E731
    ctrl = sim.ckpt_ctrl_tensor().to_torch()
    ctrl.fill_(1)
    sim.save_checkpoints()
    rec = sim.ckpt_tensor().to_torch().reshape(worlds, replay.CHECKPOINT_BYTES)[:, -16:].contiguous().view(torch.int32)      # numHiders, numSeekers, numBoxes, numRamps
    x = dict(positions=get("global_positions").reshape(worlds, 17, 2).clone(), locks=torch.cat([lock(box, 15), lock(ramp, 12)], 1).contiguous(),
             counts=rec[:, [2, 3, 0, 1]].contiguous(), prep_counter=get("prep_counter").reshape(rows).clone(), done=get("done").reshape(rows).clone(),
             self_type=get("self_type").reshape(rows).clone(), self_mask=mask.reshape(rows).clone(), grabbing=get("self_data").reshape(rows, 13).clone()[:, 12])
    return x


def _random_actions(sim, g):
    import torch
    action = sim.action_tensor().to_torch()
    hi = torch.tensor([5, 5, 5, 2, 2], device="cuda")     # move, turn, rotate, grab, lock
    action.copy_((torch.rand(action.shape, generator=g, device="cuda") * hi).to(torch.int32).clamp_(max=hi - 1))


@pytest.fixture(scope="module")
def real():
    """64 worlds of 1..3 hiders and 1..3 seekers with RandomFlipTeams, 490 steps of random actions, grab and lock drawn
    too: a BehaviourStats through null pointers, and next to it the explicit form on a second state fed from the exports."""
    import torch
    import gpu_hideseek
    from gpu_hideseek import behaviour as B
    sim = _sim(REAL_WORLDS, 3, 3, flags=int(gpu_hideseek.SimFlags.RandomFlipTeams), seed=11, min_each=1)
    sim.init()
    A = sim.agents_per_world
    bh = B.BehaviourStats(sim, move_eps=EPS).arm(from_start=True)
    st, table = B.new_state(REAL_WORLDS, A, "cuda"), torch.zeros(STATS, dtype=torch.float64, device="cuda")
    x = _exports(sim, REAL_WORLDS)
    sim.behaviour_stats(st, table, move_eps=EPS, **x)
    seen = [{k: v.cpu().numpy() for k, v in x.items()}]
    g = torch.Generator(device="cuda").manual_seed(3)
    for _ in range(REAL_STEPS):
        _random_actions(sim, g)
        sim.step()
        bh.step()
        x = _exports(sim, REAL_WORLDS)
        sim.behaviour_stats(st, table, move_eps=EPS, **x)
        seen.append({k: v.cpu().numpy() for k, v in x.items()})
    yield dict(sim=sim, bh=bh, seen=seen, null_state=_state_np(bh.state), null_table=bh.table.cpu().numpy(), state=_state_np(st), table=table.cpu().numpy(), A=A)
    sim.close()


def test_null_pointers_and_the_exports_give_the_same_bits(real):
    from gpu_hideseek import behaviour as B
    A, seen = real["A"], real["seen"]
    # the input, on the host first: every world has an active row in every observation, so `bad` must stay 0
    assert all((x["self_mask"].reshape(REAL_WORLDS, A) != 0).any(1).all() for x in seen)
    assert len({tuple(x["counts"][:, 2]) for x in seen}) >= 2 and len({tuple(x["self_type"]) for x in seen}) >= 2     # sizes changed, teams flipped
    assert any(x["locks"].any() for x in seen) and any(x["grabbing"].any() for x in seen)
    _same_state(real["null_state"], real["state"], "null against explicit")
    assert np.array_equal(_bits(real["null_table"]), _bits(real["table"]))
    t = real["table"]
    assert t[B.WORLD_EPISODES] == 2 * REAL_WORLDS and t[B.REACHED_MAIN] == 2 * REAL_WORLDS and t[B.BAD] == 0
    assert t[B.BOXES + 8] == sum(int(seen[e * EPISODE]["counts"][:, 0].sum()) for e in (0, 1))
    assert t[B.SEEKERS + 2] + t[B.HIDERS + 2] == sum(int((seen[i]["self_mask"] != 0).sum()) for i in range(2 * EPISODE))
    assert t[B.HIDERS] > 0 and t[B.SEEKERS] > 0 and t[B.BOXES] > 0
    # and the restatement on the recorded exports
    st, table, booked = H.new_state(REAL_WORLDS, A), np.zeros(STATS), {}
    for x in seen:
        H.behaviour_step(st, table, A, **x, booked=booked)
    _same_state(real["state"], st, "real")
    _check_table(real["table"], table, booked, "real")
    m = real["bh"].read()
    assert m == B.stats_to_metrics(t) and not real["bh"].table.cpu().numpy().any() and real["bh"].steps == REAL_STEPS


def test_an_independent_float64_check_on_three_worlds():
    """Three worlds as their own simulator, so that a read() after the step that ends their episodes holds those three
    episodes alone; the same quantities from the recorded exports in float64 with plain numpy, not through the
    restatement.  d has two differences, two products, a sum and a root, each rounded to f32: a maximum lies within
    4 x 2^-24 relative of the exact one (each rounding moves d by at most 2^-24 relative, the differences' and the
    products' pairwise); a travel sum of n terms adds (n - 1) roundings of at most 2^-24 of the final sum each."""
    import torch
    import gpu_hideseek
    from gpu_hideseek import behaviour as B
    worlds = 3
    sim = _sim(worlds, 3, 3, flags=int(gpu_hideseek.SimFlags.RandomFlipTeams), seed=23, min_each=1)
    sim.init()
    bh = B.BehaviourStats(sim, move_eps=EPS).arm(from_start=True)
    seen, tables = [{k: v.cpu().numpy().astype(np.float64) for k, v in _exports(sim, worlds).items()}], []
    g = torch.Generator(device="cuda").manual_seed(8)
    for i in range(1, 2 * EPISODE + 1):
        _random_actions(sim, g)
        sim.step()
        bh.step()
        seen.append({k: v.cpu().numpy().astype(np.float64) for k, v in _exports(sim, worlds).items()})
        if i % EPISODE == 0:
            assert seen[i]["done"].any()
            tables.append(bh.table.cpu().numpy().copy())
            bh.table.zero_()
    sim.close()
    u = 2.0 ** -24
    for e, t in enumerate(tables):
        assert t[B.WORLD_EPISODES] == worlds
        obs = seen[e * EPISODE:(e + 1) * EPISODE]
        release = next(i for i, x in enumerate(obs) if x["prep_counter"][x["self_mask"] != 0].max() == 0)
        assert release == PREP
        pos = np.stack([x["positions"] for x in obs])                     # [240, worlds, 17, 2]
        max_prep = max_main = travel = travel_abs = 0.0
        terms = 0
        for w in range(worlds):
            nb, nh = int(obs[0]["counts"][w, 0]), int(obs[0]["counts"][w, 2])
            assert nh >= 1
            if nb:                                        # no box: the kernel books +0
                max_prep += np.linalg.norm(pos[release, w, :nb] - pos[0, w, :nb], axis=-1).max()
                max_main += np.linalg.norm(pos[-1, w, :nb] - pos[release, w, :nb], axis=-1).max()
            d = np.linalg.norm(pos[1:, w, 11:11 + nh] - pos[:-1, w, 11:11 + nh], axis=-1)
            travel += d.sum()
            terms = max(terms, d.size)
        print(f"episode {e}: max_prep {t[BOXES]} / {max_prep}, max_main {t[BOXES + 1]} / {max_main}, hider travel {t[HIDERS]} / {travel}")
        assert abs(t[BOXES] - max_prep) <= 4 * u * max_prep and abs(t[BOXES + 1] - max_main) <= 4 * u * max_main
        assert abs(t[HIDERS] - travel) <= 4 * u * travel + (terms - 1) * u * travel and travel > 0


# ---- the hooks ----
def _count_steps(sim):
    steps = [0]
    plain = sim.step

    def counting():
        steps[0] += 1
        return plain()
    sim.step = counting
    return steps


def test_trainer_with_the_tracker_counts_every_step_once_and_changes_nothing():
    import torch
    from gpu_hideseek import behaviour as B, trainer
    from test_gpu_trainer import T, _cfg, _policy, _sim as trainer_sim
    out = []
    for tracked in (True, False):
        sim = trainer_sim()
        tr = trainer.Trainer(sim, _cfg(), net=_policy())
        assert tr.behaviour is None
        steps = _count_steps(sim)
        if tracked:
            tr.behaviour = B.BehaviourStats(sim)
        metrics = [tr.update_iter() for _ in range(2)]
        torch.cuda.synchronize()
        if tracked:
            # collect() steps T times and once more to close the first rollout; the second starts from that closing step
            assert steps[0] == 2 * T + 1 and tr.behaviour.steps == steps[0]
            stats = tr.behaviour.read()
            assert stats["world_episodes"] == 0 and stats["bad"] == 0                     # armed waiting: the first episodes are not whole
            assert (tr.behaviour.state["phase"] == B.PREP).all()                          # every world started with the done of step 240
            assert "behaviour" not in tr.state_dict() and not any("behaviour" in k for m in metrics for k in m)
        out.append(dict(buffers={k: v.cpu().clone() for k, v in tr.rollout.tensors().items()}, params=tr.opt.flat.params.cpu().clone(),
                        metrics=[{k: v for k, v in m.items() if k != "fps"} for m in metrics], keys=set(tr.state_dict())))
        del sim.step
        sim.close()
    a, b = out
    assert a["keys"] == b["keys"]
    for k in a["buffers"]:
        x, y = a["buffers"][k], b["buffers"][k]
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)) if x.dtype.is_floating_point else torch.equal(x, y), k
    assert torch.equal(a["params"].view(torch.int32), b["params"].view(torch.int32))
    assert a["metrics"] == b["metrics"]


def test_population_evaluator_and_league_call_the_tracker_once_per_step():
    import torch
    from gpu_hideseek import behaviour as B, evaluate, league, policy, population
    import test_gpu_population as TP
    # a population of two policies on four worlds
    sim = TP._sim(4, policies=2)
    pop = population.Population(sim, TP._cfg(2), nets=TP._policies(2))
    assert pop.behaviour is None
    steps = _count_steps(sim)
    pop.behaviour = B.BehaviourStats(sim)
    for _ in range(2):
        pop.update_iter()
    torch.cuda.synchronize()
    assert pop.behaviour.steps == steps[0] >= 2 * TP.T and "behaviour" not in pop.state_dict()
    del sim.step
    sim.close()
    # the evaluator and the league, from sim.init(): 243 steps hold one whole episode of every world
    net = policy.make_policy(generator=torch.Generator().manual_seed(7)).cuda()
    for kind in ("evaluator", "league"):
        sim = TP._sim(4, policies=2 if kind == "league" else 1, presteps=0)
        run = evaluate.Evaluator(sim, net, None, seed=2) if kind == "evaluator" else league.League(sim, [(net, None), (net, None)], TP.K_TEAM, seed=2)
        assert run.behaviour is None
        steps = _count_steps(sim)
        run.behaviour = B.BehaviourStats(sim).arm(from_start=True)
        run.run(243)
        assert steps[0] == 243 and run.behaviour.steps == 243
        stats = run.behaviour.read()
        assert stats["world_episodes"] == 4 and stats["reached_main"] == 4 and stats["bad"] == 0
        assert stats["hiders"]["agent_steps"] == 4 * TP.K_TEAM * 240 and stats["boxes"]["objects"] > 0
        del sim.step
        sim.close()


# ---- the sharded face ----
def test_two_shards_equal_the_unsharded_table():
    import torch
    import gpu_hideseek
    from gpu_hideseek import behaviour as B
    devices = [0, 1] if torch.cuda.device_count() >= 2 else [0, 0]
    worlds, steps = 10, 245
    kw = dict(sim_flags=int(gpu_hideseek.SimFlags.RandomFlipTeams), rand_seed=4, min_hiders=1, max_hiders=3, min_seekers=1, max_seekers=2, num_pbt_policies=1)
    one = gpu_hideseek.HideAndSeekSimulator(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, **kw)
    one.init()
    bh = B.BehaviourStats(one, move_eps=EPS).arm(from_start=True)
    ss = gpu_hideseek.ShardedSimulator(devices, worlds, **kw)
    ss.init()
    A = one.agents_per_world
    states = [B.new_state(s.num_worlds, A, torch.device("cuda", s.gpu_id)) for s in ss.shards]
    tables = [torch.zeros(STATS, dtype=torch.float64, device=torch.device("cuda", s.gpu_id)) for s in ss.shards]
    ss.behaviour_stats(states, tables, move_eps=EPS)      # no world is armed: this latches, as arm(from_start=True) does
    for _ in range(steps):
        one.step()
        bh.step()
        ss.step()
        res = ss.behaviour_stats(states, tables, move_eps=EPS)
    assert len(res) == 2 and res[0]["table"] is tables[0]
    want = bh.table.cpu().numpy()
    got = sum(t.cpu().numpy() for t in tables)
    assert want[B.WORLD_EPISODES] == worlds and want[B.HIDERS] > 0
    for k in KEYS:
        assert np.array_equal(_bits(np.concatenate([s[k].cpu().numpy() for s in states])), _bits(bh.state[k].cpu().numpy())), k
    for i in range(STATS):
        # a sum of f32 values: `worlds` terms in another order, (n - 1) 2^-53 sum |x| with every term positive
        assert abs(got[i] - want[i]) <= ((worlds - 1) * 2.0 ** -53 * want[i] if i in F32_SUMS else 0), (i, got[i], want[i])
    with pytest.raises(ValueError, match="one tensor per shard"):
        ss.behaviour_stats(states[0], tables)
    one.close()
    ss.close()
