"""Episode statistics on the GPU (sim.episode_stats, hs_episode_stats, csrc/hs_k_episode.h) against the numpy restatement
of tests/test_episodes_host.py: synthetic inputs through explicit pointers, bit for bit after every call; the simulator's
own exports through null pointers; the trainer with the tracker set; the evaluator and its replay log; the sharded face;
the refusals of the C ABI."""
import ctypes as C
import math

import numpy as np
import pytest

import test_episodes_host as H
from test_episodes_host import GAMMA, ROW_KEYS, SIDE, STATS, WORLD_KEYS

pytestmark = pytest.mark.gpu

SHAPES = {(13, 5): (3, 2), (22, 6): (3, 3)}       # (worlds, A): 65 rows, a world across the wave boundary; 132 rows, a partial last workgroup
CALLS = 300
INPUTS = ("reward", "done", "self_type", "self_mask", "episode_result", "hider_team")


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
    for k in ROW_KEYS + WORLD_KEYS:
        ne = _bits(got[k]) != _bits(want[k])
        assert not ne.any(), (tag, k, int(ne.sum()), np.argwhere(ne)[:3].tolist())


def _disc_bound(booked):
    """(N - 1) 2^-53 sum |x| of a side's booked f32 discounted returns, and their exact sum rounded once."""
    x = [float(v) for v in booked]
    return max(len(x) - 1, 0) * 2.0 ** -53 * sum(abs(v) for v in x), math.fsum(x)


def _check_table(got, want, booked, tag):
    """Counts, sum ret, sum ret^2, sum len and the world counters bit-equal (integers: exact in any order); sum disc within
    the bound of a reordered sum."""
    for side in (0, 1):
        o = side * SIDE
        for i in (0, 1, 2, 4):
            assert got[o + i] == want[o + i], (tag, side, i, got[o + i], want[o + i])
        bound, exact = _disc_bound(booked[side])
        print(f"{tag} side {side}: |sum disc - exact| = {abs(got[o + 3] - exact):.3e}, bound {bound:.3e}, N = {len(booked[side])}")
        assert abs(got[o + 3] - exact) <= bound, (tag, side, got[o + 3], exact, bound)
    assert got[10:].tolist() == want[10:].tolist(), (tag, got[10:], want[10:])


_RUNS = {}


def _synthetic(worlds, A):
    """The CALLS synthetic calls through the kernel, checked against the restatement after every call, once per shape:
    (final device state as numpy, table as numpy, the restatement's booked discounted returns)."""
    import torch
    from gpu_hideseek import episodes as E
    if (worlds, A) in _RUNS:
        return _RUNS[worlds, A]
    calls = H.synthetic_calls(worlds, A, CALLS)
    dev = {k: torch.from_numpy(np.stack([c[k] for c in calls])).cuda() for k in INPUTS}
    sim = _sim(worlds, *SHAPES[worlds, A])
    sim.init()
    assert sim.agents_per_world == A
    st, table = E.new_state(worlds, A, "cuda"), torch.zeros(STATS, dtype=torch.float64, device="cuda")
    want_st, want_table, booked = H.new_state(worlds, A), np.zeros(STATS), ([], [])
    for i, c in enumerate(calls):
        sim.episode_stats(st, table, gamma=GAMMA, **{k: dev[k][i] for k in INPUTS})
        H.episode_step(want_st, want_table, A, c["reward"], c["done"], c["self_type"], c["self_mask"], c["episode_result"], c["hider_team"], GAMMA, booked)
        _same_state(_state_np(st), want_st, (worlds, A, i))
    got = table.cpu().numpy()
    assert np.isfinite(got).all() and got[0] > 50 and got[SIDE] > 50
    _check_table(got, want_table, booked, f"{worlds}x{A}")
    _RUNS[worlds, A] = dict(sim=sim, calls=calls, dev=dev, state=_state_np(st), table=got, want_state=want_st)
    return _RUNS[worlds, A]


@pytest.fixture(scope="module", autouse=True)
def _close_sims():
    yield
    for r in _RUNS.values():
        r["sim"].close()
    _RUNS.clear()


@pytest.mark.parametrize("shape", list(SHAPES), ids=["13x5", "22x6"])
def test_synthetic_calls_equal_the_restatement_after_every_call(shape):
    _synthetic(*shape)


@pytest.mark.parametrize("shape", list(SHAPES), ids=["13x5", "22x6"])
def test_a_second_run_gives_the_same_bits_and_the_table_does_not_reach_the_state(shape):
    import torch
    from gpu_hideseek import episodes as E
    worlds, A = shape
    r = _synthetic(worlds, A)
    sim, dev = r["sim"], r["dev"]
    st, table = E.new_state(worlds, A, "cuda"), torch.zeros(STATS, dtype=torch.float64, device="cuda")
    st2, table2 = E.new_state(worlds, A, "cuda"), torch.full((STATS,), 12345.678, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    for i in range(CALLS):
        kw = {k: dev[k][i] for k in INPUTS}
        sim.episode_stats(st, table, gamma=GAMMA, **kw)
        with torch.cuda.stream(stream):               # the stream form, and another table
            sim.episode_stats(st2, table2, gamma=GAMMA, stream=stream, **kw)
        stream.synchronize()
    _same_state(_state_np(st), r["state"], "second run")
    assert np.array_equal(_bits(table.cpu().numpy()), _bits(r["table"]))
    _same_state(_state_np(st2), r["state"], "another table")
    assert not np.array_equal(table2.cpu().numpy(), r["table"])


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import episodes as E
    from lockstep import EXT_SKIP_OBSERVATIONS
    INVALID, UNSUPPORTED = 1, 3
    worlds, A = 4, 4
    rows = worlds * A
    f32 = lambda n: torch.full((n + 8,), -7.0, device="cuda")                        # noqa: E731
    i32 = lambda n: torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")       # noqa: E731
    state = dict(ret=f32(rows), disc=f32(rows), gpow=f32(rows), len=i32(rows), type=i32(rows), phase=i32(rows), world_hider_team=i32(worlds),
                 world_phase=i32(worlds))
    table = torch.full((STATS + 2,), -7.0, dtype=torch.float64, device="cuda")
    inputs = dict(reward=f32(rows), done=i32(rows), self_type=i32(rows), self_mask=f32(rows), episode_result=f32(2 * worlds), hider_team=i32(worlds))
    big = f32(4 * rows)

    def req(gamma=GAMMA, **kw):
        p = {k: t.data_ptr() for k, t in {**inputs, **state, "table": table}.items()}
        p.update(kw)
        return E.HsEpisodeRequest(p["reward"], p["done"], p["self_type"], p["self_mask"], p["episode_result"], p["hider_team"], gamma, 0,
                                  *(p[k] for k in ROW_KEYS + WORLD_KEYS), p["table"])

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in (*state.values(), *inputs.values(), table, big))

    def call(sim, r, stream=False):
        p = C.byref(r) if r is not None else None
        if stream:
            return sim._L.hs_episode_stats_async(sim._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p)
        return sim._L.hs_episode_stats(sim._h, p)

    def message(sim):
        return sim._L.hs_last_error().decode()

    sim = _sim(worlds, 2, 2)
    for stream in (False, True):
        assert call(sim, req(), stream) == INVALID and "before hs_init" in message(sim)
    assert untouched()
    sim.init()
    nan, inf = float("nan"), float("inf")
    bad = {"null request": (None, "null request"), "null table": (req(table=None), "null table"),
           "gamma 1.5": (req(gamma=1.5), "gamma"), "gamma -0": (req(gamma=-0.001), "gamma"), "gamma nan": (req(gamma=nan), "gamma"),
           "gamma inf": (req(gamma=inf), "gamma"), "gamma -inf": (req(gamma=-inf), "gamma"),
           "reward +2": (req(reward=inputs["reward"].data_ptr() + 2), "aligned"), "done +1": (req(done=inputs["done"].data_ptr() + 1), "aligned"),
           "hider_team +2": (req(hider_team=inputs["hider_team"].data_ptr() + 2), "aligned"), "ret +2": (req(ret=state["ret"].data_ptr() + 2), "aligned"),
           "world_phase +1": (req(world_phase=state["world_phase"].data_ptr() + 1), "aligned"), "table +4": (req(table=table.data_ptr() + 4), "8-byte"),
           "ret = disc": (req(ret=big.data_ptr(), disc=big.data_ptr() + 4 * (rows - 1)), "disc overlaps ret"),
           "len in reward": (req(len=inputs["reward"].data_ptr()), "len overlaps reward"),
           "table in phase": (req(table=state["phase"].data_ptr() + 8), "table overlaps phase"),
           "world team in result": (req(world_hider_team=inputs["episode_result"].data_ptr() + 4 * (2 * worlds - 1)), "world_hider_team overlaps episode_result"),
           "the sim's own reward": (req(reward=None, gpow=sim.reward_tensor().to_torch().data_ptr()), "gpow overlaps reward")}
    for k in ROW_KEYS + WORLD_KEYS:
        bad["null " + k] = (req(**{k: None}), "null state pointer")
    before = sim.reward_tensor().to_torch().clone()
    for stream in (False, True):
        for name, (r, what) in bad.items():
            assert call(sim, r, stream) == INVALID, (name, stream)
            assert what in message(sim) and message(sim).startswith("hs_episode_stats"), (name, message(sim))
    assert untouched() and torch.equal(before, sim.reward_tensor().to_torch())
    # inside an open step
    sim.step_begin()
    assert call(sim, req()) == INVALID and "open step" in message(sim)
    sim.step_end()
    assert untouched()
    sim.close()
    # no observations: the null form is refused, the explicit one works
    skip = _sim(worlds, 2, 2, flags=EXT_SKIP_OBSERVATIONS)
    skip.init()
    for k in ("self_type", "self_mask"):
        assert call(skip, req(**{k: None})) == UNSUPPORTED and "HS_FLAG_EXT_SKIP_OBSERVATIONS" in message(skip)
    assert untouched()
    st, tb = E.new_state(worlds, A, "cuda"), torch.zeros(STATS, dtype=torch.float64, device="cuda")
    with pytest.raises(NotImplementedError, match="SKIP_OBSERVATIONS"):
        skip.episode_stats(st, tb)
    skip.episode_stats(st, tb, self_type=torch.ones(rows, dtype=torch.int32, device="cuda"), self_mask=torch.ones(rows, device="cuda"))
    assert st["phase"].cpu().tolist() == [1] * rows and st["world_phase"].cpu().tolist() == [1] * worlds
    skip.close()


# ---- the simulator's own exports ----
REAL_WORLDS, REAL_STEPS, EPISODE, PREP = 64, 490, 240, 96


@pytest.fixture(scope="module")
def real():
    """64 worlds of 1..3 hiders and 1..3 seekers with RandomFlipTeams, 490 steps of random actions, an EpisodeStats armed
    from the start; the exports copied out after init and after each step."""
    import torch
    import gpu_hideseek
    from gpu_hideseek import episodes as E
    sim = _sim(REAL_WORLDS, 3, 3, flags=int(gpu_hideseek.SimFlags.RandomFlipTeams), seed=11, min_each=1)
    sim.init()
    A = sim.agents_per_world
    rows = REAL_WORLDS * A
    ep = E.EpisodeStats(sim, gamma=GAMMA).arm(from_start=True)

    def exports():
        get = lambda n, k: getattr(sim, n + "_tensor")().to_torch().reshape(k, -1).cpu().numpy().copy()       # noqa: E731
        x = dict(reward=get("reward", rows)[:, 0], done=get("done", rows)[:, 0], self_type=get("self_type", rows)[:, 0],
                 self_mask=get("self_mask", rows)[:, 0], episode_result=get("episode_result", REAL_WORLDS))
        x["hider_team"] = (x["self_type"].reshape(REAL_WORLDS, A)[:, 0] == 0).astype(np.int32)      # team 0 is the world's first rows
        return x
    seen = [exports()]
    g = torch.Generator(device="cuda").manual_seed(3)
    action = sim.action_tensor().to_torch()
    hi = torch.tensor([5, 5, 5, 2, 2], device="cuda")
    for _ in range(REAL_STEPS):
        action.copy_((torch.rand(action.shape, generator=g, device="cuda") * hi).to(torch.int32).clamp_(max=hi - 1))
        sim.step()
        ep.step()
        seen.append(exports())
    table = ep.table.cpu().numpy()
    state = _state_np(ep.state)
    yield dict(sim=sim, ep=ep, seen=seen, table=table, state=state, A=A)
    sim.close()


def test_real_simulator_table_equals_the_restatement(real):
    A, seen = real["A"], real["seen"]
    st, table, booked = H.new_state(REAL_WORLDS, A), np.zeros(STATS), ([], [])
    for i, x in enumerate(seen):                      # seen[0] arms: every row is out and restarts
        H.episode_step(st, table, A, x["reward"], x["done"], x["self_type"], x["self_mask"], x["episode_result"], x["hider_team"], GAMMA, booked)
    _same_state(real["state"], st, "real")
    _check_table(real["table"], table, booked, "real")
    types = {tuple(x["hider_team"]) for x in seen}
    masks = {tuple(x["self_mask"]) for x in seen}
    assert len(types) >= 2 and len(masks) >= 2        # teams flipped and sizes changed between the episodes


def test_real_simulator_counts_lengths_and_winners(real):
    from gpu_hideseek import episodes as E
    A, seen, table = real["A"], real["seen"], real["table"]
    m = E.stats_to_metrics(table)
    assert m["world_episodes"] == REAL_WORLDS * 2
    assert m["hiders"]["length_mean"] == EPISODE and m["seekers"]["length_mean"] == EPISODE
    assert m["hiders"]["episodes"] + m["seekers"]["episodes"] == sum(int(seen[e * EPISODE]["self_mask"].sum()) for e in (0, 1))
    assert all(math.isfinite(v) for s in ("hiders", "seekers") for v in m[s].values())
    wins = np.zeros(3)                                # hiders, seekers, draws
    for e in (0, 1):
        first, last = seen[e * EPISODE], seen[(e + 1) * EPISODE]          # the episode's first observation; its done step
        assert (last["done"][first["self_mask"] != 0] != 0).all()
        for w in range(REAL_WORLDS):
            rows = np.arange(w * A, (w + 1) * A)
            hider = rows[(first["self_type"][rows] == 1) & (first["self_mask"][rows] != 0)][0]
            r = np.array([seen[e * EPISODE + 1 + s]["reward"][hider] for s in range(PREP, EPISODE)])
            r = np.where(r < -5, r + 10, r)           # the -10 boundary penalty removed
            pos, neg = int((r > 0).sum()), int((r < 0).sum())
            assert pos + neg == EPISODE - PREP
            want = 1.0 if pos > neg else 0.0 if pos < neg else 0.5
            assert last["episode_result"][w, first["hider_team"][w]] == want, (e, w, pos, neg)
            wins[0 if pos > neg else 1 if pos < neg else 2] += 1
    assert table[10:13].tolist() == wins.tolist()
    assert abs(m["hider_win_rate"] + m["seeker_win_rate"] + m["draw_rate"] - 1.0) < 1e-12
    # read() is stats_to_metrics of the table, and starts it again
    got = real["ep"].read()
    assert got == m and not real["ep"].table.cpu().numpy().any() and real["ep"].steps == REAL_STEPS


# ---- the trainer ----
def test_trainer_with_the_tracker_counts_every_step_once_and_changes_nothing():
    import torch
    from gpu_hideseek import episodes as E, trainer
    from test_gpu_trainer import T, _cfg, _policy, _sim as trainer_sim
    out = []
    for tracked in (True, False):
        sim = trainer_sim()
        tr = trainer.Trainer(sim, _cfg(), net=_policy())
        assert tr.episodes is None
        steps = [0]
        plain_step = sim.step

        def counting_step(plain_step=plain_step, steps=steps):
            steps[0] += 1
            return plain_step()
        sim.step = counting_step
        if tracked:
            tr.episodes = E.EpisodeStats(sim, gamma=tr.cfg.gamma)
        metrics = [tr.update_iter() for _ in range(2)]
        torch.cuda.synchronize()
        if tracked:
            # collect() steps T times and once more to close the first rollout; the second starts from that closing step:
            # T - 1 and one.  Every one of them reached the tracker, and none twice.
            assert steps[0] == 2 * T + 1 and tr.episodes.steps == steps[0]
            stats = tr.episodes.read()
            assert stats["world_episodes"] == 0 and stats["hiders"]["episodes"] == 0       # armed waiting: the first episodes are not whole
            assert (tr.episodes.state["phase"] == E.TRACKED).all()                         # every row started with the done of step 240
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


# ---- the evaluator ----
def _evaluate(mode, log=None, steps=250, worlds=16):
    import torch
    import gpu_hideseek
    from gpu_hideseek import evaluate, policy
    F = gpu_hideseek.SimFlags
    sim = _sim(worlds, 3, 3, flags=int(F.UseFixedWorld | F.ZeroAgentVelocity), seed=5)
    sim.init()
    net = policy.make_policy(generator=torch.Generator().manual_seed(7)).cuda()
    ev = evaluate.Evaluator(sim, net, None, mode=mode, seed=2)
    positions = []
    stats = ev.run(steps, record_log=log, on_step=lambda i, ev: positions.append(sim.global_positions_tensor().to_torch().cpu().clone()))
    return sim, ev, stats, positions


def test_evaluator_records_a_log_that_plays_back(tmp_path):
    import torch
    from gpu_hideseek import replay
    path = tmp_path / "run.log"
    with open(path, "wb") as f:
        sim, ev, stats, positions = _evaluate("draw", f)
    flat = [v for s in ("hiders", "seekers") for v in stats[s].values()] + [stats[k] for k in ("world_episodes", "hider_win_rate", "seeker_win_rate", "draw_rate")]
    assert all(math.isfinite(v) for v in flat)
    assert stats["world_episodes"] == 16 and stats["hiders"]["episodes"] == 48 and stats["seekers"]["length_mean"] == 240
    log = replay.read_log(str(path), 16)
    assert log.shape[0] == 250 and len(positions) == 250
    replay.replay_step(sim, log, 249)
    assert torch.equal(sim.global_positions_tensor().to_torch().cpu(), positions[249])
    assert not torch.equal(positions[249], positions[100])
    sim.close()


def test_greedy_evaluation_is_deterministic():
    tables = []
    for _ in range(2):
        sim, ev, stats, _ = _evaluate("greedy")
        tables.append(stats)
        sim.close()
    assert tables[0] == tables[1] and tables[0]["world_episodes"] == 16
    with pytest.raises(ValueError, match="mode"):
        from gpu_hideseek import evaluate
        evaluate.Evaluator(None, None, mode="best")


def test_infer_tool_loads_a_trainer_checkpoint_and_writes_a_log(tmp_path, capsys):
    import importlib.util
    import json
    import os
    import torch
    from gpu_hideseek import evaluate, replay, trainer
    from test_gpu_trainer import _cfg, _sim as trainer_sim
    sim = trainer_sim(presteps=0)
    tr = trainer.Trainer(sim, _cfg())
    tr.normaliser.state.copy_(torch.rand(tr.normaliser.state.shape, dtype=torch.float64) + 0.5)
    ckpt = tmp_path / "7"
    torch.save(tr.state_dict(), ckpt)
    net, normaliser = evaluate.load_policy(str(ckpt))
    mine, theirs = dict(tr.net.named_parameters()), dict(net.named_parameters())
    assert list(mine) == list(theirs) and all(torch.equal(mine[k].detach().view(torch.int32), theirs[k].detach().view(torch.int32)) for k in mine)
    assert torch.equal(normaliser.state, tr.normaliser.state)
    with pytest.raises(ValueError, match="laid out"):
        evaluate.load_policy({**tr.state_dict(), "params": torch.zeros(5)})
    sim.close()
    spec = importlib.util.spec_from_file_location("infer_tool", os.path.join(H.ROOT, "tools", "infer.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    log = tmp_path / "run.log"
    stats = tool.main(["--num-worlds", "4", "--num-steps", "243", "--ckpt-path", str(ckpt), "--record-log", str(log), "--greedy"])
    out = capsys.readouterr().out
    assert stats["world_episodes"] == 4 and json.loads(out.strip().splitlines()[-1]) == stats
    assert "hiders" in out and "seekers" in out and "world episodes 4" in out
    assert replay.read_log(str(log), 4).shape[0] == 243


# ---- the sharded face ----
def test_two_shards_equal_the_unsharded_table():
    import torch
    import gpu_hideseek
    from gpu_hideseek import episodes as E
    devices = [0, 1] if torch.cuda.device_count() >= 2 else [0, 0]
    worlds, steps = 10, 245
    kw = dict(sim_flags=int(gpu_hideseek.SimFlags.RandomFlipTeams), rand_seed=4, min_hiders=1, max_hiders=3, min_seekers=1, max_seekers=2, num_pbt_policies=1)
    one = gpu_hideseek.HideAndSeekSimulator(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, **kw)
    one.init()
    ep = E.EpisodeStats(one, gamma=GAMMA).arm(from_start=True)
    ss = gpu_hideseek.ShardedSimulator(devices, worlds, **kw)
    ss.init()
    A = one.agents_per_world
    states = [E.new_state(s.num_worlds, A, torch.device("cuda", s.gpu_id)) for s in ss.shards]
    tables = [torch.zeros(STATS, dtype=torch.float64, device=torch.device("cuda", s.gpu_id)) for s in ss.shards]
    ss.episode_stats(states, tables, gamma=GAMMA)     # every row is out: this latches, as arm(from_start=True) does
    for _ in range(steps):
        one.step()
        ep.step()
        ss.step()
        res = ss.episode_stats(states, tables, gamma=GAMMA)
    assert len(res) == 2 and res[0]["table"] is tables[0]
    want = ep.table.cpu().numpy()
    got = sum(t.cpu().numpy() for t in tables)
    assert want[13] == worlds and want[0] > 0 and want[SIDE] > 0
    for k in ROW_KEYS:
        assert np.array_equal(_bits(np.concatenate([s[k].cpu().numpy() for s in states])), _bits(ep.state[k].cpu().numpy())), k
    for i in range(STATS):
        if i in (3, SIDE + 3):                        # sum disc: N terms of at most 11 x 240 each, in another order
            n = want[i - 3]
            assert abs(got[i] - want[i]) <= 2 * n * 2.0 ** -53 * n * 11 * 240, (i, got[i], want[i])
        else:
            assert got[i] == want[i], (i, got[i], want[i])
    with pytest.raises(ValueError, match="one tensor per shard"):
        ss.episode_stats(states[0], tables)
    one.close()
    ss.close()
