"""What can be checked of the table-driven league schedule and of the pool of past policies without a GPU
(gpu_hideseek.league: check_schedule, all_pairs_schedule, past_play_schedule, host_step(pairs=);
gpu_hideseek.population: plan_snapshot; include/hideseek.h: hs_league_set_schedule, hs_league_step_scheduled).
tests/test_gpu_league_scheduled.py compares the kernel with host_step(pairs=) on the synthetic steps of test_league_host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_league_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOLS = [(T, Q, fill) for T in range(1, 16) for Q in range(1, T + 1) if T + Q <= 16 for fill in ("cross", "self")]


# ---- the schedules ----
def test_every_past_play_schedule_is_valid_regular_and_never_past_against_past():
    from gpu_hideseek import league as G
    assert len(POOLS) == 2 * sum(min(T, 16 - T) for T in range(1, 16))
    for T, Q, fill in POOLS:
        pairs = G.past_play_schedule(T, Q, fill)
        N = T + Q
        assert G.check_schedule(pairs, N) == pairs, (T, Q, fill)
        assert len(pairs) == T * (T + Q) <= G.MAX_GROUP == 256, (T, Q, fill)
        sides = np.bincount(np.asarray(pairs).reshape(-1), minlength=N)
        assert sides.tolist() == [2 * T] * N, (T, Q, fill)
        assert not any(i >= T and j >= T for i, j in pairs), (T, Q, fill)
        if fill == "cross":
            assert not any(i == j for i, j in pairs), (T, Q)
        elif Q < T:
            assert sum(i == j for i, j in pairs) == T * (T - Q)
        # the order the contract states
        assert pairs[:2 * T * Q] == [x for t in range(T) for u in range(Q) for x in ((t, T + u), (T + u, t))]
    assert G.past_play_schedule(2, 1) == [(0, 2), (2, 0), (1, 2), (2, 1), (0, 1), (1, 0)]
    assert G.past_play_schedule(2, 1, "self") == [(0, 2), (2, 0), (1, 2), (2, 1), (0, 0), (1, 1)]
    assert G.past_play_schedule(1, 1) == [(0, 1), (1, 0)]


def test_past_play_schedule_refuses_a_pool_larger_than_the_learners_and_more_than_16_policies():
    from gpu_hideseek import league as G
    for T, Q, what in ((2, 3, "num_past must be in"), (2, 0, "num_past must be in"), (0, 0, "num_past must be in"), (9, 8, "at most 16"),
                       (2.0, 1, "num_train must be an integer"), (2, True, "num_past must be an integer")):
        with pytest.raises(ValueError, match=what):
            G.past_play_schedule(T, Q)
    with pytest.raises(ValueError, match="fill"):
        G.past_play_schedule(2, 1, fill="past")


def test_all_pairs_schedule_is_the_fixed_schedule():
    from gpu_hideseek import league as G
    for P in (1, 2, 3, 16):
        pairs = G.all_pairs_schedule(P)
        hp, sp = G.schedule(P * P, P)
        assert pairs == list(zip(hp, sp)) and G.check_schedule(pairs, P) == pairs


def test_check_schedule_names_the_rule():
    from gpu_hideseek import league as G
    ok = [(0, 1), (1, 0)]
    for pairs, N, what in (([(0, 1), (0, 1), (1, 1)], 2, "not regular"), ([(0, 1)], 3, "not regular"), ([(0, 1), (1, 2)], 2, "out of range"),
                           ([(0, -1), (1, 0)], 2, "out of range"), ([], 2, r"group.*\[1, 256\], got 0"), (ok * 128 + [(0, 0)], 2, r"group.*got 257"),
                           (ok, 17, "num_policies must be an integer in"), (ok, 0, "num_policies must be an integer in"), (ok, True, "num_policies"),
                           ([(0, 1, 2)], 2, "pairs must be a list"), (5, 2, "pairs must be a list")):
        with pytest.raises(ValueError, match=what):
            G.check_schedule(pairs, N)
    # the order of the rules: N, then G, then the entries, then regularity
    with pytest.raises(ValueError, match="num_policies"):
        G.check_schedule([], 17)
    with pytest.raises(ValueError, match="group"):
        G.check_schedule([(9, 9)] * 257, 2)
    with pytest.raises(ValueError, match="out of range"):
        G.check_schedule([(0, 1), (0, 1), (0, 5)], 2)
    assert G.check_schedule(ok * 128, 2) == ok * 128 and G.check_schedule([(0, 0)], 1) == [(0, 0)]
    assert G.check_schedule(np.array([[0, 1], [1, 0]]), 2) == ok


# ---- host_step(pairs=) ----
def _host_run(worlds, N, k, calls, pairs):
    from gpu_hideseek import league as G
    st, counts, elo = H.new_state(worlds), np.zeros((N, N, 4), np.int64), np.full(N, 1500.0)
    res, elos = [], []
    for c in calls:
        r = G.host_step(st, counts, elo, N, k, c["done"], c["self_type"], c["self_mask"], c["episode_result"], c["hider_team"], pairs=pairs)
        r.update(world_hider_team=st["world_hider_team"].copy(), world_phase=st["world_phase"].copy(), counts=counts.copy())
        res.append(r)
        elos.append(elo.copy())
    return res, st, counts, elos


@pytest.mark.parametrize("P,k,worlds", [(2, 1, 4), (3, 3, 261)])
def test_the_all_pairs_table_is_the_fixed_schedule_bit_for_bit(P, k, worlds):
    from gpu_hideseek import league as G
    calls = H.synthetic_steps(worlds, P, k, 24, seed=100 + P)
    want, wst, wcounts, welos = H.host_run(worlds, P, k, calls)
    got, gst, gcounts, gelos = _host_run(worlds, P, k, calls, G.all_pairs_schedule(P))
    assert wcounts.sum() > 0
    for a, b in zip(want, got):
        assert a["bad"] == b["bad"]
        for n in ("policy_assignments", "slot", "row_of_slot", "clear_slot", "world_hider_team", "world_phase", "counts"):
            assert np.array_equal(a[n], b[n]) and a[n].dtype == b[n].dtype, n
    for a, b in zip(welos, gelos):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert np.array_equal(wcounts, gcounts) and all(np.array_equal(wst[n], gst[n]) for n in wst)


def test_a_pool_schedule_routes_a_permutation_with_equal_blocks_that_survives_flips():
    from gpu_hideseek import league as G
    T, Q, k, worlds = 3, 2, 3, 270
    N, A = T + Q, 2 * k
    R = worlds * A
    pairs = G.past_play_schedule(T, Q)
    calls = H.synthetic_steps(worlds, N, k, 24, seed=7)
    res, _, counts, elos = _host_run(worlds, N, k, calls, pairs)
    owned = None
    for c, r in zip(calls, res):
        pol, slot = r["policy_assignments"], r["slot"]
        assert sorted(slot.tolist()) == list(range(R))
        assert np.array_equal(r["row_of_slot"][slot], np.arange(R)) and np.array_equal(r["clear_slot"][slot], c["done"])
        assert np.array_equal(pol, slot // (R // N))                           # block p holds only policy p's rows
        assert np.bincount(pol, minlength=N).tolist() == [R // N] * N
        sets = [frozenset(slot[w * A:(w + 1) * A].tolist()) for w in range(worlds)]
        assert owned is None or sets == owned                                  # a world's slots are the same before and after a flip
        owned = sets
        st, mask = c["self_type"].reshape(worlds, A), c["self_mask"].reshape(worlds, A)
        malformed = ((st != 0).sum(1) != k) | (mask == 0).any(1)
        for w in range(0, worlds, 7):
            i, j = pairs[w % len(pairs)]
            side = (np.arange(A) < k) if malformed[w] else st[w] != 0
            assert np.array_equal(pol[w * A:(w + 1) * A], np.where(side, i, j))
    assert len({tuple(c["self_type"]) for c in calls}) > 10                    # teams did flip
    present = np.zeros((N, N), bool)
    for i, j in pairs:
        present[i, j] = True
    assert counts.sum() > 0 and (counts[~present] == 0).all() and (counts[T:, T:] == 0).all()
    assert (counts[present].sum(1) > 0).all()
    for e in elos:
        assert abs(e.sum() - N * 1500.0) <= H.ELO_TOL
    assert float(np.abs(elos[-1] - 1500.0).max()) > 1.0


def test_repeated_self_pairs_book_into_one_cell():
    from gpu_hideseek import league as G
    pairs = G.past_play_schedule(2, 1, "self") + G.past_play_schedule(2, 1, "self")      # every pair twice: G = 12
    assert G.check_schedule(pairs, 3) == pairs
    worlds, k = 24, 1
    st = dict(world_hider_team=np.zeros(worlds, np.int32), world_phase=np.ones(worlds, np.int32))
    counts, elo = np.zeros((3, 3, 4), np.int64), np.full(3, 1500.0)
    er = np.tile(np.array([1.0, 0.0], np.float32), (worlds, 1))
    r = G.host_step(st, counts, elo, 3, k, np.ones(2 * worlds, np.int32), np.tile(np.array([1, 0], np.int32), worlds), np.ones(2 * worlds, np.float32), er,
                    np.zeros(worlds, np.int32), pairs=pairs)
    assert sorted(r["slot"].tolist()) == list(range(2 * worlds))
    assert counts[0, 0, 0] == 4 and counts[1, 1, 0] == 4 and counts[0, 2, 0] == 4 and counts[2, 2].sum() == 0 and counts.sum() == worlds


def test_request_takes_the_group_for_the_shape_rule():
    import torch
    from gpu_hideseek import league as G

    class Sim:
        num_worlds, agents_per_world, gpu_id = 12, 6, 0

    def call(sim, N, **kw):
        return G.request(sim.num_worlds, sim.agents_per_world, sim.gpu_id, N, 3, G.new_state(sim.num_worlds, "cpu"), torch.zeros(N, N, 4, dtype=torch.int64),
                         torch.full((N,), 1500.0, dtype=torch.float64), **kw)
    with pytest.raises(ValueError, match=r"multiple of num_policies\^2"):
        call(Sim, 3)
    with pytest.raises(ValueError, match="multiple of the schedule's group = 8"):
        call(Sim, 3, group=8)
    for g in (0, 257, 6.0, True):
        with pytest.raises(ValueError, match="group must be an integer in"):
            call(Sim, 3, group=g)
    with pytest.raises(ValueError, match="world_hider_team must be on cuda:0"):          # the shape passes with G = 6
        call(Sim, 3, group=6)
    # the simulator's faces refuse before the library is involved
    sim = Sim()
    with pytest.raises(ValueError, match="no schedule is set"):
        G.compute_scheduled(sim, 3, 3, G.new_state(12, "cpu"), torch.zeros(3, 3, 4, dtype=torch.int64), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="not regular"):
        G.set_schedule(sim, [(0, 1)], 3)
    sim._league_schedule = (6, 3)
    with pytest.raises(ValueError, match="num_policies must equal the schedule's 3"):
        G.compute_scheduled(sim, 2, 3, G.new_state(12, "cpu"), torch.zeros(2, 2, 4, dtype=torch.int64), torch.zeros(2, dtype=torch.float64))


# ---- the snapshots ----
def test_plan_snapshot_fills_the_pool_as_a_ring_from_the_best_learner():
    from gpu_hideseek import population as Pn
    T, Q = 4, 3
    elo = [1500.0, 1620.0, 1480.0, 1400.0]
    assert [Pn.plan_snapshot(elo, taken, Q) for taken in range(7)] == [(4 + taken % 3, 1) for taken in range(7)]
    assert Pn.plan_snapshot([1500.0, 1600.0, 1600.0, 1600.0], 0, Q) == (T, 1)          # ties go to the lower index
    assert Pn.plan_snapshot([1500.0] * 4, 5, Q) == (T + 2, 0)
    assert [Pn.plan_snapshot([1400.0, 1500.0], taken, 1) for taken in range(3)] == [(2, 1)] * 3      # Q = 1: always the one slot
    assert Pn.plan_snapshot([1500.0], 0, 1) == (1, 0)
    for bad in (dict(taken=-1), dict(num_past=0), dict(elo_train=[])):
        with pytest.raises(ValueError):
            Pn.plan_snapshot(**dict(dict(elo_train=elo, taken=0, num_past=Q), **bad))


def test_population_config_applies_the_schedules_shape_rules():
    from gpu_hideseek import population as Pn
    cfg = lambda **kw: Pn.PopulationConfig(**dict(dict(steps_per_update=8, num_bptt_chunks=2, num_minibatches=2, num_epochs=1, num_policies=2, team_size=3,      # noqa: E731
                                                       num_past_policies=1), **kw))
    Pn.check_population_config(cfg(), 12, 6)
    Pn.check_population_config(cfg(num_past_policies=0), 12, 6)
    for kw, worlds, what in ((dict(), 8, "multiple of the schedule's group = 6"), (dict(num_past_policies=3), 12, "num_past must be in"),
                             (dict(num_past_policies=-1), 12, "num_past_policies"), (dict(num_past_policies=1.0), 12, "num_past_policies"),
                             (dict(snapshot_interval=-1), 12, "snapshot_interval"), (dict(snapshot_interval=2, num_past_policies=0), 12, "snapshot_interval"),
                             (dict(past_fill="past"), 12, "fill"), (dict(num_minibatches=5), 12, "minibatches"),
                             (dict(num_policies=9, num_past_policies=8), 9 * 17, "at most 16")):
        with pytest.raises(ValueError, match=what):
            Pn.check_population_config(cfg(**kw), worlds, 6)


# ---- tools/train.py ----
def test_train_tool_takes_the_pools_flags(capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("hs_train_tool", os.path.join(ROOT, "tools", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    base = ["--num-worlds", "32", "--num-updates", "1"]
    for argv, what in ((["--pbt-past-policies", "2"], "--pbt-past-policies needs --pbt-ensemble-size"),
                       (["--pbt-ensemble-size", "2", "--pbt-snapshot-interval", "3"], "--pbt-snapshot-interval needs --pbt-past-policies")):
        with pytest.raises(SystemExit):
            train.parse(base + argv)
        assert what in capsys.readouterr().err
    cfg = train.config(train.parse(base + ["--pbt-ensemble-size", "4", "--pbt-past-policies", "2", "--pbt-snapshot-interval", "5"]))
    assert (cfg.num_policies, cfg.num_past_policies, cfg.snapshot_interval, cfg.past_fill) == (4, 2, 5, "cross")
    assert train.config(train.parse(base + ["--pbt-ensemble-size", "4"])).num_past_policies == 0
    assert "Not here: pools of past policies" not in train.__doc__ and "--pbt-past-policies Q" in train.__doc__


# ---- the header ----
def test_header_mirror_and_symbols_agree(hideseek_lib):
    from gpu_hideseek import league as G
    src = open(os.path.join(ROOT, "include", "hideseek.h")).read()
    flat = " ".join(src.split())
    assert "int32_t hs_league_set_schedule(hs_sim *sim, const int32_t *pairs_host, int32_t group, int32_t num_policies);" in flat
    assert "int32_t hs_league_step_scheduled(hs_sim *sim, const hs_league_request *req);" in flat
    assert "int32_t hs_league_step_scheduled_async(hs_sim *sim, void *hip_stream, const hs_league_request *req);" in flat
    assert int(re.search(r"#define HS_LEAGUE_MAX_GROUP (\d+)", src).group(1)) == G.MAX_GROUP == G.MAX_POLICIES ** 2
    assert C.sizeof(G.HsLeagueRequest) == 128                 # the scheduled step takes the same request
    L = C.CDLL(hideseek_lib)
    for name in ("hs_league_set_schedule", "hs_league_step_scheduled", "hs_league_step_scheduled_async"):
        assert hasattr(L, name), name
