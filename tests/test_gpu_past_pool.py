"""The pool of past policies in the population trainer on the GPU (gpu_hideseek.population with num_past_policies > 0):
T = 2 learners and Q = 1 frozen policy on 12 worlds of 3 + 3 agents (G = 6, R = 72, 24 slots per policy), with
tests/test_gpu_population.py's flags, presteps and config, so that an episode ends and teams flip inside the first rollout.
The routing, the bookings and the ratings are replayed on the host from the recorded exports with
league.host_step(pairs=); the pool stays frozen while the learners learn, and what its columns of the rollout hold cannot
reach a learner; snapshots, their order with exploit, and the checkpoint."""
import numpy as np
import pytest

import test_gpu_population as TP
from test_gpu_population import AGENTS, K_TEAM, T as STEPS
from test_league_host import ELO_TOL, new_state

pytestmark = pytest.mark.gpu

NT, NQ = 2, 1                      # the learners, the pool
N = NT + NQ
WORLDS = 12
R = WORLDS * AGENTS
M = R // N


def _cfg(T=NT, Q=NQ, **kw):
    return TP._cfg(T, num_past_policies=Q, **kw)


def _pop(sim, T=NT, Q=NQ, nets=True, **kw):
    from gpu_hideseek import population
    return population.Population(sim, _cfg(T, Q, **kw), nets=TP._policies(T) if nets else None)


@pytest.fixture(scope="module")
def pooled():
    """Two rollouts and two updates of T = 2, Q = 1, every sim.step() and every league step recorded on the host."""
    from gpu_hideseek import episodes
    sim = TP._sim(WORLDS, N)

    def exports():
        get = lambda n, k: getattr(sim, n + "_tensor")().to_torch().reshape(k, -1).cpu().numpy().copy()       # noqa: E731
        x = dict(done=get("done", R)[:, 0], reward=get("reward", R)[:, 0], self_type=get("self_type", R)[:, 0], self_mask=get("self_mask", R)[:, 0],
                 episode_result=get("episode_result", WORLDS), action=get("action", R))
        x["hider_team"] = (x["self_type"].reshape(WORLDS, -1)[:, 0] == 0).astype(np.int32)        # team 0 is the world's first rows
        return x

    seen, steps, routes = [exports()], [], []
    pop = _pop(sim)
    built = dict(past=pop.past[0].flat.params.clone(), table=pop.tables[NT].clone(), learners=[mb.opt.flat.params.clone() for mb in pop.members],
                 tables=[pop.tables[p].clone() for p in range(NT)])
    pop.episodes = episodes.EpisodeStats(sim).arm(from_start=True)
    routes.append(pop.row_of_slot.cpu().numpy().copy())
    step, league_step = sim.step, pop.league_step

    def recorded_step():
        action_in = sim.action_tensor().to_torch().reshape(R, 5).cpu().numpy().copy()
        step()
        steps.append(dict(exports(), action_in=action_in))

    def recorded_league_step():
        league_step()
        routes.append(pop.row_of_slot.cpu().numpy().copy())
    sim.step, pop.league_step = recorded_step, recorded_league_step
    rollouts, outs = [], []
    for _ in range(2):
        pop.collect()
        rollouts.append({k: getattr(pop.rollout, k).cpu().numpy().copy() for k in ("action", "reward", "done", "clear")})
        outs.append(pop.update())
    table = pop.episodes.table.cpu().numpy()
    sim.step = step
    yield dict(pop=pop, built=built, seen=seen, steps=steps, routes=routes, rollouts=rollouts, outs=outs, table=table)
    sim.close()


def test_slots_hold_what_their_rows_exported_across_a_flip(pooled):
    steps, routes, rollouts = pooled["steps"], pooled["routes"], pooled["rollouts"]
    assert len(steps) == 2 * STEPS + 1 and len(routes) == 2 * STEPS + 2
    for ro in routes:
        assert sorted(ro.tolist()) == list(range(R))
    first = np.stack([s["self_type"].reshape(WORLDS, -1)[:, 0] for s in steps])
    assert (first[0] != first[-1]).any()                                           # some world's sides changed: the flip is crossed
    assert any((a != b).any() for a, b in zip(routes[:-1], routes[1:]))
    for i, buf in enumerate(rollouts):
        for t in range(STEPS):
            g = i * STEPS + t
            ro, nxt = routes[g + 1], steps[g + 1]
            assert np.array_equal(buf["action"][t], nxt["action_in"][ro]), (i, t)
            assert np.array_equal(buf["reward"][t].view(np.int32), nxt["reward"][ro].view(np.int32)), (i, t)
            assert np.array_equal(buf["done"][t], nxt["done"][ro]), (i, t)
            if t + 1 < STEPS:
                assert np.array_equal(buf["clear"][t + 1], buf["done"][t]), (i, t)
    assert np.array_equal(rollouts[1]["clear"][0], rollouts[0]["done"][STEPS - 1])
    assert any((b["done"] != 0).any() for b in rollouts)
    blocks = [rollouts[0]["action"][0][p * M:(p + 1) * M] for p in range(N)]
    assert not np.array_equal(blocks[0], blocks[1])                                # the two learners act differently: a misrouted slot would show


def test_every_game_is_booked_once_and_rated_as_the_restatement_and_none_is_past_against_past(pooled):
    from gpu_hideseek import episodes as E, league as G
    pop, out, table = pooled["pop"], pooled["outs"][-1], pooled["table"]
    pairs = G.past_play_schedule(NT, NQ)
    assert pop.schedule == pairs and pop.sim._league_schedule == (6, N)
    assert out["bad"] == 0 and len(out["elo"]) == N and out["past"] == [0] and "snapshot" not in out
    counts = pop.counts.cpu().numpy()
    assert counts.shape == (N, N, 4)
    assert out["games"] == counts.sum() == table[E.WORLD_EPISODES] == WORLDS           # every world finished one episode
    assert counts[:, :, 0].sum() == table[E.HIDER_WINS] and counts[:, :, 1].sum() == table[E.SEEKER_WINS]
    st, ref_counts, elo = new_state(WORLDS), np.zeros((N, N, 4), np.int64), np.full(N, 1500.0)
    for s, ro in zip(pooled["seen"] + pooled["steps"], pooled["routes"]):
        r = G.host_step(st, ref_counts, elo, N, K_TEAM, s["done"], s["self_type"], s["self_mask"], s["episode_result"], s["hider_team"], pairs=pairs)
        assert r["bad"] == 0 and np.array_equal(r["row_of_slot"], ro)
    assert np.array_equal(ref_counts, counts)
    err = float(np.abs(np.asarray(out["elo"]) - elo).max())
    print(f"max |elo - host| = {err:.3e} (bound {ELO_TOL:.0e})")
    assert err <= ELO_TOL, (out["elo"], elo.tolist())
    assert counts[NT:, NT:].sum() == 0                                             # no past-vs-past cell
    present = np.zeros((N, N), bool)
    for i, j in pairs:
        present[i, j] = True
    assert (counts[~present] == 0).all() and (counts[present].sum(1) == WORLDS // 6).all()


def test_the_pool_stays_frozen_while_the_learners_learn(pooled):
    import torch
    pop, built = pooled["pop"], pooled["built"]
    assert pooled["outs"][-1]["update"] == 2
    pm = pop.past[0]
    assert torch.equal(pm.flat.params, built["past"]) and torch.equal(pop.tables[NT], built["table"])
    assert torch.equal(built["past"], built["learners"][0]) and torch.equal(built["table"], built["tables"][0])       # a copy of learner 0 % T
    assert pm.flat.detached() is None                                              # its net runs on the flat buffer a snapshot copies into
    assert pm.normaliser.table.data_ptr() == pop.tables[NT].data_ptr() and float(pm.normaliser.state.abs().sum()) == 0.0
    for p, mb in enumerate(pop.members):
        assert not torch.equal(mb.opt.flat.params, built["learners"][p]), p
        assert not torch.equal(pop.tables[p], built["tables"][p]), p
    assert not hasattr(pm, "opt") and not hasattr(pm, "generator")
    assert all(tuple(x.shape)[0] == M for x in pm.state)


def test_a_learner_learns_whatever_the_pools_columns_hold():
    import torch
    sim = TP._sim(WORLDS, N)
    try:
        pop = _pop(sim)
        pop.collect()
        saved = pop.state_dict()
        before = [mb.opt.flat.params.clone() for mb in pop.members]
        pop.update()
        after = [mb.opt.flat.params.clone() for mb in pop.members]
        assert all(not torch.equal(a, b) for a, b in zip(after, before))
        pop.load_state_dict(saved)
        assert all(torch.equal(mb.opt.flat.params, b) for mb, b in zip(pop.members, before))
        buf, g, lo = pop.rollout, torch.Generator(device="cuda").manual_seed(9), NT * M
        for k in ("actor", "critic", "log_prob", "value", "advantage", "returns", "reward", "actor_h", "actor_c", "critic_h", "critic_c"):
            x = getattr(buf, k)
            x[:, lo:] = torch.randn(x[:, lo:].shape, generator=g, device="cuda").to(x.dtype)
        for k in ("action", "clear", "done"):
            x = getattr(buf, k)
            x[:, lo:] = torch.randint(0, 2, x[:, lo:].shape, generator=g, device="cuda", dtype=torch.int32)
        pop.update()
        for mb, a in zip(pop.members, after):
            assert torch.equal(mb.opt.flat.params, a)                              # bit for bit
    finally:
        sim.close()


def test_a_snapshot_copies_the_best_learner_and_its_rating():
    import torch
    sim = TP._sim(WORLDS, N)
    try:
        pop = _pop(sim, snapshot_interval=1)
        pop.collect()
        pop.elo.copy_(torch.tensor([1400.0, 1600.0, 1500.0], dtype=torch.float64))
        carried = [x.clone() for x in pop.past[0].state]
        out = pop.update()
        assert out["snapshot"] == (NT, 1) and out["past"] == [1] and out["elo"] == [1400.0, 1600.0, 1500.0] and "exploit" not in out
        pm, src = pop.past[0], pop.members[1]
        assert torch.equal(pm.flat.params, src.opt.flat.params) and torch.equal(pm.net.actor_head.weight, src.net.actor_head.weight)
        assert not torch.equal(pm.flat.params, pop.members[0].opt.flat.params)
        assert torch.equal(pop.tables[NT], pop.tables[1]) and torch.equal(pm.normaliser.state, src.normaliser.state) and src.normaliser.state[-1].item() > 0
        assert torch.equal(pop.elo.view(torch.int64)[NT], pop.elo.view(torch.int64)[1]) and pop.elo.tolist() == [1400.0, 1600.0, 1600.0]
        assert all(torch.equal(a, b) for a, b in zip(pop.past[0].state, carried))   # the carried LSTM state stays
        assert pop.taken == 1 and pop.state_dict()["taken"] == 1
    finally:
        sim.close()


def test_snapshots_fill_the_pool_as_a_ring():
    import torch
    sim = TP._sim(16, 4)
    try:
        pop = _pop(sim, 2, 2, snapshot_interval=1)                                 # G = 8, 24 slots per policy
        assert len(pop.schedule) == 8 and pop.block == 24
        pop.collect()
        outs = []
        for _ in range(3):                                                         # the same rollout again: only the order matters here
            outs.append(pop.update())
        assert [o["snapshot"][0] for o in outs] == [2, 3, 2]
        assert [o["past"] for o in outs] == [[1, 0], [1, 2], [3, 2]]
        best = outs[-1]["snapshot"][1]
        assert torch.equal(pop.past[0].flat.params, pop.members[best].opt.flat.params)
        assert not torch.equal(pop.past[1].flat.params, pop.past[0].flat.params)   # slot 3 holds the second update's snapshot
        assert (pop.counts[2:, 2:] == 0).all().item()
    finally:
        sim.close()


def test_the_snapshot_is_planned_before_exploit_and_exploit_names_no_pool_member():
    import torch
    sim = TP._sim(WORLDS, N)
    try:
        pop = _pop(sim, snapshot_interval=1, pbt_interval=1)
        pop.collect()
        pop.elo.copy_(torch.tensor([1400.0, 1600.0, 1300.0], dtype=torch.float64))      # the pool member rates lowest of all
        taken = pop.members[1].opt.flat.params.clone()
        out = pop.update()
        assert list(out).index("snapshot") < list(out).index("exploit")
        # planned after exploit the learners would tie at 1600 and the snapshot would name learner 0
        assert out["snapshot"] == (NT, 1) and out["exploit"] == [(0, 1)]
        assert all(0 <= d < NT and 0 <= s < NT for d, s in out["exploit"])
        assert pop.elo.tolist() == [1600.0, 1600.0, 1600.0]
        assert torch.equal(pop.past[0].flat.params, pop.members[1].opt.flat.params) and not torch.equal(pop.past[0].flat.params, taken)
        assert torch.equal(pop.members[0].opt.flat.params, pop.members[1].opt.flat.params)
    finally:
        sim.close()


def test_checkpoint_round_trip(tmp_path):
    import torch
    from gpu_hideseek import evaluate, population
    sims = [TP._sim(WORLDS, N) for _ in range(2)]
    try:
        a, b = (_pop(s, snapshot_interval=1) for s in sims)
        ma, mb = a.update_iter(), b.update_iter()                                        # the twins: the yardstick
        torch.save(a.state_dict(), str(tmp_path / "1"))
        sd = torch.load(str(tmp_path / "1"), map_location=a.device, weights_only=False)
        assert set(sd) == {"members", "league", "hyper", "update_index", "counter", "past", "taken"} and sd["taken"] == 1 and len(sd["past"]) == NQ
        assert {"params", "optimizer", "normaliser"} <= set(sd["past"][0]) and sd["past"][0]["taken"] == 1
        assert tuple(sd["league"]["table"].shape) == (N * N * 4 + N + 1,)
        fresh = _pop(sims[1], nets=False, snapshot_interval=1)                           # other parameters, on the twin simulator
        assert not torch.equal(fresh.past[0].flat.params, a.past[0].flat.params)
        fresh.load_state_dict(sd)
        a.load_state_dict(sd)
        assert torch.equal(fresh.past[0].flat.params, a.past[0].flat.params) and torch.equal(fresh.tables, a.tables) and fresh.taken == 1
        assert torch.equal(a._table, fresh._table) and all(torch.equal(x, y) for x, y in zip(a.past[0].state, fresh.past[0].state))
        oa, of = a.update_iter(), fresh.update_iter()
        na, nf = TP._numbers(oa), TP._numbers(of)
        ta, tb = TP._numbers(ma), TP._numbers(mb)
        assert oa["past"] == of["past"] == [2]
        if ta == tb:
            assert na == nf
            for x, y in zip(a.members, fresh.members):
                assert torch.equal(x.opt.flat.params, y.opt.flat.params)
            assert torch.equal(a.past[0].flat.params, fresh.past[0].flat.params)
        else:                                             # the twins differ: 4 x their largest difference per metric
            for k in na:
                print(f"twins differ: {k}: twins {abs(ta[k] - tb[k]):.3e}, loaded {abs(na[k] - nf[k]):.3e}")
                assert abs(na[k] - nf[k]) <= 4.0 * abs(ta[k] - tb[k]), k
        net, norm = evaluate.load_policy(sd, past=0)
        assert torch.equal(net._flat.params, sd["past"][0]["params"]) and norm is not None
        net, _ = evaluate.load_policy(sd, member=1)
        assert torch.equal(net._flat.params, sd["members"][1]["params"])
        for kw in (dict(past=1), dict(past=0, member=0), dict(past=True)):
            with pytest.raises(ValueError, match="past"):
                evaluate.load_policy(sd, **kw)
        # a state with another Q is refused, either way
        other = population.Population(sims[1], TP._cfg(NT))
        with pytest.raises(ValueError, match="pool of 1 past policies: expected 0"):
            other.load_state_dict(sd)
        with pytest.raises(ValueError, match="pool of 0 past policies: expected 1"):
            fresh.load_state_dict(other.state_dict())
    finally:
        for s in sims:
            s.close()


def test_without_a_pool_no_schedule_is_set_and_the_scheduled_step_is_never_called(monkeypatch):
    import ctypes as C
    from gpu_hideseek import league as G, population
    sim = TP._sim(WORLDS, NT)
    try:
        called = []
        run = G._run                                                                   # the league's step runs from league.Table
        monkeypatch.setattr(G, "_run", lambda s, fn, *a: (called.append(fn), run(s, fn, *a))[1])
        monkeypatch.setattr(type(sim), "set_league_schedule", lambda *a: pytest.fail("a schedule was set"))
        pop = population.Population(sim, TP._cfg(NT), nets=TP._policies(NT))
        pop.collect()
        out = pop.update()
        assert set(called) == {"hs_league_step"} and len(called) == STEPS + 2
        assert pop.past == [] and pop.schedule is None and getattr(sim, "_league_schedule", None) is None
        assert "past" not in out and "snapshot" not in out and len(out["elo"]) == NT and set(pop.state_dict()) == {"members", "league", "hyper", "update_index", "counter"}
        req = G.request(WORLDS, AGENTS, 0, NT, K_TEAM, pop.world, pop.counts, pop.elo, group=4)[1]
        assert sim._L.hs_league_step_scheduled(sim._h, C.byref(req)) == 1 and b"no schedule is set" in sim._L.hs_last_error()
    finally:
        sim.close()
