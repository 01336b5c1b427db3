"""The population trainer on the GPU (gpu_hideseek.population): test_gpu_trainer's config (T = 8 steps in K = 2 chunks, two
minibatches, two epochs, float32) under RandomFlipTeams | UseFixedWorld | ZeroAgentVelocity, the simulator first stepped to
two steps before an episode's end so that a done and a team flip fall inside the rollout.

P = 1 is the Trainer: a Population of one policy against a Trainer on a twin simulator.  The yardstick is two plain
Trainers on twin simulators run in the same test: where they agree bit for bit (the shapes and launches are identical), the
Population must agree bit for bit with the Trainer; where they do not, slot 0 of the first rollout is compared within 4 x
the twins' largest difference per quantity.  The checkpoint test uses the same rule on the metrics."""
import numpy as np
import pytest

import test_gpu_trainer as TT
from test_league_host import ELO_TOL, new_state

pytestmark = pytest.mark.gpu

K_TEAM, AGENTS = 3, 6
T = TT.T
STORED = ("actor", "critic", "action", "reward", "done", "clear", "log_prob", "value", "advantage")


def _sim(worlds, policies=1, seed=5, presteps=TT.EPISODE - 2):
    import gpu_hideseek
    F = gpu_hideseek.SimFlags
    s = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=int(F.RandomFlipTeams | F.UseFixedWorld | F.ZeroAgentVelocity),
        rand_seed=seed, min_hiders=K_TEAM, max_hiders=K_TEAM, min_seekers=K_TEAM, max_seekers=K_TEAM, num_pbt_policies=policies)
    s.init()
    for _ in range(presteps):
        s.step()
    return s


def _cfg(P, **kw):
    from gpu_hideseek import population
    return population.PopulationConfig(**dict(dict(steps_per_update=T, num_bptt_chunks=TT.K, num_minibatches=2, num_epochs=2, num_policies=P, team_size=K_TEAM), **kw))


def _policies(P):
    """P different policies: test_gpu_trainer's, the later ones with another actor head."""
    import torch
    nets = [TT._policy() for _ in range(P)]
    for p, net in enumerate(nets[1:], 1):
        with torch.no_grad():
            net.actor_head.weight.add_(0.05 * torch.randn(net.actor_head.weight.shape, generator=torch.Generator().manual_seed(40 + p)))
    return nets


def _numbers(m, path=""):
    """{path: number} of the numeric leaves of a metrics dict, without the wall-clock "fps"."""
    out = {}
    if isinstance(m, dict):
        for k, v in m.items():
            if k != "fps":
                out.update(_numbers(v, f"{path}.{k}"))
    elif isinstance(m, (list, tuple)):
        for i, v in enumerate(m):
            out.update(_numbers(v, f"{path}[{i}]"))
    else:
        out[path] = float(m)
    return out


def _largest(a, b):
    return float((a.double() - b.double()).abs().max())


# ---- P = 1 is the Trainer ----
def test_a_population_of_one_is_the_trainer():
    import torch
    from gpu_hideseek import population, trainer
    sims = [_sim(6) for _ in range(3)]
    try:
        runs = [trainer.Trainer(sims[0], TT._cfg(), net=TT._policy()), trainer.Trainer(sims[1], TT._cfg(), net=TT._policy()),
                population.Population(sims[2], _cfg(1), nets=[TT._policy()])]
        assert torch.equal(runs[2].row_of_slot, torch.arange(36, dtype=torch.int32, device="cuda"))      # one policy: the identity routing
        first, stored, metrics = [], [], []
        for r in runs:
            r.collect()
            first.append({k: getattr(r.rollout, k)[0].clone() for k in STORED})
            assert (r.rollout.done != 0).any().item() and (r.rollout.done == 0).any().item()          # an episode ended inside the first rollout
            r.update()
            metrics.append(r.update_iter())
            stored.append({k: getattr(r.rollout, k).clone() for k in STORED})
        tr_a, tr_b, pop = runs
        assert torch.equal(pop.row_of_slot, torch.arange(36, dtype=torch.int32, device="cuda")) and pop.metrics()["bad"] == 0
        params = [tr_a.opt.flat.params, tr_b.opt.flat.params, pop.members[0].opt.flat.params]
        ma, mb, mp = _numbers(metrics[0]), _numbers(metrics[1]), _numbers(metrics[2]["policies"][0])
        twins = all(torch.equal(stored[0][k], stored[1][k]) for k in STORED) and torch.equal(params[0], params[1]) and ma == mb
        if twins:
            for k in STORED:
                assert torch.equal(stored[0][k], stored[2][k]), k
            assert torch.equal(params[0], params[2])
            assert {k: mp[k] for k in ma} == ma
            assert metrics[2]["update"] == 2 and metrics[2]["policies"][0]["adam_step"] == metrics[0]["adam_step"]
        else:                                             # the fallback: slot 0 of the first rollout, 4 x the twins' largest difference
            for k in STORED:
                bound = 4.0 * _largest(first[0][k], first[1][k])
                got = _largest(first[0][k], first[2][k])
                print(f"twins differ: {k}: twins {bound / 4.0:.3e}, population {got:.3e}")
                assert got <= bound, (k, got, bound)
    finally:
        for s in sims:
            s.close()


# ---- P = 2: the routing ----
WORLDS2, P2 = 8, 2
R2 = WORLDS2 * AGENTS


@pytest.fixture(scope="module")
def routed():
    """Two rollouts of a population of two on 8 worlds, every sim.step() and every league step recorded on the host."""
    from gpu_hideseek import episodes, population
    sim = _sim(WORLDS2, P2)

    def exports():
        get = lambda n, k: getattr(sim, n + "_tensor")().to_torch().reshape(k, -1).cpu().numpy().copy()       # noqa: E731
        x = dict(done=get("done", R2)[:, 0], reward=get("reward", R2)[:, 0], self_type=get("self_type", R2)[:, 0], self_mask=get("self_mask", R2)[:, 0],
                 episode_result=get("episode_result", WORLDS2), action=get("action", R2))
        x["hider_team"] = (x["self_type"].reshape(WORLDS2, -1)[:, 0] == 0).astype(np.int32)        # team 0 is the world's first rows
        return x

    seen, steps, routes = [exports()], [], []              # seen[0]: what the constructor's league step routed from
    pop = population.Population(sim, _cfg(P2), nets=_policies(P2))
    pop.episodes = episodes.EpisodeStats(sim).arm(from_start=True)
    routes.append(pop.row_of_slot.cpu().numpy().copy())
    step, league_step = sim.step, pop.league_step

    def recorded_step():
        action_in = sim.action_tensor().to_torch().reshape(R2, 5).cpu().numpy().copy()
        step()
        steps.append(dict(exports(), action_in=action_in))

    def recorded_league_step():
        league_step()
        routes.append(pop.row_of_slot.cpu().numpy().copy())
    sim.step, pop.league_step = recorded_step, recorded_league_step
    rollouts = []
    for _ in range(2):
        pop.collect()
        rollouts.append({k: getattr(pop.rollout, k).cpu().numpy().copy() for k in ("action", "reward", "done", "clear")})
    out = pop.metrics()
    table = pop.episodes.table.cpu().numpy()
    sim.step = step
    yield dict(pop=pop, seen=seen, steps=steps, routes=routes, rollouts=rollouts, out=out, table=table)
    sim.close()


def test_slots_hold_what_their_rows_exported(routed):
    steps, routes, rollouts = routed["steps"], routed["routes"], routed["rollouts"]
    assert len(steps) == 2 * T + 1 and len(routes) == 2 * T + 2                  # one league step per sim.step(), and the constructor's
    for ro in routes:
        assert sorted(ro.tolist()) == list(range(R2))
    first = np.stack([s["self_type"].reshape(WORLDS2, -1)[:, 0] for s in steps])
    assert (first[0] != first[-1]).any()                                           # some world's sides changed: the flip is crossed
    assert any((a != b).any() for a, b in zip(routes[:-1], routes[1:]))
    for i, buf in enumerate(rollouts):
        for t in range(T):
            g = i * T + t                                   # slot g observes step g + 1 under routes[g + 1]; step g + 2 consumes its action
            ro, nxt = routes[g + 1], steps[g + 1]
            assert np.array_equal(buf["action"][t], nxt["action_in"][ro]), (i, t)
            assert np.array_equal(buf["reward"][t].view(np.int32), nxt["reward"][ro].view(np.int32)), (i, t)
            assert np.array_equal(buf["done"][t], nxt["done"][ro]), (i, t)
            if t + 1 < T:
                assert np.array_equal(buf["clear"][t + 1], buf["done"][t]), (i, t)
    assert np.array_equal(rollouts[1]["clear"][0], rollouts[0]["done"][T - 1])
    assert any((b["done"] != 0).any() for b in rollouts)
    # the two policies act differently, so a misrouted slot would show: the slots of a policy hold its rows' actions
    assert not np.array_equal(rollouts[0]["action"][0][:R2 // 2], rollouts[0]["action"][0][R2 // 2:])


def test_one_league_step_per_sim_step_books_every_game_once(routed):
    from gpu_hideseek import episodes as E, league as G
    out, table, pop = routed["out"], routed["table"], routed["pop"]
    assert out["bad"] == 0
    counts = pop.counts.cpu().numpy()
    assert out["games"] == counts.sum() == table[E.WORLD_EPISODES] == WORLDS2         # every world finished one episode
    assert counts[:, :, 0].sum() == table[E.HIDER_WINS] and counts[:, :, 1].sum() == table[E.SEEKER_WINS]
    st, ref_counts, elo = new_state(WORLDS2), np.zeros((P2, P2, 4), np.int64), np.full(P2, 1500.0)
    for s, ro in zip(routed["seen"] + routed["steps"], routed["routes"]):
        r = G.host_step(st, ref_counts, elo, P2, K_TEAM, s["done"], s["self_type"], s["self_mask"], s["episode_result"], s["hider_team"])
        assert r["bad"] == 0 and np.array_equal(r["row_of_slot"], ro)
    assert np.array_equal(ref_counts, counts)
    assert np.allclose(out["elo"], elo, rtol=0.0, atol=ELO_TOL), (out["elo"], elo.tolist())


# ---- P = 2: the policies learn independently ----
def test_a_policy_learns_from_its_own_slots_alone():
    import torch
    from gpu_hideseek import population
    sim = _sim(WORLDS2, P2)
    try:
        pop = population.Population(sim, _cfg(P2), nets=_policies(P2))
        pop.collect()
        saved = pop.state_dict()
        before = [mb.opt.flat.params.clone() for mb in pop.members]
        pop.update()
        after = [mb.opt.flat.params.clone() for mb in pop.members]
        assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])
        pop.load_state_dict(saved)
        assert all(torch.equal(mb.opt.flat.params, b) for mb, b in zip(pop.members, before))
        m, buf, g = pop.block, pop.rollout, torch.Generator(device="cuda").manual_seed(9)
        for k in ("actor", "critic", "log_prob", "value", "advantage", "returns", "actor_h", "actor_c", "critic_h", "critic_c"):
            x = getattr(buf, k)
            x[:, m:] = torch.randn(x[:, m:].shape, generator=g, device="cuda").to(x.dtype)
        buf.action[:, m:] = torch.randint(0, 2, buf.action[:, m:].shape, generator=g, device="cuda", dtype=torch.int32)
        buf.clear[:, m:] = torch.randint(0, 2, buf.clear[:, m:].shape, generator=g, device="cuda", dtype=torch.int32)
        pop.members[1].set_hyper(0.0, pop.members[1].entropy_coef)
        out = pop.update()
        assert torch.equal(pop.members[0].opt.flat.params, after[0])                    # bit for bit, whatever policy 1's slots hold
        assert torch.equal(pop.members[1].opt.flat.params, before[1])                   # lr = 0
        assert out["policies"][1]["lr"] == 0.0 and out["policies"][0]["lr"] == pop.cfg.lr
        assert "exploit" not in out                                                      # pbt_interval = 0: nothing is planned
    finally:
        sim.close()


# ---- exploit / explore and checkpoints ----
def test_exploit_applies_the_planned_pair():
    import torch
    from gpu_hideseek import population
    sim = _sim(WORLDS2, P2)
    try:
        cfg = _cfg(P2, pbt_interval=1)
        pop = population.Population(sim, cfg, nets=_policies(P2))
        pop.collect()
        pop.elo.copy_(torch.tensor([1400.0, 1600.0], dtype=torch.float64))              # hand-set: policy 0 is the one to replace
        carried = [[t.clone() for s in mb.state for t in s] for mb in pop.members]
        out = pop.update()
        plan = population.plan_exploit([1400.0, 1600.0], cfg.exploit_fraction, np.random.Generator(np.random.PCG64(cfg.seed)))
        assert out["exploit"] == plan == [(0, 1)] and out["elo"] == [1400.0, 1600.0]
        dst, src = pop.members
        assert torch.equal(dst.opt.flat.params, src.opt.flat.params) and torch.equal(dst.net.actor_head.weight, src.net.actor_head.weight)
        assert torch.equal(dst.opt.m, src.opt.m) and torch.equal(dst.opt.v, src.opt.v) and torch.equal(dst.opt.adam_state, src.opt.adam_state)
        assert torch.equal(dst.normaliser.state, src.normaliser.state) and torch.equal(pop.tables[0], pop.tables[1])
        assert dst.normaliser.table.data_ptr() == pop.tables[0].data_ptr() and src.normaliser.state[-1].item() > 0
        assert pop.elo.tolist() == [1600.0, 1600.0]
        assert dst.lr in (cfg.lr * 0.8, cfg.lr * 1.25) and dst.entropy_coef in (cfg.entropy_coef * 0.8, cfg.entropy_coef * 1.25)
        assert cfg.lr * 0.1 <= dst.lr <= cfg.lr * 10.0
        assert (src.lr, src.entropy_coef) == (cfg.lr, cfg.entropy_coef)                  # the source is untouched
        for mb, was in zip(pop.members, carried):                                        # the carried LSTM states stay
            assert all(torch.equal(a, b) for a, b in zip((t for s in mb.state for t in s), was))
        assert pop.state_dict()["hyper"]["lr"] == [dst.lr, cfg.lr]
    finally:
        sim.close()


def test_checkpoint_round_trip(tmp_path):
    import torch
    from gpu_hideseek import evaluate, population
    sims = [_sim(WORLDS2, P2) for _ in range(2)]
    try:
        a, b = (population.Population(s, _cfg(P2), nets=_policies(P2)) for s in sims)
        ma, mb = a.update_iter(), b.update_iter()                                        # the twins: the yardstick
        torch.save(a.state_dict(), str(tmp_path / "1"))                                 # through a file, as tools/train.py --restore reads it
        sd = torch.load(str(tmp_path / "1"), map_location=a.device, weights_only=False)
        assert set(sd) == {"members", "league", "hyper", "update_index", "counter"} and sd["update_index"] == 1 and sd["counter"] == T
        assert all(set(m) == {"params", "optimizer", "normaliser", "state", "clear", "generator", "update_index", "counter"} for m in sd["members"])
        fresh = population.Population(sims[1], _cfg(P2))                                 # other parameters, on the twin simulator
        assert not torch.equal(fresh.members[1].opt.flat.params, a.members[1].opt.flat.params)
        fresh.load_state_dict(sd)
        a.load_state_dict(sd)                                                            # both step before their next slot 0
        for x, y in zip(a.members, fresh.members):
            assert torch.equal(x.opt.flat.params, y.opt.flat.params) and torch.equal(x.opt.m, y.opt.m) and torch.equal(x.normaliser.state, y.normaliser.state)
            assert torch.equal(x.normaliser.table, y.normaliser.table) and all(torch.equal(p, q) for p, q in zip((t for s in x.state for t in s), (t for s in y.state for t in s)))
        assert torch.equal(a._table, fresh._table) and (fresh.update_index, fresh.counter) == (1, T)
        na, nf = _numbers(a.update_iter()), _numbers(fresh.update_iter())
        ta, tb = _numbers(ma), _numbers(mb)
        if ta == tb:
            assert na == nf
        else:                                             # the twins differ: 4 x their largest difference per metric
            for k in na:
                print(f"twins differ: {k}: twins {abs(ta[k] - tb[k]):.3e}, loaded {abs(na[k] - nf[k]):.3e}")
                assert abs(na[k] - nf[k]) <= 4.0 * abs(ta[k] - tb[k]), k
        net, norm = evaluate.load_policy(sd["members"][1])
        assert torch.equal(net._flat.params, sd["members"][1]["params"]) and norm is not None
    finally:
        for s in sims:
            s.close()
