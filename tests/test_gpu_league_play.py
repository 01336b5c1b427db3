"""league.League on a real simulator: 36 worlds of 3 hiders and 3 seekers with RandomFlipTeams | UseFixedWorld |
ZeroAgentVelocity, float32, two policies, 245 steps (every world finishes one episode of 240 steps, so the flips at the
episode start are crossed).  One run, shared by the tests: the routing reaches the actions, the table agrees with the
episode tracker that already counts games, the run leaves policies and normalisers alone, and the ratings are those of
league.host_step replayed over the recorded exports."""
import numpy as np
import pytest

import test_league_host as H
from test_league_host import ELO_TOL

pytestmark = pytest.mark.gpu

WORLDS, K, STEPS, P = 36, 3, 245, 2
CHOICE = ((1, 3, 2, 1, 0), (3, 0, 4, 0, 1))           # the bucket every head of policy p prefers: they differ in every head


def _sim(worlds=WORLDS):
    import gpu_hideseek
    F = gpu_hideseek.SimFlags
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=int(F.RandomFlipTeams | F.UseFixedWorld | F.ZeroAgentVelocity),
        rand_seed=5, min_hiders=K, max_hiders=K, min_seekers=K, max_seekers=K, num_pbt_policies=P)


def _constant_policy(seed, choice):
    """A policy whose actor head has zero weights and a bias that makes bucket choice[h] head h's greedy action."""
    import torch
    from gpu_hideseek import policy
    net = policy.make_policy(generator=torch.Generator().manual_seed(seed)).cuda()
    with torch.no_grad():
        net.actor_head.weight.zero_()
        off = 0
        for h, n in enumerate(net.buckets):
            net.actor_head.bias[off + choice[h]] = 4.0
            off += n
    return net


@pytest.fixture(scope="module")
def played():
    import torch
    from gpu_hideseek import episodes, league
    from gpu_hideseek.policy_inputs import NORM_STATE, ObsNormaliser
    sim = _sim()
    sim.init()
    rows = WORLDS * 2 * K
    nets = [_constant_policy(7 + p, CHOICE[p]) for p in range(P)]
    norm = ObsNormaliser(0)
    norm.load_state_dict({"state": torch.rand(NORM_STATE, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) + 0.5, "decay": norm.decay, "eps": norm.eps})
    normalisers = [norm, None]

    def exports():
        get = lambda n, k: getattr(sim, n + "_tensor")().to_torch().reshape(k, -1).cpu().numpy().copy()       # noqa: E731
        x = dict(done=get("done", rows)[:, 0], self_type=get("self_type", rows)[:, 0], self_mask=get("self_mask", rows)[:, 0],
                 episode_result=get("episode_result", WORLDS), policy=get("policy_assignments", rows)[:, 0])
        x["hider_team"] = (x["self_type"].reshape(WORLDS, -1)[:, 0] == 0).astype(np.int32)        # team 0 is the world's first rows
        return x

    def frozen():
        return [p.detach().clone() for net in nets for p in net.parameters()] + [norm.state.clone(), norm.table.clone()]

    before = frozen()
    lg = league.League(sim, list(zip(nets, normalisers)), K, mode="greedy", seed=2)
    lg.episodes = episodes.EpisodeStats(sim).arm(from_start=True)
    seen = [exports()]                                  # what arm() routed from
    wrong = []
    const = torch.tensor(CHOICE, dtype=torch.int32, device="cuda")
    act = lg.act

    def checked_act():
        act()
        action = sim.action_tensor().to_torch().reshape(rows, 5)
        policy = sim.policy_assignments_tensor().to_torch().reshape(rows).long()
        wrong.append(int((action != const[policy]).any(1).sum()))
    lg.act = checked_act
    out = lg.run(STEPS, on_step=lambda i, lg: seen.append(exports()))
    table = lg.episodes.table.cpu().numpy()
    yield dict(sim=sim, lg=lg, out=out, seen=seen, wrong=wrong, table=table, before=before, after=frozen())
    sim.close()


def test_routing_reaches_the_actions(played):
    assert len(played["wrong"]) == STEPS and sum(played["wrong"]) == 0
    seen = played["seen"]
    first = np.stack([s["self_type"].reshape(WORLDS, -1)[:, 0] for s in seen])
    assert (first[0] != first[-1]).any()                # flips were crossed
    from gpu_hideseek import league
    hp, sp = league.schedule(WORLDS, P)
    for s in (seen[0], seen[100], seen[-1]):
        hider = s["self_type"].reshape(WORLDS, -1) != 0
        assert np.array_equal(s["policy"].reshape(WORLDS, -1), np.where(hider, np.array(hp)[:, None], np.array(sp)[:, None]))
        assert np.bincount(s["policy"], minlength=P).tolist() == [WORLDS * K] * P


def test_the_table_agrees_with_the_episode_tracker(played):
    from gpu_hideseek import episodes as E
    out, table = played["out"], played["table"]
    counts = np.array(out["counts"])
    assert counts.shape == (P, P, 4) and out["bad"] == 0
    assert counts[:, :, :3].sum() == table[E.HIDER_WINS] + table[E.SEEKER_WINS] + table[E.DRAWS]
    assert counts[:, :, 0].sum() == table[E.HIDER_WINS]
    assert out["games"] == table[E.WORLD_EPISODES] == WORLDS
    assert counts.sum(2).tolist() == [[WORLDS // (P * P)] * P] * P                    # every pair played its worlds once


def test_a_run_leaves_policies_and_normalisers_bit_identical(played):
    import torch
    assert len(played["before"]) == len(played["after"])
    for a, b in zip(played["before"], played["after"]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_ratings_equal_the_restatement_replayed_over_the_recorded_steps(played):
    from gpu_hideseek import league as G
    st, counts, elo = H.new_state(WORLDS), np.zeros((P, P, 4), np.int64), np.full(P, 1500.0)
    for s in played["seen"]:
        r = G.host_step(st, counts, elo, P, K, s["done"], s["self_type"], s["self_mask"], s["episode_result"], s["hider_team"])
        assert r["bad"] == 0 and np.array_equal(r["policy_assignments"], s["policy"])
    out = played["out"]
    err = float(np.abs(np.array(out["elo"]) - elo).max())
    print(f"max |elo - host| = {err:.3e} (bound {ELO_TOL:.0e}); elo = {out['elo']}")
    assert np.array_equal(np.array(out["counts"]), counts) and err <= ELO_TOL
    assert abs(sum(out["elo"]) - P * 1500.0) <= ELO_TOL


def test_a_number_of_worlds_that_is_no_multiple_of_the_pairs_is_refused():
    from gpu_hideseek import league
    sim = _sim(6)
    sim.init()
    with pytest.raises(ValueError, match="multiple of num_policies\\^2"):
        league.League(sim, [(None, None)] * 2, K)
    with pytest.raises(ValueError, match="team_size"):
        league.League(sim, [(None, None)], 2)
    sim.close()


def test_league_tool_loads_trainer_checkpoints_and_prints_the_tables(tmp_path, capsys):
    import importlib.util
    import json
    import os
    import torch
    from gpu_hideseek import trainer
    from test_gpu_trainer import _cfg, _sim as trainer_sim
    sim = trainer_sim(presteps=0)
    tr = trainer.Trainer(sim, _cfg())
    paths = []
    for i in range(2):                                  # two checkpoints of one trainer, the second with other parameters
        state = tr.state_dict()
        if i:
            state["params"] = state["params"] + 0.05 * torch.randn(state["params"].shape, generator=torch.Generator().manual_seed(9)).to(state["params"].device)
        paths.append(str(tmp_path / str(i)))
        torch.save(state, paths[-1])
    sim.close()
    spec = importlib.util.spec_from_file_location("league_tool", os.path.join(H.ROOT, "tools", "league.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    log = tmp_path / "run.log"
    out = tool.main(["--num-worlds", "8", "--num-steps", "243", "--ckpt-path", *paths, "--record-log", str(log), "--k-factor", "16"])
    text = capsys.readouterr().out
    lines = text.strip().splitlines()
    assert json.loads(lines[-1]) == out and out["games"] == 8 and out["bad"] == 0
    assert np.array(out["counts"]).sum(2).tolist() == [[2, 2], [2, 2]] and abs(sum(out["elo"]) - 3000.0) <= ELO_TOL
    assert lines[0] == "Elo before:" and lines[1].rstrip() == "  0:  1500.00         1:  1500.00"
    assert "Elo after 8 games:" in text and "hider win rate" in text
    from gpu_hideseek import replay
    assert replay.read_log(str(log), 8).shape[0] == 243
    with pytest.raises(SystemExit):
        tool.parse(["--num-worlds", "6", "--ckpt-path", "a", "b"])
