"""The key sets of the three drivers' state_dict()s, as the module docstrings of gpu_hideseek.trainer and
gpu_hideseek.population state them: a checkpoint written by one version of the drivers is read by the next, so the keys
are pinned here and not only by round trips within one version.  8 worlds x (3 + 3) agents (12 for the pooled population:
a multiple of T (T + Q) = 6), T = 4 steps in 2 chunks, one update each."""
import pytest

pytestmark = pytest.mark.gpu

K_TEAM = 3
LEARNER = {"params", "optimizer", "normaliser", "state", "clear", "generator", "update_index", "counter"}
OPTIMIZER = {"m", "v", "state", "layout", "param_groups"}
NORMALISER = {"state", "decay", "eps"}
WORLD = {"world_hider_team", "world_phase"}


def _kw(worlds, policies=1):
    import gpu_hideseek
    F = gpu_hideseek.SimFlags
    return dict(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, num_worlds=worlds, sim_flags=int(F.RandomFlipTeams | F.UseFixedWorld | F.ZeroAgentVelocity),
                rand_seed=5, min_hiders=K_TEAM, max_hiders=K_TEAM, min_seekers=K_TEAM, max_seekers=K_TEAM, num_pbt_policies=policies)


def _cfg(cls, **kw):
    return cls(steps_per_update=4, num_bptt_chunks=2, num_minibatches=2, num_epochs=1, **kw)


def _learner_keys(d):
    assert set(d) >= LEARNER and set(d["optimizer"]) == OPTIMIZER and set(d["normaliser"]) == NORMALISER
    return set(d)


def test_trainer_state_keys():
    import torch
    import gpu_hideseek
    from gpu_hideseek import trainer
    sim = gpu_hideseek.HideAndSeekSimulator(gpu_id=0, **_kw(8))
    sim.init()
    try:
        tr = trainer.Trainer(sim, _cfg(trainer.TrainConfig))
        tr.update_iter()
        d = tr.state_dict()
        assert _learner_keys(d) == LEARNER
        assert [len(s) for s in d["state"]] == [2, 2] and all(isinstance(t, torch.Tensor) for s in d["state"] for t in s)
        assert isinstance(d["clear"], torch.Tensor) and isinstance(d["generator"], torch.Tensor) and (d["update_index"], d["counter"]) == (1, 4)
        scaled = trainer.Trainer(sim, _cfg(trainer.TrainConfig, dtype=torch.float16, loss_scale="dynamic", normalise_obs=False)).state_dict()
        assert set(scaled) == LEARNER and scaled["normaliser"] is None and set(scaled["optimizer"]) == OPTIMIZER | {"loss_scale"}
    finally:
        sim.close()


def test_sharded_trainer_state_keys():
    import torch
    from gpu_hideseek import trainer
    from gpu_hideseek.sharded import ShardedSimulator
    ssim = ShardedSimulator([0, 0], **_kw(8))
    ssim.init()
    try:
        tr = trainer.ShardedTrainer(ssim, _cfg(trainer.TrainConfig))
        tr.update_iter()
        d = tr.state_dict()
        assert _learner_keys(d) == LEARNER | {"generators", "ranges"}
        assert len(d["state"]) == len(d["clear"]) == len(d["generators"]) == len(d["ranges"]) == 2
        assert all([len(s) for s in shard] == [2, 2] for shard in d["state"]) and all(isinstance(t, torch.Tensor) for t in d["clear"] + d["generators"])
        assert d["ranges"] == [list(r) for r in ssim.ranges]
    finally:
        ssim.close()


def test_pooled_population_state_keys():
    import torch
    import gpu_hideseek
    from gpu_hideseek import evaluate, population
    sim = gpu_hideseek.HideAndSeekSimulator(gpu_id=0, **_kw(12, 3))
    sim.init()
    try:
        pop = population.Population(sim, _cfg(population.PopulationConfig, num_policies=2, team_size=K_TEAM, num_past_policies=1, snapshot_interval=1, pbt_interval=1))
        pop.update_iter()
        d = pop.state_dict()
        assert set(d) == {"members", "league", "hyper", "update_index", "counter", "past", "taken"}
        assert len(d["members"]) == 2 and all(_learner_keys(m) == LEARNER for m in d["members"])
        assert set(d["league"]) == {"world", "table"} and set(d["league"]["world"]) == WORLD
        assert d["league"]["table"].dtype == torch.int64 and tuple(d["league"]["table"].shape) == (3 * 3 * 4 + 3 + 1,)
        assert set(d["hyper"]) == {"lr", "entropy_coef", "rng"} and len(d["hyper"]["lr"]) == len(d["hyper"]["entropy_coef"]) == 2
        assert len(d["past"]) == 1 and set(d["past"][0]) == {"params", "optimizer", "normaliser", "state", "taken"}
        assert set(d["past"][0]["optimizer"]) == {"layout"} and set(d["past"][0]["normaliser"]) == NORMALISER and len(d["past"][0]["state"]) == 2
        assert (d["update_index"], d["counter"], d["taken"], d["past"][0]["taken"]) == (1, 4, 1, 1)
        for kw in (dict(member=0), dict(member=1), dict(past=0)):
            net, normaliser = evaluate.load_policy(d, **kw)
            assert normaliser is not None and sum(p.numel() for p in net.parameters()) > 0
    finally:
        sim.close()
