"""What can be checked of the population trainer (gpu_hideseek.population) without a GPU: plan_exploit and explore, which
are pure host functions, and the configs PopulationConfig refuses."""
import numpy as np
import pytest


def _rng(seed=0):
    return np.random.Generator(np.random.PCG64(seed))


def test_plan_exploit_ranks_by_rating_and_breaks_ties_by_index():
    from gpu_hideseek.population import plan_exploit
    # P = 4, fraction 0.25: one policy is replaced, the lowest, by the single best
    assert plan_exploit([1500.0, 1490.0, 1520.0, 1510.0], 0.25, _rng()) == [(1, 2)]
    # ties: the lower index ranks higher, so of equal ratings the HIGHER index is replaced and the lower index is the source
    assert plan_exploit([1500.0] * 4, 0.25, _rng()) == [(3, 0)]
    assert plan_exploit([1500.0, 1600.0, 1500.0, 1600.0], 0.25, _rng()) == [(2, 1)]
    # n = max(1, floor(P * fraction)): 8 policies at 0.25 replace the lowest two, each from the top two
    elo = [1500.0 + 10 * i for i in range(8)]
    for seed in range(20):
        pairs = plan_exploit(elo, 0.25, _rng(seed))
        assert [d for d, _ in pairs] == [1, 0] and all(s in (7, 6) for _, s in pairs)
    assert {s for seed in range(40) for _, s in plan_exploit(elo, 0.25, _rng(seed))} == {6, 7}
    # floor(3 * 0.5) = 1, floor(2 * 0.25) = 0 -> 1
    assert plan_exploit([3.0, 1.0, 2.0], 0.5, _rng()) == [(1, 0)]
    assert plan_exploit([1.0, 2.0], 0.25, _rng()) == [(0, 1)]


def test_plan_exploit_edges():
    from gpu_hideseek.population import plan_exploit
    assert plan_exploit([1500.0], 0.25, _rng()) == [] and plan_exploit([], 0.25, _rng()) == []
    for P in range(2, 17):
        for f in (0.01, 0.25, 0.34, 0.5):
            for seed in range(5):
                elo = _rng(100 + seed).normal(1500.0, 50.0, P).round(0).tolist()       # rounded: ties occur
                pairs = plan_exploit(elo, f, _rng(seed))
                assert len(pairs) == max(1, int(P * f)) and all(d != s for d, s in pairs)
                assert len({d for d, _ in pairs}) == len(pairs) and not {d for d, _ in pairs} & {s for _, s in pairs}
                assert pairs == plan_exploit(elo, f, _rng(seed))                        # deterministic under a seed
    for f in (0.0, -0.1, 0.51, 1.0, float("nan")):
        with pytest.raises(ValueError, match="exploit_fraction"):
            plan_exploit([1.0, 2.0], f, _rng())


def test_explore_scales_and_clamps():
    from gpu_hideseek.population import explore
    base = 1e-4
    for seed in range(10):
        v = explore(base, base, (0.8, 1.25), (0.1, 10.0), _rng(seed))
        assert v in (base * 0.8, base * 1.25)
    assert {explore(base, base, (0.8, 1.25), (0.1, 10.0), _rng(s)) for s in range(20)} == {base * 0.8, base * 1.25}
    # clamped to base * range on both sides
    assert explore(9.5 * base, base, (1.25,), (0.1, 10.0), _rng()) == base * 10.0
    assert explore(0.11 * base, base, (0.8,), (0.1, 10.0), _rng()) == base * 0.1
    v = base
    for _ in range(100):
        v = explore(v, base, (0.8, 1.25), (0.1, 10.0), _rng(7))
        assert base * 0.1 <= v <= base * 10.0
    for bad in ((1.0,), (0.0, 10.0), (2.0, 10.0), (0.1, 0.5), "ab", None):
        with pytest.raises(ValueError, match="explore_range"):
            explore(base, base, (0.8,), bad, _rng())


def test_population_config_refusals():
    from gpu_hideseek.population import PopulationConfig, check_population_config
    from gpu_hideseek.trainer import TrainConfig

    def cfg(**kw):
        return PopulationConfig(**dict(dict(steps_per_update=8, num_bptt_chunks=2, num_minibatches=2, num_epochs=2, num_policies=2, team_size=3), **kw))
    check_population_config(cfg(), 8, 6)
    assert issubclass(PopulationConfig, TrainConfig)
    d = PopulationConfig()
    assert (d.k_factor, d.pbt_interval, d.exploit_fraction, d.explore_scales, d.explore_range) == (32.0, 0, 0.25, (0.8, 1.25), (0.1, 10.0))
    cases = [
        (cfg(num_policies=0), 8, 6, "num_policies"), (cfg(num_policies=17), 17 * 17, 6, "num_policies"), (cfg(num_policies=2.0), 8, 6, "num_policies must be an integer"),
        (cfg(team_size=2), 8, 6, "team_size"), (cfg(team_size=0), 8, 6, "team_size"), (cfg(), 6, 6, "multiple of num_policies\\^2"),
        (cfg(num_policies=3), 8, 6, "multiple of num_policies\\^2"), (cfg(k_factor=0.0), 8, 6, "k_factor"),
        # trainer.check_config with rows = m = R / P: 2 chunks x 24 slots do not divide into 5 minibatches (the 96 of all rows would not either; 32 shows m)
        (cfg(num_minibatches=5), 8, 6, "48 sequences"), (cfg(num_minibatches=32), 8, 6, "48 sequences"), (cfg(steps_per_update=9), 8, 6, "multiple of num_bptt_chunks"),
        (cfg(pbt_interval=-1), 8, 6, "pbt_interval"), (cfg(pbt_interval=1.0), 8, 6, "pbt_interval"), (cfg(pbt_interval=True), 8, 6, "pbt_interval"),
        (cfg(exploit_fraction=0.0), 8, 6, "exploit_fraction"), (cfg(exploit_fraction=0.6), 8, 6, "exploit_fraction"),
        (cfg(explore_scales=()), 8, 6, "explore_scales"), (cfg(explore_scales=(0.8, 0.0)), 8, 6, "explore_scales"),
        (cfg(explore_range=(2.0, 10.0)), 8, 6, "explore_range"), (cfg(explore_range=(0.1,)), 8, 6, "explore_range"),
    ]
    for c, worlds, agents, what in cases:
        with pytest.raises(ValueError, match=what):
            check_population_config(c, worlds, agents)
