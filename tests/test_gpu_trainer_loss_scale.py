"""The update loop with the dynamic loss scale on the GPU (trainer.TrainConfig.loss_scale; gpu_hideseek.optim.LossScale) in
test_gpu_trainer's shape: 6 worlds x (3 + 3) agents, T = 8 steps in K = 2 chunks, 2 epochs x 2 minibatches.  A scale far too
large backs off without touching anything; a moderate one trains float16; a fixed power of two in float32 changes no bit
of an update; the scaler's state travels through the checkpoint and through a population's exploit step."""
import math

import pytest

import test_gpu_trainer as TT
from test_gpu_trainer import T, _cfg, _same, _sim

pytestmark = pytest.mark.gpu

STEPS = 4                         # 2 epochs x 2 minibatches


def _policy(dtype):
    """test_gpu_trainer's policy in `dtype`: the critic head off its zero initialisation, so that every parameter has a
    gradient from the first step on."""
    import torch
    from gpu_hideseek import policy as P
    src = TT._policy()
    net = P.make_policy(dtype, generator=torch.Generator().manual_seed(31))
    with torch.no_grad():
        for (name, p), (other, q) in zip(net.named_parameters(), src.named_parameters()):
            assert name == other and p.shape == q.shape and p.dtype == q.dtype
            p.copy_(q)
    return net


def _finite(m):
    return all(math.isfinite(v) for v in [v for v in m.values() if not isinstance(v, list)] + m["value_loss_epochs"])


def test_a_scale_far_too_large_backs_off_and_touches_nothing():
    """float16 from 2^30: every grad_logits entry above 0.02 / 2^30 x 2^16 in size is infinite, so every step is skipped:
    the scaler's ordinary back-off, not a fault."""
    import torch
    from gpu_hideseek import trainer
    s = _sim()
    try:
        tr = trainer.Trainer(s, _cfg(dtype=torch.float16, loss_scale=dict(init_scale=2.0 ** 30, max_scale=2.0 ** 30)), net=_policy(torch.float16))
        before = [t.clone() for t in (tr.opt.flat.params, tr.opt.m, tr.opt.v)]
        m = tr.update_iter()
        print("trainer, float16 from 2^30:", {k: m[k] for k in ("skipped", "adam_step", "loss_scale", "grad_norm")})
        assert m["skipped"] == STEPS and m["adam_step"] == 0 and m["loss_scale"] == 2.0 ** 26
        for a, b in zip(before, (tr.opt.flat.params, tr.opt.m, tr.opt.v)):
            _same(a, b)
        assert not tr.opt.flat.grads.any().item()
        assert tr.opt.loss_scale.read() == {"scale": 2.0 ** 26, "good_steps": 0, "backoffs": STEPS, "growths": 0}
        assert tr.opt.adam_state.tolist() == [1.0, 1.0, 0.0, float(STEPS)]
    finally:
        s.close()


def test_float16_trains_with_a_moderate_scale():
    import torch
    from gpu_hideseek import trainer
    s = _sim()
    try:
        tr = trainer.Trainer(s, _cfg(dtype=torch.float16, loss_scale=dict(init_scale=2.0 ** 8, growth_interval=2)), net=_policy(torch.float16))
        before = tr.opt.flat.params.clone()
        m = tr.update_iter()
        state = tr.opt.loss_scale.read()
        print("trainer, float16 from 2^8:", {k: m[k] for k in ("skipped", "adam_step", "loss_scale", "grad_norm")}, state)
        assert _finite(m), m
        assert m["skipped"] + m["adam_step"] == STEPS
        assert m["loss_scale"] == state["scale"] == 2.0 ** 8 * 2.0 ** (state["growths"] - state["backoffs"])
        assert state["backoffs"] == m["skipped"]
        if m["adam_step"]:
            for name, (lo, hi, _) in tr.opt.layout().items():
                assert (tr.opt.flat.params[lo:hi] != before[lo:hi]).any().item(), f"{name} did not move"
        assert not tr.opt.flat.grads.any().item()
        assert set(m) - set(trainer.Trainer.METRIC_NAMES) == {"loss_scale", "value_loss_epochs", "loss", "update", "fps"}
    finally:
        s.close()


def test_a_fixed_power_of_two_changes_no_bit_in_float32():
    """Every operation of the backward pass is linear in the upstream gradient, and a power of two commutes with rounding
    in the normal range: with S fixed at 2^4 the parameters, the moments and the stored rollout after one update are
    those of the plain trainer from the same seed and policy, bit for bit."""
    import torch
    from gpu_hideseek import trainer
    sims = [_sim(), _sim()]
    try:
        plain = trainer.Trainer(sims[0], _cfg(), net=TT._policy())
        scaled = trainer.Trainer(sims[1], _cfg(loss_scale=dict(init_scale=2.0 ** 4, growth_interval=2 ** 30)), net=TT._policy())
        a, b = plain.update_iter(), scaled.update_iter()
        assert b["loss_scale"] == 16.0 and "loss_scale" not in a and a["skipped"] == b["skipped"] == 0 and a["adam_step"] == b["adam_step"] == STEPS
        for k in ("actor", "critic", "action", "reward", "done", "clear", "mask", "log_prob", "value", "advantage", "returns"):
            _same(getattr(plain.rollout, k), getattr(scaled.rollout, k), k)
        layout = plain.opt.layout()
        for k, x, y in (("params", plain.opt.flat.params, scaled.opt.flat.params), ("m", plain.opt.m, scaled.opt.m), ("v", plain.opt.v, scaled.opt.v)):
            for name, (lo, hi, _) in layout.items():
                gap = (x[lo:hi].double() - y[lo:hi].double()).abs().max().item()
                assert torch.equal(x[lo:hi].view(torch.int32), y[lo:hi].view(torch.int32)), (k, name, gap)
        _same(plain.opt.adam_state, scaled.opt.adam_state)
        assert {k: v for k, v in a.items() if k != "fps"} == {k: v for k, v in b.items() if k not in ("fps", "loss_scale")}
    finally:
        for s in sims:
            s.close()


def test_the_checkpoint_carries_the_scaler():
    import torch
    from gpu_hideseek import trainer
    s = _sim(presteps=0)
    try:
        cfg = dict(dtype=torch.float16, loss_scale=dict(init_scale=2.0 ** 8, growth_interval=2))
        tr = trainer.Trainer(s, _cfg(**cfg))
        tr.update_iter()
        sd = tr.state_dict()
        assert set(sd["optimizer"]) == {"m", "v", "state", "layout", "param_groups", "loss_scale"}
        assert set(sd["optimizer"]["loss_scale"]) == {"state", "growth", "backoff", "growth_interval", "min_scale", "max_scale"}
        fresh = trainer.Trainer(s, _cfg(**dict(cfg, loss_scale=dict(init_scale=2.0 ** 4))))
        assert fresh.opt.loss_scale.growth_interval == 2000
        fresh.load_state_dict(sd)
        _same(sd, fresh.state_dict())
        assert fresh.opt.loss_scale.growth_interval == 2 and fresh.opt.loss_scale.state.data_ptr() != tr.opt.loss_scale.state.data_ptr()
        # the two continue bit for bit: the same gradients (one step's worth, then an overflow) through either optimiser
        g = torch.Generator(device="cuda").manual_seed(11)
        for bad in (False, True, False, False):
            grads = torch.randn(tr.opt.flat.grads.shape, generator=g, device="cuda") * tr.opt.loss_scale.state[0].float()
            if bad:
                grads[-1] = float("inf")
            for x in (tr, fresh):
                x.opt.flat.grads.copy_(grads)
                x.opt.step()
            for a, b in ((tr.opt.flat.params, fresh.opt.flat.params), (tr.opt.m, fresh.opt.m), (tr.opt.v, fresh.opt.v), (tr.opt.adam_state, fresh.opt.adam_state),
                         (tr.opt.loss_scale.state, fresh.opt.loss_scale.state), (tr.opt.stats, fresh.opt.stats)):
                _same(a, b)
        assert tr.opt.loss_scale.read()["backoffs"] >= 1
        with pytest.raises(ValueError, match="loss scale"):
            trainer.Trainer(s, _cfg(dtype=torch.float16)).load_state_dict(sd)
        plain = trainer.Trainer(s, _cfg(dtype=torch.float16)).state_dict()
        assert "loss_scale" not in plain["optimizer"]
        with pytest.raises(ValueError, match="loss scale"):
            fresh.load_state_dict(plain)
    finally:
        s.close()


def test_a_population_keeps_a_scale_per_member():
    import torch
    from gpu_hideseek import population
    from test_gpu_population import P2, WORLDS2, _cfg as _pop_cfg, _sim as _pop_sim
    sim = _pop_sim(WORLDS2, P2)
    try:
        pop = population.Population(sim, _pop_cfg(P2, dtype=torch.float16, loss_scale="dynamic"))
        a, b = pop.members
        assert a.opt.loss_scale is not b.opt.loss_scale and a.opt.loss_scale.state.data_ptr() != b.opt.loss_scale.state.data_ptr()
        b.opt.loss_scale.state[0] = 2.0 ** 10
        out = pop.update_iter()
        scales = [m["loss_scale"] for m in out["policies"]]
        print("population, float16, dynamic:", [(m["loss_scale"], m["skipped"], m["adam_step"]) for m in out["policies"]])
        for m, mb, start in zip(out["policies"], pop.members, (2.0 ** 16, 2.0 ** 10)):
            st = mb.opt.loss_scale.read()
            assert m["loss_scale"] == st["scale"] == start * 2.0 ** -st["backoffs"] and st["backoffs"] == m["skipped"] and m["skipped"] + m["adam_step"] == STEPS
        assert scales[0] != scales[1] or out["policies"][0]["skipped"] != out["policies"][1]["skipped"]
        a.opt.loss_scale.state.copy_(torch.tensor([2.0 ** 5, 1.0, 7.0, 3.0], dtype=torch.float64))
        pop.apply_exploit(1, 0)
        assert b.opt.loss_scale.state.tolist() == [2.0 ** 5, 1.0, 7.0, 3.0] and torch.equal(b.opt.m, a.opt.m)
        assert b.opt.loss_scale.state.data_ptr() != a.opt.loss_scale.state.data_ptr()
    finally:
        sim.close()
