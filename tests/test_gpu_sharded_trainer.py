"""Data-parallel training over shards on the GPU (gpu_hideseek.trainer.ShardedTrainer): test_gpu_trainer's shape and policy,
6 worlds as 3 + 3 (and 7 as 3 + 2 + 2), T = 8 steps in K = 2 chunks, two minibatches, float32, on the devices [0, 1] where a
second one exists and on [0, 0] otherwise.  The simulator draws 1 to 3 hiders and 1 to 3 seekers per world, and the seed is
one at which the shards' numbers of active samples differ (asserted: it is a condition of these tests, chosen by looking at
the first seeds), so that a mean of the shards' gradients that ignored the counts would be another gradient.

What is pinned: the replicas stay bit-equal; the advantage moments and the normalisers are the global ones; the reduced
gradient is that of ONE policy over the union of the shards' minibatches, within test_gpu_trainer's allowance (4 x the
largest difference between that computation in float32 and in float64 on the CPU); one shard is the Trainer bit for bit;
the metrics; a checkpoint; bfloat16 and float16 under a loss scale that is far too large; a config that does not fit."""
import math

import pytest

import test_gpu_trainer as TT
from test_gpu_trainer import AGENTS, K, L, T

pytestmark = pytest.mark.gpu

SEED = 3
LAYOUTS = {2: 6, 3: 7}            # shards: worlds (3 + 3; 3 + 2 + 2)


def _devices(G):
    import torch
    return [g % 2 for g in range(G)] if torch.cuda.device_count() >= 2 else [0] * G


def _kw(seed=SEED, teams=(1, 3)):
    import gpu_hideseek
    return dict(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, sim_flags=0, rand_seed=seed, min_hiders=teams[0], max_hiders=teams[1],
                min_seekers=teams[0], max_seekers=teams[1], num_pbt_policies=1)


def _ssim(G=2, worlds=None, **kw):
    from gpu_hideseek.sharded import ShardedSimulator
    s = ShardedSimulator(_devices(G), LAYOUTS[G] if worlds is None else worlds, **_kw(**kw))
    s.init()
    return s


def _same(a, b, tag=""):
    TT._same(a, b, tag)


def _finite(m):
    return all(math.isfinite(v) for v in [v for v in m.values() if not isinstance(v, list)] + m["value_loss_epochs"])


def _active(tr):
    """Every shard's number of active samples in its rollout."""
    return [float(m.rollout.mask.sum().item()) for m in tr.members]


def _replica_tensors(m):
    return {"params": m.opt.flat.params, "m": m.opt.m, "v": m.opt.v, "adam_state": m.opt.adam_state, "normaliser.state": m.normaliser.state,
            "normaliser.table": m.normaliser.table, "adv_moments": m.adv_moments}


@pytest.mark.parametrize("G", sorted(LAYOUTS))
def test_replicas_agree(G):
    import torch
    from gpu_hideseek import trainer
    s = _ssim(G)
    try:
        cfg = TT._cfg(lr=3e-4)
        tr = trainer.ShardedTrainer(s, cfg, net=TT._policy())
        assert [m.sim.num_worlds for m in tr.members] == {2: [3, 3], 3: [3, 2, 2]}[G] and tr.rows == LAYOUTS[G] * AGENTS
        assert [m.device.index for m in tr.members] == _devices(G)
        before = tr.members[0].opt.flat.params.clone()
        for it in range(2):
            out = tr.update_iter()
            active = _active(tr)
            print(f"sharded trainer, {G} shards, update {it + 1}: active samples per shard {active}, count of the last minibatch {out['count']}")
            assert len(set(active)) > 1, active                                # the condition: the shards' counts differ
            assert _finite(out) and out["shards"] == G and out["skipped"] == 0 and out["adam_step"] == (it + 1) * cfg.num_epochs * cfg.num_minibatches
            ref = _replica_tensors(tr.members[0])
            for g, m in enumerate(tr.members[1:], 1):
                for k, t in _replica_tensors(m).items():
                    _same(ref[k], t, f"update {it + 1}, shard {g}: {k}")
                assert not m.opt.flat.grads.any().item()
            assert not tr.members[0].opt.flat.grads.any().item()
        for name, (lo, hi, _) in tr.members[0].opt.layout().items():
            assert (tr.members[0].opt.flat.params[lo:hi] != before[lo:hi]).any().item(), f"{name} did not move"
        # the count is that of the last minibatch over all shards, on every device the same
        assert out["count"] == sum(float(m._ppo_out[6].item()) for m in tr.members) > 0
        assert all(t.item() == out["count"] for t in tr.totals) and all(torch.equal(c.cpu(), tr.counts[0].cpu()) for c in tr.counts)
    finally:
        s.close()


@pytest.fixture(scope="module")
def collected():
    """(ssim, ShardedTrainer over two shards after one collect(), each normaliser's state before it)."""
    from gpu_hideseek import trainer
    s = _ssim(2)
    tr = trainer.ShardedTrainer(s, TT._cfg(), net=TT._policy())
    tr.collect()
    yield s, tr
    s.close()


def test_global_moments(collected):
    import numpy as np
    import torch
    from gpu_hideseek.policy_inputs import ObsNormaliser
    _, tr = collected
    cfg = tr.cfg
    own = []
    for m in tr.members:
        buf = m.rollout
        out = m.sim.compute_advantages(buf.reward, buf.done, buf.value, m.bootstrap, gamma=cfg.gamma, gae_lambda=cfg.gae_lambda, mask=buf.mask, moments=True)
        _same(out["advantages"], buf.advantage, "advantages")
        own.append(out["moments"].cpu().numpy())
    assert own[0][4] != own[1][4] and own[0][4] + own[1][4] == sum(_active(tr))         # the shards' counts differ
    want = own[0].copy()
    for x in own[1:]:
        want = want + x                                                                 # float64, in shard order
    for g, m in enumerate(tr.members):
        assert np.array_equal(m.adv_moments.cpu().numpy().view(np.uint64), want.view(np.uint64)), g
    stack = torch.cat([m.rollout.moments.to(tr.device) for m in tr.members])
    assert tuple(stack.shape) == (2 * T, 593)
    fresh = ObsNormaliser(tr.members[0].sim.gpu_id)
    fresh.update(tr.members[0].sim, stack)
    for g, m in enumerate(tr.members):
        _same(m.normaliser.state, fresh.state, f"normaliser state {g}")
        _same(m.normaliser.table, fresh.table, f"normaliser table {g}")
    assert fresh.state[-1].item() > 0


def test_the_reduced_gradient_is_the_unions(collected):
    """Every member's forward_backward on the same fixed index of its own rollout, then the trainer's exchange and
    reduction; the reference is one policy over the members' gathered minibatches, concatenated along the sequence
    dimension: its logits on the GPU give the two losses' upstream gradients over the union (hs_ppo_loss and
    hs_twohot_value with the global moments: they divide by the union's count), and the backward under those runs on the
    CPU in float64, and in float32 for the allowance."""
    import types
    import torch
    from gpu_hideseek import rollout, trainer
    _, tr = collected
    cfg, first = tr.cfg, tr.members[0]
    seqs = K * first.rows
    index = torch.randperm(seqs, generator=torch.Generator().manual_seed(41)).to(torch.int32)[:seqs // 2]
    assert all(m.rows == first.rows for m in tr.members) and not any(m.opt.flat.grads.any().item() for m in tr.members)
    mbs, counts = [], []
    for m in tr.members:
        with torch.cuda.device(m.device):
            m.forward_backward(index.to(m.device))
        mbs.append({k: v.to(tr.device).clone() for k, v in m._mb.items()})
        counts.append(float(m._ppo_out[6].item()))
    own = [m.opt.flat.grads.clone() for m in tr.members]
    print(f"sharded trainer: active samples of the minibatch per shard {counts}")
    assert counts[0] != counts[1] and min(counts) > 0                                   # the condition
    tr.exchange_gradients()
    tr.reduce_gradients()
    reduced = first.opt.flat.grads.clone()
    for g, m in enumerate(tr.members):
        _same(m.opt.flat.grads, reduced, f"reduced gradient on shard {g}")
        assert tr.totals[g].item() == sum(counts)
    # the kernel's contract on the real buffers
    from gpu_hideseek import optim
    want, _ = optim.host_reduce([x.cpu().numpy() for x in own], counts)
    _same(reduced, torch.from_numpy(want), "host_reduce")
    for m in tr.members:
        m.opt.zero_grad()
    # the union
    union = {k: torch.cat([mb[k] for mb in mbs], dim=0 if k in rollout.PER_CHUNK else 1) for k in mbs[0]}
    S = union["clear"].numel()
    mask = union["mask"].reshape(S)
    assert float(mask.sum().item()) == sum(counts)
    with torch.no_grad(), torch.cuda.device(tr.device):
        lg, cl = first.sequence_logits(union)
        pol = first.sim.ppo_loss(lg.reshape(S, -1), union["action"].reshape(S, -1), union["log_prob"].reshape(S), union["advantage"].reshape(S),
                                 buckets=first.net.buckets, adv_moments=first.adv_moments, mask=mask, clip_coef=cfg.clip_coef, entropy_coef=cfg.entropy_coef)
        val = first.sim.value_head(cl.reshape(S, -1), union["returns"].reshape(S), bins=first.net.bins, mask=mask, value=None, loss_coef=cfg.value_loss_coef,
                                   stats=True)
    assert pol["stats"][6].item() == sum(counts)
    up = pol["grad_logits"].cpu(), val["grad_logits"].cpu()
    rows = {k: v.cpu() for k, v in union.items()}
    ref = {}
    for name, ft in (("f32", torch.float32), ("f64", torch.float64)):
        net = TT._policy().set_fused(False).to(ft)
        x = {k: v.to(ft) if k in ("actor", "critic") + rollout.PER_CHUNK else v for k, v in rows.items()}
        lg, cl = trainer.Trainer.sequence_logits(types.SimpleNamespace(net=net, sim=None), x)
        torch.autograd.backward([lg.reshape(up[0].shape), cl.reshape(up[1].shape)], [up[0].to(ft), up[1].to(ft)])
        ref[name] = {k: p.grad.double() for k, p in net.named_parameters()}
    layout = first.opt.layout()
    assert set(layout) == set(ref["f64"]) and len(layout) == 24
    worst = []
    for k, (lo, hi, shape) in layout.items():
        allow = 4.0 * float((ref["f32"][k] - ref["f64"][k]).abs().max())
        got = reduced[lo:hi].view(shape).double().cpu()
        plain = (0.5 * (own[0].to(tr.device) + own[1].to(tr.device)))[lo:hi].view(shape).double().cpu()
        diff, unweighted = float((got - ref["f64"][k]).abs().max()), float((plain - ref["f64"][k]).abs().max())
        print(f"sharded trainer: grad {k}: reduced - union in float64 {diff:.3e} (allowance {allow:.3e}, largest value "
              f"{float(ref['f64'][k].abs().max()):.3e}); the unweighted mean of the shards is off by {unweighted:.3e}")
        assert float(ref["f64"][k].abs().max()) > 0 and allow > 0, k
        worst.append((k, diff, allow))
    for k, diff, allow in worst:
        assert diff <= allow, (k, diff, allow)


def test_one_shard_is_the_trainer():
    import gpu_hideseek
    from gpu_hideseek import trainer
    from gpu_hideseek.sharded import ShardedSimulator
    s = ShardedSimulator([0], 6, **_kw())
    s.init()
    plain = gpu_hideseek.HideAndSeekSimulator(gpu_id=0, num_worlds=6, **_kw())
    plain.init()
    try:
        cfg = TT._cfg(lr=3e-4)
        st, tr = trainer.ShardedTrainer(s, cfg, net=TT._policy()), trainer.Trainer(plain, cfg, net=TT._policy())
        a, b = st.update_iter(), tr.update_iter()
        one = st.members[0]
        for k, t in tr.rollout.tensors().items():
            _same(getattr(one.rollout, k), t, f"rollout.{k}")
        for k, t in _replica_tensors(tr).items():
            _same(_replica_tensors(one)[k], t, k)
        _same(one.bootstrap, tr.bootstrap, "bootstrap")
        _same([x for s_ in one.state for x in s_], [x for s_ in tr.state for x in s_], "state")
        assert a.pop("shards") == 1 and a.pop("count") == float(one._ppo_out[6].item()) > 0
        a.pop("fps"), b.pop("fps")
        assert a == b and _finite(a), (a, b)
        assert (st.update_index, one.counter, st.stepped) == (tr.update_index, tr.counter, tr.stepped) == (1, T, True)
    finally:
        s.close()
        plain.close()


def test_a_checkpoint_continues_bit_for_bit():
    """Two sharded simulators of one seed, a trainer on each, one update on both.  The first trainer's state goes into a
    fresh trainer on its simulator; the second trainer loads its own (so that both start the next rollout with the step
    that load_state_dict() asks for).  The next update is the same on both, bit for bit."""
    import torch
    from gpu_hideseek import trainer
    sa, sb = _ssim(2), _ssim(2)
    try:
        ta, tb = trainer.ShardedTrainer(sa, TT._cfg()), trainer.ShardedTrainer(sb, TT._cfg())
        ma, mb = ta.update_iter(), tb.update_iter()
        ma.pop("fps"), mb.pop("fps")
        assert ma == mb
        sd = ta.state_dict()
        assert set(sd) == {"params", "optimizer", "normaliser", "state", "clear", "generator", "generators", "ranges", "update_index", "counter"}
        assert sd["ranges"] == [[0, 3], [3, 3]] and len(sd["state"]) == len(sd["clear"]) == len(sd["generators"]) == 2 and sd["update_index"] == 1
        fresh = trainer.ShardedTrainer(sa, TT._cfg())
        assert not torch.equal(fresh.members[0].opt.flat.params, ta.members[0].opt.flat.params)      # ta has learnt
        fresh.load_state_dict(sd)
        TT._same(sd, fresh.state_dict())
        for g, m in enumerate(fresh.members):
            for k, t in _replica_tensors(ta.members[g]).items():
                if k != "adv_moments":
                    _same(_replica_tensors(m)[k], t, f"loaded, shard {g}: {k}")
        tb.load_state_dict(tb.state_dict())
        del ta
        x, y = fresh.update_iter(), tb.update_iter()
        x.pop("fps"), y.pop("fps")
        assert x == y and x["update"] == 2, (x, y)
        for g in range(2):
            for k, t in _replica_tensors(tb.members[g]).items():
                _same(_replica_tensors(fresh.members[g])[k], t, f"continued, shard {g}: {k}")
        # another layout of the same worlds is refused
        three = _ssim(3, worlds=6)
        try:
            with pytest.raises(ValueError, match="shards hold the worlds"):
                trainer.ShardedTrainer(three, TT._cfg()).load_state_dict(sd)
        finally:
            three.close()
    finally:
        sa.close()
        sb.close()


def test_bfloat16_and_a_loss_scale_far_too_large():
    import torch
    from gpu_hideseek import trainer
    from test_gpu_trainer_loss_scale import STEPS, _policy
    s = _ssim(2)
    try:
        tr = trainer.ShardedTrainer(s, TT._cfg(dtype=torch.bfloat16))
        m = tr.update_iter()
        assert _finite(m) and m["adam_step"] == STEPS and m["skipped"] == 0 and tr.members[1].rollout.actor.dtype == torch.bfloat16
        for k, t in _replica_tensors(tr.members[1]).items():
            _same(_replica_tensors(tr.members[0])[k], t, f"bfloat16: {k}")
    finally:
        s.close()
    # float16 from 2^30: every step overflows on every replica alike, and all of them end at the same scale
    s = _ssim(2)
    try:
        tr = trainer.ShardedTrainer(s, TT._cfg(dtype=torch.float16, loss_scale=dict(init_scale=2.0 ** 30, max_scale=2.0 ** 30)), net=_policy(torch.float16))
        before = tr.members[0].opt.flat.params.clone()
        m = tr.update_iter()
        print("sharded trainer, float16 from 2^30:", {k: m[k] for k in ("skipped", "adam_step", "loss_scale", "grad_norm")})
        assert m["skipped"] == STEPS and m["adam_step"] == 0 and m["loss_scale"] == 2.0 ** 26
        for g, member in enumerate(tr.members):
            assert member.opt.loss_scale.read() == {"scale": 2.0 ** 26, "good_steps": 0, "backoffs": STEPS, "growths": 0}, g
            _same(member.opt.flat.params, before, f"float16, shard {g}")
            assert member.opt.adam_state.tolist() == [1.0, 1.0, 0.0, float(STEPS)] and not member.opt.flat.grads.any().item()
    finally:
        s.close()


def test_a_config_that_does_not_fit_a_shard_names_it():
    from gpu_hideseek import trainer
    s = _ssim(3)                                                     # 3 + 2 + 2 worlds: 18, 12 and 12 rows
    try:
        # K n = 36, 24, 24 sequences: 9 minibatches divide the first shard's and not the second's
        with pytest.raises(ValueError, match=r"shard 1 \(2 worlds on GPU \d\): the 24 sequences .* do not divide into 9 minibatches"):
            trainer.ShardedTrainer(s, TT._cfg(num_minibatches=9))
        with pytest.raises(ValueError, match=r"shard 0 \(3 worlds on GPU 0\): steps_per_update \(9\) must be a multiple"):
            trainer.ShardedTrainer(s, TT._cfg(steps_per_update=9))
    finally:
        s.close()
