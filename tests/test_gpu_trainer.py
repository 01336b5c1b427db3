"""The update loop on the GPU (gpu_hideseek.trainer): 6 worlds x (3 + 3) agents, T = 8 steps in K = 2 chunks, two
minibatches, float32, the simulator first stepped to two steps before an episode's end so that a done falls inside the
rollout.  What collect() stored is replayed on a second simulator, recomputed from the stored chunk-start states, and
checked against a fresh compute_advantages; one minibatch's gradient is compared between the fused and the eager trainer;
then whole update_iter() calls, bfloat16, and a checkpoint.

The allowance is test_gpu_policy's rule: per quantity 4 x the largest difference of the eager composition in torch
float32 from the same in float64, both on the CPU on this test's own rows.  It covers what float32 GEMMs in another order
of summation may differ by; everything after the GEMMs is the kernels' and is pinned by their own tests."""
import math

import pytest

pytestmark = pytest.mark.gpu

WORLDS, AGENTS = 6, 6
ROWS = WORLDS * AGENTS
EPISODE = 240                     # every world resets with step 240 (test_gpu_policy)
T, K = 8, 2
L = T // K


def _sim(seed=3, presteps=EPISODE - 2):
    import gpu_hideseek
    k = AGENTS // 2
    s = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=WORLDS, sim_flags=0, rand_seed=seed,
        min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=1)
    s.init()
    for _ in range(presteps):
        s.step()
    return s


def _cfg(**kw):
    from gpu_hideseek import trainer
    return trainer.TrainConfig(**dict(dict(steps_per_update=T, num_bptt_chunks=K, num_minibatches=2, num_epochs=2), **kw))


def _policy():
    """test_gpu_policy's: make_policy with seeded parameters, a critic head off its zero initialisation, so that the
    critic's backbone has a gradient and the values differ, and the encoders' biases and shifts off theirs, which keeps a
    masked-out entity off the kink of the leaky ReLU, where the kernel and torch take different subgradients."""
    import torch
    from gpu_hideseek import policy as P
    net = P.make_policy(generator=torch.Generator().manual_seed(31))
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        net.critic_head.weight.copy_(0.05 * torch.randn(net.critic_head.weight.shape, generator=g))
        for enc in (net.actor.encoder, net.critic.encoder):
            for parts in enc.named_views().values():
                parts["bias"].copy_(0.1 * torch.randn(parts["bias"].shape, generator=g))
                parts["shift"].copy_(0.1 * torch.randn(parts["shift"].shape, generator=g))
    return net


@pytest.fixture(scope="module")
def collected():
    """(sim, trainer after one collect(), the normaliser's table during that collect)."""
    from gpu_hideseek import trainer
    s = _sim()
    tr = trainer.Trainer(s, _cfg(), net=_policy())
    table = tr.normaliser.table.clone()
    tr.collect()
    yield s, tr, table
    s.close()


def _log_prob(logits, action, buckets):
    import torch
    lp, off = 0.0, 0
    for h, k in enumerate(buckets):
        lp = lp + torch.log_softmax(logits[..., off:off + k], dim=-1).gather(-1, action[..., h:h + 1].long()).squeeze(-1)
        off += k
    return lp


def _decode(critic_logits):
    """symexp(softmax(logits) . bins) in the dtype of the logits (value_head.decode is float32 only)."""
    import torch
    from gpu_hideseek import value_head
    b = value_head.bins().to(critic_logits.dtype)
    return value_head.symexp((torch.softmax(critic_logits, dim=-1) * b).sum(-1))


def test_a_done_falls_inside_the_rollout_and_the_slots_are_aligned(collected):
    import torch
    _, tr, _ = collected
    buf = tr.rollout
    ended = (buf.done != 0).any(dim=1).cpu().tolist()
    assert True in ended[:-1] and False in ended, ended
    assert torch.equal(buf.clear[1:], buf.done[:-1]) and torch.equal(tr.clear, buf.done[-1])
    assert (buf.mask == 1).all().item() and tr.counter == T and tr.stepped
    assert buf.actor.dtype == torch.float32 and tuple(buf.actor.shape) == (T, ROWS, 296) and torch.isfinite(buf.actor).all().item()
    assert buf.moments[:, -1].tolist() == [float(ROWS)] * T


def test_replay_on_a_second_simulator(collected):
    """The stored actions drive a second simulator of the same seed through the same rewards, dones and observations."""
    import torch
    _, tr, table = collected
    buf = tr.rollout
    s2 = _sim()
    try:
        action = s2.action_tensor().to_torch()
        for t in range(T + 1):
            s2.step()
            done = s2.done_tensor().to_torch().reshape(ROWS)
            if t > 0:
                assert torch.equal(s2.reward_tensor().to_torch().reshape(ROWS), buf.reward[t - 1]), t
                assert torch.equal(done, buf.done[t - 1]), t
            if t < T:
                assert torch.equal(done, buf.clear[t]), t
                out = s2.pack_policy_inputs(actor=True, critic=True, normaliser=table)
                assert torch.equal(out["actor"].view(torch.int32), buf.actor[t].view(torch.int32)), t
                assert torch.equal(out["critic"].view(torch.int32), buf.critic[t].view(torch.int32)), t
                action.copy_(buf.action[t].view(action.shape))
    finally:
        s2.close()


def _seq_to_slots(x):
    """[L, K * ROWS, ...] of all sequences in order (id = k ROWS + r) -> [T, ROWS, ...]."""
    return x.reshape(L, K, ROWS, *x.shape[2:]).transpose(0, 1).reshape(T, ROWS, *x.shape[2:])


def test_stored_quantities_belong_to_the_stored_policy(collected):
    """The reference is the episode loop of test_trainer_host from the stored states of chunk 0: it knows neither done nor
    clear.  The recomputation is the trainer's own forward of a minibatch of all sequences, from the stored chunk starts."""
    import torch
    from test_trainer_host import episode_loop, zero_in
    sim, tr, _ = collected
    buf, net = tr.rollout, tr.net
    zero = zero_in(buf.mask.cpu(), buf.critic.cpu())
    assert zero.any(dim=1).tolist() == (buf.clear != 0).any(dim=1).cpu().tolist()             # the done falls on the episode's first slot
    got, want = {}, {}
    index = torch.arange(K * ROWS, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        logits, critic_logits = (_seq_to_slots(x) for x in tr.sequence_logits(buf.minibatch(index)))
        for t in range(T):
            lp = sim.sample_actions(logits[t].contiguous(), mode="evaluate", action=buf.action[t].clone(), log_prob=True)["log_prob"]
            v = sim.value_head(critic_logits[t].contiguous(), value_dtype=torch.float32)["value"]
            got.setdefault("log_prob", []).append(lp.double().cpu())
            got.setdefault("value", []).append(v.double().cpu())
        state0 = ((buf.actor_h[0], buf.actor_c[0]), (buf.critic_h[0], buf.critic_c[0]))
        for name, ft in (("f32", torch.float32), ("f64", torch.float64)):
            ref = _policy().set_fused(False).to(ft)
            st = tuple(tuple(x.cpu().to(ft) for x in s) for s in state0)
            lg, cl, _ = episode_loop(ref, buf.actor.cpu().to(ft), buf.critic.cpu().to(ft), zero, st)
            want[name] = {"log_prob": _log_prob(lg, buf.action.cpu(), net.buckets).double(), "value": _decode(cl).double()}
    stored = {"log_prob": buf.log_prob.double().cpu(), "value": buf.value.double().cpu()}
    for q in ("log_prob", "value"):
        f64, f32, again = want["f64"][q], want["f32"][q], torch.stack(got[q])
        allow = 4.0 * float((f32 - f64).abs().max())
        es, ea = float((stored[q] - f64).abs().max()), float((again - f64).abs().max())
        print(f"trainer: {q}: stored {es:.3e}, recomputed from the chunk starts {ea:.3e} from float64 (allowance {allow:.3e}, "
              f"largest value {float(f64.abs().max()):.3e})")
        assert f64.shape == stored[q].shape == again.shape == (T, ROWS) and allow > 0
        assert es <= allow and ea <= allow, q


def test_advantages_are_those_of_the_stored_buffers(collected):
    import torch
    sim, tr, _ = collected
    buf, cfg = tr.rollout, tr.cfg
    out = sim.compute_advantages(buf.reward, buf.done, buf.value, tr.bootstrap, gamma=cfg.gamma, gae_lambda=cfg.gae_lambda, mask=buf.mask, moments=True)
    assert torch.equal(out["advantages"].view(torch.int32), buf.advantage.view(torch.int32))
    assert torch.equal(out["returns"].view(torch.int32), buf.returns.view(torch.int32))
    assert torch.equal(out["moments"], tr.adv_moments) and tr.adv_moments[4].item() == T * ROWS
    assert buf.advantage.abs().max().item() > 0 and torch.isfinite(tr.bootstrap).all().item()
    # the bootstrap is the critic's value of the observation after the last step, and taking it did not advance the state
    before = [t.clone() for s in tr.state for t in s]
    again = tr.bootstrap_value().clone()
    assert torch.equal(again, tr.bootstrap) and all(torch.equal(a, b) for a, b in zip(before, [t for s in tr.state for t in s]))


def test_gradient_of_one_minibatch_fused_against_eager(collected):
    import torch
    from gpu_hideseek import trainer
    sim, tr, _ = collected
    eager = trainer.Trainer(sim, _cfg(), net=_policy(), fused=False)
    assert torch.equal(eager.opt.flat.params, tr.opt.flat.params) and not eager.net.actor.fused and tr.net.actor.fused
    for k, t in tr.rollout.tensors().items():
        getattr(eager.rollout, k).copy_(t)
    eager.adv_moments.copy_(tr.adv_moments)
    index = torch.randperm(K * ROWS, generator=torch.Generator().manual_seed(41)).to(torch.int32).cuda()[:K * ROWS // 2]
    # the fused trainer's forward_backward gives the two losses' upstream gradients; the eager trainer's forward of the
    # same minibatch is put under the same ones, so that the two flat gradients differ by the policy's backward alone
    assert not tr.opt.flat.grads.any().item() and not eager.opt.flat.grads.any().item()
    pol, val = tr.forward_backward(index)
    up = pol["grad_logits"].clone(), val["grad_logits"].clone()
    lg, cl = eager.sequence_logits(eager.minibatch(index))
    torch.autograd.backward([lg.reshape(up[0].shape), cl.reshape(up[1].shape)], list(up))
    grads = {"fused": tr.opt.flat.grads.clone(), "eager": eager.opt.flat.grads.clone()}
    assert grads["eager"].any().item()
    tr.opt.zero_grad()
    eager.opt.zero_grad()
    # the allowance: the trainer's own forward of a minibatch on the CPU in float64 and float32 (with eager pieces it needs
    # the policy and no simulator), on this minibatch's rows, under the fused trainer's upstream gradients
    import types
    mb = {k: v.cpu() for k, v in tr.rollout.minibatch_eager(index).items()}
    ref = {}
    for name, ft in (("f32", torch.float32), ("f64", torch.float64)):
        net = _policy().set_fused(False).to(ft)
        rows = {k: v.to(ft) if k in ("actor", "critic", "actor_h", "actor_c", "critic_h", "critic_c") else v for k, v in mb.items()}
        lg, cl = trainer.Trainer.sequence_logits(types.SimpleNamespace(net=net, sim=None), rows)
        torch.autograd.backward([lg.reshape(up[0].shape), cl.reshape(up[1].shape)], [up[0].cpu().to(ft), up[1].cpu().to(ft)])
        ref[name] = {k: p.grad.double() for k, p in net.named_parameters()}
    layout = tr.opt.layout()
    assert set(layout) == set(ref["f64"]) and len(layout) == 24
    worst = []
    for k, (lo, hi, shape) in layout.items():
        allow = 4.0 * float((ref["f32"][k] - ref["f64"][k]).abs().max())
        gf, ge = grads["fused"][lo:hi].view(shape).double().cpu(), grads["eager"][lo:hi].view(shape).double().cpu()
        diff, ef, ee = float((gf - ge).abs().max()), float((gf - ref["f64"][k]).abs().max()), float((ge - ref["f64"][k]).abs().max())
        print(f"trainer: grad {k}: fused - eager {diff:.3e}; from float64: fused {ef:.3e}, eager {ee:.3e} (allowance {allow:.3e}, "
              f"largest value {float(ref['f64'][k].abs().max()):.3e})")
        assert float(ref["f64"][k].abs().max()) > 0, k
        worst.append((k, diff, allow))
    for k, diff, allow in worst:
        assert diff <= allow, (k, diff, allow)


def test_a_whole_update_iter():
    import torch
    from gpu_hideseek import trainer
    s = _sim()
    try:
        cfg = _cfg(lr=3e-4, num_epochs=4)
        tr = trainer.Trainer(s, cfg)
        before = tr.opt.flat.params.clone()
        m = tr.update_iter()
        print("trainer: update_iter:", m)
        flat = [v for v in m.values() if not isinstance(v, list)] + m["value_loss_epochs"]
        assert all(math.isfinite(v) for v in flat), m
        assert m["adam_step"] == cfg.num_epochs * cfg.num_minibatches == int(tr.opt.adam_state[2].item()) and m["skipped"] == 0 and m["update"] == 1
        assert m["fps"] > 0 and m["grad_norm"] > 0 and 0 <= m["clip_fraction"] <= 1 and m["entropy"] > 0
        for name, (lo, hi, _) in tr.opt.layout().items():
            assert (tr.opt.flat.params[lo:hi] != before[lo:hi]).any().item(), f"{name} did not move"
        assert not tr.opt.flat.grads.any().item()
        first, last = m["value_loss_epochs"][0], m["value_loss_epochs"][-1]
        # the critic head starts at zero, so the first minibatch's cross-entropy is log 255 = 5.541
        print(f"trainer: value cross-entropy per epoch {m['value_loss_epochs']} (log 255 = {math.log(255):.4f})")
        assert len(m["value_loss_epochs"]) == 4 and last < first
        assert (tr.rollout.done != 0).any().item()
        # the next rollout starts from the observation the bootstrap was taken from, without another step
        assert tr.stepped
        tr.collect()
        assert tr.counter == 2 * T and torch.equal(tr.rollout.clear[1:], tr.rollout.done[:-1])
    finally:
        s.close()


def test_bfloat16():
    import torch
    from gpu_hideseek import trainer
    s = _sim(presteps=0)
    try:
        tr = trainer.Trainer(s, _cfg(dtype=torch.bfloat16))
        m = tr.update_iter()
        assert all(math.isfinite(v) for v in [v for v in m.values() if not isinstance(v, list)] + m["value_loss_epochs"]), m
        assert tr.rollout.actor.dtype == tr.rollout.actor_h.dtype == tr.state[0][0].dtype == tr.state[1][0].dtype == torch.bfloat16
        assert tr.rollout.actor_c.dtype == tr.state[0][1].dtype == tr.state[1][1].dtype == torch.float32
        assert m["adam_step"] == 4 and m["skipped"] == 0
    finally:
        s.close()


def _same(a, b, path=""):
    import torch
    if isinstance(a, torch.Tensor):
        assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape, path
        assert torch.equal(a.cpu().contiguous().view(-1).view(torch.uint8), b.cpu().contiguous().view(-1).view(torch.uint8)), path
    elif isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b, (path, a, b)


def test_checkpoint():
    import torch
    from gpu_hideseek import trainer
    s = _sim(presteps=0)
    try:
        tr = trainer.Trainer(s, _cfg())
        tr.update_iter()
        sd = tr.state_dict()
        assert sd["update_index"] == 1 and sd["counter"] == T and sd["optimizer"]["state"][2].item() == 4
        assert set(sd) == {"params", "optimizer", "normaliser", "state", "clear", "generator", "update_index", "counter"}
        fresh = trainer.Trainer(s, _cfg())
        assert not torch.equal(fresh.opt.flat.params, tr.opt.flat.params)
        fresh.load_state_dict(sd)
        _same(sd, fresh.state_dict())
        assert torch.equal(fresh.opt.flat.params, tr.opt.flat.params) and torch.equal(fresh.opt.m, tr.opt.m) and torch.equal(fresh.opt.v, tr.opt.v)
        assert torch.equal(fresh.normaliser.state, tr.normaliser.state) and (fresh.update_index, fresh.counter) == (1, T)
        # the parameters the modules see are the loaded ones (views of the flat buffer)
        assert torch.equal(fresh.net.actor_head.weight, tr.net.actor_head.weight)
        # the same permutation comes next
        a = torch.randperm(16, generator=tr.generator, device="cuda")
        b = torch.randperm(16, generator=fresh.generator, device="cuda")
        assert torch.equal(a, b)
        with pytest.raises(ValueError, match="normalise_obs"):
            trainer.Trainer(s, _cfg(normalise_obs=False)).load_state_dict(sd)
    finally:
        s.close()


def test_configs_that_do_not_fit_are_refused():
    from gpu_hideseek import trainer
    s = _sim(presteps=0)
    try:
        for kw, what in ((dict(steps_per_update=9), "multiple of num_bptt_chunks"), (dict(num_minibatches=5), "do not divide into 5 minibatches"),
                         (dict(num_epochs=0), "num_epochs must be a positive integer")):
            with pytest.raises(ValueError, match=what):
                trainer.Trainer(s, _cfg(**kw))
    finally:
        s.close()
