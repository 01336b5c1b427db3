"""The policy modules on the GPU (gpu_hideseek.policy: Backbone, ActorCritic, make_policy) on the packed rows of a stepped
simulator, 6 worlds x 6 agents over T = 3 steps around an episode's end, with the done export as clear: the fused
composition against the same modules with eager pieces (fused=False: entity_encoder.eager, mlp.eager and
recurrent.eager_sequence) in logits, critic logits and every parameter's gradient; sequence() against the step loop; and
five Adam steps of ppo_loss + value_head on one tiny minibatch.

The allowance is the one of the LSTM and MLP module tests: per quantity 4 x the largest difference of the eager
composition in torch float32 from the same in float64, both on the CPU on the test's own rows.  It covers what float32
GEMMs in another order of summation may differ by; everything after the GEMMs is the kernels' and is pinned by their own
tests."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WORLDS, AGENTS, T = 6, 6, 3
ROWS = WORLDS * AGENTS
EPISODE = 240                     # every world resets with step 240 (test_gpu_lstm_cell.test_the_done_export_as_clear)


def _sim(seed=3):
    import gpu_hideseek
    k = AGENTS // 2
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=WORLDS, sim_flags=0, rand_seed=seed,
        min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=1)


@pytest.fixture(scope="module")
def rollout():
    """(sim, actor rows [T, ROWS, 296], critic rows, clears [T, ROWS] int32): the last step before an episode's end, the
    step that ends it and the first of the next."""
    import torch
    s = _sim()
    s.init()
    for _ in range(EPISODE - 2):
        s.step()
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


def _policy():
    """make_policy with seeded parameters, a critic head off its zero initialisation, so that the critic's backbone has a
    gradient, and the encoders' biases and shifts off theirs.  With bias = shift = 0 a masked-out (all-zero) entity of the
    actor's rows has y = 0 exactly, the kink of the leaky ReLU, and wins the max-pool wherever the visible entities are
    negative; there hs_entity_encode_backward takes the derivative 1 (its header: y >= 0) and torch's leaky_relu takes
    `slope`.  Both are subgradients; a comparison of gradients has to stay off the kink, as the central differences of
    the host tests do."""
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


def _weights(device, dtype):
    import torch
    g = torch.Generator().manual_seed(33)
    return torch.randn(T, ROWS, 19, generator=g).to(device, dtype), torch.randn(T, ROWS, 255, generator=g).to(device, dtype)


def _chunk(net, sim, actor, critic, clears, loop=False):
    """logits, critic logits, the final state's four tensors and every parameter's gradient of
    loss = sum(logits * w1) + sum(critic_logits * w2) over the chunk, as float64 numpy; with loop=True step by step."""
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
    w1, w2 = _weights(actor.device, dtype)
    ((logits * w1).sum() + (critic_logits * w2).sum()).backward()
    out = {"logits": logits, "critic_logits": critic_logits, "actor h": state[0][0], "actor c": state[0][1], "critic h": state[1][0], "critic c": state[1][1]}
    out.update({"grad " + k: p.grad for k, p in net.named_parameters()})
    return {k: v.detach().double().cpu().numpy() for k, v in out.items()}


def test_fused_against_eager_and_sequence_against_the_step_loop(rollout):
    import torch
    sim, actor, critic, clears = rollout
    net = _policy()
    # the reference and the allowance: the eager composition on the CPU, float64 and float32
    cpu = [t.cpu() for t in (actor, critic, clears)]
    f64 = _chunk(copy.deepcopy(net).set_fused(False).double(), None, cpu[0].double(), cpu[1].double(), cpu[2])
    f32 = _chunk(copy.deepcopy(net).set_fused(False), None, *cpu)
    allow = {k: 4.0 * float(np.abs(f32[k] - f64[k]).max()) for k in f64}
    assert set(f64) >= {"logits", "critic_logits", "grad actor.mlp.layers.2.params", "grad critic.core.cell_params", "grad actor_head.weight"}
    assert f64["logits"].shape == (T, ROWS, 19) and f64["critic_logits"].shape == (T, ROWS, 255)
    assert all(np.abs(f64[k]).max() > 0 for k in f64), "every parameter has a gradient"
    net = net.cuda()
    fused = _chunk(net, sim, actor, critic, clears)
    eager = _chunk(copy.deepcopy(net).set_fused(False), None, actor, critic, clears)
    loop = _chunk(net, sim, actor, critic, clears, loop=True)
    for k in f64:
        ef, ee, el = (float(np.abs(r[k] - f64[k]).max()) for r in (fused, eager, loop))
        print(f"policy: {k}: fused sequence {ef:.3e}, eager on the device {ee:.3e}, fused step loop {el:.3e} from float64 "
              f"(allowance {allow[k]:.3e}, largest value {float(np.abs(f64[k]).max()):.3e})")
    for k in f64:
        for name, r in (("fused sequence", fused), ("eager on the device", eager), ("fused step loop", loop)):
            assert r[k].shape == f64[k].shape and float(np.abs(r[k] - f64[k]).max()) <= allow[k], (name, k)
    # the clear: the rows whose episode ended carry a zero state out of that step
    ended = int((clears != 0).any(dim=1).float().argmax())
    state = net.init_state(ROWS, "cuda")
    with torch.no_grad():
        _, _, mid = net.sequence(sim, actor[:ended + 1], critic[:ended + 1], state, clears[:ended + 1])
    rows = clears[ended] != 0
    for s in mid:
        assert not s[0][rows].any().item() and not s[1][rows].any().item()


def test_bf16_and_five_adam_steps(rollout):
    import torch
    from gpu_hideseek import policy as P, ppo_loss, value_head
    sim, actor, critic, clears = rollout
    # the compute dtype: bf16 rows, features, GEMMs and h; float32 c
    nb = P.make_policy(torch.bfloat16, generator=torch.Generator().manual_seed(34)).cuda()
    state = nb.init_state(ROWS, "cuda")
    with torch.no_grad():
        lg, cl, state = nb(sim, actor[0].bfloat16(), critic[0].bfloat16(), state, clears[0])
    assert lg.dtype == cl.dtype == state[0][0].dtype == torch.bfloat16 and state[0][1].dtype == torch.float32
    assert lg.shape == (ROWS, 19) and cl.shape == (ROWS, 255) and torch.isfinite(lg.float()).all().item() and not cl.any().item()
    # one tiny minibatch: the chunk's T * ROWS samples, actions drawn from the first policy, fixed advantages and returns
    net = _policy().cuda()
    n = T * ROWS
    state0 = net.init_state(ROWS, "cuda")
    with torch.no_grad():
        logits, _, _ = net.sequence(sim, actor, critic, state0, clears)
    action = torch.empty(T, ROWS, 5, dtype=torch.int32, device="cuda")
    old_log_prob = torch.empty(T, ROWS, device="cuda")
    for t in range(T):
        sim.sample_actions(logits[t].contiguous(), seed=(5, 6), counter=t, action=action[t], log_prob=old_log_prob[t])
    g = torch.Generator().manual_seed(35)
    advantage, returns = torch.randn(n, generator=g).cuda(), (2.0 * torch.randn(n, generator=g)).cuda()
    opt = torch.optim.Adam(net.parameters(), lr=3e-4)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        logits, critic_logits, _ = net.sequence(sim, actor, critic, state0, clears)
        logits, critic_logits = logits.reshape(n, 19), critic_logits.reshape(n, 255)
        pol = sim.ppo_loss(logits.detach(), action.view(n, 5), old_log_prob.view(n), advantage)
        val = sim.value_head(critic_logits.detach(), returns, loss_coef=0.5)
        loss = ppo_loss.attach(logits, None, pol) + value_head.attach(critic_logits, val)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("policy under Adam:", losses)
    assert all(np.isfinite(losses)) and all(b < a for a, b in zip(losses, losses[1:]))
    assert all(p.grad is not None and torch.isfinite(p.grad).all().item() for p in net.parameters())
