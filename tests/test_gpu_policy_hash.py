"""The SimHash policy on the GPU (policy.make_policy(encoder="hash"): HashEncoder -> LSTMCore(32, 256) and the two heads)
at test_gpu_policy_attention's shapes, 6 worlds x 6 agents, T = 8 steps in K = 2 chunks, float32: forward step by step
against sequence() against the eager composition; one Trainer.update_iter(), after which the projections hold their bits
and the tables have moved; a Population whose exploit step carries the projection along; and a checkpoint through a file
and evaluate.load_policy with the kind inferred.

The allowance is test_gpu_policy_attention's rule: per quantity 4 x the largest difference of the eager composition in
torch float32 from the same in float64, both on the CPU on this test's own rows.  The bins are a step function of the
rows, so the comparison is made on rows with no near tie (tests/test_hash_encoder_host.py's band): the projections are
drawn again, from seeds 0, 1, ..., until none of the rollout's rows has a bit inside the band."""
import copy
import math

import numpy as np
import pytest

import test_hash_encoder_host as H
from test_gpu_policy_attention import AGENTS, EPISODE, K, ROWS, T, _cfg, _chunk, _sim

pytestmark = pytest.mark.gpu


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


def _policy(actor_rows, critic_rows, seed=31):
    """make_policy(encoder="hash") with seeded parameters, a critic head off its zero initialisation, so that the critic's
    backbone has a gradient, and projections under which none of these rows is near a tie."""
    import torch
    from gpu_hideseek import policy as P
    net = P.make_policy(generator=torch.Generator().manual_seed(seed), encoder="hash")
    with torch.no_grad():
        net.critic_head.weight.copy_(0.05 * torch.randn(net.critic_head.weight.shape, generator=torch.Generator().manual_seed(32)))
        for bb, rows in ((net.actor, actor_rows), (net.critic, critic_rows)):
            proj = bb.encoder.named_views()["proj"]
            for s in range(256):
                proj.normal_(0.0, 1.0, generator=torch.Generator().manual_seed(s))
                if not H.near_ties(rows, proj.numpy()).any():
                    break
            else:
                raise AssertionError("no projection among 256 seeds keeps every row off a tie")
            print(f"hash policy: projection seed {s} keeps all {len(rows)} rows off a tie")
    return net


def test_step_loop_sequence_and_eager_agree(rollout):
    sim, actor, critic, clears = rollout
    cpu = [t.cpu() for t in (actor, critic, clears)]
    net = _policy(cpu[0].reshape(T * ROWS, 296).numpy(), cpu[1].reshape(T * ROWS, 296).numpy())
    assert net.encoder == "hash" and not hasattr(net.actor, "mlp") and net.actor.core.hidden == 256
    bins = [H.forward(np.float64, r.reshape(T * ROWS, 296).numpy(), bb.encoder.params.detach().numpy())["bin"] for r, bb in zip(cpu, (net.actor, net.critic))]
    assert (bins[0].reshape(T, ROWS) != bins[1].reshape(T, ROWS)).any() and len(set(bins[0])) > 8
    f64 = _chunk(copy.deepcopy(net).set_fused(False).double(), None, cpu[0].double(), cpu[1].double(), cpu[2])
    f32 = _chunk(copy.deepcopy(net).set_fused(False), None, *cpu)
    allow = {k: 4.0 * float(np.abs(f32[k] - f64[k]).max()) for k in f64}
    assert set(f64) >= {"logits", "critic_logits", "grad actor.encoder.params", "grad critic.encoder.params", "grad critic.core.cell_params"}
    assert f64["logits"].shape == (T, ROWS, 19) and all(np.abs(f64[k]).max() > 0 for k in f64), "every parameter has a gradient"
    net = net.cuda()
    fused = _chunk(net, sim, actor, critic, clears)
    loop = _chunk(net, sim, actor, critic, clears, loop=True)
    eager = _chunk(copy.deepcopy(net).set_fused(False), None, actor, critic, clears)
    for k in f64:
        ef, el, ee = (float(np.abs(r[k] - f64[k]).max()) for r in (fused, loop, eager))
        print(f"hash policy: {k}: fused sequence {ef:.3e}, fused step loop {el:.3e}, eager on the device {ee:.3e} from float64 "
              f"(allowance {allow[k]:.3e}, largest value {float(np.abs(f64[k]).max()):.3e})")
    # What forward and sequence() return is held to the allowance, as in test_gpu_policy_attention; the parameters'
    # gradients are printed there and here, and the encoder's own gradient is held to its derived bound in
    # tests/test_gpu_hash_encoder.py.  The projection's gradient is +0 in every composition.
    for k in f64:
        for name, r in (("fused sequence", fused), ("fused step loop", loop), ("eager on the device", eager)):
            assert r[k].shape == f64[k].shape and np.isfinite(r[k]).all(), (name, k)
            if not k.startswith("grad "):
                assert float(np.abs(r[k] - f64[k]).max()) <= allow[k], (name, k)
    for name, r in (("fused sequence", fused), ("fused step loop", loop), ("eager on the device", eager), ("float64", f64)):
        for side in ("actor", "critic"):
            assert not r[f"grad {side}.encoder.params"][:H.PROJ].any(), (name, side)


def test_one_update_iter_and_the_checkpoint(tmp_path):
    import torch
    from gpu_hideseek import evaluate, policy, trainer
    s = _sim(presteps=EPISODE - 2)
    try:
        cfg = _cfg(lr=3e-4, num_epochs=4)
        tr = trainer.Trainer(s, cfg, net=policy.make_policy(generator=torch.Generator().manual_seed(cfg.seed), encoder="hash"))
        before = tr.opt.flat.params.clone()
        views0 = [{k: v.detach().clone() for k, v in bb.encoder.named_views().items()} for bb in (tr.net.actor, tr.net.critic)]
        m = tr.update_iter()
        print("hash trainer: update_iter:", m)
        flat = [v for v in m.values() if not isinstance(v, list)] + m["value_loss_epochs"]
        assert all(math.isfinite(v) for v in flat), m
        assert m["adam_step"] == cfg.num_epochs * cfg.num_minibatches == int(tr.opt.adam_state[2].item()) and m["skipped"] == 0 and m["update"] == 1
        assert m["grad_norm"] > 0 and m["entropy"] > 0
        for name, (lo, hi, _) in tr.opt.layout().items():
            assert (tr.opt.flat.params[lo:hi] != before[lo:hi]).any().item(), f"{name} did not move"
        for bb, v0 in zip((tr.net.actor, tr.net.critic), views0):
            v1 = bb.encoder.named_views()
            assert torch.equal(v1["proj"].view(torch.int32), v0["proj"].view(torch.int32)), "the projection moved"
            moved = (v1["table"] != v0["table"]).any(1)
            assert moved.any().item() and not moved.all().item()              # 288 rows cannot visit every bin
            assert (v1["scale"] != v0["scale"]).any().item() and (v1["shift"] != v0["shift"]).any().item()
        assert not tr.opt.flat.grads.any().item()
        # the checkpoint, through a file: load_policy finds the kind from the flat length
        sd = tr.state_dict()
        path = str(tmp_path / "hash.pt")
        torch.save(sd, path)
        net, norm = evaluate.load_policy(path, device="cuda:0")
        assert net.encoder == "hash" and norm is not None and [k for k, _ in net.named_parameters()] == [k for k, _ in tr.net.named_parameters()]
        for (k, a), (_, b) in zip(net.named_parameters(), tr.net.named_parameters()):
            assert torch.equal(a, b), k
        assert evaluate.load_policy(sd, device="cuda:0", encoder="hash")[0].encoder == "hash"
        for other in ("simple", "attention"):
            with pytest.raises(ValueError, match="not laid out"):
                evaluate.load_policy(sd, device="cuda:0", encoder=other)
        ev = evaluate.Evaluator(s, net, norm, mode="greedy", from_start=False)      # the loaded policy plays
        ev.run(2)
    finally:
        s.close()


def test_exploit_carries_the_projection():
    import gpu_hideseek
    import torch
    from gpu_hideseek import policy, population
    F = gpu_hideseek.SimFlags
    s = _sim(seed=5, worlds=8, policies=2, flags=int(F.RandomFlipTeams | F.UseFixedWorld | F.ZeroAgentVelocity))
    try:
        cfg = population.PopulationConfig(steps_per_update=T, num_bptt_chunks=K, num_minibatches=2, num_epochs=2, num_policies=2, team_size=AGENTS // 2)
        nets = [policy.make_policy(generator=torch.Generator().manual_seed(7 + i), encoder="hash") for i in range(2)]
        pop = population.Population(s, cfg, nets=nets)
        proj = [[bb.encoder.named_views()["proj"] for bb in (n.actor, n.critic)] for n in pop.nets]
        assert all(not torch.equal(a, b) for a, b in zip(*proj)) and not torch.equal(pop.members[0].opt.flat.params, pop.members[1].opt.flat.params)
        pop.apply_exploit(1, 0)
        assert torch.equal(pop.members[1].opt.flat.params.view(torch.int32), pop.members[0].opt.flat.params.view(torch.int32))
        proj = [[bb.encoder.named_views()["proj"] for bb in (n.actor, n.critic)] for n in pop.nets]
        assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(*proj))
        m = pop.update_iter()                                                 # and both still train
        assert [n.encoder for n in pop.nets] == ["hash", "hash"] and all(pm["skipped"] == 0 and math.isfinite(pm["loss"]) for pm in m["policies"])
    finally:
        s.close()
