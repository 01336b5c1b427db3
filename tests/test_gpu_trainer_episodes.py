"""The trainer at an episode's end, with teams that change (gpu_hideseek.trainer): 8 worlds of seed 1 with 1..3 hiders and
1..3 seekers, 6 agent rows per world, T = 8 steps in K = 2 chunks, float32.  With the episode the active rows of a world
change: rows stay, join, leave or stay out.  The simulator is stepped so that the next episode's first observation falls
on a chosen slot.

The reference is the episode loop of test_trainer_host (plain torch on the CPU, float64 and float32, eager pieces): per
slot, zero the state where the row is out or the slot's observation is an episode's first (prep_counter = 96, read from
the stored critic rows), then one forward with no clear.  It uses neither done nor clear nor sequence().  The allowance is
the project's rule: per quantity 4 x the largest |float32 loop - float64 loop| over the compared elements, which are those
of the active rows."""
import pytest

from test_gpu_trainer import L, K, T, _cfg, _decode, _log_prob, _policy
from test_trainer_host import episode_loop, zero_in

pytestmark = pytest.mark.gpu

WORLDS, AGENTS = 8, 6
ROWS = WORLDS * AGENTS
EPISODE = 240
ACTIVE = ([3, 3, 5, 6, 5, 2, 4, 4], [5, 5, 6, 6, 4, 5, 2, 4])        # active rows per world in episodes 0 and 1: a prefix of its rows
KINDS = {"stay": 29, "join": 8, "leave": 3, "out": 8}
STATES = ("actor_h", "actor_c", "critic_h", "critic_c")


def _sim(presteps):
    import gpu_hideseek
    s = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=WORLDS, sim_flags=0, rand_seed=1,
        min_hiders=1, max_hiders=3, min_seekers=1, max_seekers=3, num_pbt_policies=1)
    s.init()
    for _ in range(presteps):
        s.step()
    return s


def _prefix(counts):
    import torch
    return torch.tensor([[float(a < c) for a in range(AGENTS)] for c in counts]).reshape(ROWS)


def _kinds(before, after):
    """{kind: bool [ROWS]} of the rows by whether they are active before and after the boundary."""
    b, a = before != 0, after != 0
    return {"stay": b & a, "join": ~b & a, "leave": b & ~a, "out": ~b & ~a}


def _collect(presteps, collects=1, noise=None):
    """A simulator stepped `presteps` times and a trainer on it after `collects` collect() calls (the carried state
    filled with seeded randn first, with `noise`); what every collect() stored, on the CPU."""
    import torch
    from gpu_hideseek import trainer
    s = _sim(presteps)
    tr = trainer.Trainer(s, _cfg(), net=_policy())
    if noise is not None:
        g = torch.Generator().manual_seed(noise)
        for x in (t for st in tr.state for t in st):
            x.copy_(torch.randn(x.shape, generator=g))
    stored, dicts = [], []
    for _ in range(collects):
        tr.collect()
        torch.cuda.synchronize()
        stored.append({k: v.cpu().clone() for k, v in tr.rollout.tensors().items()})
        dicts.append(tr.state_dict())
    return {"sim": s, "trainer": tr, "stored": stored, "state_dicts": dicts, "presteps": presteps}


@pytest.fixture(scope="module")
def mid():
    """The boundary in mid-chunk: slot 1."""
    c = _collect(EPISODE - 2)
    yield c
    c["sim"].close()


@pytest.fixture(scope="module")
def chunk_start():
    """The boundary on slot 4, the first slot of chunk 1."""
    c = _collect(EPISODE - 5)
    yield c
    c["sim"].close()


@pytest.fixture(scope="module")
def closing():
    """The closing step of the first collect() ends the episode: the boundary is slot 0 of the second."""
    c = _collect(EPISODE - 9, collects=2)
    yield c
    c["sim"].close()


def _boundary(buf):
    """The slot that holds the episode's first observation, from the prep_counter column alone; None without one."""
    import torch
    first = (buf["critic"][..., 0] == 1.0) & (buf["mask"] != 0)
    slots = torch.nonzero(first.any(dim=1)).reshape(-1).tolist()
    assert len(slots) <= 1, slots
    return slots[0] if slots else None


def _seq_to_slots(x):
    """[L, K * ROWS, ...] of all sequences in order (id = k ROWS + r) -> [T, ROWS, ...]."""
    return x.reshape(L, K, ROWS, *x.shape[2:]).transpose(0, 1).reshape(T, ROWS, *x.shape[2:])


_REFERENCES = {}


def _reference(c, i=0):
    """The episode loop over what collect() number i stored, from its stored states of chunk 0, once per fixture:
    {"f64" / "f32": {"log_prob", "value" [T, ROWS] float64, "states": what each forward received}, "allow": {...}}."""
    import torch
    key = (c["presteps"], i, id(c))
    if key in _REFERENCES:
        return _REFERENCES[key]
    buf = c["stored"][i]
    zero = zero_in(buf["mask"], buf["critic"])
    out = {}
    for name, ft in (("f64", torch.float64), ("f32", torch.float32)):
        net = _policy().set_fused(False).to(ft)
        state0 = ((buf["actor_h"][0].to(ft), buf["actor_c"][0].to(ft)), (buf["critic_h"][0].to(ft), buf["critic_c"][0].to(ft)))
        with torch.no_grad():
            lg, cl, received = episode_loop(net, buf["actor"].to(ft), buf["critic"].to(ft), zero, state0)
        out[name] = {"log_prob": _log_prob(lg, buf["action"], net.buckets).double(), "value": _decode(cl).double(),
                     "states": [dict(zip(STATES, (x.double() for s in st for x in s))) for st in received]}
    active = buf["mask"] != 0
    allow = {q: 4.0 * float((out["f32"][q] - out["f64"][q])[active].abs().max()) for q in ("log_prob", "value")}
    for k in STATES:
        allow[k] = 4.0 * float((out["f32"]["states"][L][k] - out["f64"]["states"][L][k])[active[L]].abs().max())
    assert all(v > 0 for k, v in allow.items() if k in ("log_prob", "value")), allow
    out["allow"], out["active"], out["zero"] = allow, active, zero
    _REFERENCES[key] = out
    return out


def _check_stored(c, i, boundary):
    """collect() number i of `c` against the loop: the exports' facts, the stored log-probabilities and values, the stored
    states of chunk 1, and the recomputation through the trainer's own forward of a minibatch, gathered both ways."""
    import torch
    tr, buf = c["trainer"], c["stored"][i]
    ref = _reference(c, i)
    active, allow, f64 = ref["active"], ref["allow"], ref["f64"]
    assert _boundary(buf) == boundary
    assert torch.equal(buf["clear"][1:], buf["done"][:-1])
    label = f"episodes: presteps {c['presteps']}, collect {i}"
    for q in ("log_prob", "value"):
        err = (buf[q].double() - f64[q]).abs() * active
        at = "" if boundary is None else f", {float(err[boundary].max()):.3e} at the boundary slot"
        print(f"{label}: stored {q}: {float(err.max()):.3e} from the float64 loop{at} (allowance {allow[q]:.3e}, "
              f"largest value {float(f64[q][active].abs().max()):.3e})")
    for q in ("log_prob", "value"):
        assert float(((buf[q].double() - f64[q]).abs() * active).max()) <= allow[q], q
    for k in STATES:
        err = float((buf[k][1].double() - f64["states"][L][k])[active[L]].abs().max())
        print(f"{label}: stored {k} of chunk 1: {err:.3e} from the float64 loop (allowance {allow[k]:.3e})")
        assert err <= allow[k], k
    if i != len(c["stored"]) - 1:
        return                     # the trainer's buffers hold a later collect()
    index = torch.arange(K * ROWS, dtype=torch.int32, device="cuda")
    for how, mb in (("minibatch_eager", tr.rollout.minibatch_eager(index)), ("minibatch", tr.rollout.minibatch(index))):
        with torch.no_grad():
            logits, critic_logits = tr.sequence_logits(mb)
        assert tuple(logits.shape) == (L, K * ROWS, 19) and tuple(critic_logits.shape) == (L, K * ROWS, 255)
        again = {"log_prob": _log_prob(_seq_to_slots(logits.double().cpu()), buf["action"], tr.net.buckets),
                 "value": _decode(_seq_to_slots(critic_logits.double().cpu()))}
        for q in ("log_prob", "value"):
            err = float(((again[q] - f64[q]).abs() * active).max())
            print(f"{label}: {q} recomputed from the chunk starts ({how}): {err:.3e} from the float64 loop (allowance {allow[q]:.3e})")
            assert err <= allow[q], (how, q)


def test_teams_change_with_the_episode(mid):
    """The set-up is what the oracle says of seed 1, and the exports around the boundary are what the rule relies on."""
    import torch
    buf = mid["stored"][0]
    assert _boundary(buf) == 1
    for e, t in ((0, 0), (1, 1), (1, T - 1)):
        assert buf["mask"][t].reshape(WORLDS, AGENTS).sum(1).tolist() == [float(a) for a in ACTIVE[e]], (e, t)
        assert torch.equal(buf["mask"][t], _prefix(ACTIVE[e])), (e, t)
    kinds = _kinds(buf["mask"][0], buf["mask"][1])
    assert {k: int(v.sum()) for k, v in kinds.items()} == KINDS and min(KINDS.values()) >= 2
    # with the episode's first observation: done = 1 on the rows that were in the episode that ended, 0 on those that join
    assert (buf["clear"][1][kinds["stay"]] == 1).all() and (buf["clear"][1][kinds["join"]] == 0).all() and (buf["clear"][0] == 0).all()
    assert (buf["critic"][1][..., 0][buf["mask"][1] != 0] == 1.0).all()
    # 50 steps later the rows that left still export done = 1 (and the others 0)
    s = _sim(EPISODE + 50)
    try:
        done = s.done_tensor().to_torch().reshape(ROWS).cpu()
        mask = s.self_mask_tensor().to_torch().reshape(ROWS).cpu()
        assert torch.equal(mask, buf["mask"][1])
        assert (done[kinds["leave"]] == 1).all() and (done[kinds["stay"] | kinds["join"]] == 0).all()
    finally:
        s.close()


def test_stored_quantities_with_the_boundary_in_mid_chunk(mid):
    _check_stored(mid, 0, boundary=1)


def test_the_boundary_at_a_chunk_start(chunk_start):
    _check_stored(chunk_start, 0, boundary=L)
    buf = chunk_start["stored"][0]
    active = buf["mask"][L] != 0
    assert int(active.sum()) == sum(ACTIVE[1])
    for k in STATES:
        assert not buf[k][1][active].any(), k


def test_the_boundary_at_the_closing_step(closing):
    import torch
    _check_stored(closing, 0, boundary=None)
    _check_stored(closing, 1, boundary=0)
    first, second = closing["stored"]
    assert (first["done"][T - 1][first["mask"][T - 1] != 0] == 1).all()
    kinds = _kinds(first["mask"][T - 1], second["mask"][0])
    assert {k: int(v.sum()) for k, v in kinds.items()} == KINDS
    active = second["mask"][0] != 0
    for k in STATES:
        assert not second[k][0][active].any(), k
    # the carried state the second collect() started from is the stored one, and the first's was not zero at its end
    carried = closing["state_dicts"][0]["state"]
    for k, x in zip(STATES, (t for s in carried for t in s)):
        assert torch.equal(x.cpu(), second[k][0]), k
    assert torch.equal(closing["state_dicts"][0]["clear"].cpu(), second["clear"][0])


def test_history_does_not_reach_the_new_episode(mid):
    """Two trainers of the same policy on two simulators of the same seed, the second with a carried state of noise: at
    the episode's first observation they see the same rows and, with no memory left, do the same."""
    import torch
    other = _collect(EPISODE - 2, noise=71)
    try:
        a, b = mid["stored"][0], other["stored"][0]
        allow = _reference(mid)["allow"]
        act0 = a["mask"][0] != 0
        assert torch.equal(a["actor"][0].view(torch.int32), b["actor"][0].view(torch.int32))
        assert (a["action"][0][act0] != b["action"][0][act0]).any()                  # the noise was felt: the two runs differ
        assert (a["value"][0][act0] != b["value"][0][act0]).any()
        act = a["mask"][1] != 0
        assert torch.equal(a["mask"][1], b["mask"][1]) and int(act.sum()) == sum(ACTIVE[1])
        for k in ("actor", "critic"):
            assert torch.equal(a[k][1][act].view(torch.int32), b[k][1][act].view(torch.int32)), k
        for q in ("value", "log_prob"):
            d = float((a[q][1] - b[q][1])[act].abs().max())
            print(f"episodes: two histories, {q} at the boundary slot: they differ by {d:.3e} (allowance {allow[q]:.3e})")
        for q in ("value", "log_prob"):
            assert float((a[q][1] - b[q][1])[act].abs().max()) <= allow[q], q
        assert torch.equal(a["action"][1][act], b["action"][1][act])
    finally:
        other["sim"].close()


def _half():
    """A fixed half of the 96 sequences."""
    import torch
    return torch.randperm(K * ROWS, generator=torch.Generator().manual_seed(41)).to(torch.int32)[:K * ROWS // 2]


def test_gradient_of_one_minibatch(mid):
    """test_gpu_trainer's gradient test with rows of every kind: the fused and the eager trainer's flat gradients of one
    minibatch, under the fused one's upstream gradients, against each other and against the episode loop's."""
    import torch
    from gpu_hideseek import trainer
    sim, tr, buf = mid["sim"], mid["trainer"], mid["stored"][0]
    eager = trainer.Trainer(sim, _cfg(), net=_policy(), fused=False)
    assert torch.equal(eager.opt.flat.params, tr.opt.flat.params) and not eager.net.actor.fused and tr.net.actor.fused
    for k, t in tr.rollout.tensors().items():
        getattr(eager.rollout, k).copy_(t)
    eager.adv_moments.copy_(tr.adv_moments)
    index = _half()
    chunk, row = torch.div(index.long(), ROWS, rounding_mode="floor"), index.long() % ROWS
    kinds = _kinds(buf["mask"][0], buf["mask"][1])
    assert set(chunk.tolist()) == {0, 1}
    for k, v in kinds.items():
        assert v[row[chunk == 0]].any(), k                    # chunk 0 holds the boundary
    index = index.cuda()
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
    mb = {k: v.cpu() for k, v in tr.rollout.minibatch_eager(index).items()}
    zero = zero_in(mb["mask"], mb["critic"])
    ref = {}
    for name, ft in (("f32", torch.float32), ("f64", torch.float64)):
        net = _policy().set_fused(False).to(ft)
        st = ((mb["actor_h"].to(ft), mb["actor_c"].to(ft)), (mb["critic_h"].to(ft), mb["critic_c"].to(ft)))
        lg, cl, _ = episode_loop(net, mb["actor"].to(ft), mb["critic"].to(ft), zero, st)
        torch.autograd.backward([lg.reshape(up[0].shape), cl.reshape(up[1].shape)], [up[0].cpu().to(ft), up[1].cpu().to(ft)])
        ref[name] = {k: p.grad.double() for k, p in net.named_parameters()}
    layout = tr.opt.layout()
    assert set(layout) == set(ref["f64"]) and len(layout) == 24
    worst = []
    for k, (lo, hi, shape) in layout.items():
        allow = 4.0 * float((ref["f32"][k] - ref["f64"][k]).abs().max())
        gf, ge = grads["fused"][lo:hi].view(shape).double().cpu(), grads["eager"][lo:hi].view(shape).double().cpu()
        diff, ef, ee = float((gf - ge).abs().max()), float((gf - ref["f64"][k]).abs().max()), float((ge - ref["f64"][k]).abs().max())
        print(f"episodes: grad {k}: fused - eager {diff:.3e}; from the float64 loop: fused {ef:.3e}, eager {ee:.3e} (allowance {allow:.3e}, "
              f"largest value {float(ref['f64'][k].abs().max()):.3e})")
        assert float(ref["f64"][k].abs().max()) > 0, k
        worst.append((k, diff, ef, ee, allow))
    for k, diff, ef, ee, allow in worst:
        assert diff <= allow and ef <= allow and ee <= allow, (k, diff, ef, ee, allow)


def test_masks_reach_every_count(mid):
    import torch
    from gpu_hideseek import ppo_loss, value_head
    tr, buf = mid["trainer"], mid["stored"][0]
    mask = buf["mask"]
    active = mask != 0
    assert 0 < int(active.sum()) < T * ROWS
    assert buf["moments"][:, -1].tolist() == mask.sum(1).double().tolist()
    assert tr.adv_moments[4].item() == float(mask.sum())
    for q in ("advantage", "returns"):
        assert not buf[q][~active].view(torch.int32).any(), q             # +0 bit for bit where the row is out
        assert torch.isfinite(buf[q]).all(), q
    assert buf["advantage"][active].abs().max() > 0
    # the rows that left keep the reward of their last step in the export: the mask keeps it out of everything above
    left = _kinds(mask[0], mask[1])["leave"]
    assert (buf["reward"][1:, left] != 0).all() and (buf["done"][1:, left] == 1).all()
    # the first minibatch of an update, before any optimiser step
    assert int(tr.opt.adam_state[2].item()) == 0
    index = _half().cuda()
    pol, val = tr.forward_backward(index)
    tr.opt.zero_grad()
    count = float(tr.rollout.minibatch_eager(index)["mask"].sum())
    p, v = ppo_loss.stats_to_metrics(pol["stats"]), value_head.stats_to_metrics(val["stats"])
    assert 0 < count < L * index.shape[0] and float(p["count"]) == count and float(v["count"]) == count
    ref = _reference(mid)
    gap = float((ref["f32"]["log_prob"] - ref["f64"]["log_prob"])[ref["active"]].abs().max())
    print(f"episodes: first minibatch: count {count:.0f}, clip_fraction {float(p['clip_fraction']):.3e}, approx_kl {float(p['approx_kl']):.3e} "
          f"(allowance {4.0 * gap:.3e})")
    assert float(p["clip_fraction"]) == 0.0
    assert abs(float(p["approx_kl"])) <= 4.0 * gap


def test_checkpoint_across_the_boundary(closing):
    """A fresh trainer on a second simulator driven to where the first collect() left the first one takes the state_dict
    of that moment: its next collect() is the first trainer's second one."""
    import torch
    from gpu_hideseek import trainer
    first, second = closing["stored"]
    s2 = _sim(closing["presteps"])
    try:
        action = s2.action_tensor().to_torch()
        for t in range(T):                       # o_0 .. o_{T-1}: the loaded trainer takes the step that leads to o_T itself
            s2.step()
            action.copy_(first["action"][t].view(action.shape))
        fresh = trainer.Trainer(s2, _cfg(), net=_policy())
        fresh.load_state_dict(closing["state_dicts"][0])
        fresh.collect()
        got = {k: v.cpu() for k, v in fresh.rollout.tensors().items()}
        assert torch.equal(got["mask"], second["mask"]) and torch.equal(got["clear"], second["clear"])
        assert torch.equal(got["actor"].view(torch.int32), second["actor"].view(torch.int32))
        active = second["mask"] != 0
        allow = _reference(closing, 1)["allow"]["value"]
        err = float((got["value"] - second["value"])[active].abs().max())
        print(f"episodes: checkpoint: value of the loaded trainer's collect() {err:.3e} from the first trainer's (allowance {allow:.3e})")
        assert err <= allow
        for k in STATES:
            assert not got[k][0][second["mask"][0] != 0].any(), k
    finally:
        s2.close()
