"""The PPO loss on the GPU (sim.ppo_loss, hs_ppo_loss, csrc/hs_k_ppo.h) against the numpy restatement of
tests/test_ppo_loss_host.py within the tolerances derived there: sizes around the block of samples and past the grid
cap, dtypes, bucket sets, mask and value modes, strided logits; the bits shared with sample_actions(mode="evaluate");
crafted clipping; -inf buckets and NaN in inactive samples; the count, grad_scale and adv_moments; determinism, position
independence and the outputs that were not asked for; the autograd face; a rollout of the simulator itself; the stream
form, the shards and the refusals of the C ABI."""
import ctypes as C
import math

import numpy as np
import pytest

import test_ppo_loss_host as H
from test_ppo_loss_host import BIG, BUCKETS, CLIP, DTYPES, ENTROPY_COEF, ROUNDING, SIZES, VALUE_COEF, VALUE_MODES, f32, ppo

pytestmark = pytest.mark.gpu

STRIDED = 40


def _sim(worlds=6, agents=6, seed=0, flags=0):
    import gpu_hideseek
    k = agents // 2
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=flags, rand_seed=seed,
        min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=1)


@pytest.fixture(scope="module")
def sim():
    """One initialised handle of 6 x 6 rows: n is not tied to it."""
    s = _sim()
    s.init()
    yield s
    s.close()


def _dev(x, dtype="float32", strided=False):
    """The inputs of H.inputs on the device; logits and value in `dtype` (they are representable in it)."""
    import torch
    dt = getattr(torch, dtype)
    d = {}
    for k in ("action", "old_log_prob", "advantage", "mask", "returns", "old_value", "adv_moments"):
        d[k] = None if x[k] is None else torch.from_numpy(np.array(x[k])).cuda()
    lg = torch.from_numpy(np.array(x["logits"])).cuda().to(dt)
    if strided:
        wide = torch.full((lg.shape[0], STRIDED), float("nan"), dtype=dt, device="cuda")
        wide[:, :lg.shape[1]] = lg
        lg = wide[:, :lg.shape[1]]
    d["logits"] = lg
    d["value"] = None if x["value"] is None else torch.from_numpy(np.array(x["value"])).cuda().to(dt)
    d["buckets"] = x["buckets"]
    return d


def _call(sim, d, **kw):
    a = dict(d, **kw)
    return sim.ppo_loss(a.pop("logits"), a.pop("action"), a.pop("old_log_prob"), a.pop("advantage"), **a)


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype.is_floating_point and t.element_size() < 8 else t.detach().cpu().numpy()


def _bits(t):
    import torch
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _close(got, want32, tol, dtype, tag):
    """|got - want| <= tol + what rounding a value to `dtype` adds (half an ulp of it, relative, and half the
    subnormal spacing)."""
    rel, absolute = ROUNDING[dtype]
    err = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    bound = tol + rel * np.abs(want32.astype(np.float64)) + absolute
    assert np.isfinite(got).all(), tag
    assert (err <= bound).all(), (tag, float((err - bound).max()), float(err.max()), tol)


def _check(out, x, r32, r64, dtype, tag):
    """Parity with the f32 restatement within the derived tolerances, leaving out the near-edge samples (at most
    NEAR_EDGE_CAP of the case); exact zeros where the contract says so; the statistics."""
    tol = H.tolerances(x["logits"].shape[0])              # the gradient tolerances of the case's own size
    ne = H.near_edge(r64, tol)
    assert ne.sum() <= H.NEAR_EDGE_CAP * ne.size, (tag, int(ne.sum()))
    ok, on = ~ne, r32["active"]
    L = x["logits"].shape[1]
    if "grad_logits" in out:
        g = _np(out["grad_logits"])[:, :L]
        _close(g[ok], r32["grad_logits"][ok], tol["grad_logits"], dtype, (tag, "grad_logits"))
        raw = _bits(out["grad_logits"][:, :L]).cpu().numpy()
        assert not raw[~on].any(), (tag, "inactive samples get +0")
        assert not raw[np.isneginf(x["logits"])].any(), (tag, "-inf buckets get +0")
    if "grad_value" in out:
        gv = _np(out["grad_value"]).reshape(-1)
        _close(gv[ok], r32["grad_value"][ok], tol["grad_value"], dtype, (tag, "grad_value"))
        assert not _bits(out["grad_value"]).cpu().numpy().reshape(-1)[~on].any(), tag
    if "stats" in out:
        s, want = out["stats"].cpu().numpy(), r32["stats"]
        assert s.dtype == np.float64 and s.shape == (7,)
        assert s[6] == want[6] == r32["cnt"], (tag, "cnt is exact")
        cnt = max(r32["cnt"], 1)
        for k in range(4):
            dev = abs(s[k] - want[k]) / cnt
            assert dev <= tol["stats"], (tag, "stats", k, dev, tol["stats"])
        slack = int((ne & on).sum())                      # a near-edge sample may fall on either side
        assert abs(s[4] - want[4]) <= slack and abs(s[5] - want[5]) <= slack, (tag, s[4:6], want[4:6], slack)


@pytest.mark.parametrize("vmode", VALUE_MODES)
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_with_the_restatement(sim, dtype, masked, vmode):
    for buckets in BUCKETS:
        for n in SIZES:
            case = (n, buckets, dtype, masked, vmode)
            x = H.inputs(*case)
            r32, r64 = H.both(case)
            for strided in (False, True) if n in (SIZES[3], SIZES[4]) else (False,):
                out = _call(sim, _dev(x, dtype, strided))
                assert out["grad_logits"].dtype == getattr(__import__("torch"), dtype)
                assert set(out) == {"grad_logits", "stats", "coefficients"} | ({"grad_value"} if vmode != "none" else set())
                _check(out, x, r32, r64, dtype, (case, strided))


def test_natural_draws(sim):
    """The case whose draws are left as drawn (H.NATURAL): the near-edge exclusion at work at 1 806 samples."""
    x, r32, r64 = H.natural_both()
    _check(_call(sim, _dev(x)), x, r32, r64, "float32", "natural")


def test_past_the_grid_cap(sim):
    from gpu_hideseek import ppo_loss as P
    assert BIG == P.MAX_GRID * P.ROWS_PER_BLOCK + P.ROWS_PER_BLOCK + 1
    case = H.CASES[-1]
    assert case[0] == BIG
    x = H.inputs(*case)
    r32, r64 = H.both(case)
    _check(_call(sim, _dev(x, case[2])), x, r32, r64, case[2], case)


def test_shares_its_bits_with_evaluate(sim):
    big = _sim(301, 6)                                      # sample_actions works over the handle's rows: 36 and 1 806
    big.init()
    try:
        for s, n in ((sim, 36), (big, 1806)):
            _shares_its_bits_with_evaluate(s, n)
    finally:
        big.close()


def _shares_its_bits_with_evaluate(sim, n):
    for dtype, buckets in (("float32", BUCKETS[0]), ("bfloat16", BUCKETS[1])):
        x = H.inputs(n, buckets, dtype, True, "none", seed=21)
        d = _dev(x, dtype)
        ev = sim.sample_actions(d["logits"], buckets=buckets, mode="evaluate", action=d["action"], log_prob=True, entropy=True)
        on = x["mask"] != 0
        out = _call(sim, d, old_log_prob=ev["log_prob"], entropy_coef=0.0)
        s = out["stats"].cpu().numpy()
        ent = ev["entropy"].cpu().numpy().astype(np.float64)[on]
        assert abs(s[2] - math.fsum(ent)) <= n * 2.0 ** -53 * np.abs(ent).sum()
        assert s[3] == 0.0 and s[4] == 0.0, "ratio is exactly 1: kl is 0 and nothing is clipped"
        assert s[0] == -math.fsum(x["advantage"].astype(np.float64)[on]) or abs(s[0] + math.fsum(x["advantage"].astype(np.float64)[on])) <= n * 2.0 ** -53 * np.abs(x["advantage"][on]).sum()
        # grad_logits = -w A (onehot - p)
        want = np.zeros(x["logits"].shape, np.float64)
        off = np.concatenate([[0], np.cumsum(buckets)])
        w = 1.0 / on.sum()
        for h, l in enumerate(H.heads_of(x["logits"], buckets)):
            _, S, _, _, e = H.head_tables(l, np.float64)
            onehot = np.arange(buckets[h])[None, :] == x["action"][:, h:h + 1]
            want[:, off[h]:off[h + 1]] = -w * x["advantage"].astype(np.float64)[:, None] * (onehot - e / S[:, None]) * on[:, None]
        _close(_np(out["grad_logits"]), want.astype(np.float32), H.tolerances(n)["grad_logits"], dtype, ("evaluate", n, dtype))


def test_crafted_clipping(sim):
    n, buckets = 1806, BUCKETS[0]
    x = H.inputs(n, buckets, "float32", True, "clipped")
    lp = ppo(np.float32, x)["lp"]
    A = x["advantage"]
    assert (A != 0).all()
    on = x["mask"] != 0
    # the ratio far outside the clip range on the side the minimum takes the clipped term: no policy gradient
    x1 = dict(x, old_log_prob=np.where(A > 0, lp - 1, lp + 1).astype(np.float32))
    out = _call(sim, _dev(x1), entropy_coef=0.0)
    assert not _bits(out["grad_logits"]).any().item()
    assert out["stats"][4].item() == on.sum() == out["stats"][6].item()
    # mirrored: the unclipped term is the minimum
    x2 = dict(x, old_log_prob=np.where(A > 0, lp + 1, lp - 1).astype(np.float32))
    out = _call(sim, _dev(x2), entropy_coef=0.0)
    assert out["stats"][4].item() == 0
    g = _np(out["grad_logits"])
    assert (np.abs(g[on]).max(1) > 0).all()
    _check(out, x2, ppo(np.float32, x2, entropy_coef=0.0), ppo(np.float64, x2, entropy_coef=0.0), "float32", "mirrored")
    # v - vo = +-2c with R on the side that makes the clipped term the larger: no value gradient
    c = f32(CLIP)
    sign = np.where(np.arange(n) % 2 == 0, f32(1), f32(-1))
    vo = x["old_value"]
    v = (vo + sign * (c + c)).astype(np.float32)
    x3 = dict(x, value=v, returns=(v + sign * f32(3)).astype(np.float32))
    out = _call(sim, _dev(x3))
    assert not _bits(out["grad_value"]).any().item()
    assert out["stats"][5].item() == on.sum()
    x4 = dict(x, value=v, returns=(v - sign * f32(3)).astype(np.float32))          # the other side: the plain term is larger
    out = _call(sim, _dev(x4))
    assert out["stats"][5].item() == 0 and (np.abs(_np(out["grad_value"]))[on] > 0).all()


def test_masked_buckets_and_nan_in_inactive_samples(sim):
    import torch
    n, buckets = 1806, BUCKETS[1]
    for dtype in ("float32", "float16"):
        x = H.inputs(n, buckets, dtype, True, "clipped")
        assert np.isneginf(x["logits"]).any(1).sum() > 800
        d = _dev(x, dtype)
        clean = _call(sim, d)
        for k in ("grad_logits", "grad_value", "stats"):
            assert not torch.isnan(clean[k]).any().item(), k
        assert not _bits(clean["grad_logits"]).cpu().numpy()[np.isneginf(x["logits"])].any()
        off = torch.from_numpy(x["mask"] == 0).cuda()
        e = dict(d)
        for k in ("logits", "advantage", "value", "old_log_prob", "returns", "old_value"):
            e[k] = d[k].clone()
            e[k][off] = float("nan")
        dirty = _call(sim, e)
        for k in ("grad_logits", "grad_value", "stats"):
            assert torch.equal(_bits(dirty[k]), _bits(clean[k])), (dtype, k)
        assert not _bits(dirty["grad_logits"])[off].any().item() and not _bits(dirty["grad_value"])[off].any().item()


def test_count_scale_and_moments(sim):
    import torch
    n, buckets = 1806, BUCKETS[0]
    x = H.inputs(n, buckets, "bfloat16", True, "clipped")
    d = _dev(x, "bfloat16")
    none = _call(sim, d, mask=torch.zeros(n, device="cuda"), grad_dtype=torch.float32)
    for k in ("grad_logits", "grad_value", "stats"):
        assert not _bits(none[k]).any().item(), k
    one = _call(sim, d, grad_dtype=torch.float32)
    two = _call(sim, d, grad_dtype=torch.float32, grad_scale=2.0)
    assert torch.equal(_bits(two["grad_logits"]), _bits(2 * one["grad_logits"]))
    assert torch.equal(_bits(two["grad_value"].float()), _bits(2 * one["grad_value"].float()))
    assert torch.equal(_bits(two["stats"]), _bits(one["stats"]))
    # the normaliser from the moments of a real compute_advantages call
    T, rows = 7, 36
    g = torch.Generator(device="cuda").manual_seed(5)
    rew = torch.randn(T, rows, device="cuda", generator=g)
    done = (torch.rand(T, rows, device="cuda", generator=g) < 0.1).to(torch.int32)
    val = torch.randn(T, rows, device="cuda", generator=g)
    msk = (torch.rand(T, rows, device="cuda", generator=g) < 0.8).float()
    gae = sim.compute_advantages(rew, done, val, val[0].clone(), mask=msk, moments=True)
    m = T * rows
    y = H.inputs(m, buckets, "float32", False, "value", seed=22)
    e = _dev(y)
    adv = gae["advantages"].reshape(m)
    M = gae["moments"].cpu().numpy()
    mu = M[0] / M[4]
    mean, std = f32(mu), f32(np.sqrt(max(M[1] / M[4] - mu * mu, 0.0)))
    pre = torch.from_numpy(((adv.cpu().numpy() - mean) / (std + f32(1e-8))).astype(np.float32)).cuda()
    a = _call(sim, e, advantage=adv, adv_moments=gae["moments"], mask=msk.reshape(m))
    b = _call(sim, e, advantage=pre, mask=msk.reshape(m))
    for k in ("grad_logits", "grad_value", "stats"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert a["stats"][6].item() == M[4]


def test_determinism_position_and_unrequested_outputs(sim):
    import torch
    n, buckets = 1806, BUCKETS[1]
    L = sum(buckets)
    x = H.inputs(n, buckets, "float16", True, "clipped")
    d = _dev(x, "float16")
    first, again = _call(sim, d), _call(sim, d)
    for k in ("grad_logits", "grad_value", "stats"):
        assert torch.equal(_bits(first[k]), _bits(again[k])), k
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
    p = {k: (v[perm].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    moved = _call(sim, p)
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n, device="cuda")
    for k in ("grad_logits", "grad_value"):
        assert torch.equal(_bits(moved[k][inv]), _bits(first[k])), k
    assert moved["stats"][4:].tolist() == first["stats"][4:].tolist()
    # only what is requested is written, and of a strided grad_logits only columns 0 .. L-1
    wide = torch.full((n + 2, STRIDED), -7.0, dtype=torch.float16, device="cuda")
    gv = torch.full((n + 2,), -7.0, dtype=torch.float16, device="cuda")
    st = torch.full((9,), -7.0, dtype=torch.float64, device="cuda")
    out = _call(sim, d, grad_logits=wide[1:n + 1, :L], grad_value=False, stats=None)
    assert set(out) == {"grad_logits", "coefficients"} and bool((gv == -7).all()) and bool((st == -7).all())
    assert torch.equal(_bits(wide[1:n + 1, :L]), _bits(first["grad_logits"]))
    assert bool((wide[1:n + 1, L:] == -7).all()) and bool((wide[[0, n + 1]] == -7).all())
    wide.fill_(-7)
    out = _call(sim, d, grad_logits=None, grad_value=gv[1:n + 1], stats=None)
    assert set(out) == {"grad_value", "coefficients"} and bool((wide == -7).all()) and bool((gv[[0, n + 1]] == -7).all())
    assert torch.equal(_bits(gv[1:n + 1]), _bits(first["grad_value"]))
    gv.fill_(-7)
    out = _call(sim, d, grad_logits=None, grad_value=False, stats=st[1:8])
    assert set(out) == {"stats", "coefficients"} and bool((wide == -7).all()) and bool((gv == -7).all())
    assert torch.equal(_bits(st[1:8]), _bits(first["stats"])) and st[0].item() == -7 and st[8].item() == -7


def test_the_autograd_face(sim):
    import torch
    from gpu_hideseek import ppo_loss as P
    n, buckets = 1806, BUCKETS[0]
    x = H.inputs(n, buckets, "float32", True, "none")         # its actions, advantages and mask; the rest follows the network
    d = _dev(x)
    torch.manual_seed(0)
    feat = torch.randn(n, 16, device="cuda")
    actor, critic = torch.nn.Linear(16, 19).cuda(), torch.nn.Linear(16, 1).cuda()
    params = list(actor.parameters()) + list(critic.parameters())
    off = np.concatenate([[0], np.cumsum(buckets)])

    def forward():
        for q in params:
            q.grad = None
        return actor(feat), critic(feat)

    def log_prob_entropy(logits):
        lp, ent = 0.0, 0.0
        for h in range(5):
            logp = torch.log_softmax(logits[:, off[h]:off[h + 1]], dim=1)
            lp = lp + logp.gather(1, d["action"][:, h:h + 1].long())[:, 0]
            ent = ent - (logp.exp() * logp).sum(1)
        return lp, ent

    def away_from_edges(base, sigma, edge_of):
        """base + sigma N(0,1), drawn again where edge_of(result) is within EDGE_MARGIN of a clipping edge (as H.inputs does)."""
        t = base + sigma * torch.randn_like(base)
        for _ in range(50):
            near = edge_of(t.double()) <= H.EDGE_MARGIN
            if not near.any():
                return t
            t = torch.where(near, base + sigma * torch.randn_like(base), t)
        raise AssertionError("a sample stayed near an edge")

    with torch.no_grad():
        logits, value = forward()
        lp0, v0 = log_prob_entropy(logits)[0], value[:, 0]
        d["old_log_prob"] = away_from_edges(lp0, 0.15, lambda t: torch.minimum((torch.exp(lp0.double() - t) - (1 - CLIP)).abs(),
                                                                                 (torch.exp(lp0.double() - t) - (1 + CLIP)).abs()))
        d["old_value"] = away_from_edges(v0, 0.3, lambda t: ((v0.double() - t).abs() - CLIP).abs())
        d["returns"] = v0 + torch.randn_like(v0)

    logits, value = forward()
    out = sim.ppo_loss(logits.detach(), d["action"], d["old_log_prob"], d["advantage"], mask=d["mask"], value=value.detach(),
                       returns=d["returns"], old_value=d["old_value"], clip_coef=CLIP, value_loss_coef=VALUE_COEF, entropy_coef=ENTROPY_COEF)
    loss = P.attach(logits, value, out)
    assert loss.dtype == torch.float64 and loss.shape == ()
    want = P.stats_to_metrics(out["stats"], entropy_coef=float(f32(ENTROPY_COEF)), value_loss_coef=float(f32(VALUE_COEF)))["loss"]
    assert loss.item() == want.item()
    loss.backward()
    fused = [q.grad.clone() for q in params]

    logits, value = forward()
    torch.autograd.backward([logits, value], [out["grad_logits"], out["grad_value"].view_as(value)])
    for a, b in zip(fused, params):
        assert torch.equal(a, b.grad)                       # the path with no extra op hands on the same gradients

    logits, value = forward()
    lp, ent = log_prob_entropy(logits)
    ratio = torch.exp(lp - d["old_log_prob"])
    pg = -torch.minimum(ratio * d["advantage"], torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * d["advantage"])
    v = value[:, 0]
    vl = 0.5 * torch.maximum((v - d["returns"]) ** 2, ((d["old_value"] + torch.clamp(v - d["old_value"], -CLIP, CLIP)) - d["returns"]) ** 2)
    m = d["mask"]
    eager = ((pg - ENTROPY_COEF * ent + VALUE_COEF * vl) * m).sum() / m.sum()
    eager.backward()
    # each of the three means is within the statistics tolerance of the exact one on both sides: 2 x (1 + 0.01 + 0.5) < 4
    assert abs(eager.item() - loss.item()) <= 4 * H.tolerances()["stats"]
    # A parameter gradient is a sum over the n rows of the matmul of (output gradient x feature).  Every output gradient
    # is within the gradient tolerance of this size (H.tolerances(1806): w = 1 / cnt is that of the 1 806-sample cases,
    # whose logits are the harsher ones) of the exact one, on both sides; so two weight gradients differ by at most
    # 2 x tolerance x sum_i |feature_ij| and two bias gradients by 2 x tolerance x n.  That is below the issue's bound
    # (the overall grad_logits tolerance x n) by three orders of magnitude, and it must be far below the gradients
    # themselves, or it would test nothing.  No sample is near an edge (the draws above), so no branch may differ.
    tol = H.tolerances(n)
    assert tol["grad_logits"] <= H.tolerances()["grad_logits"] and tol["grad_value"] <= H.tolerances()["grad_value"]
    colsum = float(feat.abs().sum(0).max())
    bounds = (2 * tol["grad_logits"] * colsum, 2 * tol["grad_logits"] * n, 2 * tol["grad_value"] * colsum, 2 * tol["grad_value"] * n)
    for a, b, bound in zip(fused, params, bounds):
        err, size = float((a - b.grad).abs().max()), float(b.grad.abs().max())
        print(f"parameter {tuple(a.shape)}: |fused - eager| = {err:.3e} (bound {bound:.3e}, largest gradient {size:.3e})")
        assert bound <= H.tolerances()["grad_logits"] * n and 50 * bound < size, (bound, size)
        assert err <= bound


def test_a_rollout_of_the_simulator_itself():
    import torch
    worlds, agents, T, buckets = 6, 6, 7, BUCKETS[0]
    s = _sim(worlds, agents, seed=3)
    s.init()
    rows = worlds * agents
    g = torch.Generator(device="cuda").manual_seed(1)
    W = torch.randn(296, 19, device="cuda", generator=g) * 0.05
    Wv = torch.randn(296, device="cuda", generator=g) * 0.05
    obs = torch.empty(T, rows, 296, device="cuda")
    act = torch.empty(T, rows, 5, dtype=torch.int32, device="cuda")
    lp = torch.empty(T, rows, device="cuda")
    rew, val, msk = torch.empty(T, rows, device="cuda"), torch.empty(T, rows, device="cuda"), torch.empty(T, rows, device="cuda")
    done = torch.empty(T, rows, dtype=torch.int32, device="cuda")
    for t in range(T):
        s.pack_policy_inputs(actor=obs[t])
        msk[t].copy_(s.self_mask_tensor().to_torch().reshape(rows))
        val[t] = obs[t] @ Wv
        s.sample_actions(obs[t] @ W, buckets=buckets, seed=(9, 0), counter=t, log_prob=lp[t])
        act[t].copy_(s.action_tensor().to_torch())
        s.step()
        rew[t].copy_(s.reward_tensor().to_torch().reshape(rows))
        done[t].copy_(s.done_tensor().to_torch().reshape(rows))
    boot = torch.zeros(rows, device="cuda")
    gae = s.compute_advantages(rew, done, val, boot, mask=msk, moments=True)
    n = T * rows
    W2, Wv2 = W + 0.01 * torch.randn(296, 19, device="cuda", generator=g), Wv + 0.01 * torch.randn(296, device="cuda", generator=g)
    flat = obs.reshape(n, 296)
    logits, value = (flat @ W2).contiguous(), (flat @ Wv2).contiguous()
    args = dict(adv_moments=gae["moments"], mask=msk.reshape(n), value=value, returns=gae["returns"].reshape(n), old_value=val.reshape(n))
    out = s.ppo_loss(logits, act.reshape(n, 5), lp.reshape(n), gae["advantages"].reshape(n), **args)
    x = dict(logits=logits.cpu().numpy(), buckets=buckets, action=act.reshape(n, 5).cpu().numpy(), old_log_prob=lp.reshape(n).cpu().numpy(),
             advantage=gae["advantages"].reshape(n).cpu().numpy(), adv_moments=gae["moments"].cpu().numpy(),
             mask=msk.reshape(n).cpu().numpy(), value=value.cpu().numpy(), returns=gae["returns"].reshape(n).cpu().numpy(),
             old_value=val.reshape(n).cpu().numpy())
    assert 0 < (x["mask"] != 0).sum()
    r32, r64 = ppo(np.float32, x), ppo(np.float64, x)
    assert not H.near_edge(r64, H.tolerances()).any(), "252 samples: the cap admits none near an edge"
    _check(out, x, r32, r64, "float32", "simulator")
    s.close()


def test_the_stream_form_and_the_shards(sim):
    import gpu_hideseek
    import torch
    n, buckets = 1806, BUCKETS[0]
    x = H.inputs(n, buckets, "bfloat16", True, "clipped")
    d = _dev(x, "bfloat16")
    blocking = _call(sim, d)
    side = torch.cuda.Stream()
    ev = torch.cuda.Event()
    ev.record()
    side.wait_event(ev)
    got = _call(sim, d, stream=side)
    raw = _call(sim, d, stream=side.cuda_stream)
    side.synchronize()
    for k in ("grad_logits", "grad_value", "stats"):
        assert torch.equal(_bits(got[k]), _bits(blocking[k])) and torch.equal(_bits(raw[k]), _bits(blocking[k])), k
    kw = dict(sim_flags=0, rand_seed=0, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0], 6, **kw)
    ss.init()
    cut = 1000
    halves = [{k: (v[:cut] if isinstance(v, torch.Tensor) else v) for k, v in d.items()},
              {k: (v[cut:] if isinstance(v, torch.Tensor) else v) for k, v in d.items()}]
    singles = [_call(sim, h) for h in halves]
    res = ss.ppo_loss(*[[h[k] for h in halves] for k in ("logits", "action", "old_log_prob", "advantage")], buckets=buckets,
                      **{k: [h[k] for h in halves] for k in ("mask", "value", "returns", "old_value")})
    assert len(res) == 2
    for r, one in zip(res, singles):
        for k in ("grad_logits", "grad_value", "stats"):
            assert torch.equal(_bits(r[k]), _bits(one[k])), k
    ss.close()


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import ppo_loss as P
    from lockstep import EXT_SKIP_OBSERVATIONS
    INVALID = 1
    n, buckets, L = 48, BUCKETS[0], 19
    x = H.inputs(n, buckets, "float32", True, "clipped", seed=23)
    pad = 8

    def buf(a, dtype=None):
        t = torch.zeros(a.size + pad, dtype=dtype or torch.from_numpy(np.array(a)).dtype, device="cuda")
        t[:a.size] = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1).to(t.dtype)
        return t
    lg, ac, olp, adv, msk = buf(x["logits"]), buf(x["action"]), buf(x["old_log_prob"]), buf(x["advantage"]), buf(x["mask"])
    val, ret, vo = buf(x["value"]), buf(x["returns"]), buf(x["old_value"])
    mom = torch.tensor([0.0, float(n), 0.0, 0.0, float(n), 0.0], dtype=torch.float64, device="cuda")
    lgh = torch.zeros(n * L + pad, dtype=torch.bfloat16, device="cuda")
    valh = torch.zeros(n + pad, dtype=torch.bfloat16, device="cuda")
    gl = torch.full((n * L + pad,), -7.0, device="cuda")
    gv = torch.full((n + pad,), -7.0, device="cuda")
    st = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    ins = (lg, ac, olp, adv, msk, val, ret, vo, mom)
    saved = [t.clone() for t in ins]

    def req(logits=lg.data_ptr(), action=ac.data_ptr(), old_log_prob=olp.data_ptr(), advantage=adv.data_ptr(), adv_moments=mom.data_ptr(),
            mask=msk.data_ptr(), value=val.data_ptr(), returns=ret.data_ptr(), old_value=vo.data_ptr(), n=n, ldt=1, lstride=L, gdt=1,
            gstride=L, vdt=1, buckets=buckets, clip=CLIP, vcoef=VALUE_COEF, ecoef=ENTROPY_COEF, scale=1.0, grad_logits=gl.data_ptr(),
            grad_value=gv.data_ptr(), stats=st.data_ptr()):
        return P.HsPpoRequest(logits, action, old_log_prob, advantage, adv_moments, mask, value, returns, old_value, n, ldt, lstride,
                              gdt, gstride, vdt, (C.c_int32 * 5)(*buckets), clip, vcoef, ecoef, scale, grad_logits, grad_value, stats)

    def untouched():
        torch.cuda.synchronize()
        same = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ins, saved))
        return same and all(bool((t == -7).all()) for t in (gl, gv, st))

    def call(s, r, stream=False):
        p = C.byref(r) if r is not None else None
        if stream:
            return s._L.hs_ppo_loss_async(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p)
        return s._L.hs_ppo_loss(s._h, p)

    def message(s):
        return s._L.hs_last_error().decode()

    s = _sim(4, 4)
    for stream in (False, True):
        assert call(s, req(), stream) == INVALID and "before hs_init" in message(s)
    assert untouched()
    s.init()
    nan, inf = float("nan"), float("inf")
    bad = {
        "null request": (None, "null request"), "null logits": (req(logits=None), "null logits"), "null action": (req(action=None), "null action"),
        "null old_log_prob": (req(old_log_prob=None), "null old_log_prob"), "null advantage": (req(advantage=None), "null advantage"),
        "no output": (req(grad_logits=None, grad_value=None, stats=None), "every output is null"),
        "grad_value without value": (req(value=None, returns=None, old_value=None), "grad_value without value"),
        "value without returns": (req(returns=None), "value without returns"),
        "logits dtype": (req(ldt=0), "dtype"), "grad dtype": (req(gdt=2), "dtype"), "value dtype": (req(vdt=7), "dtype"),
        "bucket 0": (req(buckets=(5, 5, 5, 2, 0)), "bucket"), "bucket 17": (req(buckets=(17, 5, 5, 2, 2), lstride=40, gstride=40), "bucket"),
        "too many logits": (req(buckets=(16,) * 5, lstride=80, gstride=80), "HS_SAMPLE_MAX_LOGITS"),
        "logits stride": (req(lstride=L - 1), "logits_stride"), "grad stride": (req(gstride=L - 1), "grad_stride"),
        "n 0": (req(n=0), "n must"), "n -1": (req(n=-1), "n must"), "n x stride": (req(n=2 ** 27, lstride=16 + L), "n must"),
        "clip 0": (req(clip=0.0), "clip_coef"), "clip -1": (req(clip=-1.0), "clip_coef"), "clip nan": (req(clip=nan), "clip_coef"),
        "clip inf": (req(clip=inf), "clip_coef"), "vcoef nan": (req(vcoef=nan), "finite"), "ecoef inf": (req(ecoef=inf), "finite"),
        "scale -inf": (req(scale=-inf), "finite"),
        "action +2": (req(action=ac.data_ptr() + 2), "aligned"), "mask +1": (req(mask=msk.data_ptr() + 1), "aligned"),
        "returns +2": (req(returns=ret.data_ptr() + 2), "aligned"), "logits f32 +2": (req(logits=lg.data_ptr() + 2), "aligned"),
        "logits bf16 +1": (req(logits=lgh.data_ptr() + 1, ldt=3), "aligned"), "value f16 +1": (req(value=valh.data_ptr() + 1, vdt=4), "aligned"),
        "grad_logits +2": (req(grad_logits=gl.data_ptr() + 2), "aligned"), "grad_value +1": (req(grad_value=gv.data_ptr() + 1), "aligned"),
        "stats +4": (req(stats=st.data_ptr() + 4), "8-byte aligned"), "moments +4": (req(adv_moments=mom.data_ptr() + 4), "8-byte aligned"),
        "grad_logits is logits": (req(grad_logits=lg.data_ptr()), "grad_logits overlaps logits"),
        "grad_logits in action": (req(grad_logits=ac.data_ptr() + 16), "grad_logits overlaps action"),
        "grad_value is returns": (req(grad_value=ret.data_ptr()), "grad_value overlaps returns"),
        "grad_value on mask": (req(grad_value=msk.data_ptr() + 8), "grad_value overlaps mask"),
        "grad_value in grad_logits": (req(grad_value=gl.data_ptr() + 4 * (n * L - 1)), "grad_value overlaps grad_logits"),
        "stats in moments": (req(stats=mom.data_ptr() + 8), "stats overlaps adv_moments"),
        "stats in grad_value": (req(stats=gv.data_ptr() + 8), "stats overlaps grad_value"),
    }
    for what, (r, msg) in bad.items():
        for stream in (False, True):
            assert call(s, r, stream) == INVALID, what
            assert msg in message(s), (what, message(s))
    assert untouched()
    s.step_begin()
    for stream in (False, True):
        assert call(s, req(), stream) == INVALID and "open step" in message(s)
    s.step_end()
    assert untouched()
    assert call(s, req()) == 0                                   # the call does write
    assert not untouched()
    want = ppo(np.float32, dict(x, adv_moments=mom.cpu().numpy()[:5]))
    tol = H.tolerances(n)
    _close(gl.cpu().numpy()[:n * L].reshape(n, L), want["grad_logits"], tol["grad_logits"], "float32", "abi")
    assert st[6].item() == want["cnt"] and bool((gl[n * L:] == -7).all()) and bool((gv[n:] == -7).all())
    s.close()
    skip = _sim(4, 4, flags=EXT_SKIP_OBSERVATIONS)                # it reads no export: it works without observations
    skip.init()
    gl.fill_(-7)
    assert call(skip, req()) == 0
    _close(gl.cpu().numpy()[:n * L].reshape(n, L), want["grad_logits"], tol["grad_logits"], "float32", "abi, no observations")
    skip.close()
