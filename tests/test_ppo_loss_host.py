"""The PPO loss without a GPU (gpu_hideseek.ppo_loss, hs_ppo_loss): a numpy restatement of what include/hideseek.h
states, in f32 in the header's order and the same in float64; the float64 one against torch autograd of the textbook
composition; the tolerances the GPU tests use, derived from the two restatements on the GPU tests' own cases; the cap on
samples near a clipping edge; the refusals of request(); and the header.

Tolerances (printed by test_tolerances_are_derived; DESIGN.md quotes them): each is 4 x the largest deviation of the f32
restatement from the float64 one over every case of CASES, for grad_logits, for grad_value, for every statistic divided
by the count, and for the two quantities a branch is chosen by (ratio, v - old_value).  A sample is near an edge when its
float64 ratio is within the ratio tolerance of 1 +- c or its float64 |v - old_value| within that tolerance of c: the
f32 and float64 branches may differ there, so its gradients are left out of a comparison; at most NEAR_EDGE_CAP of the
samples of a case may be."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_action_sampling_host import BUCKETS, DTYPES, HEADS, head_tables, heads_of, logits_of, sum5, to_dtype

STATS = 7
CLIP, VALUE_COEF, ENTROPY_COEF = 0.2, 0.5, 0.01
ROWS_PER_BLOCK, MAX_GRID = 32, 2048                       # asserted against the module in test_header_states_the_request
SIZES = (1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 1806)
BIG = MAX_GRID * ROWS_PER_BLOCK + ROWS_PER_BLOCK + 1     # one workgroup takes a second block, the last block is partial
VALUE_MODES = ("none", "value", "clipped")               # no value term, value, value + old_value
CASES = [(n, b, d, m, v) for n in SIZES for b in BUCKETS for d in DTYPES for m in (False, True) for v in VALUE_MODES]
CASES.append((BIG, BUCKETS[0], "bfloat16", True, "clipped"))
NEAR_EDGE_CAP = 1e-3
# The cap holds per case, so a case of 31 samples may have no sample near an edge at all and one of 1 806 a single one,
# while a draw lands within the tolerance of an edge with a probability of about 3e-4: among the 180 cases of up to
# 1 806 samples a few always would break it.  Their draws are therefore kept EDGE_MARGIN (twenty times the tolerance)
# away from the edges: a sample that lands closer draws its noise again.  The large case stays as drawn, so that the
# edges are exercised there.
EDGE_MARGIN = 1e-3
SEED = 0
# What rounding a gradient to the output type adds to a comparison: half an ulp, which for p significant bits (bf16: 8,
# f16: 11) is at most 2^-p of the value, and half the subnormal spacing (bf16: 2^-133, f16: 2^-24) below the normal range.
ROUNDING = {"float32": (0.0, 0.0), "bfloat16": (2.0 ** -8, 2.0 ** -134), "float16": (2.0 ** -11, 2.0 ** -25)}


def f32(x):
    return np.float32(x)


# ---- the contract, in the type `ft` ----
def ppo(ft, x, clip=CLIP, value_coef=VALUE_COEF, entropy_coef=ENTROPY_COEF, grad_scale=1.0):
    """hs_ppo_loss on the inputs x (dict: logits [n,L] f32, buckets, action [n,5], old_log_prob, advantage, adv_moments,
    mask, value, returns, old_value; None = absent) in float type `ft`, in the header's order.  Returns grad_logits,
    grad_value, stats (float64 sums of the `ft` values) and the per-sample quantities the tests look at."""
    n, buckets = x["logits"].shape[0], x["buckets"]
    c, vc_, ec, gs = (ft(f32(v)) for v in (clip, value_coef, entropy_coef, grad_scale))
    heads = []
    for h, l in enumerate(heads_of(x["logits"], buckets)):
        _, S, lp, ent, e = head_tables(l, ft)
        a = np.clip(x["action"][:, h], 0, buckets[h] - 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = l.astype(ft) - l.astype(ft).max(1, keepdims=True)
            logS = np.log(S)
        heads.append(dict(S=S, lp=lp, ent=ent, e=e, a=a, d=d, logS=logS))
    r = np.arange(n)
    lp = sum5(np.stack([hd["lp"][r, hd["a"]] for hd in heads], 1))
    ent = sum5(np.stack([hd["ent"] for hd in heads], 1))
    adv = x["advantage"].astype(ft)
    if x["adv_moments"] is not None:
        M = np.asarray(x["adv_moments"], np.float64)
        mu = M[0] / M[4] if M[4] else 0.0
        sd = np.sqrt(max(M[1] / M[4] - mu * mu, 0.0)) if M[4] else 0.0
        mean, std = (f32(mu), f32(sd)) if ft is np.float32 else (np.float64(f32(mu)), np.float64(f32(sd)))
        adv = (adv - mean) / (std + ft(f32(1e-8)))
    with np.errstate(invalid="ignore", over="ignore"):
        dlp = lp - x["old_log_prob"].astype(ft)
        ratio = np.exp(dlp)
        s1 = ratio * adv
        s2 = np.minimum(np.maximum(ratio, ft(1) - c), ft(1) + c) * adv
        unclipped = s1 <= s2
        pg = np.where(unclipped, -s1, -s2)
        g_lp = np.where(unclipped, -s1, ft(0))
        kl = (ratio - ft(1)) - dlp
    active = np.ones(n, bool) if x["mask"] is None else x["mask"] != 0
    cnt = int(active.sum())
    with np.errstate(divide="ignore"):
        w = gs / ft(f32(cnt))
    out = dict(lp=lp, ent=ent, ratio=ratio, unclipped=unclipped, active=active, cnt=cnt, pclip=s2 < s1)
    G = np.zeros(x["logits"].shape, ft)
    off = np.concatenate([[0], np.cumsum(buckets)])
    for h, hd in enumerate(heads):
        K = buckets[h]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            p = hd["e"] / hd["S"][:, None]
            t = p * ((hd["d"] - hd["logS"][:, None]) + hd["ent"][:, None])
            onehot = (np.arange(K)[None, :] == hd["a"][:, None]).astype(ft)
            y = w * (g_lp[:, None] * (onehot - p) + ec * t)
        G[:, off[h]:off[h + 1]] = np.where(active[:, None] & (hd["e"] > 0) & (y != 0), y, ft(0))
    out["grad_logits"] = G
    vl, vclip = np.zeros(n, ft), np.zeros(n, bool)
    if x["value"] is not None:
        v, R = x["value"].astype(ft), x["returns"].astype(ft)
        with np.errstate(invalid="ignore", over="ignore"):
            dv = v - R
            if x["old_value"] is not None:
                vo = x["old_value"].astype(ft)
                dvo = v - vo
                inner = np.abs(dvo) <= c
                dvc = np.where(inner, dv, (vo + np.where(dvo < 0, -c, c)) - R)
                u1, u2 = dv * dv, dvc * dvc
                first = u1 >= u2
                vl = ft(0.5) * np.where(first, u1, u2)
                g_v = np.where(first, dv, ft(0))
                vclip = u2 > u1
                out.update(dvo=dvo, first=first, inner=inner)
            else:
                vl, g_v = ft(0.5) * (dv * dv), dv
            y = w * (vc_ * g_v)
        out["grad_value"] = np.where(active & (y != 0), y, ft(0))
    on = active
    stats = np.array([pg[on].astype(np.float64).sum(), vl[on].astype(np.float64).sum(), ent[on].astype(np.float64).sum(),
                      kl[on].astype(np.float64).sum(), float((out["pclip"] & on).sum()), float((vclip & on).sum()), float(cnt)])
    out.update(stats=stats, vclip=vclip, pg=pg, vl=vl, kl=kl)
    for k in ("grad_logits", "grad_value", "lp", "ent", "ratio"):
        assert k not in out or out[k].dtype == ft, k
    return out


# ---- the inputs of the GPU tests ----
@functools.lru_cache(maxsize=None)
def _inputs(n, buckets, dtype, masked, vmode, seed, natural):
    rng = np.random.default_rng([seed, n, sum(buckets), DTYPES.index(dtype), int(masked), VALUE_MODES.index(vmode)])
    logits = logits_of(n, buckets, dtype)
    action = np.empty((n, HEADS), np.int32)
    for h, l in enumerate(heads_of(logits, buckets)):                  # drawn among the live buckets
        score = np.where(np.isfinite(l), rng.random(l.shape), -1.0)
        action[:, h] = score.argmax(1)
    x = dict(logits=logits, buckets=buckets, action=action, adv_moments=None, mask=None, value=None, returns=None, old_value=None,
             old_log_prob=np.zeros(n, np.float32), advantage=rng.standard_normal(n).astype(np.float32))
    lp = ppo(np.float32, x)["lp"]
    x["old_log_prob"] = (lp + f32(0.15) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    if masked:
        x["mask"] = (rng.random(n) < 0.8).astype(np.float32)
    if vmode != "none":
        x["value"] = to_dtype(rng.standard_normal(n), dtype)
        x["returns"] = to_dtype(x["value"] + rng.standard_normal(n).astype(np.float32), dtype)
    if vmode == "clipped":
        x["old_value"] = to_dtype(x["value"] + f32(0.3) * rng.standard_normal(n).astype(np.float32), dtype)
    c = np.float64(f32(CLIP))
    for _ in range(50 if n * NEAR_EDGE_CAP < 10 and not natural else 0):
        r = ppo(np.float64, x)
        near_p = np.minimum(np.abs(r["ratio"] - (1 - c)), np.abs(r["ratio"] - (1 + c))) <= EDGE_MARGIN
        near_v = np.abs(np.abs(r["dvo"]) - c) <= EDGE_MARGIN if vmode == "clipped" else np.zeros(n, bool)
        if not (near_p | near_v).any():
            break
        x["old_log_prob"] = np.where(near_p, lp + f32(0.15) * rng.standard_normal(n).astype(np.float32), x["old_log_prob"]).astype(np.float32)
        if vmode == "clipped":
            x["old_value"] = np.where(near_v, to_dtype(x["value"] + f32(0.3) * rng.standard_normal(n).astype(np.float32), dtype), x["old_value"])
    else:
        assert n * NEAR_EDGE_CAP >= 10 or natural, "a small case kept a sample near an edge"
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


def inputs(n, buckets, dtype, masked, vmode, seed=SEED, natural=False):
    """A fresh dict of the (shared, read-only) arrays of a case.  natural: the draws stay as drawn, whatever their
    distance to a clipping edge."""
    return dict(_inputs(n, buckets, dtype, masked, vmode, seed, natural))


# The issue's own trial, with the draws as drawn: old_log_prob = lp + 0.15 N and old_value = value + 0.3 N, nothing redrawn.
NATURAL = (1806, BUCKETS[0], "float32", True, "clipped")


@functools.lru_cache(maxsize=None)
def natural_both():
    x = inputs(*NATURAL, natural=True)
    return x, ppo(np.float32, x), ppo(np.float64, x)


@functools.lru_cache(maxsize=None)
def both(case):
    """(f32 restatement, float64 restatement) of a case of CASES: computed once, shared, left unchanged."""
    x = inputs(*case)
    return ppo(np.float32, x), ppo(np.float64, x)


def near_edge(r64, tol, clip=CLIP):
    """[n] bool: the float64 ratio within tol["ratio"] of 1 +- c, or the float64 |v - old_value| within it of c."""
    c = np.float64(f32(clip))
    ne = (np.abs(r64["ratio"] - (1 - c)) <= tol["ratio"]) | (np.abs(r64["ratio"] - (1 + c)) <= tol["ratio"])
    if "dvo" in r64:
        ne |= np.abs(np.abs(r64["dvo"]) - c) <= tol["ratio"]
    return ne


def branches_differ(r32, r64):
    d = r32["unclipped"] != r64["unclipped"]
    if "first" in r64:
        d |= (r32["first"] != r64["first"]) | (r32["inner"] != r64["inner"])
    return d & r64["active"]


def size_class(n):
    """The case size whose gradient tolerances a call over n samples is held to: the largest size of CASES not above n.
    A gradient is a per-sample term times w = grad_scale / cnt, and so is its f32 rounding error: it falls as n grows, so
    the tolerance of a smaller size is never too tight for a larger n, and that of n's own size is the tightest."""
    return max(s for s in SIZES + (BIG,) if s <= n)


@functools.lru_cache(maxsize=None)
def tolerances(n=None):
    """{"grad_logits", "grad_value", "stats", "ratio"}: 4 x the largest f32-vs-float64 deviation over CASES; "stats" is
    of a statistic divided by the count, "ratio" covers ratio and v - old_value.  Samples whose branches differ between
    the two (they are near an edge: asserted below) do not enter the gradient and statistic deviations.
    tolerances() is over all cases: the one tolerance each that the documents quote.  tolerances(n) takes the two
    gradient tolerances from the cases of size_class(n) alone — never wider than the overall ones, which the cases of 1
    and 31 samples set (w = 1 and about 1 / 25) and which would be half a typical gradient at 65 569 samples; "stats"
    and "ratio" do not scale with n and stay the overall ones."""
    if n is not None:
        return dict(tolerances(), **{k: v for k, v in _tolerances(size_class(n)).items() if k in ("grad_logits", "grad_value")})
    return _tolerances(None)


@functools.lru_cache(maxsize=None)
def _tolerances(size):
    dev = dict(grad_logits=0.0, grad_value=0.0, stats=0.0, ratio=0.0)
    for case in CASES:
        if size is not None and case[0] != size:
            continue
        r32, r64 = both(case)
        on = r64["active"]
        if not on.any():
            continue
        dev["ratio"] = max(dev["ratio"], float(np.abs(r32["ratio"].astype(np.float64) - r64["ratio"])[on].max()))
        if "dvo" in r64:
            dev["ratio"] = max(dev["ratio"], float(np.abs(r32["dvo"].astype(np.float64) - r64["dvo"])[on].max()))
        ok = ~branches_differ(r32, r64)
        dev["grad_logits"] = max(dev["grad_logits"], float(np.abs(r32["grad_logits"].astype(np.float64) - r64["grad_logits"])[ok].max()))
        if "grad_value" in r64:
            dev["grad_value"] = max(dev["grad_value"], float(np.abs(r32["grad_value"].astype(np.float64) - r64["grad_value"])[ok].max()))
        sel = ok & on
        for k in ("pg", "vl", "ent", "kl"):                      # the mean of the per-sample deviations bounds that of the sums / cnt
            dev["stats"] = max(dev["stats"], float(np.abs(r32[k].astype(np.float64) - r64[k])[sel].max()))
    # (grad_value has no transcendental: at one sample, w = 1, the f32 and float64 values can be equal, and then the GPU's
    # IEEE f32 operations give those bits too)
    assert all(np.isfinite(v) and (v > 0 or (k == "grad_value" and v == 0 and size is not None)) for k, v in dev.items()), dev
    return {k: 4.0 * v for k, v in dev.items()}


# ---- torch autograd of the textbook composition, float64 ----
def autograd64(x, live_only, clip=CLIP, value_coef=VALUE_COEF, entropy_coef=ENTROPY_COEF):
    """(grad_logits, grad_value) of loss = masked mean of pg - ec * ent + vc * vl by torch autograd in float64.
    live_only: every head is reduced over its finite logits alone (no -inf enters the graph)."""
    c = float(f32(clip))
    n, buckets = x["logits"].shape[0], x["buckets"]
    logits = torch.tensor(np.asarray(x["logits"], np.float64), requires_grad=True)
    off = np.concatenate([[0], np.cumsum(buckets)])
    lp, ent = 0.0, 0.0
    for h in range(HEADS):
        l = logits[:, off[h]:off[h + 1]]
        a = torch.tensor(np.clip(x["action"][:, h], 0, buckets[h] - 1).astype(np.int64))[:, None]
        if live_only:
            live = torch.isfinite(l.detach())
            z = l.masked_fill(~live, 0.0)
            m = torch.where(live, z, torch.full_like(z, -1e300)).max(1, keepdim=True).values.detach()
            e = torch.exp(z - m) * live
            logp = (z - m) - torch.log(e.sum(1, keepdim=True))
            p = e / e.sum(1, keepdim=True)
            ent = ent - (live * p * logp).sum(1)
        else:
            logp = torch.log_softmax(l, dim=1)
            p = torch.exp(logp)
            ent = ent - torch.where(p > 0, p * logp, torch.zeros_like(p)).sum(1)        # 0 log 0 = 0
        lp = lp + logp.gather(1, a)[:, 0]
    adv = torch.tensor(x["advantage"].astype(np.float64))
    ratio = torch.exp(lp - torch.tensor(x["old_log_prob"].astype(np.float64)))
    pg = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - c, 1 + c) * adv)
    loss = pg - float(f32(entropy_coef)) * ent
    value = None
    if x["value"] is not None:
        value = torch.tensor(x["value"].astype(np.float64), requires_grad=True)
        R = torch.tensor(x["returns"].astype(np.float64))
        u1 = (value - R) ** 2
        if x["old_value"] is not None:
            vo = torch.tensor(x["old_value"].astype(np.float64))
            u1 = torch.maximum(u1, ((vo + torch.clamp(value - vo, -c, c)) - R) ** 2)
        loss = loss + float(f32(value_coef)) * 0.5 * u1
    mask = torch.ones(n, dtype=torch.float64) if x["mask"] is None else torch.tensor((x["mask"] != 0).astype(np.float64))
    (loss * mask).sum().div(mask.sum()).backward()
    return logits.grad.numpy(), None if value is None else value.grad.numpy()


# ---- tests ----
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("vmode", VALUE_MODES)
def test_float64_restatement_is_autograd_of_the_textbook_loss(vmode, masked):
    x = inputs(1806, BUCKETS[0], "float32", masked, vmode)
    r = ppo(np.float64, x)
    clean = np.isfinite(x["logits"]).all(1)
    assert 700 < clean.sum() < 900
    plain_l, plain_v = autograd64(x, live_only=False)
    live_l, live_v = autograd64(x, live_only=True)
    err = float(np.abs(r["grad_logits"][clean] - plain_l[clean]).max())
    print(f"{vmode} {'masked' if masked else 'unmasked'}: |restatement - autograd| on rows without -inf: grad_logits {err:.3e}")
    assert err <= 1e-12
    # rows with a -inf bucket: plain autograd is NaN there; the restatement is autograd over the live buckets
    assert np.isnan(plain_l[~clean]).any(1).all(), "plain autograd is expected to be NaN on every row with a -inf bucket"
    assert np.isfinite(r["grad_logits"]).all() and not r["grad_logits"][np.isneginf(x["logits"])].view(np.int64).any()
    assert not live_l[np.isneginf(x["logits"])].any()
    assert float(np.abs(r["grad_logits"] - live_l).max()) <= 1e-12
    if vmode != "none":
        errv = float(np.abs(r["grad_value"] - live_v).max())
        print(f"    grad_value {errv:.3e}")
        assert errv <= 1e-12 and float(np.abs(r["grad_value"] - plain_v).max()) <= 1e-12
    # the loss the gradients belong to, from the statistics
    s = r["stats"]
    assert s[6] == r["cnt"] and (masked or s[6] == 1806)


def test_inputs_are_what_the_issue_describes():
    x = inputs(1806, BUCKETS[0], "bfloat16", True, "clipped")
    r = ppo(np.float32, x)
    for h, l in enumerate(heads_of(x["logits"], x["buckets"])):
        assert np.isfinite(l[np.arange(1806), x["action"][:, h]]).all()         # actions among the live buckets
    assert 0.12 < (r["lp"] - x["old_log_prob"]).std() < 0.18
    assert 0.75 < x["mask"].mean() < 0.85 and set(np.unique(x["mask"])) == {0.0, 1.0}
    for k in ("value", "returns", "old_value"):
        assert np.array_equal(to_dtype(x[k], "bfloat16"), x[k])
    assert 0.25 < (x["old_value"] - x["value"]).std() < 0.35 and 0.9 < (x["returns"] - x["value"]).std() < 1.1
    # both sides of both clips occur
    assert r["pclip"].any() and (~r["pclip"]).any() and r["vclip"].any() and (~r["vclip"]).any() and (~r["inner"]).any()


def test_tolerances_are_derived():
    tol = tolerances()
    print("ppo loss tolerances (4 x max f32-vs-f64 deviation): " + ", ".join(f"{k} {v:.3e}" for k, v in tol.items()))
    # f32 arithmetic on log-probabilities of magnitude up to ~60 and gradients of magnitude up to ~|A| / cnt
    assert 2.0 ** -24 < tol["ratio"] < 1e-3 and 2.0 ** -24 < tol["stats"] < 1e-2
    for k in ("grad_logits", "grad_value"):
        assert 2.0 ** -30 < tol[k] < 1e-4, (k, tol[k])
    for n in SIZES + (BIG,):
        t = tolerances(n)
        print(f"    n = {n}: grad_logits {t['grad_logits']:.3e}, grad_value {t['grad_value']:.3e}")
        assert 0 < t["grad_logits"] <= tol["grad_logits"] and 0 <= t["grad_value"] <= tol["grad_value"]
        assert t["stats"] == tol["stats"] and t["ratio"] == tol["ratio"]
    assert tolerances(1806)["grad_logits"] < tol["grad_logits"] / 100 and tolerances(BIG)["grad_logits"] < tol["grad_logits"] / 1000
    assert size_class(36) == 33 and size_class(252) == 33 and size_class(1806) == 1806 and size_class(BIG) == BIG


def test_natural_draws_stay_within_the_near_edge_cap():
    """The issue's trial: 1 806 samples, buckets (5, 5, 5, 2, 2), the draws as drawn."""
    x, r32, r64 = natural_both()
    tol = tolerances(NATURAL[0])
    ne, diff = near_edge(r64, tol), branches_differ(r32, r64)
    c = np.float64(f32(CLIP))
    closest = min(float(np.abs(r64["ratio"] - (1 - c)).min()), float(np.abs(r64["ratio"] - (1 + c)).min()), float(np.abs(np.abs(r64["dvo"]) - c).min()))
    print(f"natural draws: {int(ne.sum())} of {ne.size} samples near an edge, {int(diff.sum())} branches differ, closest to an edge {closest:.3e}")
    assert closest < EDGE_MARGIN, "these draws are not kept away from the edges"
    assert ne.sum() <= NEAR_EDGE_CAP * ne.size
    assert not (diff & ~ne).any()
    ok = ~ne
    assert float(np.abs(r32["grad_logits"].astype(np.float64) - r64["grad_logits"])[ok].max()) <= tol["grad_logits"]
    assert float(np.abs(r32["grad_value"].astype(np.float64) - r64["grad_value"])[ok].max()) <= tol["grad_value"]


def test_f32_restatement_keeps_its_branches_outside_the_near_edge_cap():
    near = total = 0
    for case in CASES:
        tol = tolerances(case[0])
        r32, r64 = both(case)
        ne, diff = near_edge(r64, tol), branches_differ(r32, r64)
        assert not (diff & ~ne).any(), (case, int((diff & ~ne).sum()))
        assert ne.sum() <= NEAR_EDGE_CAP * ne.size, (case, int(ne.sum()))
        ok = ~ne
        assert float(np.abs(r32["grad_logits"].astype(np.float64) - r64["grad_logits"])[ok].max(initial=0)) <= tol["grad_logits"]
        if "grad_value" in r64:
            assert float(np.abs(r32["grad_value"].astype(np.float64) - r64["grad_value"])[ok].max(initial=0)) <= tol["grad_value"]
        near, total = near + int(ne.sum()), total + ne.size
    print(f"samples within the tolerance of a clipping edge: {near} of {total}")
    assert near <= NEAR_EDGE_CAP * total


def test_request_refuses_before_the_library_is_called():
    from gpu_hideseek import ppo_loss as P

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    n, L = 48, 19
    good = dict(logits=torch.zeros(n, L), action=torch.zeros(n, 5, dtype=torch.int32), old_log_prob=torch.zeros(n), advantage=torch.zeros(n))
    full = dict(good, value=torch.zeros(n), returns=torch.zeros(n), old_value=torch.zeros(n), mask=torch.ones(n),
                adv_moments=torch.zeros(5, dtype=torch.float64))

    def call(base=good, **kw):
        a = dict(base, **kw)
        return P.compute(Sim(), a.pop("logits"), a.pop("action"), a.pop("old_log_prob"), a.pop("advantage"), **a)

    for bad, what in ((torch.zeros(n, L - 1), "shape"), (torch.zeros(n * L), "shape"), (torch.zeros(0, L), "shape"), (torch.zeros(n, 2, L), "shape"),
                      (torch.zeros(n, L, dtype=torch.float64), "dtype"), (torch.zeros(L, n).t(), "stride"), (torch.zeros(n, 2 * L)[:, ::2], "stride"),
                      (torch.zeros(n * L).as_strided((n, L), (L - 1, 1)), "stride")):
        with pytest.raises(ValueError, match=what):
            call(logits=bad)
    for name in ("logits", "action", "old_log_prob", "advantage"):
        with pytest.raises(ValueError, match=name):
            call(**{name: None})
    for name, bad, what in (("action", torch.zeros(n, 5), "dtype"), ("action", torch.zeros(n, 4, dtype=torch.int32), "shape"),
                            ("old_log_prob", torch.zeros(n + 1), "shape"), ("advantage", torch.zeros(n, dtype=torch.float16), "dtype"),
                            ("advantage", torch.zeros(2 * n)[::2], "contiguous"), ("mask", torch.ones(n, dtype=torch.bool), "dtype"),
                            ("adv_moments", torch.zeros(5), "dtype"), ("adv_moments", torch.zeros(4, dtype=torch.float64), "shape"),
                            ("value", torch.zeros(n, dtype=torch.float64), "dtype"), ("returns", torch.zeros(n - 1), "shape"),
                            ("old_value", torch.zeros(n, dtype=torch.bfloat16), "dtype"),
                            ("grad_logits", torch.zeros(n, L - 1), "shape"), ("grad_logits", torch.zeros(n + 1, L), "shape"),
                            ("grad_logits", torch.zeros(n, L, dtype=torch.float64), "dtype"), ("grad_logits", torch.zeros(n, 2 * L)[:, ::2], "stride"),
                            ("grad_value", torch.zeros(n, dtype=torch.bfloat16), "dtype"), ("grad_value", torch.zeros(n + 1), "shape"),
                            ("stats", torch.zeros(7), "dtype"), ("stats", torch.zeros(8, dtype=torch.float64), "shape")):
        with pytest.raises(ValueError, match=what):
            call(full, **{name: bad})
    with pytest.raises(ValueError, match="nothing to do"):
        call(grad_logits=None, stats=None)
    with pytest.raises(ValueError, match="grad_value needs value"):
        call(grad_value=True)
    with pytest.raises(ValueError, match="value needs returns"):
        call(value=torch.zeros(n))
    with pytest.raises(ValueError, match="need value"):
        call(returns=torch.zeros(n))
    with pytest.raises(ValueError, match="grad_dtype"):
        call(grad_dtype=torch.float64)
    for buckets in ((5, 5, 5, 2, 0), (17, 5, 5, 2, 2), (5, 5, 5, 2), (16, 16, 16, 16, 16)):
        with pytest.raises(ValueError, match="buckets"):
            call(logits=torch.zeros(n, 80), buckets=buckets)
    with pytest.raises(ValueError, match="shape"):                # wide enough for [5,5,5,2,2] only
        call(buckets=BUCKETS[1])
    for k in ("clip_coef", "value_loss_coef", "entropy_coef", "grad_scale"):
        for v in (float("nan"), float("inf"), 1e39):
            with pytest.raises(ValueError, match=k):
                call(**{k: v})
    for v in (0.0, -0.2, 1e-50):
        with pytest.raises(ValueError, match="clip_coef"):
            call(clip_coef=v)
    shared = torch.zeros(n * L + n)
    with pytest.raises(ValueError, match="grad_logits overlaps logits"):
        call(logits=shared[:n * L].view(n, L), grad_logits=shared[n:n + n * L].view(n, L))
    with pytest.raises(ValueError, match="grad_value overlaps returns"):
        call(full, grad_value=full["returns"])
    with pytest.raises(ValueError, match="grad_value overlaps grad_logits"):
        call(full, grad_logits=shared[:n * L].view(n, L), grad_value=shared[n * L - 1:n * L - 1 + n])
    with pytest.raises(ValueError, match="on cpu"):               # well-formed tensors on the wrong device
        call(full)
    with pytest.raises(ValueError, match="on cpu"):
        call(logits=torch.zeros(n, 40)[:, :L])


def test_stats_to_metrics():
    from gpu_hideseek import ppo_loss as P
    s = torch.tensor([3.0, 8.0, 20.0, 0.5, 2.0, 1.0, 4.0], dtype=torch.float64)
    m = P.stats_to_metrics(s, entropy_coef=0.01, value_loss_coef=0.5, grad_scale=2.0)
    assert all(v.dtype == torch.float64 for v in m.values())
    assert float(m["policy_loss"]) == 0.75 and float(m["value_loss"]) == 2.0 and float(m["entropy"]) == 5.0
    assert float(m["approx_kl"]) == 0.125 and float(m["clip_fraction"]) == 0.5 and float(m["value_clip_fraction"]) == 0.25
    assert float(m["count"]) == 4.0 and abs(float(m["loss"]) - 2.0 * (0.75 - 0.05 + 1.0)) < 1e-15
    z = P.stats_to_metrics(torch.zeros(7, dtype=torch.float64))
    assert all(float(v) == 0.0 for v in z.values())
    with pytest.raises(ValueError):
        P.stats_to_metrics(torch.zeros(5, dtype=torch.float64))


def test_header_states_the_request(hideseek_lib):
    """include/hideseek.h declares both entry points, the ctypes mirror agrees with it field by field, and the kernel's
    block constants are the module's."""
    from gpu_hideseek import ppo_loss as P
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hideseek.h")).read()
    assert re.search(r"HS_PPO_STATS = (\d+)", src).group(1) == str(P.STATS) == str(STATS)
    assert re.search(r"int32_t hs_ppo_loss\(hs_sim \*\w*, const hs_ppo_request \*\w*\);", src)
    assert re.search(r"int32_t hs_ppo_loss_async\(hs_sim \*\w*, void \*hip_stream, const hs_ppo_request \*\w*\);", src)
    body = re.search(r"typedef struct hs_ppo_request \{(.*?)\} hs_ppo_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*", "", n.strip(" *")) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("int32_t", "").replace("float", "").split(",")]
    names = [n.split()[-1].lstrip("*") for n in names]
    assert names == [f[0] for f in P.HsPpoRequest._fields_], names
    R = P.HsPpoRequest
    assert C.sizeof(R) == 160 and R.n.offset == 72 and R.buckets.offset == 96 and R.clip_coef.offset == 116
    assert R.grad_scale.offset == 128 and R.grad_logits.offset == 136 and R.grad_value.offset == 144 and R.stats.offset == 152
    lib = C.CDLL(hideseek_lib)
    assert hasattr(lib, "hs_ppo_loss") and hasattr(lib, "hs_ppo_loss_async")
    kernel = open(os.path.join(root, "marl-hideandseek_amd", "csrc", "hs_k_ppo.h")).read()
    assert int(re.search(r"kPpoMaxGrid = (\d+);", kernel).group(1)) == P.MAX_GRID == MAX_GRID
    assert "kPpoRows = kPpoThreads / kPpoLanesPerRow" in kernel and "static_assert(kPpoRows == 32" in kernel
    assert P.ROWS_PER_BLOCK == ROWS_PER_BLOCK == 32
