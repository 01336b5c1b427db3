"""The two-hot symlog critic head without a GPU (gpu_hideseek.value_head, hs_twohot_value): a numpy restatement of what
include/hideseek.h states, in f32 in the header's order and the same in float64; the float64 one against torch autograd
of the textbook composition; a first-principles anchor (the logits log t of a two-hot target decode back to the
return); the continuity of the target across a bin; the tolerances the GPU tests use, derived from the two
restatements on the GPU tests' own cases; the refusals of request(); and the header.

Tolerances (printed by test_tolerances_are_derived; DESIGN.md quotes them): each is 4 x (the project's margin) the
largest deviation of the f32 restatement from the float64 one over every case of CASES: for y (the expectation in symlog
space), for ce, for grad_logits per case size (a gradient is a per-sample term times w = grad_scale / cnt), and for each
statistic divided by the count (the largest per-sample deviation bounds that of the mean).  The decoded value is held
to |got - want| <= tol_y (1 + |want|), since v = symexp(y) has dv = (1 + |v|) dy.  The target is continuous across a bin
(test_target_is_continuous_across_a_bin), so a sample whose f32 and float64 bins differ deviates like any other and no
sample is left out of a comparison.  Two statistics, sum R and sum R^2, are float64 sums of the same float64 terms in
both restatements, so their derived tolerance is 0; what a different order of a float64 sum of n terms can change is at
most n 2^-53 sum |term| (summation_slack), which the GPU tests add for every statistic."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_action_sampling_host import DTYPES, to_dtype
from test_ppo_loss_host import ROUNDING, f32

STATS = 6
LANES = 8
ROWS_PER_BLOCK, MAX_GRID = 32, 2048                       # asserted against the module in test_header_states_the_request
SIZES = (1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 1806)
BINS = ((2, -1.0, 1.0), (63, -5.0, 5.0), (255, -20.0, 20.0), (256, -20.0, 20.0))
BIG = MAX_GRID * ROWS_PER_BLOCK + ROWS_PER_BLOCK + 1     # one workgroup takes a second block, the last block is partial
CASES = [(n, b, d, m) for n in SIZES for b in BINS for d in DTYPES for m in (False, True)]
CASES.append((BIG, BINS[2], "bfloat16", True))
STAT_NAMES = ("ce", "sq", "v", "R", "R2")
SEED = 0


# ---- the contract, in the type `ft` ----
def lane_sum(a, ft):
    """sum over the last axis in the header's order: lane h of 8 adds columns h, h + 8, ... in ascending order onto 0,
    the 8 partials are combined as ((0+1)+(2+3)) + ((4+5)+(6+7))."""
    n, B = a.shape
    J = -(-B // LANES)
    pad = np.zeros((n, J * LANES), ft)
    pad[:, :B] = a
    pad = pad.reshape(n, J, LANES)
    acc = np.zeros((n, LANES), ft)
    for j in range(J):
        acc = acc + pad[:, j, :]
    return ((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])) + ((acc[:, 4] + acc[:, 5]) + (acc[:, 6] + acc[:, 7]))


def bin_values(ft, B, lo, hi):
    lo, hi = ft(f32(lo)), ft(f32(hi))
    step = (hi - lo) / ft(f32(B - 1))
    return lo, hi, step, lo + np.arange(B).astype(ft) * step


def target(ft, R, B, lo, hi):
    """(k, f) of the two-hot target of the returns R."""
    lo, hi, step, _ = bin_values(ft, B, lo, hi)
    R = np.asarray(R).astype(ft)
    with np.errstate(invalid="ignore"):
        z = np.copysign(np.log1p(np.abs(R)), R)
        zc = np.fmin(np.fmax(z, lo), hi)
        u = (zc - lo) / step
        k = np.clip(np.nan_to_num(np.floor(u), nan=0.0), 0, B - 2).astype(np.int64)
        f = np.fmin(np.fmax(u - k.astype(ft), ft(0)), ft(1))
    assert f.dtype == ft
    return k, f


def twohot(ft, x, loss_coef=1.0, grad_scale=1.0):
    """hs_twohot_value on the inputs x (dict: logits [n, B], lo, hi, returns or None, mask or None) in float type `ft`,
    in the header's order.  Returns value, grad_logits, stats (float64 sums of the `ft` values) and the per-sample
    quantities the tests look at."""
    L = np.asarray(x["logits"]).astype(ft)
    n, B = L.shape
    lo, hi, step, b = bin_values(ft, B, x["lo"], x["hi"])
    active = np.ones(n, bool) if x["mask"] is None else np.asarray(x["mask"]) != 0
    cnt = int(active.sum())
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = L.max(1, keepdims=True)
        d = L - m
        e = np.exp(d)
        S, Y = lane_sum(e, ft), lane_sum(e * b[None, :], ft)
        rS = ft(1) / S
        y = Y * rS
        v = np.copysign(np.expm1(np.abs(y)), y)
        out = dict(y=y, v=v, active=active, cnt=cnt, value=np.where(active & (v != 0), v, ft(0)))
        if x["returns"] is not None:
            R = np.asarray(x["returns"], np.float32)
            k, f = target(ft, R, B, x["lo"], x["hi"])
            r = np.arange(n)
            logS = np.log(S)
            ce = -((ft(1) - f) * (d[r, k] - logS) + f * (d[r, k + 1] - logS))
            t = np.zeros((n, B), ft)
            t[r, k] = ft(1) - f
            t[r, k + 1] = f
            w = ft(f32(grad_scale)) / ft(f32(cnt))
            g = w * (ft(f32(loss_coef)) * (e * rS[:, None] - t))
            G = np.where(active[:, None] & (g != 0), g, ft(0))
            R64, v64 = R.astype(np.float64), v.astype(np.float64)
            per = dict(ce=ce.astype(np.float64), sq=(v64 - R64) ** 2, v=v64, R=R64, R2=R64 * R64)
            stats = np.array([per[q][active].sum() for q in STAT_NAMES] + [float(cnt)])
            out.update(k=k, f=f, t=t, ce=ce, grad_logits=G, stats=stats, per=per)
    for q in ("y", "v", "value", "ce", "grad_logits", "f"):
        assert q not in out or out[q].dtype == ft, q
    return out


# ---- the inputs of the GPU tests ----
def draw_returns(rng, n):
    return (rng.standard_normal(n) * np.exp(rng.uniform(-3.0, 6.0, n))).astype(np.float32)


def peaked_logits(rng, near, B, lo, hi, dtype):
    """Logits with std 3 around a peak at the place of symlog(near) among the bins, representable in `dtype`."""
    n = near.shape[0]
    k, f = target(np.float64, near, B, lo, hi)
    pos = (k + f)[:, None]
    peak = 12.0 * np.exp(-0.5 * ((np.arange(B)[None, :] - pos) / 1.5) ** 2)
    return to_dtype((3.0 * rng.standard_normal((n, B)) + peak).astype(np.float32), dtype)


@functools.lru_cache(maxsize=None)
def _inputs(n, bins, dtype, masked, seed):
    B, lo, hi = bins
    rng = np.random.default_rng([seed, n, B, DTYPES.index(dtype), int(masked)])
    R = draw_returns(rng, n)
    near = (R * (1.0 + 0.3 * rng.standard_normal(n))).astype(np.float32)
    logits = peaked_logits(rng, near, B, lo, hi, dtype).copy()
    mask = (rng.random(n) < 0.8).astype(np.float32) if masked else None
    # planted returns: 0, +-1e12 (beyond the last bin), a return exactly on a bin; they go to the first samples there are
    _, _, _, b32 = bin_values(np.float32, B, lo, hi)
    on_bin = np.copysign(np.expm1(np.abs(b32[B // 3])), b32[B // 3])
    planted = [0.0, 1e12, -1e12, on_bin]
    for i, p in enumerate(planted[:max(n - 1, 1)]):
        R[(i * 7) % n] = p
        if mask is not None and n > 1:
            mask[(i * 7) % n] = 1.0
    if mask is not None:                                    # NaN in inactive samples: logits and returns
        off = np.flatnonzero(mask == 0)[:3]
        R[off] = np.nan
        logits[off, ::2] = np.nan
    x = dict(logits=logits, lo=lo, hi=hi, returns=R, mask=mask)
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


def inputs(n, bins, dtype, masked, seed=SEED):
    """A fresh dict of the (shared, read-only) arrays of a case."""
    return dict(_inputs(n, bins, dtype, masked, seed))


@functools.lru_cache(maxsize=None)
def both(case):
    """(f32 restatement, float64 restatement) of a case of CASES: computed once, shared, left unchanged."""
    x = inputs(*case)
    return twohot(np.float32, x), twohot(np.float64, x)


def size_class(n):
    """The case size whose gradient tolerance a call over n samples is held to: the largest size of CASES not above n (a
    gradient's rounding error falls with w = 1 / cnt as n grows)."""
    return max(s for s in SIZES + (BIG,) if s <= n)


@functools.lru_cache(maxsize=None)
def _tolerances(size):
    dev = dict(y=0.0, ce=0.0, grad_logits=0.0, **{"stat_" + q: 0.0 for q in STAT_NAMES})
    for case in CASES:
        if size is not None and case[0] != size:
            continue
        r32, r64 = both(case)
        on = r64["active"]
        if not on.any():
            continue
        dev["y"] = max(dev["y"], float(np.abs(r32["y"].astype(np.float64) - r64["y"])[on].max()))
        dev["ce"] = max(dev["ce"], float(np.abs(r32["ce"].astype(np.float64) - r64["ce"])[on].max()))
        dev["grad_logits"] = max(dev["grad_logits"], float(np.abs(r32["grad_logits"].astype(np.float64) - r64["grad_logits"]).max()))
        for q in STAT_NAMES:
            dev["stat_" + q] = max(dev["stat_" + q], float(np.abs(r32["per"][q] - r64["per"][q])[on].max()))
    assert all(np.isfinite(v) for v in dev.values()), dev
    return {k: 4.0 * v for k, v in dev.items()}


@functools.lru_cache(maxsize=None)
def tolerances(n=None):
    """{"y", "ce", "grad_logits", "stat_ce", "stat_sq", "stat_v", "stat_R", "stat_R2"}: 4 x the largest f32-vs-float64
    deviation over CASES.  tolerances() is over all cases; tolerances(n) takes grad_logits from the cases of
    size_class(n) alone, never wider than the overall one."""
    if n is not None:
        return dict(tolerances(), grad_logits=_tolerances(size_class(n))["grad_logits"])
    return _tolerances(None)


def summation_slack(terms):
    """What the order of a float64 sum of these terms can change at the most: (n - 1) 2^-53 sum |term| to first order."""
    terms = np.asarray(terms, np.float64)
    return terms.size * 2.0 ** -53 * float(np.abs(terms).sum())


def value_bound(want, tol_y, dtype):
    """The bound on |got - want| of a decoded value stored in `dtype`."""
    rel, absolute = ROUNDING[dtype]
    a = np.abs(np.asarray(want, np.float64))
    return tol_y * (1.0 + a) + rel * a + absolute


# ---- torch autograd of the textbook composition, float64 ----
def autograd64(x):
    from gpu_hideseek import value_head as V
    n, B = x["logits"].shape
    on = np.ones(n, bool) if x["mask"] is None else x["mask"] != 0
    logits = torch.tensor(np.asarray(x["logits"], np.float64)[on], requires_grad=True)
    R = torch.tensor(np.asarray(x["returns"], np.float64)[on])
    ce = -(V.twohot(R, B, x["lo"], x["hi"]) * torch.log_softmax(logits, dim=1)).sum(1)
    loss = ce.mean()
    loss.backward()
    g = np.zeros((n, B))
    g[on] = logits.grad.numpy()
    return float(loss.detach()), g, ce.detach().numpy()


# ---- tests ----
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("bins", BINS, ids=lambda b: f"B{b[0]}")
def test_float64_restatement_is_autograd_of_the_textbook_loss(bins, masked):
    x = inputs(1806, bins, "float32", masked)
    r = twohot(np.float64, x)
    loss, g, ce = autograd64(x)
    on = r["active"]
    err_g = float(np.abs(r["grad_logits"] - g).max())
    err_ce = float(np.abs(r["ce"][on] - ce).max())
    err_loss = abs(r["stats"][0] / r["cnt"] - loss)
    print(f"B = {bins[0]} {'masked' if masked else 'unmasked'}: |restatement - autograd|: grad_logits {err_g:.3e}, ce {err_ce:.3e}, loss {err_loss:.3e}")
    # measured: 2e-16 and below for the gradient (magnitudes up to 1 / cnt), 3e-14 for a cross-entropy of magnitude up to 60
    assert err_g <= 1e-15 and err_ce <= 1e-12 and err_loss <= 1e-12
    assert not r["grad_logits"][~on].view(np.int64).any() and not r["value"][~on].view(np.int64).any()
    assert r["stats"][5] == r["cnt"] and (masked or r["cnt"] == 1806)


def test_eager_functions_are_the_restatement():
    """value_head.bins / symlog / symexp / twohot / decode / eager_loss, the composition the bench times, against the
    float64 restatement (they are f32 torch in another order, so within the derived tolerances)."""
    from gpu_hideseek import value_head as V
    tol = tolerances(1806)
    for bins in BINS:
        B, lo, hi = bins
        x = inputs(1806, bins, "float32", False)
        r64 = twohot(np.float64, x)
        assert np.array_equal(V.bins(B, lo, hi).numpy(), bin_values(np.float32, B, lo, hi)[3])
        L, R = torch.from_numpy(np.array(x["logits"])), torch.from_numpy(np.array(x["returns"]))
        t = V.twohot(R, B, lo, hi).numpy()
        assert float(np.abs(t - r64["t"]).max()) <= tol["grad_logits"] * 1806        # the target's share of a gradient at w = 1
        v = V.decode(L, B, lo, hi).numpy()
        assert (np.abs(v - r64["v"]) <= 4 * value_bound(r64["v"], tol["y"], "float32")).all()
        assert abs(float(V.eager_loss(L, R, None, B, lo, hi)) - r64["stats"][0] / 1806) <= 4 * tol["stat_ce"]
    z = torch.tensor([-3.0, 0.0, 1e-3, 7.5])
    assert torch.allclose(V.symexp(V.symlog(z)), z, rtol=1e-6, atol=0)


@pytest.mark.parametrize("bins", BINS, ids=lambda b: f"B{b[0]}")
def test_log_of_a_twohot_target_decodes_back_to_the_return(bins):
    """First principles: softmax(log t) = t, and the expectation of the bins under a two-hot target of R is symlog(R)
    clamped into [lo, hi]; so the logits log t decode to R, and beyond the last bin to +-symexp(hi).  Empty bins hold
    -1e4 (e = 0 exactly), not -inf."""
    B, lo, hi = bins
    rng = np.random.default_rng([SEED, B, 77])
    top = float(np.expm1(np.float64(hi)))
    inside = np.concatenate([draw_returns(rng, 400), [0.0, 1.0, -1.0]]).astype(np.float32)
    inside = inside[np.abs(inside.astype(np.float64)) <= float(np.expm1(np.float64(min(-lo, hi))))]
    beyond = np.array([1e12, -1e12, np.inf, -np.inf], np.float32)
    R = np.concatenate([inside, beyond])
    want = np.concatenate([inside.astype(np.float64), np.sign(beyond[:]) * np.where(beyond > 0, top, float(np.expm1(np.float64(-lo))))])
    assert inside.size > 20
    tol = tolerances()
    for ft, bound in ((np.float64, 1e-12 * (1 + np.abs(want))), (np.float32, value_bound(want, tol["y"], "float32"))):
        k, f = target(np.float64, R, B, lo, hi)
        t = np.zeros((R.size, B))
        r = np.arange(R.size)
        t[r, k], t[r, k + 1] = 1 - f, f
        with np.errstate(divide="ignore"):
            logits = np.where(t > 0, np.log(np.where(t > 0, t, 1.0)), -1e4)
        out = twohot(ft, dict(logits=logits if ft is np.float64 else logits.astype(np.float32), lo=lo, hi=hi, returns=R, mask=None))
        err = np.abs(out["v"].astype(np.float64) - want)
        print(f"B = {B} {ft.__name__}: largest |decoded - R| / (1 + |R|) = {float((err / (1 + np.abs(want))).max()):.3e}")
        assert (err <= bound).all(), (ft, float((err - bound).max()))
        # and the loss of the exact target is its entropy; its gradient is 0
        assert float(np.abs(out["grad_logits"]).max()) <= (1e-12 if ft is np.float64 else tol["grad_logits"]) / 1.0


@pytest.mark.parametrize("bins", BINS, ids=lambda b: f"B{b[0]}")
def test_target_is_continuous_across_a_bin(bins):
    """A return exactly on a bin and the f32 neighbours either side of it: the three targets differ by no more than the
    gradient tolerance at w = 1, in f32 and in float64."""
    B, lo, hi = bins
    b32 = bin_values(np.float32, B, lo, hi)[3]
    tol = tolerances(1)["grad_logits"]
    worst = 0.0
    for k in sorted({0, 1, B // 3, B // 2, B - 2, B - 1}):
        R0 = np.float32(np.copysign(np.expm1(np.abs(b32[k])), b32[k]))
        Rs = np.array([np.nextafter(R0, np.float32(-np.inf)), R0, np.nextafter(R0, np.float32(np.inf))], np.float32)
        for ft in (np.float32, np.float64):
            kk, f = target(ft, Rs, B, lo, hi)
            t = np.zeros((3, B))
            t[np.arange(3), kk], t[np.arange(3), kk + 1] = 1 - f.astype(np.float64), f.astype(np.float64)
            worst = max(worst, float(np.abs(t[0] - t[1]).max()), float(np.abs(t[2] - t[1]).max()))
            assert abs(t[1, k] - 1.0) <= tol, (k, ft, t[1, k])
    print(f"B = {B}: the target moves by at most {worst:.3e} across a bin (tolerance {tol:.3e})")
    assert worst <= tol


def test_inputs_are_what_the_issue_describes():
    case = (1806, BINS[2], "bfloat16", True)
    x = inputs(*case)
    r32, _ = both(case)
    on = x["mask"] != 0
    assert np.array_equal(to_dtype(np.nan_to_num(x["logits"]), "bfloat16"), np.nan_to_num(x["logits"]))
    assert 0.75 < x["mask"].mean() < 0.85 and set(np.unique(x["mask"])) == {0.0, 1.0}
    R = x["returns"]
    assert (R[on] == 0).any() and (R[on] == f32(1e12)).any() and (R[on] == f32(-1e12)).any() and not np.isnan(R[on]).any()
    assert np.isnan(R[~on]).sum() == 3 and np.isnan(x["logits"][~on]).any(1).sum() == 3 and np.isfinite(x["logits"][on]).all()
    b32 = bin_values(np.float32, 255, -20.0, 20.0)[3]
    assert (R[on] == np.expm1(np.abs(b32[85])) * np.sign(b32[85])).any()
    # realistic values: the decoded value follows the return it was drawn near (in symlog space, within a few bins)
    sl = lambda a: np.sign(a) * np.log1p(np.abs(a))                         # noqa: E731
    ok = on & (np.abs(R) < 1e11)
    assert np.median(np.abs(sl(r32["v"][ok]) - sl(R[ok]))) < 1.0
    assert 1e-3 < np.median(np.abs(R[ok])) < 100 and np.abs(R[ok]).max() > 300
    assert CASES[-1][0] == BIG == 65569 and len(CASES) == 121


def test_tolerances_are_derived():
    tol = tolerances()
    print("two-hot value head tolerances (4 x max f32-vs-f64 deviation): " + ", ".join(f"{k} {v:.3e}" for k, v in tol.items()))
    # y: an f32 sum of up to 256 products of magnitude up to 20; ce: log-probabilities of magnitude up to ~60
    assert 2.0 ** -24 < tol["y"] < 1e-3 and 2.0 ** -24 < tol["ce"] < 1e-2 and 2.0 ** -24 < tol["grad_logits"] < 1e-3
    assert tol["stat_ce"] == tol["ce"] and tol["stat_R"] == 0.0 and tol["stat_R2"] == 0.0 and tol["stat_v"] > 0 and tol["stat_sq"] > 0
    for n in SIZES + (BIG,):
        t = tolerances(n)
        print(f"    n = {n}: grad_logits {t['grad_logits']:.3e}")
        assert 0 < t["grad_logits"] <= tol["grad_logits"] and all(t[k] == tol[k] for k in tol if k != "grad_logits")
    assert tolerances(1806)["grad_logits"] < tol["grad_logits"] / 100 and tolerances(BIG)["grad_logits"] < tol["grad_logits"] / 1000
    assert size_class(36) == 33 and size_class(252) == 33 and size_class(1806) == 1806 and size_class(BIG) == BIG
    # the f32 restatement itself stays within a quarter of each: by construction, and the value within its own bound
    for case in CASES:
        r32, r64 = both(case)
        on = r64["active"]
        assert (np.abs(r32["v"].astype(np.float64) - r64["v"])[on] <= value_bound(r64["v"], tol["y"], "float32")[on]).all(), case


def test_request_refuses_before_the_library_is_called():
    from gpu_hideseek import value_head as V

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    n, B = 48, 255
    good = dict(logits=torch.zeros(n, B), returns=torch.zeros(n))
    full = dict(good, mask=torch.ones(n))

    def call(base=good, **kw):
        a = dict(base, **kw)
        return V.compute(Sim(), a.pop("logits"), a.pop("returns"), **a)

    for bad, what in ((torch.zeros(n, B - 1), "shape"), (torch.zeros(n * B), "shape"), (torch.zeros(0, B), "shape"), (torch.zeros(n, 2, B), "shape"),
                      (torch.zeros(n, B, dtype=torch.float64), "dtype"), (torch.zeros(B, n).t(), "stride"), (torch.zeros(n, 2 * B)[:, ::2], "stride"),
                      (torch.zeros(n * B).as_strided((n, B), (B - 1, 1)), "stride"), (None, "logits")):
        with pytest.raises(ValueError, match=what):
            call(logits=bad)
    for name, bad, what in (("returns", torch.zeros(n + 1), "shape"), ("returns", torch.zeros(n, dtype=torch.bfloat16), "dtype"),
                            ("returns", torch.zeros(2 * n)[::2], "contiguous"), ("mask", torch.ones(n, dtype=torch.bool), "dtype"),
                            ("mask", torch.ones(n - 1), "shape"),
                            ("value", torch.zeros(n + 1), "shape"), ("value", torch.zeros(n, dtype=torch.float64), "dtype"),
                            ("value", torch.zeros(2 * n)[::2], "contiguous"), ("value", 3.0, "value"),
                            ("grad_logits", torch.zeros(n, B - 1), "shape"), ("grad_logits", torch.zeros(n + 1, B), "shape"),
                            ("grad_logits", torch.zeros(n, B, dtype=torch.float64), "dtype"), ("grad_logits", torch.zeros(n, 2 * B)[:, ::2], "stride"),
                            ("stats", torch.zeros(6), "dtype"), ("stats", torch.zeros(7, dtype=torch.float64), "shape")):
        with pytest.raises(ValueError, match=what):
            call(full, **{name: bad})
    with pytest.raises(ValueError, match="nothing to do"):
        call(value=None, grad_logits=None, stats=False, returns=None)
    with pytest.raises(ValueError, match="nothing to do"):
        call(value=None, grad_logits=False, stats=False)
    with pytest.raises(ValueError, match="need returns"):
        call(returns=None, grad_logits=True)
    with pytest.raises(ValueError, match="need returns"):
        call(returns=None, stats=True)
    for k in ("grad_dtype", "value_dtype"):
        with pytest.raises(ValueError, match=k):
            call(**{k: torch.float64})
    for bins in (1, 0, -3, 257, 2.0, True):
        with pytest.raises(ValueError, match="bins"):
            call(bins=bins)
    with pytest.raises(ValueError, match="shape"):                # wide enough for 255 bins only
        call(bins=256)
    for k in ("lo", "hi", "loss_coef", "grad_scale"):
        for v in (float("nan"), float("inf"), 1e39):
            with pytest.raises(ValueError, match=k):
                call(**{k: v})
    for lo, hi in ((1.0, 1.0), (2.0, -2.0), (1.0, 1.0 + 1e-12)):
        with pytest.raises(ValueError, match="lo must be below hi"):
            call(lo=lo, hi=hi)
    shared = torch.zeros(n * B + n)
    with pytest.raises(ValueError, match="grad_logits overlaps logits"):
        call(logits=shared[:n * B].view(n, B), grad_logits=shared[n:n + n * B].view(n, B))
    with pytest.raises(ValueError, match="value overlaps returns"):
        call(full, value=full["returns"])
    with pytest.raises(ValueError, match="grad_logits overlaps value"):
        call(full, value=shared[n * B - 1:n * B - 1 + n], grad_logits=shared[:n * B].view(n, B))
    with pytest.raises(ValueError, match="on cpu"):               # well-formed tensors on the wrong device
        call(full)
    with pytest.raises(ValueError, match="on cpu"):
        call(logits=torch.zeros(n, 300)[:, :B], returns=None)


def test_stats_to_metrics():
    from gpu_hideseek import value_head as V
    # four samples: returns 1, 2, 3, 6 (mean 3, var 3.5), values off by 1, -1, 0, 2 (mse 1.5)
    s = torch.tensor([10.0, 6.0, 14.0, 12.0, 50.0, 4.0], dtype=torch.float64)
    m = V.stats_to_metrics(s)
    assert all(v.dtype == torch.float64 for v in m.values()) and set(m) == {"value_loss", "mse", "explained_variance", "mean_value", "count"}
    assert float(m["value_loss"]) == 2.5 and float(m["mse"]) == 1.5 and float(m["mean_value"]) == 3.5 and float(m["count"]) == 4.0
    assert abs(float(m["explained_variance"]) - (1 - 1.5 / 3.5)) < 1e-15
    z = V.stats_to_metrics(torch.zeros(6, dtype=torch.float64))
    assert all(float(v) == 0.0 for v in z.values())
    const = V.stats_to_metrics(torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0, 4.0], dtype=torch.float64))      # var(R) = 0
    assert float(const["explained_variance"]) == 0.0
    with pytest.raises(ValueError):
        V.stats_to_metrics(torch.zeros(7, dtype=torch.float64))


def test_header_states_the_request(hideseek_lib):
    """include/hideseek.h declares both entry points, the ctypes mirror agrees with it field by field, and the kernel's
    block constants are the module's."""
    from gpu_hideseek import value_head as V
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hideseek.h")).read()
    assert re.search(r"HS_TWOHOT_STATS = (\d+)", src).group(1) == str(V.STATS) == str(STATS)
    assert re.search(r"HS_TWOHOT_MAX_BINS = (\d+)", src).group(1) == str(V.MAX_BINS) == "256"
    assert re.search(r"int32_t hs_twohot_value\(hs_sim \*\w*, const hs_twohot_request \*\w*\);", src)
    assert re.search(r"int32_t hs_twohot_value_async\(hs_sim \*\w*, void \*hip_stream, const hs_twohot_request \*\w*\);", src)
    body = re.search(r"typedef struct hs_twohot_request \{(.*?)\} hs_twohot_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            for part in decl.strip().split(None, 1)[1].replace("int32_t", "").replace("float", "").replace("double", "").replace("void", "").split(","):
                names.append(part.split()[-1].lstrip("*"))
    assert names == [f[0] for f in V.HsTwohotRequest._fields_], names
    R = V.HsTwohotRequest
    assert C.sizeof(R) == 96 and R.n.offset == 24 and R.bins.offset == 36 and R.lo.offset == 40 and R.grad_scale.offset == 52
    assert R.value_dtype.offset == 56 and R.grad_stride.offset == 64 and R.value.offset == 72 and R.grad_logits.offset == 80 and R.stats.offset == 88
    lib = C.CDLL(hideseek_lib)
    assert hasattr(lib, "hs_twohot_value") and hasattr(lib, "hs_twohot_value_async")
    kernel = open(os.path.join(root, "marl-hideandseek_amd", "csrc", "hs_k_twohot.h")).read()
    assert int(re.search(r"kTwMaxGrid = (\d+);", kernel).group(1)) == V.MAX_GRID == MAX_GRID
    assert int(re.search(r"kTwLanesPerRow = (\d+);", kernel).group(1)) == LANES
    assert "kTwRows = kTwThreads / kTwLanesPerRow" in kernel and "static_assert(kTwRows == 32" in kernel
    assert V.ROWS_PER_BLOCK == ROWS_PER_BLOCK == 32
    assert (V.DEFAULT_BINS, V.DEFAULT_LO, V.DEFAULT_HI) == (255, -20.0, 20.0)
