"""The recurrent core without a GPU (gpu_hideseek.recurrent, hs_lstm_cell / hs_lstm_cell_backward): a numpy restatement
of what include/hideseek.h states, forward and backward, once in f32 in the header's order (the backward including
rounds, waves, workgroups and segments of the parameter sums) and once in float64; the float64 backward against central
differences; recurrent.eager and its autograd against both; a three-step sequence with a clear in the middle; the
tolerances the GPU tests use, derived from the two restatements on the GPU tests' own cases; the refusals of request();
and the header.

numpy has no fmaf: fmaf(x, w, z) is taken as the f32 rounding of the float64 x * w + z (test_entity_encoder_host says
why that is the same but for rare double roundings).  numpy's f32 exp and tanh are not the device library's: both are
accurate to a few ulp, neither is correctly rounded, and their bits differ.  That is why the GPU comparison is a bound.

Tolerances (printed by test_tolerances_are_derived; DESIGN.md quotes them), none a constant: per case (n, H, dtype) and
per output (y, h_next, c_next, grad_gates, grad_c_prev, and bias / scale / shift of grad_cell_params) 4 x (the project's
margin, as in test_value_head_host) the largest deviation of the f32 restatement from the float64 one, plus the
rounding of the output's dtype (ROUNDING: half an ulp relative, the smallest subnormal absolute).
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_action_sampling_host import DTYPES, to_dtype
from test_ppo_loss_host import ROUNDING

HIDDEN = (64, 128, 256, 512)
PARAM_ROWS, WAVES, MAX_GRID_BWD, SUM_SEGS = 6, 4, 512, 8                   # asserted against module and header below
EPS = 1e-6
SEED = 0
SIZES = (1, 3, 5, MAX_GRID_BWD * WAVES + 3)                                # one row; a partial round; one row past a round; past the backward's sweep
BIG_FWD = (2048 * WAVES + 3, 64, "float32")                                # past the forward's sweep of 2048 workgroups: forward only
CASES = [(n, H, d) for H in HIDDEN for n in SIZES for d in DTYPES]
FORWARD_OUTPUTS, BACKWARD_OUTPUTS = ("y", "h_next", "c_next"), ("grad_gates", "grad_c_prev", "grad_cell_params")
PARTS = ("bias", "scale", "shift")                                         # of grad_cell_params: 4 H, H and H elements


# ---- the contract, in the type `ft` ----
def fma(ft, x, w, z):
    if ft is np.float64:
        return x * w + z
    return (x.astype(np.float64) * w.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def chan_sum(p):
    """sum over the last axis (H channels) in the header's order; every lane ends with the same bits, lane 0's are taken."""
    s = p[..., :64]
    for q in range(1, p.shape[-1] // 64):
        s = s + p[..., 64 * q:64 * q + 64]
    lane = np.arange(64)
    m = 1
    while m < 64:
        s = s + s[..., lane ^ m]
        m <<= 1
    return s[..., 0]


def sigma(ft, x):
    return ft(1) / (ft(1) + np.exp(-x))


def cell(ft, gates, c_prev, params, H, eps):
    """Everything both calls compute of the rows, in `ft`."""
    gates, c_prev, params = (np.asarray(a).astype(ft) for a in (gates, c_prev, params))
    eps = ft(np.float32(eps))
    z = gates.reshape(-1, 4, H) + params[:4 * H].reshape(4, H)
    i, f, g, o = sigma(ft, z[:, 0]), sigma(ft, z[:, 1]), np.tanh(z[:, 2]), sigma(ft, z[:, 3])
    cn = fma(ft, f, c_prev, i * g)
    tc = np.tanh(cn)
    h = o * tc
    mu = chan_sum(h) / ft(H)
    d = h - mu[:, None]
    var = chan_sum(d * d) / ft(H)
    rstd = ft(1) / np.sqrt(var + eps)
    hhat = d * rstd[:, None]
    out = dict(i=i, f=f, g=g, o=o, cp=c_prev, cn=cn, tc=tc, h=h, rstd=rstd, hhat=hhat, gamma=params[4 * H:5 * H], beta=params[5 * H:])
    assert all(v.dtype == ft for v in out.values())
    return out


def forward(ft, gates, c_prev, params, clear, H, eps=EPS):
    """hs_lstm_cell in float type `ft`: y, h_next, c_next [n, H] (not yet rounded to a narrow dtype)."""
    r = cell(ft, gates, c_prev, params, H, eps)
    keep = np.ones((r["h"].shape[0], 1), bool) if clear is None else (np.asarray(clear).reshape(-1, 1) == 0)
    return dict(y=fma(ft, r["hhat"], r["gamma"], r["beta"]), h_next=np.where(keep, r["h"], ft(0)), c_next=np.where(keep, r["cn"], ft(0)))


def backward(ft, gates, c_prev, params, clear, grad_y, grad_h_next, grad_c_next, H, eps=EPS):
    """hs_lstm_cell_backward in float type `ft`: grad_gates [n, 4 H], grad_c_prev [n, H], grad_cell_params [6 H], the
    parameter sums in the header's order."""
    r = cell(ft, gates, c_prev, params, H, eps)
    n = r["h"].shape[0]
    keep = np.ones((n, 1), bool) if clear is None else (np.asarray(clear).reshape(-1, 1) == 0)
    dy = np.asarray(grad_y).astype(ft)
    gh = np.where(keep, np.asarray(grad_h_next).astype(ft), ft(0)) if grad_h_next is not None else np.zeros((n, H), ft)
    gc = np.where(keep, np.asarray(grad_c_next).astype(ft), ft(0)) if grad_c_next is not None else np.zeros((n, H), ft)
    hb = r["gamma"] * dy
    mh, mhz = chan_sum(hb) / ft(H), chan_sum(hb * r["hhat"]) / ft(H)
    dh = r["rstd"][:, None] * ((hb - mh[:, None]) - r["hhat"] * mhz[:, None]) + gh
    dc = fma(ft, dh * r["o"], ft(1) - r["tc"] * r["tc"], gc)
    one = ft(1)
    dz = [(dc * r["g"]) * (r["i"] * (one - r["i"])), (dc * r["cp"]) * (r["f"] * (one - r["f"])), (dc * r["i"]) * (one - r["g"] * r["g"]),
          (dh * r["tc"]) * (r["o"] * (one - r["o"]))]
    G = min(-(-n // WAVES), MAX_GRID_BWD)
    S = G * WAVES                                           # a row's place among the lanes' sums: row % S, in round row // S
    acc = np.zeros((S, PARAM_ROWS, H), ft)
    for t in range(-(-n // S)):
        rows = slice(t * S, min(n, (t + 1) * S))
        m = rows.stop - rows.start
        for k in range(4):
            acc[:m, k] = acc[:m, k] + dz[k][rows]
        acc[:m, 4] = fma(ft, dy[rows], r["hhat"][rows], acc[:m, 4])
        acc[:m, 5] = acc[:m, 5] + dy[rows]
    acc = acc.reshape(G, WAVES, PARAM_ROWS, H)
    wg = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    per = -(-G // SUM_SEGS)
    total = None
    for sg in range(SUM_SEGS):
        s = np.zeros((PARAM_ROWS, H), ft)
        for blk in range(sg * per, min(G, sg * per + per)):
            s = s + wg[blk]
        total = s if total is None else total + s
    out = dict(grad_gates=np.stack(dz, 1).reshape(n, 4 * H), grad_c_prev=dc * r["f"], grad_cell_params=total.reshape(-1))
    assert all(v.dtype == ft for v in out.values())
    return out


def part_slices(H):
    return {"bias": slice(0, 4 * H), "scale": slice(4 * H, 5 * H), "shift": slice(5 * H, 6 * H)}


# ---- the inputs of the GPU tests ----
@functools.lru_cache(maxsize=None)
def _inputs(n, H, dtype, seed):
    rng = np.random.default_rng([seed, n, H, DTYPES.index(dtype)])
    params = np.concatenate([0.1 * rng.standard_normal(4 * H), 1.0 + 0.2 * rng.standard_normal(H), 0.1 * rng.standard_normal(H)]).astype(np.float32)
    clear = (rng.random(n) < 0.25).astype(np.int32)
    if n >= 3:
        clear[0], clear[1] = 0, 7                            # both kinds of row in every case but n = 1; any nonzero value clears
    x = dict(gates=to_dtype(2.0 * rng.standard_normal((n, 4 * H)), dtype),                 # standard deviation 2: some gates saturate
             c_prev=rng.standard_normal((n, H)).astype(np.float32), params=params, clear=clear,
             grad_y=to_dtype(rng.standard_normal((n, H)), dtype), grad_h_next=to_dtype(rng.standard_normal((n, H)), dtype),
             grad_c_next=rng.standard_normal((n, H)).astype(np.float32))
    for v in x.values():
        v.setflags(write=False)
    return x


def inputs(n, H, dtype, seed=SEED):
    """A fresh dict of the (shared, read-only) arrays of a case: gates and the gradients of y and h_next representable in
    `dtype` (y is requested in the gates' dtype)."""
    return dict(_inputs(n, H, dtype, seed))


def run(ft, x, H, eps=EPS, clear=True, grad_h=True, grad_c=True):
    cl = x["clear"] if clear else None
    out = forward(ft, x["gates"], x["c_prev"], x["params"], cl, H, eps)
    out.update(backward(ft, x["gates"], x["c_prev"], x["params"], cl, x["grad_y"], x["grad_h_next"] if grad_h else None,
                        x["grad_c_next"] if grad_c else None, H, eps))
    return out


@functools.lru_cache(maxsize=None)
def both(case):
    """(f32 restatement, float64 restatement) of a case, forward and backward.  Computed once, shared, left unchanged."""
    x = inputs(*case)
    return run(np.float32, x, case[1]), run(np.float64, x, case[1])


def _gaps(r32, r64, H):
    out = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in FORWARD_OUTPUTS + BACKWARD_OUTPUTS[:2] if k in r32}
    if "grad_cell_params" in r32:
        gap = np.abs(r32["grad_cell_params"].astype(np.float64) - r64["grad_cell_params"])
        out.update({p: float(gap[s].max()) for p, s in part_slices(H).items()})
    return out


@functools.lru_cache(maxsize=None)
def _tolerance(case):
    return tuple(sorted((k, 4.0 * v) for k, v in _gaps(*both(case), case[1]).items()))


def tolerance(case):
    """{output or part: 4 x the largest |f32 - float64| of it in this case}."""
    if case == BIG_FWD:
        x = inputs(*case)
        f32, f64 = (forward(ft, x["gates"], x["c_prev"], x["params"], x["clear"], case[1]) for ft in (np.float32, np.float64))
        return {k: 4.0 * v for k, v in _gaps(f32, f64, case[1]).items()}
    return dict(_tolerance(case))


OUT_DTYPE = {"y": None, "h_next": None, "c_next": "float32", "grad_gates": None, "grad_c_prev": "float32", "grad_cell_params": "float32"}


def bound(name, want, case, tol=None):
    """The bound on |got - want| of output `name` of a case: the derived tolerance plus the rounding of its dtype (y,
    h_next and grad_gates are stored in the case's dtype, the rest in float32)."""
    H, tol = case[1], tolerance(case) if tol is None else tol
    rel, absolute = ROUNDING[OUT_DTYPE[name] or case[2]]
    want = np.asarray(want, np.float64)
    if name == "grad_cell_params":
        t = np.concatenate([np.full(s.stop - s.start, tol[p]) for p, s in part_slices(H).items()])
    else:
        t = tol[name]
    return t + rel * np.abs(want) + absolute


# ---- the module's sequence: the allowance for the GEMMs' dtype and order ----
SEQ = dict(T=3, n=36, F=40, H=64)


@functools.lru_cache(maxsize=None)
def sequence_inputs():
    rng = np.random.default_rng([SEED, 77])
    T, n, F, H = (SEQ[k] for k in "TnFH")
    clears = np.zeros((T, n), np.int32)
    clears[1, ::3] = 1                                       # a clear in the middle for every third row
    x = dict(xs=rng.standard_normal((T, n, F)).astype(np.float32), w_in=(rng.standard_normal((F, 4 * H)) / np.sqrt(F)).astype(np.float32),
             w_rec=(rng.standard_normal((H, 4 * H)) / np.sqrt(H)).astype(np.float32), cell_params=np.array(inputs(1, H, "float32")["params"]),
             h0=(0.5 * rng.standard_normal((n, H))).astype(np.float32), c0=rng.standard_normal((n, H)).astype(np.float32), clears=clears,
             weight=rng.standard_normal((T, n, H)).astype(np.float32))
    for v in x.values():
        v.setflags(write=False)
    return x


def sequence_eager(ft, device="cpu"):
    """recurrent.eager_sequence and its autograd in torch dtype `ft`: ys and the gradients of w_in, w_rec and cell_params
    of loss = sum(ys * weight) + 0.5 * mean(ys^2), as float64 numpy."""
    from gpu_hideseek import recurrent as N
    x = {k: torch.from_numpy(np.array(v)).to(device) for k, v in sequence_inputs().items()}
    leaves = {k: x[k].to(ft).requires_grad_() for k in ("w_in", "w_rec", "cell_params")}
    ys, _ = N.eager_sequence(x["xs"].to(ft), leaves["w_in"], leaves["w_rec"], leaves["cell_params"], (x["h0"].to(ft), x["c0"].to(ft)), x["clears"],
                             float(np.float32(EPS)))
    (ys * x["weight"].to(ft)).sum().add(0.5 * (ys ** 2).mean()).backward()
    out = {"ys": ys.detach()}
    out.update({k: v.grad for k, v in leaves.items()})
    return {k: v.double().cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def sequence_allowance():
    """({quantity: 4 x the largest |torch f32 - torch float64| of it on the CPU}, the float64 results): what a float32
    GEMM in another order of summation may differ by, for the module test on the GPU."""
    f32, f64 = sequence_eager(torch.float32), sequence_eager(torch.float64)
    return {k: 4.0 * float(np.abs(f32[k] - f64[k]).max()) for k in f64}, f64


# ---- tests ----
def test_backward_is_the_gradient_of_the_forward():
    """Central differences of the float64 forward: the function is smooth, so no input is left out."""
    n, H, h = 5, 64, 1e-6
    x = inputs(n, H, "float32")
    w = {k: x[g].astype(np.float64) for k, g in (("y", "grad_y"), ("h_next", "grad_h_next"), ("c_next", "grad_c_next"))}
    base = {k: x[k].astype(np.float64) for k in ("gates", "c_prev", "params")}
    got = backward(np.float64, base["gates"], base["c_prev"], base["params"], x["clear"], w["y"], w["h_next"], w["c_next"], H)
    assert x["clear"].any() and not x["clear"].all()

    def loss(v):
        f = forward(np.float64, v["gates"], v["c_prev"], v["params"], x["clear"], H)
        return float(sum((f[k] * w[k]).sum() for k in w))
    L = abs(loss(base))
    for name, grad in (("gates", got["grad_gates"]), ("c_prev", got["grad_c_prev"]), ("params", got["grad_cell_params"])):
        flat, gmax, worst = grad.reshape(-1), float(np.abs(grad).max()), 0.0
        picks = np.arange(0, flat.size, 7)
        # a central difference errs by the rounding of the two losses over 2 h and by h^2 f''' / 6, here taken as no more
        # than h times the largest gradient
        limit = 16 * 2.0 ** -52 * max(L, 1.0) / h + h * max(gmax, 1.0)
        for i in picks:
            v = {k: a.copy() for k, a in base.items()}
            v[name].reshape(-1)[i] += h
            up = loss(v)
            v[name].reshape(-1)[i] -= 2 * h
            worst = max(worst, abs((up - loss(v)) / (2 * h) - flat[i]))
        print(f"{name}: {picks.size} probed: largest |central difference - backward| = {worst:.3e} (bound {limit:.3e}, largest gradient {gmax:.3e})")
        assert worst <= limit and limit < 1e-3 * gmax


def test_eager_and_its_autograd_are_the_restatement():
    from gpu_hideseek import recurrent as N
    for H in HIDDEN:
        case = (5, H, "float32")
        x = inputs(*case)
        r32, r64 = both(case)
        for ft, scale in ((torch.float64, 1.0), (torch.float32, 4.0)):
            leaves = [torch.from_numpy(np.array(x[k])).to(ft).requires_grad_() for k in ("gates", "c_prev", "params")]
            y, hn, cn = N.eager(leaves[0], leaves[1], leaves[2], torch.from_numpy(np.array(x["clear"])), float(np.float32(EPS)))
            assert y.dtype == ft and y.shape == (5, H)
            (y * torch.from_numpy(np.array(x["grad_y"])).to(ft)).sum().add((hn * torch.from_numpy(np.array(x["grad_h_next"])).to(ft)).sum()).add(
                (cn * torch.from_numpy(np.array(x["grad_c_next"])).to(ft)).sum()).backward()
            got = dict(y=y, h_next=hn, c_next=cn, grad_gates=leaves[0].grad, grad_c_prev=leaves[1].grad, grad_cell_params=leaves[2].grad)
            for k, t in got.items():
                err = np.abs(t.detach().double().numpy() - r64[k])
                if ft is torch.float64:
                    # the same mathematics in another order: float64 rounding through a LayerNorm over H and sums over n rows
                    assert err.max() <= 2.0 ** -52 * 4096 * max(float(np.abs(r64[k]).max()), 1.0), (H, k)
                else:
                    # f32 eager: within the derived bound of the float64 restatement, 4 x for its own, different, order
                    assert (err <= scale * bound(k, r64[k], case)).all(), (H, k, float(err.max()))
        # without a clear and without the optional gradients
        y, hn, cn = N.eager(torch.from_numpy(np.array(x["gates"])).double(), torch.from_numpy(np.array(x["c_prev"])).double(),
                            torch.from_numpy(np.array(x["params"])).double(), None, float(np.float32(EPS)))
        f = forward(np.float64, x["gates"], x["c_prev"], x["params"], None, H)
        assert np.abs(hn.numpy() - f["h_next"]).max() <= 2.0 ** -48 and np.abs(cn.numpy() - f["c_next"]).max() <= 2.0 ** -48


def test_cleared_rows_and_null_gradients_in_the_restatement():
    case = (5, 128, "bfloat16")
    x = inputs(*case)
    r = both(case)[0]
    rows = x["clear"] != 0
    assert rows.any() and not r["h_next"][rows].view(np.uint32).any() and not r["c_next"][rows].view(np.uint32).any()
    free = run(np.float32, x, 128, clear=False)
    assert np.array_equal(free["y"], r["y"]) and free["h_next"][rows].all()          # y does not see the clear
    # a cleared row takes nothing from grad_h_next / grad_c_next; a null gradient is a zero one
    z = dict(x, grad_h_next=np.zeros_like(x["grad_h_next"]), grad_c_next=np.zeros_like(x["grad_c_next"]))
    a, b = run(np.float32, z, 128), run(np.float32, x, 128, grad_h=False, grad_c=False)
    for k in BACKWARD_OUTPUTS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert np.array_equal(r["grad_gates"][rows], a["grad_gates"][rows]) and not np.array_equal(r["grad_gates"][~rows], a["grad_gates"][~rows])
    zero = dict(x, grad_y=np.zeros_like(x["grad_y"]))
    g = run(np.float32, zero, 128, grad_h=False, grad_c=False)
    assert not g["grad_cell_params"].view(np.uint32).any() and not g["grad_gates"].any() and not g["grad_c_prev"].any()


def test_a_clear_in_the_middle_cuts_the_gradient():
    """Three steps in float64 through eager, clears[1] set for every third row: the loss of step 2 reaches the inputs of
    step 0 for the kept rows and not at all for the cleared ones."""
    from gpu_hideseek import recurrent as N
    x = {k: torch.from_numpy(np.array(v)) for k, v in sequence_inputs().items()}
    xs, h0, c0 = x["xs"].double().requires_grad_(), x["h0"].double().requires_grad_(), x["c0"].double().requires_grad_()
    ys, (h, c) = N.eager_sequence(xs, x["w_in"].double(), x["w_rec"].double(), x["cell_params"].double(), (h0, c0), x["clears"], EPS)
    assert ys.shape == (SEQ["T"], SEQ["n"], SEQ["H"]) and ys.dtype == torch.float64
    (ys[2] * x["weight"][2].double()).sum().backward()
    cleared = x["clears"][1] != 0
    assert 0 < int(cleared.sum()) < SEQ["n"]
    for t in (xs.grad[0], xs.grad[1], h0.grad, c0.grad):
        assert not t[cleared].any() and bool((t[~cleared].abs().amax(1) > 0).all())
    assert bool((xs.grad[2].abs().amax(1) > 0).all())
    # the carried state after the clear step is zero, and the final one is not (no clear at step 2)
    _, (h1, c1) = N.eager_sequence(xs[:2], x["w_in"].double(), x["w_rec"].double(), x["cell_params"].double(), (h0, c0), x["clears"][:2], EPS)
    assert not h1[cleared].any() and not c1[cleared].any() and bool(h1[~cleared].any()) and bool(h[cleared].any())


def test_tolerances_are_derived():
    for case in CASES + [BIG_FWD]:
        tol = tolerance(case)
        print(f"lstm cell, n = {case[0]}, H = {case[1]}, {case[2]}: " + ", ".join(f"{k} {v:.3e}" for k, v in tol.items()))
        assert all(v >= 0 for v in tol.values()) and tol["y"] > 0 and tol.get("grad_gates", 1) > 0, case      # shift at n = 1 is grad_y itself: exact
        if case != BIG_FWD:
            r32, r64 = both(case)
            size = float(np.abs(r64["grad_cell_params"]).max())
            # y is a LayerNorm (magnitude up to ~5): a few f32 ulps of h', amplified by rstd; the sums grow with n
            assert tol["y"] < 1e-4 and tol["h_next"] < 1e-5 and tol["c_next"] < 1e-4 and tol["grad_gates"] < 1e-3 and tol["grad_c_prev"] < 1e-3
            assert max(tol[p] for p in PARTS) < 1e-4 * max(size, 1.0), case
            for k in FORWARD_OUTPUTS + BACKWARD_OUTPUTS:
                assert (np.abs(r32[k].astype(np.float64) - r64[k]) <= bound(k, r64[k], case)).all(), (case, k)
    allow, f64 = sequence_allowance()
    print("module sequence, allowance for the float32 GEMMs (4 x max torch f32 - float64): " + ", ".join(f"{k} {v:.3e}" for k, v in allow.items()))
    assert all(0 < allow[k] < 1e-4 * max(float(np.abs(f64[k]).max()), 1.0) for k in allow)
    assert len(CASES) == 48 and SIZES[-1] == 2051 and BIG_FWD[0] == 8195


def test_inputs_are_what_the_issue_describes():
    x = inputs(2051, 256, "bfloat16")
    assert np.array_equal(to_dtype(x["gates"], "bfloat16"), x["gates"]) and np.array_equal(to_dtype(x["grad_y"], "bfloat16"), x["grad_y"])
    assert 1.9 < x["gates"].std() < 2.1 and 0.95 < x["c_prev"].std() < 1.05 and 0.2 < (x["clear"] != 0).mean() < 0.3
    assert x["clear"].dtype == np.int32 and x["c_prev"].dtype == np.float32 and x["params"].shape == (6 * 256,)
    assert all(np.isfinite(v).all() for v in both((5, 64, "float32"))[1].values())


def test_layout_and_init():
    from gpu_hideseek import recurrent as N
    assert (N.PARAM_ROWS, N.MAX_GRID_BWD, N.ROWS_PER_ROUND, N.SUM_SEGS, N.HIDDEN, N.DEFAULT_EPS) == (PARAM_ROWS, MAX_GRID_BWD, WAVES, SUM_SEGS, HIDDEN, EPS)
    for H in HIDDEN:
        flat = torch.arange(PARAM_ROWS * H, dtype=torch.float32)
        v = N.views(flat, H)
        assert list(v) == list(PARTS) and v["bias"].shape == (4, H) and v["scale"].shape == (H,) and v["shift"].shape == (H,)
        for p, s in part_slices(H).items():
            assert np.array_equal(v[p].reshape(-1).numpy(), flat.numpy()[s]) and v[p].data_ptr() == flat.data_ptr() + 4 * s.start
    for bad in (32, 65, 1024, 64.0, True, None):
        with pytest.raises(ValueError, match="hidden"):
            N.param_layout(bad)
    core = N.LSTMCore(40, 64, generator=torch.Generator().manual_seed(1))
    assert [tuple(p.shape) for p in core.parameters()] == [(40, 256), (64, 256), (6 * 64,)]
    for w in (core.w_in, core.w_rec):
        W = w.detach().double()
        assert torch.allclose(W @ W.T, torch.eye(W.shape[0], dtype=torch.float64), atol=1e-5)         # orthonormal rows
    nv = core.named_views()
    assert not nv["bias"].any() and not nv["shift"].any() and bool((nv["scale"] == 1).all())
    h, c = core.init_state(7, "cpu", torch.bfloat16)
    assert h.shape == c.shape == (7, 64) and h.dtype == torch.bfloat16 and c.dtype == torch.float32 and not h.any() and not c.any()
    with pytest.raises(ValueError, match="in_features"):
        N.LSTMCore(0)
    with pytest.raises(ValueError, match="hidden"):
        N.LSTMCore(8, 100)


def test_request_refuses_before_the_library_is_called():
    from gpu_hideseek import recurrent as N

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    n, H = 12, 64
    good = dict(gates=torch.zeros(n, 4 * H), c_prev=torch.zeros(n, H), cell_params=torch.zeros(PARAM_ROWS * H))

    def call(**kw):
        a = dict(good, **kw)
        return N.compute(Sim(), a.pop("gates"), a.pop("c_prev"), a.pop("cell_params"), **a)

    def back(**kw):
        a = dict(dict(good, grad_y=torch.zeros(n, H)), **kw)
        return N.compute_backward(Sim(), a.pop("gates"), a.pop("c_prev"), a.pop("cell_params"), a.pop("grad_y"), **a)

    for f in (call, back):
        for bad, what in ((torch.zeros(n, 4 * H - 1), "shape"), (torch.zeros(n * 4 * H), "shape"), (torch.zeros(0, 4 * H), "shape"),
                          (torch.zeros(n, 4 * H, dtype=torch.float64), "dtype"), (torch.zeros(4 * H, n).t(), "contiguous"),
                          (torch.zeros(n, 8 * H)[:, :4 * H], "contiguous"), (None, "gates")):
            with pytest.raises(ValueError, match=what):
                f(gates=bad)
        for bad, what in ((torch.zeros(n + 1, H), "shape"), (torch.zeros(n, H, dtype=torch.bfloat16), "dtype"), (torch.zeros(n, 2 * H)[:, ::2], "contiguous"),
                          (None, "c_prev")):
            with pytest.raises(ValueError, match=what):
                f(c_prev=bad, hidden=H)
        for bad, what in ((torch.zeros(PARAM_ROWS * H - 1), "shape"), (torch.zeros(PARAM_ROWS, H), "shape"), (torch.zeros(PARAM_ROWS * H, dtype=torch.float64), "dtype"),
                          (torch.zeros(2 * PARAM_ROWS * H)[::2], "contiguous"), (None, "cell_params")):
            with pytest.raises(ValueError, match=what):
                f(cell_params=bad)
        for bad, what in ((torch.zeros(n + 1, dtype=torch.int32), "shape"), (torch.zeros(n, 2, dtype=torch.int32), "shape"), (torch.zeros(n, dtype=torch.int64), "dtype"),
                          (torch.zeros(n), "dtype"), (torch.zeros(2 * n, dtype=torch.int32)[::2], "contiguous"), (3, "clear")):
            with pytest.raises(ValueError, match=what):
                f(clear=bad)
        for bad in (32, 100, 1024, 64.0, True):
            with pytest.raises(ValueError, match="hidden"):
                f(hidden=bad)
        with pytest.raises(ValueError, match="shape"):
            f(hidden=128)
        for v in (float("nan"), float("inf"), 1e39):
            with pytest.raises(ValueError, match="eps must be finite"):
                f(eps=v)
        for v in (0.0, -1e-6, 1e-50):
            with pytest.raises(ValueError, match="eps must be above 0"):
                f(eps=v)
        with pytest.raises(ValueError, match="on cpu"):               # well-formed tensors on the wrong device
            f()
        with pytest.raises(ValueError, match="on cpu"):
            f(clear=torch.zeros(n, 1, dtype=torch.int32))
    for name, bad, what in (("y", torch.zeros(n, H - 1), "shape"), ("y", torch.zeros(n, H, dtype=torch.float64), "dtype"), ("y", torch.zeros(n, 2 * H)[:, ::2], "contiguous"),
                            ("y", 3.0, "y must"), ("h_next", torch.zeros(n, H, dtype=torch.bfloat16), "dtype"), ("h_next", torch.zeros(n + 1, H), "shape"),
                            ("c_next", torch.zeros(n, H, dtype=torch.float16), "dtype"), ("c_next", "yes", "c_next")):
        with pytest.raises(ValueError, match=what):
            call(**{name: bad})
    with pytest.raises(ValueError, match="nothing to do"):
        call(y=None, h_next=None, c_next=False)
    with pytest.raises(ValueError, match="y_dtype"):
        call(y_dtype=torch.float64)
    shared = torch.zeros(n * 5 * H + 64)
    with pytest.raises(ValueError, match="y overlaps gates"):
        call(gates=shared[:n * 4 * H].view(n, 4 * H), y=shared[n:n + n * H].view(n, H))
    with pytest.raises(ValueError, match="c_next overlaps c_prev"):
        call(c_next=good["c_prev"])
    with pytest.raises(ValueError, match="h_next overlaps cell_params"):
        call(cell_params=shared[:PARAM_ROWS * H], h_next=shared[8:8 + n * H].view(n, H))
    with pytest.raises(ValueError, match="h_next overlaps y"):
        call(y=shared[:n * H].view(n, H), h_next=shared[H:H + n * H].view(n, H))
    for name, bad, what in (("grad_y", torch.zeros(n, H + 1), "shape"), ("grad_y", torch.zeros(n, H, dtype=torch.float64), "dtype"),
                            ("grad_y", torch.zeros(n, 2 * H)[:, ::2], "contiguous"), ("grad_y", None, "grad_y"),
                            ("grad_h_next", torch.zeros(n, H, dtype=torch.float16), "dtype"), ("grad_h_next", torch.zeros(n, 1), "shape"), ("grad_h_next", 1.0, "grad_h_next"),
                            ("grad_c_next", torch.zeros(n, H, dtype=torch.bfloat16), "dtype"), ("grad_c_next", torch.zeros(H, n), "shape"),
                            ("grad_gates", torch.zeros(n, H), "shape"), ("grad_gates", torch.zeros(n, 4 * H, dtype=torch.float16), "dtype"),
                            ("grad_c_prev", torch.zeros(n, H, dtype=torch.float64), "dtype"), ("grad_cell_params", torch.zeros(PARAM_ROWS * H + 1), "shape"),
                            ("grad_cell_params", 2, "grad_cell_params")):
        with pytest.raises(ValueError, match=what):
            back(**{name: bad})
    with pytest.raises(ValueError, match="nothing to do"):
        back(grad_gates=None, grad_c_prev=None, grad_cell_params=None)
    with pytest.raises(ValueError, match="grad_cell_params overlaps cell_params"):
        back(grad_cell_params=good["cell_params"])
    with pytest.raises(ValueError, match="grad_gates overlaps gates"):
        back(grad_gates=good["gates"])
    with pytest.raises(ValueError, match="grad_c_prev overlaps grad_y"):
        back(grad_y=shared[:n * H].view(n, H), grad_c_prev=shared[16:16 + n * H].view(n, H))
    with pytest.raises(ValueError, match="grad_c_prev overlaps grad_c_next"):
        g = torch.zeros(n, H)
        back(grad_c_next=g, grad_c_prev=g)


def test_header_states_the_requests(hideseek_lib):
    """include/hideseek.h declares the four entry points, the ctypes mirrors agree with it field by field, and the kernel's
    constants are the module's."""
    from gpu_hideseek import recurrent as N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hideseek.h")).read()
    for name, value in (("HS_LSTM_PARAM_ROWS", PARAM_ROWS), ("HS_LSTM_MAX_GRID_BWD", MAX_GRID_BWD), ("HS_LSTM_MAX_HIDDEN", max(HIDDEN)),
                        ("HS_LSTM_ROWS_PER_ROUND", WAVES), ("HS_EMBED_SUM_SEGS", SUM_SEGS)):
        assert re.search(rf"{name} = (\d+)", src).group(1) == str(value), name
    for fn, req in (("hs_lstm_cell", "hs_lstm_cell_request"), ("hs_lstm_cell_backward", "hs_lstm_cell_backward_request")):
        assert re.search(rf"int32_t {fn}\(hs_sim \*\w*, const {req} \*\w*\);", src)
        assert re.search(rf"int32_t {fn}_async\(hs_sim \*\w*, void \*hip_stream, const {req} \*\w*\);", src)
    for req, mirror in (("hs_lstm_cell_request", N.HsLstmCellRequest), ("hs_lstm_cell_backward_request", N.HsLstmCellBackwardRequest)):
        body = re.search(rf"typedef struct {req} \{{(.*?)\}} {req};", src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            if decl.strip():
                for word in ("const", "int32_t", "uint8_t", "float", "void"):
                    decl = re.sub(rf"\b{word}\b", "", decl)
                names += [part.split()[-1].lstrip("*") for part in decl.split(",")]
        assert names == [f[0] for f in mirror._fields_], names
    F, B = N.HsLstmCellRequest, N.HsLstmCellBackwardRequest
    assert C.sizeof(F) == 80 and F.clear.offset == 24 and F.n.offset == 32 and F.y_dtype.offset == 44 and F.eps.offset == 48 and F.y.offset == 56 and F.c_next.offset == 72
    assert C.sizeof(B) == 104 and B.grad_y.offset == 32 and B.grad_c_next.offset == 48 and B.n.offset == 56 and B.y_dtype.offset == 68 and B.eps.offset == 72
    assert B.grad_gates.offset == 80 and B.grad_cell_params.offset == 96
    lib = C.CDLL(hideseek_lib)
    for fn in ("hs_lstm_cell", "hs_lstm_cell_async", "hs_lstm_cell_backward", "hs_lstm_cell_backward_async"):
        assert hasattr(lib, fn)
    csrc = os.path.join(root, "marl-hideandseek_amd", "csrc")
    kernel, shared, host = (open(os.path.join(csrc, f)).read() for f in ("hs_k_lstm.h", "hs_rows.h", "hideseek.hip"))
    assert int(re.search(r"kLstmParamRows = (\d+);", kernel).group(1)) == PARAM_ROWS and int(re.search(r"kLstmMaxH = (\d+);", kernel).group(1)) == max(HIDDEN)
    # the grid caps, the workgroup and the segments are the ones every row-wise kernel shares (hs_rows.h)
    assert '#include "hs_rows.h"' in kernel and "HS_LSTM_MAX_GRID_BWD == hs::kRowsMaxGridBwd" in host and "HS_LSTM_ROWS_PER_ROUND == hs::kRowsWaves" in host
    assert int(re.search(r"kRowsMaxGridBwd = (\d+);", shared).group(1)) == MAX_GRID_BWD and int(re.search(r"kRowsSumSegs = (\d+),", shared).group(1)) == SUM_SEGS
    assert "kRowsWaves = kRowsThreads / 64" in shared and int(re.search(r"kRowsThreads = (\d+)", shared).group(1)) == 64 * WAVES
