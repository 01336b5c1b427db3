"""The dense layer after its GEMM without a GPU (gpu_hideseek.mlp, hs_dense_norm_act / hs_dense_norm_act_backward) and
the policy modules as far as they go without a kernel: a numpy restatement of what include/hideseek.h states, forward and
backward, once in f32 in the header's order (the backward including rounds, waves, workgroups and the eight segments of
the parameter sums) and once in float64; the float64 backward against central differences on inputs that stay clear of
the leaky ReLU's kink; mlp.eager and its autograd against both; the tolerances the GPU tests use, derived from the two
restatements on the GPU tests' own cases; the refusals of request(); the header; and gpu_hideseek.policy with eager
pieces on the CPU.

numpy has no fmaf: fmaf(x, w, z) is taken as the f32 rounding of x * w + z evaluated in the widest float numpy has (80-bit
extended where the platform has it: the product of two f32 is exact in it, and a double rounding needs a sum within
2^-40 of a tie).  Division and sqrt in numpy's f32 are correctly rounded, as the device's are, and nothing else is
involved: the f32 restatement is meant to be the kernel's f32 y bit for bit.

Tolerances (printed by test_tolerances_are_derived; DESIGN.md quotes them), none a constant: per case (n, C, dtype) and
per output (y, grad_z, and bias / scale / shift of grad_params) 4 x (the project's margin, as in test_lstm_cell_host) the
largest deviation of the f32 restatement from the float64 one, plus the rounding of the output's dtype (ROUNDING: half an
ulp relative, the smallest subnormal absolute).
"""
import copy
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_lstm_cell_host import DTYPES, ROUNDING, to_dtype

CHANNELS = (64, 128, 256, 512)
PARAM_ROWS, WAVES, MAX_GRID_BWD, SUM_SEGS = 3, 4, 512, 8                   # asserted against module and header below
EPS, SLOPE = 1e-6, 0.01
SEED = 0
SIZES = (1, 3, 5, MAX_GRID_BWD * WAVES + 3)                                # one row; a partial round; one row past a round; past the backward's sweep
BIG_FWD = (2048 * WAVES + 3, 64, "float32")                                # past the forward's sweep of 2048 workgroups: forward only
CASES = [(n, Cn, d) for Cn in CHANNELS for n in SIZES for d in DTYPES]
OUTPUTS = ("y", "grad_z", "grad_params")
PARTS = ("bias", "scale", "shift")                                         # of grad_params: C elements each
WIDE = np.longdouble if np.finfo(np.longdouble).nmant > 52 else np.float64


# ---- the contract, in the type `ft` ----
def fma(ft, x, w, z):
    if ft is np.float64:
        return x * w + z
    return (x.astype(WIDE) * w.astype(WIDE) + z.astype(WIDE)).astype(np.float32)


def chan_sum(p):
    """sum over the last axis (C channels) in the header's order: lane l adds its V = C / 64 adjacent channels in
    ascending order, then the butterfly; every lane ends with the same bits, lane 0's are taken."""
    V = p.shape[-1] // 64
    q = p.reshape(p.shape[:-1] + (64, V))
    s = q[..., 0]
    for k in range(1, V):
        s = s + q[..., k]
    lane = np.arange(64)
    m = 1
    while m < 64:
        s = s + s[..., lane ^ m]
        m <<= 1
    return s[..., 0]


def row(ft, z, params, Cn, eps):
    """Everything both calls compute of the rows, in `ft`."""
    z, params = np.asarray(z).astype(ft), np.asarray(params).astype(ft)
    eps = ft(np.float32(eps))
    bias, gamma, beta = params[:Cn], params[Cn:2 * Cn], params[2 * Cn:]
    a = z + bias
    mu = chan_sum(a) / ft(Cn)
    d = a - mu[:, None]
    var = chan_sum(d * d) / ft(Cn)
    rstd = ft(1) / np.sqrt(var + eps)
    h = d * rstd[:, None]
    u = fma(ft, np.broadcast_to(gamma, h.shape), h, np.broadcast_to(beta, h.shape))
    out = dict(h=h, u=u, rstd=rstd, gamma=gamma)
    assert all(v.dtype == ft for v in out.values())
    return out


def forward(ft, z, params, Cn, eps=EPS, slope=SLOPE):
    """hs_dense_norm_act in float type `ft`: y [n, C] (not yet rounded to a narrow dtype)."""
    r = row(ft, z, params, Cn, eps)
    return dict(y=np.where(r["u"] > 0, r["u"], ft(np.float32(slope)) * r["u"]))


def backward(ft, z, params, grad_y, Cn, eps=EPS, slope=SLOPE):
    """hs_dense_norm_act_backward in float type `ft`: grad_z [n, C] and grad_params [3 C], the parameter sums in the
    header's order."""
    r = row(ft, z, params, Cn, eps)
    n = r["h"].shape[0]
    g = np.asarray(grad_y).astype(ft)
    du = np.where(r["u"] > 0, g, ft(np.float32(slope)) * g)
    dh = du * r["gamma"]
    m1, m2 = chan_sum(dh) / ft(Cn), chan_sum(dh * r["h"]) / ft(Cn)
    da = r["rstd"][:, None] * ((dh - m1[:, None]) - r["h"] * m2[:, None])
    G = min(-(-n // WAVES), MAX_GRID_BWD)
    S = G * WAVES                                           # a row's place among the lanes' sums: row % S, in round row // S
    acc = np.zeros((S, PARAM_ROWS, Cn), ft)
    for t in range(-(-n // S)):
        rows = slice(t * S, min(n, (t + 1) * S))
        m = rows.stop - rows.start
        acc[:m, 0] = acc[:m, 0] + da[rows]
        acc[:m, 1] = fma(ft, du[rows], r["h"][rows], acc[:m, 1])
        acc[:m, 2] = acc[:m, 2] + du[rows]
    acc = acc.reshape(G, WAVES, PARAM_ROWS, Cn)
    wg = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    per = -(-G // SUM_SEGS)
    total = None
    for sg in range(SUM_SEGS):
        s = np.zeros((PARAM_ROWS, Cn), ft)
        for blk in range(sg * per, min(G, sg * per + per)):
            s = s + wg[blk]
        total = s if total is None else total + s
    out = dict(grad_z=da, grad_params=total.reshape(-1))
    assert all(v.dtype == ft for v in out.values())
    return out


def part_slices(Cn):
    return {"bias": slice(0, Cn), "scale": slice(Cn, 2 * Cn), "shift": slice(2 * Cn, 3 * Cn)}


# ---- the inputs of the GPU tests ----
@functools.lru_cache(maxsize=None)
def _inputs(n, Cn, dtype, seed):
    rng = np.random.default_rng([seed, n, Cn, DTYPES.index(dtype), 5])
    params = np.concatenate([0.1 * rng.standard_normal(Cn), 1.0 + 0.2 * rng.standard_normal(Cn), 0.1 * rng.standard_normal(Cn)]).astype(np.float32)
    # a GEMM's result: each row has its own offset and scale, so that mu and rstd differ from row to row
    z = rng.standard_normal((n, Cn)) * (0.5 + rng.random((n, 1))) + 0.5 * rng.standard_normal((n, 1))
    x = dict(z=to_dtype(z, dtype), params=params, grad_y=to_dtype(rng.standard_normal((n, Cn)), dtype))
    for v in x.values():
        v.setflags(write=False)
    return x


def inputs(n, Cn, dtype, seed=SEED):
    """A fresh dict of the (shared, read-only) arrays of a case: z and grad_y representable in `dtype` (y is requested in
    z's dtype)."""
    return dict(_inputs(n, Cn, dtype, seed))


def run(ft, x, Cn, eps=EPS, slope=SLOPE):
    out = forward(ft, x["z"], x["params"], Cn, eps, slope)
    out.update(backward(ft, x["z"], x["params"], x["grad_y"], Cn, eps, slope))
    return out


@functools.lru_cache(maxsize=None)
def both(case):
    """(f32 restatement, float64 restatement) of a case, forward and backward.  Computed once, shared, left unchanged."""
    x = inputs(*case)
    return run(np.float32, x, case[1]), run(np.float64, x, case[1])


def gaps(r32, r64, Cn):
    out = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in ("y", "grad_z") if k in r32}
    if "grad_params" in r32:
        gap = np.abs(r32["grad_params"].astype(np.float64) - r64["grad_params"])
        out.update({p: float(gap[s].max()) for p, s in part_slices(Cn).items()})
    return out


@functools.lru_cache(maxsize=None)
def _tolerance(case):
    return tuple(sorted((k, 4.0 * v) for k, v in gaps(*both(case), case[1]).items()))


def tolerance(case):
    """{output or part: 4 x the largest |f32 - float64| of it in this case}."""
    if case == BIG_FWD:
        x = inputs(*case)
        f32, f64 = (forward(ft, x["z"], x["params"], case[1]) for ft in (np.float32, np.float64))
        return {k: 4.0 * v for k, v in gaps(f32, f64, case[1]).items()}
    return dict(_tolerance(case))


OUT_DTYPE = {"y": None, "grad_z": None, "grad_params": "float32"}


def bound(name, want, case, tol=None):
    """The bound on |got - want| of output `name` of a case: the derived tolerance plus the rounding of its dtype (y and
    grad_z are stored in the case's dtype, grad_params in float32)."""
    Cn, tol = case[1], tolerance(case) if tol is None else tol
    rel, absolute = ROUNDING[OUT_DTYPE[name] or case[2]]
    want = np.asarray(want, np.float64)
    t = np.concatenate([np.full(Cn, tol[p]) for p in PARTS]) if name == "grad_params" else tol[name]
    return t + rel * np.abs(want) + absolute


# ---- the modules: the allowance for the GEMMs' dtype and order ----
MODULE = dict(n=36, F=40, C=64, layers=3)


@functools.lru_cache(maxsize=None)
def module_inputs():
    rng = np.random.default_rng([SEED, 78])
    n, F, Cn = MODULE["n"], MODULE["F"], MODULE["C"]
    x = dict(x=rng.standard_normal((n, F)).astype(np.float32), weight=rng.standard_normal((n, Cn)).astype(np.float32))
    for v in x.values():
        v.setflags(write=False)
    return x


def module_net(fused, device="cpu"):
    """mlp.MLP(F, C, layers) with the parameters every test of the module shares: the seeded he-normal weights, and
    biases, scales and shifts off their initial 0 / 1 / 0 so that their gradients matter."""
    from gpu_hideseek import mlp as M
    net = M.MLP(MODULE["F"], MODULE["C"], MODULE["layers"], fused=fused, generator=torch.Generator().manual_seed(11))
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for layer in net.layers:
            v = layer.named_views()
            v["bias"].copy_(0.1 * torch.randn(MODULE["C"], generator=g))
            v["scale"].copy_(1.0 + 0.2 * torch.randn(MODULE["C"], generator=g))
            v["shift"].copy_(0.1 * torch.randn(MODULE["C"], generator=g))
    return net.to(device)


def module_eager(ft, device="cpu"):
    """MLP(fused=False) and its autograd in torch dtype `ft`: y and every parameter's gradient of
    loss = sum(y * weight) + 0.5 * mean(y^2), as float64 numpy."""
    net = module_net(False, device).to(ft)
    x = {k: torch.from_numpy(np.array(v)).to(device).to(ft) for k, v in module_inputs().items()}
    y = net(None, x["x"])
    (y * x["weight"]).sum().add(0.5 * (y ** 2).mean()).backward()
    out = {"y": y.detach()}
    out.update({k: p.grad for k, p in net.named_parameters()})
    return {k: v.double().cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def module_allowance():
    """({quantity: 4 x the largest |torch f32 - torch float64| of it on the CPU}, the float64 results): what float32
    GEMMs in another order of summation may differ by, for the module test on the GPU."""
    f32, f64 = module_eager(torch.float32), module_eager(torch.float64)
    return {k: 4.0 * float(np.abs(f32[k] - f64[k]).max()) for k in f64}, f64


# ---- tests: the kernel's contract ----
KINK_MARGIN = 1e-3                                           # every |u_c| of the probed inputs is above it: 1000 steps h


def _clear_of_the_kink(n, Cn):
    """The first seed whose inputs have every |u_c| above KINK_MARGIN."""
    for seed in range(1, 200):
        x = inputs(n, Cn, "float32", seed)
        if float(np.abs(row(np.float64, x["z"], x["params"], Cn, EPS)["u"]).min()) > KINK_MARGIN:
            return x
    raise AssertionError("no seed keeps every u clear of the kink")


def test_backward_is_the_gradient_of_the_forward():
    """Central differences of the float64 forward.  The leaky ReLU has a kink at u = 0: the inputs have every |u_c| above
    KINK_MARGIN (asserted), and a step of h = 1e-6 in one input moves no u by more than a small multiple of h, so no
    difference straddles it."""
    n, Cn, h = 5, 64, 1e-6
    x = _clear_of_the_kink(n, Cn)
    base = {k: x[k].astype(np.float64) for k in ("z", "params")}
    w = x["grad_y"].astype(np.float64)
    r = row(np.float64, base["z"], base["params"], Cn, EPS)
    umin = float(np.abs(r["u"]).min())
    # du/dz is at most |gamma| rstd (1 + |h|^2 / C) and du/dparams at most max(1, |h|, |gamma| rstd ...): bounded by 4 rstd max|gamma| + |h|
    reach = h * (4.0 * float(r["rstd"].max()) * float(np.abs(r["gamma"]).max()) + float(np.abs(r["h"]).max()) + 1.0)
    print(f"smallest |u| = {umin:.3e} (margin {KINK_MARGIN:.0e}); a step moves u by at most {reach:.3e}")
    assert umin > KINK_MARGIN > 10 * reach and (r["u"] > 0).any() and (r["u"] < 0).any()
    got = backward(np.float64, base["z"], base["params"], w, Cn)

    def loss(v):
        return float((forward(np.float64, v["z"], v["params"], Cn)["y"] * w).sum())
    L = abs(loss(base))
    for name, grad in (("z", got["grad_z"]), ("params", got["grad_params"])):
        flat, gmax, worst = grad.reshape(-1), float(np.abs(grad).max()), 0.0
        picks = np.arange(0, flat.size, 3)
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
    from gpu_hideseek import mlp as M
    for Cn in CHANNELS:
        case = (5, Cn, "float32")
        x = inputs(*case)
        r32, r64 = both(case)
        for ft in (torch.float64, torch.float32):
            z, p = (torch.from_numpy(np.array(x[k])).to(ft).requires_grad_() for k in ("z", "params"))
            y = M.eager(z, p, float(np.float32(EPS)), float(np.float32(SLOPE)))
            assert y.dtype == ft and y.shape == (5, Cn)
            (y * torch.from_numpy(np.array(x["grad_y"])).to(ft)).sum().backward()
            for k, t in dict(y=y, grad_z=z.grad, grad_params=p.grad).items():
                err = np.abs(t.detach().double().numpy() - r64[k])
                if ft is torch.float64:
                    # the same mathematics in another order: float64 rounding through a LayerNorm over C and sums over n rows
                    assert err.max() <= 2.0 ** -52 * 4096 * max(float(np.abs(r64[k]).max()), 1.0), (Cn, k)
                else:
                    # f32 eager: within the derived bound of the float64 restatement, 4 x for its own, different, order
                    assert (err <= 4.0 * bound(k, r64[k], case)).all(), (Cn, k, float(err.max()))
        # z in a narrow dtype, params in float32: eager computes in the dtype of params
        y = M.eager(torch.from_numpy(np.array(x["z"])).bfloat16(), torch.from_numpy(np.array(x["params"])))
        assert y.dtype == torch.float32


def test_special_rows_in_the_restatement():
    Cn = 128
    x = inputs(5, Cn, "bfloat16")
    # an all-zero grad_y: every parameter sum is +0, grad_z is zero
    g = run(np.float32, dict(x, grad_y=np.zeros_like(x["grad_y"])), Cn)
    assert not g["grad_params"].view(np.uint32).any() and not g["grad_z"].any()
    # a constant row (var = 0): h = 0, y = leaky(beta) exactly, finite gradients
    z = np.array(x["z"])
    z[2] = 1.5
    p = np.array(x["params"])
    p[:Cn] = 0.25                                            # a constant bias keeps the row constant
    r = run(np.float32, dict(x, z=z, params=p), Cn)
    beta = p[2 * Cn:]
    assert np.array_equal(r["y"][2], np.where(beta > 0, beta, np.float32(SLOPE) * beta)) and all(np.isfinite(v).all() for v in r.values())
    # channels with gamma = beta = 0 give +0
    p = np.array(x["params"])
    p[Cn + 3], p[2 * Cn + 3], p[Cn + 64], p[2 * Cn + 64] = 0, 0, 0, 0
    y = forward(np.float32, x["z"], p, Cn)["y"]
    assert (y[:, [3, 64]] == 0).all() and y.any()
    # slope 0, 0.2 and 1: the negative side scales, the positive side stays
    y0, y2, y1 = (forward(np.float32, x["z"], x["params"], Cn, slope=s)["y"] for s in (0.0, 0.2, 1.0))
    u = row(np.float32, x["z"], x["params"], Cn, EPS)["u"]
    assert np.array_equal(y1, u) and np.array_equal(y0, np.where(u > 0, u, np.float32(0) * u)) and np.array_equal(y2[u > 0], u[u > 0]) and (u < 0).any()


def test_tolerances_are_derived():
    for case in CASES + [BIG_FWD]:
        tol = tolerance(case)
        print(f"dense layer, n = {case[0]}, C = {case[1]}, {case[2]}: " + ", ".join(f"{k} {v:.3e}" for k, v in tol.items()))
        assert all(v >= 0 for v in tol.values()) and tol["y"] > 0 and tol.get("grad_z", 1) > 0, case          # shift at n = 1 is du itself: exact
        if case != BIG_FWD:
            r32, r64 = both(case)
            size = float(np.abs(r64["grad_params"]).max())
            # y is a LayerNorm (magnitude up to ~5): a few f32 ulps; grad_z carries rstd; the sums grow with n
            assert tol["y"] < 1e-4 and tol["grad_z"] < 1e-3
            assert max(tol[p] for p in PARTS) < 1e-4 * max(size, 1.0), case
            for k in OUTPUTS:
                assert (np.abs(r32[k].astype(np.float64) - r64[k]) <= bound(k, r64[k], case)).all(), (case, k)
    allow, f64 = module_allowance()
    print("MLP module, allowance for the float32 GEMMs (4 x max torch f32 - float64): " + ", ".join(f"{k} {v:.3e}" for k, v in allow.items()))
    assert all(0 < allow[k] < 1e-4 * max(float(np.abs(f64[k]).max()), 1.0) for k in allow)
    assert len(CASES) == 48 and SIZES[-1] == 2051 and BIG_FWD[0] == 8195


def test_inputs_are_what_the_issue_describes():
    x = inputs(2051, 256, "bfloat16")
    assert np.array_equal(to_dtype(x["z"], "bfloat16"), x["z"]) and np.array_equal(to_dtype(x["grad_y"], "bfloat16"), x["grad_y"])
    assert x["params"].dtype == np.float32 and x["params"].shape == (3 * 256,) and 0.5 < x["z"].std() < 2.0
    u = row(np.float32, x["z"], x["params"], 256, EPS)["u"]
    assert 0.3 < (u > 0).mean() < 0.7                        # both branches of the leaky ReLU, in numbers
    assert all(np.isfinite(v).all() for v in both((5, 64, "float32"))[1].values())


def test_layout_and_init():
    from gpu_hideseek import mlp as M
    assert (M.PARAM_ROWS, M.MAX_GRID_BWD, M.ROWS_PER_ROUND, M.SUM_SEGS, M.CHANNELS, M.DEFAULT_EPS, M.DEFAULT_SLOPE, M.ALIGN) == (
        PARAM_ROWS, MAX_GRID_BWD, WAVES, SUM_SEGS, CHANNELS, EPS, SLOPE, 16)
    from gpu_hideseek import recurrent
    assert M.CHANNELS == recurrent.HIDDEN
    for Cn in CHANNELS:
        flat = torch.arange(PARAM_ROWS * Cn, dtype=torch.float32)
        v = M.views(flat, Cn)
        assert list(v) == list(PARTS) and all(t.shape == (Cn,) for t in v.values())
        for p, s in part_slices(Cn).items():
            assert np.array_equal(v[p].numpy(), flat.numpy()[s]) and v[p].data_ptr() == flat.data_ptr() + 4 * s.start
        p = M.init_params(Cn)
        pv = M.views(p, Cn)
        assert p.dtype == torch.float32 and not pv["bias"].any() and not pv["shift"].any() and bool((pv["scale"] == 1).all())
    for bad in (32, 65, 1024, 64.0, True, None):
        with pytest.raises(ValueError, match="channels"):
            M.param_layout(bad)
    layer = M.DenseNormAct(512, 256, generator=torch.Generator().manual_seed(1))
    assert [(k, tuple(p.shape)) for k, p in layer.named_parameters()] == [("weight", (512, 256)), ("params", (3 * 256,))]
    std = float(layer.weight.detach().std())
    assert abs(std - (2.0 / 512) ** 0.5) < 0.02 * (2.0 / 512) ** 0.5, std            # he-normal: 131 072 draws, 0.2 % standard error
    net = M.MLP(40, 64, 3)
    assert [tuple(p.shape) for p in net.parameters()] == [(40, 64), (192,), (64, 64), (192,), (64, 64), (192,)] and net.fused
    assert not M.MLP(40, 64, 2, fused=False).fused
    for kw, what in ((dict(in_features=0), "in_features"), (dict(channels=100), "channels"), (dict(layers=0), "layers")):
        with pytest.raises(ValueError, match=what):
            M.MLP(**dict(dict(in_features=8, channels=64, layers=1), **kw))


def test_request_refuses_before_the_library_is_called():
    from gpu_hideseek import mlp as M

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    n, Cn = 12, 64
    good = dict(z=torch.zeros(n, Cn), params=torch.zeros(PARAM_ROWS * Cn))

    def call(**kw):
        a = dict(good, **kw)
        return M.compute(Sim(), a.pop("z"), a.pop("params"), **a)

    def back(**kw):
        a = dict(dict(good, grad_y=torch.zeros(n, Cn)), **kw)
        return M.compute_backward(Sim(), a.pop("z"), a.pop("params"), a.pop("grad_y"), **a)

    def off(dtype=torch.float32, by=1):
        """A contiguous [n, C] view that starts `by` elements into its allocation: not 16-byte aligned."""
        t = torch.zeros(n * Cn + 8, dtype=dtype)[by:by + n * Cn].view(n, Cn)
        assert t.is_contiguous() and t.data_ptr() % 16
        return t

    for f in (call, back):
        for bad, what in ((torch.zeros(n, Cn - 1), "channels"), (torch.zeros(n * Cn), "shape"), (torch.zeros(0, Cn), "shape"),
                          (torch.zeros(n, Cn, dtype=torch.float64), "dtype"), (torch.zeros(Cn, n).t(), "contiguous"),
                          (torch.zeros(n, 2 * Cn)[:, :Cn], "contiguous"), (None, "z must"), (off(), "16-byte aligned"), (off(torch.bfloat16, 3), "16-byte aligned"),
                          (off(torch.float16, 4), "16-byte aligned")):
            with pytest.raises(ValueError, match=what):
                f(z=bad)
        with pytest.raises(ValueError, match="shape"):
            f(channels=128)
        for bad, what in ((torch.zeros(PARAM_ROWS * Cn - 1), "shape"), (torch.zeros(PARAM_ROWS, Cn), "shape"), (torch.zeros(PARAM_ROWS * Cn, dtype=torch.float64), "dtype"),
                          (torch.zeros(2 * PARAM_ROWS * Cn)[::2], "contiguous"), (None, "params")):
            with pytest.raises(ValueError, match=what):
                f(params=bad)
        for bad in (32, 100, 1024, 64.0, True):
            with pytest.raises(ValueError, match="channels"):
                f(channels=bad)
        for v in (float("nan"), float("inf"), 1e39):
            with pytest.raises(ValueError, match="eps must be finite"):
                f(eps=v)
        for v in (0.0, -1e-6, 1e-50):
            with pytest.raises(ValueError, match="eps must be above 0"):
                f(eps=v)
        for v in (float("nan"), float("inf"), -0.01, 1.5, -1e39):
            with pytest.raises(ValueError, match="slope must be finite and in"):
                f(slope=v)
        with pytest.raises(ValueError, match="on cpu"):               # well-formed tensors on the wrong device
            f()
        with pytest.raises(ValueError, match="on cpu"):
            f(slope=0.0, eps=1e-3)
    for bad, what in ((torch.zeros(n, Cn - 1), "shape"), (torch.zeros(n, Cn, dtype=torch.float64), "dtype"), (torch.zeros(n, 2 * Cn)[:, ::2], "contiguous"),
                      (3.0, "y must"), (off(), "16-byte aligned"), (off(torch.bfloat16), "16-byte aligned")):
        with pytest.raises(ValueError, match=what):
            call(y=bad)
    for none in (None, False):
        with pytest.raises(ValueError, match="nothing to do"):
            call(y=none)
    with pytest.raises(ValueError, match="y_dtype"):
        call(y_dtype=torch.float64)
    shared = torch.zeros(n * 2 * Cn + 64)
    with pytest.raises(ValueError, match="y overlaps z"):
        call(z=shared[:n * Cn].view(n, Cn), y=shared[Cn:Cn + n * Cn].view(n, Cn))
    with pytest.raises(ValueError, match="y overlaps z"):
        call(y=good["z"])
    with pytest.raises(ValueError, match="y overlaps params"):
        call(params=shared[:PARAM_ROWS * Cn], y=shared[8:8 + n * Cn].view(n, Cn))
    for name, bad, what in (("grad_y", torch.zeros(n, Cn + 1), "shape"), ("grad_y", torch.zeros(n, Cn, dtype=torch.float64), "dtype"),
                            ("grad_y", torch.zeros(n, 2 * Cn)[:, ::2], "contiguous"), ("grad_y", None, "grad_y"), ("grad_y", off(), "16-byte aligned"),
                            ("grad_z", torch.zeros(n + 1, Cn), "shape"), ("grad_z", torch.zeros(n, Cn, dtype=torch.float16), "dtype"), ("grad_z", off(), "16-byte aligned"),
                            ("grad_params", torch.zeros(PARAM_ROWS * Cn + 1), "shape"), ("grad_params", torch.zeros(PARAM_ROWS * Cn, dtype=torch.float64), "dtype"),
                            ("grad_params", 2, "grad_params")):
        with pytest.raises(ValueError, match=what):
            back(**{name: bad})
    with pytest.raises(ValueError, match="nothing to do"):
        back(grad_z=None, grad_params=None)
    with pytest.raises(ValueError, match="grad_params overlaps params"):
        back(grad_params=good["params"])
    with pytest.raises(ValueError, match="grad_z overlaps z"):
        back(grad_z=good["z"])
    with pytest.raises(ValueError, match="grad_z overlaps grad_y"):
        back(grad_y=shared[:n * Cn].view(n, Cn), grad_z=shared[16:16 + n * Cn].view(n, Cn))


def test_header_states_the_requests(hideseek_lib):
    """include/hideseek.h declares the four entry points, the ctypes mirrors agree with it field by field, and the kernel's
    constants are the module's."""
    from gpu_hideseek import mlp as M
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hideseek.h")).read()
    for name, value in (("HS_DENSE_PARAM_ROWS", PARAM_ROWS), ("HS_DENSE_MAX_GRID_BWD", MAX_GRID_BWD), ("HS_DENSE_MAX_CHANNELS", max(CHANNELS)),
                        ("HS_DENSE_ROWS_PER_ROUND", WAVES), ("HS_EMBED_SUM_SEGS", SUM_SEGS)):
        assert re.search(rf"{name} = (\d+)", src).group(1) == str(value), name
    for fn, req in (("hs_dense_norm_act", "hs_dense_norm_act_request"), ("hs_dense_norm_act_backward", "hs_dense_norm_act_backward_request")):
        assert re.search(rf"int32_t {fn}\(hs_sim \*\w*, const {req} \*\w*\);", src)
        assert re.search(rf"int32_t {fn}_async\(hs_sim \*\w*, void \*hip_stream, const {req} \*\w*\);", src)
    for req, mirror in (("hs_dense_norm_act_request", M.HsDenseNormActRequest), ("hs_dense_norm_act_backward_request", M.HsDenseNormActBackwardRequest)):
        body = re.search(rf"typedef struct {req} \{{(.*?)\}} {req};", src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            if decl.strip():
                for word in ("const", "int32_t", "uint8_t", "float", "void"):
                    decl = re.sub(rf"\b{word}\b", "", decl)
                names += [part.split()[-1].lstrip("*") for part in decl.split(",")]
        assert names == [f[0] for f in mirror._fields_], names
    F, B = M.HsDenseNormActRequest, M.HsDenseNormActBackwardRequest
    assert C.sizeof(F) == 48 and F.params.offset == 8 and F.n.offset == 16 and F.y_dtype.offset == 28 and F.eps.offset == 32 and F.slope.offset == 36 and F.y.offset == 40
    assert C.sizeof(B) == 64 and B.grad_y.offset == 16 and B.n.offset == 24 and B.y_dtype.offset == 36 and B.eps.offset == 40 and B.slope.offset == 44
    assert B.grad_z.offset == 48 and B.grad_params.offset == 56
    lib = C.CDLL(hideseek_lib)
    for fn in ("hs_dense_norm_act", "hs_dense_norm_act_async", "hs_dense_norm_act_backward", "hs_dense_norm_act_backward_async"):
        assert hasattr(lib, fn)
    # the stated defaults: eps and slope in the header's text
    assert "eps = 1e-6 and slope = 0.01" in src
    csrc = os.path.join(root, "marl-hideandseek_amd", "csrc")
    kernel, shared, host = (open(os.path.join(csrc, f)).read() for f in ("hs_k_dense.h", "hs_rows.h", "hideseek.hip"))
    assert int(re.search(r"kDenseParamRows = (\d+);", kernel).group(1)) == PARAM_ROWS and int(re.search(r"kDenseMaxC = (\d+);", kernel).group(1)) == max(CHANNELS)
    # the grid caps, the workgroup and the segments are the ones every row-wise kernel shares (hs_rows.h)
    assert '#include "hs_rows.h"' in kernel and "HS_DENSE_MAX_GRID_BWD == hs::kRowsMaxGridBwd" in host and "HS_DENSE_ROWS_PER_ROUND == hs::kRowsWaves" in host
    assert int(re.search(r"kRowsMaxGridBwd = (\d+);", shared).group(1)) == MAX_GRID_BWD and int(re.search(r"kRowsSumSegs = (\d+),", shared).group(1)) == SUM_SEGS
    assert "kRowsWaves = kRowsThreads / 64" in shared and int(re.search(r"kRowsThreads = (\d+)", shared).group(1)) == 64 * WAVES


# ---- the policy modules on the CPU, with eager pieces ----
POLICY = dict(T=3, n=36, W=296)


@functools.lru_cache(maxsize=None)
def policy_rows():
    """Random rows [T, n, 296] for the actor and the critic and clears with an episode's end in the middle."""
    rng = np.random.default_rng([SEED, 79])
    T, n, W = (POLICY[k] for k in "TnW")
    clears = np.zeros((T, n), np.int32)
    clears[1, ::3] = 1
    x = dict(actor=rng.standard_normal((T, n, W)).astype(np.float32), critic=rng.standard_normal((T, n, W)).astype(np.float32), clears=clears)
    for v in x.values():
        v.setflags(write=False)
    return x


def small_policy(fused, dtype=None):
    """An ActorCritic of small sizes (embed 32, two layers of 64 channels, 64 hidden) with seeded parameters and a critic
    head off its zero initialisation, so that every parameter has a gradient."""
    from gpu_hideseek import policy as P
    net = P.ActorCritic(dtype=dtype, generator=torch.Generator().manual_seed(21), embed=32, channels=64, layers=2, hidden=64, fused=fused)
    with torch.no_grad():
        net.critic_head.weight.copy_(0.05 * torch.randn(net.critic_head.weight.shape, generator=torch.Generator().manual_seed(22)))
    return net


def test_policy_names_shapes_and_heads():
    from gpu_hideseek import policy as P
    net = P.make_policy(fused=False, generator=torch.Generator().manual_seed(3))
    shapes = {k: tuple(p.shape) for k, p in net.named_parameters()}
    per = {"encoder.params": (102 * 64,), "mlp.layers.0.weight": (256, 256), "mlp.layers.0.params": (768,), "mlp.layers.1.weight": (256, 256),
           "mlp.layers.1.params": (768,), "mlp.layers.2.weight": (256, 256), "mlp.layers.2.params": (768,), "core.w_in": (256, 1024),
           "core.w_rec": (256, 1024), "core.cell_params": (1536,)}
    want = {f"{b}.{k}": s for b in ("actor", "critic") for k, s in per.items()}
    want.update({"actor_head.weight": (19, 256), "actor_head.bias": (19,), "critic_head.weight": (255, 256), "critic_head.bias": (255,)})
    assert shapes == want
    assert net.actor.encoder.params.data_ptr() != net.critic.encoder.params.data_ptr()           # separate backbones
    assert not net.critic_head.weight.any() and not net.critic_head.bias.any() and not net.actor_head.bias.any()
    Wa = net.actor_head.weight.detach().double()
    assert torch.allclose(Wa @ Wa.T, 1e-4 * torch.eye(19, dtype=torch.float64), atol=1e-9)         # orthogonal rows of gain 0.01
    n = 7
    rng = torch.Generator().manual_seed(4)
    state = net.init_state(n, "cpu")
    assert [t.shape for s in state for t in s] == [(n, 256)] * 4 and all(t.dtype == torch.float32 and not t.any() for s in state for t in s)
    assert P.make_policy(torch.bfloat16, fused=False).init_state(2, "cpu")[0][0].dtype == torch.bfloat16
    logits, critic_logits, new = net(None, torch.randn(n, 296, generator=rng), torch.randn(n, 296, generator=rng), state,
                                     clear=torch.tensor([0, 1, 0, 0, 1, 0, 0], dtype=torch.int32))
    assert logits.shape == (n, 19) and critic_logits.shape == (n, 255) and logits.dtype == torch.float32
    assert not critic_logits.any() and bool(logits.any()) and torch.isfinite(logits).all()
    (ha, ca), (hc, cc) = new
    for t in (ha, ca, hc, cc):
        assert t.shape == (n, 256) and not t[[1, 4]].any() and bool(t[[0, 2, 3, 5, 6]].any())


def test_policy_sequence_is_the_step_loop():
    """With eager pieces on the CPU, running the encoder and the MLP once over the T * n flattened rows changes a row's
    result by no more than the GEMM's batching: the allowance is 4 x (torch f32 against float64) of the same chunk."""
    x = {k: torch.from_numpy(np.array(v)) for k, v in policy_rows().items()}
    T, n = POLICY["T"], POLICY["n"]
    net = small_policy(False)
    net64 = copy.deepcopy(net).double()
    state = net.init_state(n, "cpu")
    seq = net.sequence(None, x["actor"], x["critic"], state, x["clears"])
    seq64 = net64.sequence(None, x["actor"].double(), x["critic"].double(), net64.init_state(n, "cpu", torch.float64), x["clears"])
    assert seq[0].shape == (T, n, 19) and seq[1].shape == (T, n, 255) and seq64[0].dtype == torch.float64
    s, steps = state, []
    for t in range(T):
        logits, critic_logits, s = net(None, x["actor"][t], x["critic"][t], s, x["clears"][t])
        steps.append((logits, critic_logits))
    loop = (torch.stack([a for a, _ in steps]), torch.stack([b for _, b in steps]), s)
    flat = lambda r: [r[0], r[1], r[2][0][0], r[2][0][1], r[2][1][0], r[2][1][1]]        # noqa: E731
    for name, a, b, ref in zip(("logits", "critic_logits", "actor h", "actor c", "critic h", "critic c"), flat(seq), flat(loop), flat(seq64)):
        a, b, ref = a.detach(), b.detach(), ref.detach()
        allow = 4.0 * float((a.double() - ref).abs().max())
        diff = float((a - b).abs().max())
        print(f"policy sequence against the step loop: {name}: largest difference {diff:.3e} (allowance {allow:.3e}, largest value {float(ref.abs().max()):.3e})")
        assert allow > 0 and diff <= allow, name
    cleared = x["clears"][1] != 0
    assert bool(cleared.any()) and bool(seq[2][0][0][cleared].any())                       # no clear at the last step: the state is carried on
    _, _, mid = net.sequence(None, x["actor"][:2], x["critic"][:2], state, x["clears"][:2])
    assert not mid[0][0][cleared].any() and not mid[1][1][cleared].any()


# ---- what the request builders share (gpu_hideseek._request) ----
def test_the_tensor_check():
    """_request._tensor: a free leading dimension, alternative shapes, the 2^31 bound at n * width == 2^31 exactly and one
    element below it (meta tensors: nothing that large is allocated), and the alignment of a view."""
    from gpu_hideseek._request import _OUTPUT, _tensor
    meta = lambda *shape, dtype=torch.bfloat16: torch.empty(*shape, dtype=dtype, device="meta")      # noqa: E731
    lead, three = ("n >= 1", 256), ("float32", "bfloat16", "float16")
    odd = torch.zeros(12 * 64 + 8)[1:1 + 12 * 64].view(12, 64)
    assert odd.is_contiguous() and odd.data_ptr() % 16
    table = [
        # (tensor, shapes, dtypes, keywords, None or what the refusal says)
        (torch.zeros(1, 256), lead, three, {}, None), (torch.zeros(7, 256), lead, three, {}, None),
        (torch.zeros(0, 256), lead, three, {}, r"shape \(n >= 1, 256\) on cuda:0: its shape is \(0, 256\)"),
        (torch.zeros(7, 255), lead, three, {}, "its shape is"), (torch.zeros(7, 256, 1), lead, three, {}, "its shape is"),
        (torch.zeros(7), [(7,), (7, 1)], three, {}, None), (torch.zeros(7, 1), [(7,), (7, 1)], three, {}, None),
        (torch.zeros(1, 7), [(7,), (7, 1)], three, {}, r"shape \(7,\) or \(7, 1\) on cuda:0: its shape is \(1, 7\)"),
        (torch.zeros(7, 2), [(7,), (7, 1)], three, {}, "its shape is"),
        (torch.zeros(7, dtype=torch.float64), (7,), three, {}, r"a contiguous float32 / bfloat16 / float16 tensor of shape \(7,\) on cuda:0: its dtype is torch.float64"),
        (torch.zeros(14)[::2], (7,), three, {}, "it is not contiguous"), (torch.zeros(256, 7).t(), lead, three, {}, "it is not contiguous"),
        (meta(2 ** 23, 256), lead, three, dict(bound=256), r"n \* 256 must stay below 2\^31"), (meta(2 ** 23 - 1, 256), lead, three, dict(bound=256), None),
        (meta(2 ** 31, dtype=torch.int8), ("n >= 1",), ("int8",), dict(bound=1), r"must stay below 2\^31"),
        (meta(2 ** 31 - 1, dtype=torch.int8), ("n >= 1",), ("int8",), dict(bound=1), None),
        (meta(2 ** 22, 256), lead, three, dict(bound=512), r"n \* 512 must stay below 2\^31"),          # the bound's width is the caller's, not the tensor's
        (meta(2 ** 23, 256), lead, three, {}, None),                                                    # no bound asked for
        (odd, (12, 64), three, dict(align=16), "odd must be 16-byte aligned: its address is 0x"), (odd, (12, 64), three, dict(align=4), None),
        (odd, (12, 64), three, {}, None), (odd, (12, 65), three, dict(align=16), "its shape is"),       # shape before alignment
        (3.0, (7,), three, {}, "odd must be a torch tensor"), (None, (7,), three, dict(kind=_OUTPUT), "odd must be True, None or a torch tensor"),
    ]
    for i, (t, shapes, dtypes, kw, what) in enumerate(table):
        if what is None:
            _tensor("odd", t, shapes, dtypes, "cuda:0", **kw)              # the device is not this check's business
        else:
            with pytest.raises(ValueError, match=what):
                _tensor("odd", t, shapes, dtypes, "cuda:0", **kw)
            print(f"row {i}: refused")


def test_each_autograd_function_is_defined_once():
    from gpu_hideseek import entity_encoder, mlp, recurrent
    for module in (entity_encoder, mlp, recurrent):
        f = module._function()
        assert f is module._function() and issubclass(f, torch.autograd.Function), module.__name__


def test_the_sharded_face():
    """_request._shard_calls against two fake shards: a list of the wrong length is refused by its name, None and True
    go to every shard, one params tensor is handed to every shard, and every shard's call lands on its own stream."""
    from gpu_hideseek._request import _shard_calls
    calls = []

    class Lib:
        def __init__(self, shard):
            self.shard = shard

        def __getattr__(self, name):
            return lambda h, stream, req: calls.append((self.shard, name, stream.value)) or 0

    class Shard:
        def __init__(self, i):
            self.gpu_id, self.num_worlds, self.agents_per_world, self._L, self._h = i, 8 + i, 6, Lib(i), None

    class SSim:
        shards = [Shard(0), Shard(1)]

    def request(gpu_id, **kw):
        return dict(kw, gpu_id=gpu_id), C.c_int32(gpu_id)
    z, params, y1 = [torch.zeros(2, 4), torch.zeros(3, 4)], torch.zeros(12), torch.zeros(3, 4)
    res = _shard_calls(SSim(), "hs_fake", request, [11, 12], dict(z=z), dict(params=params), dict(y=True, mask=None, out=[None, y1]), dict(eps=0.5))
    assert calls == [(0, "hs_fake_async", 11), (1, "hs_fake_async", 12)]
    for i, r in enumerate(res):
        assert r["gpu_id"] == i and r["z"] is z[i] and r["params"] is params and r["y"] is True and r["mask"] is None and r["eps"] == 0.5
    assert res[0]["out"] is None and res[1]["out"] is y1
    res = _shard_calls(SSim(), "hs_fake", request, [11, 12], dict(z=z), dict(params=[params, z[1]]), lead=lambda s: (s.num_worlds * s.agents_per_world,))
    assert [r["gpu_id"] for r in res] == [48, 54] and res[1]["params"] is z[1]
    for kw, what in ((dict(required=dict(z=z[:1])), r"z: one tensor per shard \(2\) expected"), (dict(required=dict(z=z[0])), "z: one tensor per shard"),
                     (dict(required=dict(z=None)), "z: one tensor per shard"), (dict(shared=dict(params=[params] * 3)), r"params: one entry per shard \(2\) expected"),
                     (dict(per_shard=dict(y=[True])), "y: one entry per shard"), (dict(per_shard=dict(mask=y1)), "mask: one entry per shard"),
                     (dict(stream=[11]), "stream: one entry per shard")):
        a = dict(dict(required=dict(z=z), stream=[11, 12]), **kw)
        with pytest.raises(ValueError, match=what):
            _shard_calls(SSim(), "hs_fake", request, a.pop("stream"), a.pop("required"), **a)
    assert len(calls) == 4                                         # nothing was run by a refused call
