"""The optimiser without a GPU (gpu_hideseek.optim, hs_adam_step): a numpy restatement of what include/hideseek.h states —
the sum of squares in float64 in the stated workgroup / lane / trip order, the state's running products in float64 and
the update in f32, operation by operation in the stated order (numpy's f32 division and sqrt are correctly rounded, as the
device's are, and nothing else is involved: the f32 restatement is meant to be the kernel's result bit for bit) — and the
same with every rounding to f32 removed; the restatement against the textbook formulas in float64 over five steps;
skipped steps, zero gradients and padding; optim.flatten on CPU tensors and under autograd; the refusals of request();
and the header.

Tolerance (printed by test_tolerances_are_derived; DESIGN.md quotes it), derived, not chosen: per quantity (p, m, v)
4 x (the project's margin, as in test_mlp_host) the largest deviation of the f32 restatement from the unrounded one over
the five steps of ADAM_CASES, kept as the named constant TOL with the test that recomputes it.  The parameters of those
cases are standard normal, so the constant is an absolute bound for parameters of magnitude up to P_MAX.
"""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

THREADS, VEC, MAX_GRID, STATE, STATS, PAD = 256, 4, 256, 4, 4, 64             # asserted against module and header below
HYPER = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=5.0, grad_scale=1.0)
SEED = 0
SIZES = (1, 5, 255, 1025, MAX_GRID * THREADS * VEC + 7)      # one element; a full and a short quad; lanes idle; two workgroups; a second trip and a ragged tail
POLICY_FLAT = 1532992                                        # the padded length of make_policy()'s 24 parameters


# ---- the contract ----
def grid(n):
    """Workgroups of the norm kernel: min(ceil(ceil(n / 4) / 256), MAX_GRID)."""
    return min(-(-(-(-n // VEC)) // THREADS), MAX_GRID)


def sum_squares(g):
    """(sum, partials [G]) of (double)g * (double)g in the header's order: quad q = (trip * G + b) * 256 + lane; a lane
    adds its quads in trip order and a quad's elements in index order onto +0; a workgroup adds its lanes in lane order;
    the partials are added in index order.  Elements past n add +0, which changes no bit."""
    g = np.asarray(g, np.float32).reshape(-1)
    n, G = g.size, grid(g.size)
    per = G * THREADS * VEC
    trips = -(-n // per)
    sq = np.zeros(trips * per, np.float64)
    with np.errstate(all="ignore"):
        sq[:n] = g.astype(np.float64) * g.astype(np.float64)
        sq = sq.reshape(trips, G, THREADS, VEC)
        acc = np.zeros((G, THREADS), np.float64)
        for t in range(trips):
            for k in range(VEC):
                acc = acc + sq[t, :, :, k]
        part = acc[:, 0].copy()
        for lane in range(1, THREADS):
            part = part + acc[:, lane]
        s = part[0]
        for b in range(1, G):
            s = s + part[b]
    return s, part


def fresh_state():
    return np.array([1.0, 1.0, 0.0, 0.0], np.float64)


def step(ft, x, state, lr, betas, eps, weight_decay, max_grad_norm, grad_scale, zero_grad=True):
    """hs_adam_step in float type `ft` over x = {p, g, m, v} (f32 arrays; g always) and state (float64 [4]): ({p, g, m, v}, the new
    state, stats).  With ft = np.float32 this is the contract; with np.float64 the same operations in the same order with
    no rounding to f32 anywhere (the hyper-parameters are the f32 the request carries; 1 - beta, s and the bias
    corrections stay unrounded)."""
    f32 = np.float32
    rnd = (lambda a: ft(f32(a))) if ft is np.float32 else (lambda a: np.float64(a))     # "rounded once"
    b1, b2 = np.float64(f32(betas[0])), np.float64(f32(betas[1]))
    lr_, eps_, wd = ft(f32(lr)), ft(f32(eps)), ft(f32(weight_decay))
    gs, mgn = np.float64(grad_scale), np.float64(0.0 if max_grad_norm is None else max_grad_norm)
    p, g, m, v = (np.asarray(x[k]).astype(ft) for k in "pgmv")               # f32 arrays; ft = np.float64 also takes carried float64 ones
    total, _ = sum_squares(x["g"])
    with np.errstate(all="ignore"):
        gnorm = gs * np.sqrt(total)
        skipped = not np.isfinite(gnorm)
        clip = np.float64(0.0) if skipped else (mgn / gnorm if (mgn > 0 and gnorm > mgn) else np.float64(1.0))
        new = np.array(state, np.float64)
        zeros = np.zeros_like(g) if zero_grad else g
        if skipped:
            new[3] = new[3] + 1.0
            out = dict(p=p, g=zeros, m=m, v=v)
        else:
            s = rnd(gs * clip)
            new[0], new[1], new[2] = new[0] * b1, new[1] * b2, new[2] + 1.0
            bc1, bc2 = rnd(1.0 - new[0]), rnd(1.0 - new[1])
            omb1, omb2 = rnd(1.0 - b1), rnd(1.0 - b2)
            b1f, b2f = ft(b1), ft(b2)
            gk = g * s
            m = b1f * m + omb1 * gk
            v = b2f * v + omb2 * (gk * gk)
            u = (m / bc1) / (np.sqrt(v / bc2) + eps_)
            p = p - lr_ * ((u + wd * p) if wd != 0 else u)
            out = dict(p=p, g=zeros, m=m, v=v)
    assert all(a.dtype == ft for a in out.values())
    stats = np.array([gnorm, clip, 1.0 if skipped else 0.0, new[2]], np.float64)
    return out, new, stats


def textbook(x, t, lr, betas, eps, weight_decay, max_grad_norm, grad_scale):
    """Adam (AdamW with weight_decay) after optax's clip_by_global_norm in float64, bias corrections by pow, the sum of
    squares by numpy: ({p, m, v}, t + 1).  The hyper-parameters are the f32 the request carries, widened."""
    f = lambda a: np.float64(np.float32(a))                                     # noqa: E731
    b1, b2, lr, eps, wd = f(betas[0]), f(betas[1]), f(lr), f(eps), f(weight_decay)
    p, g, m, v = (np.asarray(x[k]).astype(np.float64) for k in "pgmv")
    g = g * grad_scale
    norm = math.sqrt(math.fsum(g * g))
    if max_grad_norm and max_grad_norm > 0 and norm > max_grad_norm:
        g = g * (max_grad_norm / norm)
    t = t + 1
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    u = (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
    return dict(p=p - lr * (u + wd * p), m=m, v=v), t


# ---- the inputs the GPU tests share ----
@functools.lru_cache(maxsize=None)
def _inputs(n, seed):
    rng = np.random.default_rng([seed, n, 91])
    x = dict(p=rng.standard_normal(n).astype(np.float32), g=rng.standard_normal(n).astype(np.float32),
             m=(0.1 * rng.standard_normal(n)).astype(np.float32), v=(0.01 * rng.random(n)).astype(np.float32))
    for a in x.values():
        a.setflags(write=False)
    return x


def inputs(n, seed=SEED):
    """A fresh dict of the (shared, read-only) arrays of a size: standard normal parameters and gradients, moments as
    after some steps."""
    return dict(_inputs(n, seed))


def gradients(n, k, norm, seed=SEED):
    """The gradient of step k of a run of size n: standard normal, scaled so that its norm is about `norm`."""
    g = np.random.default_rng([seed, n, k, 92]).standard_normal(n)
    return (g * (norm / math.sqrt(float((g * g).sum())))).astype(np.float32)


# clip active (the norm 4 x the limit), inactive, off; each with and without weight decay; one with a loss scale of 1024
CONFIGS = {
    "active": dict(HYPER, norm=20.0), "active, decay": dict(HYPER, norm=20.0, weight_decay=0.01),
    "inactive": dict(HYPER, norm=2.0), "inactive, decay": dict(HYPER, norm=2.0, weight_decay=0.01),
    "off": dict(HYPER, norm=20.0, max_grad_norm=0.0), "off, decay": dict(HYPER, norm=20.0, max_grad_norm=0.0, weight_decay=0.01),
    "active, decay, grad_scale 1/1024": dict(HYPER, norm=20.0 * 1024, weight_decay=0.01, grad_scale=1.0 / 1024),
}


def run(ft, n, config, steps=3, seed=SEED):
    """`steps` consecutive steps of a config from inputs(n) and a fresh state: [(arrays, state, stats, the gradient used)]."""
    kw = dict(CONFIGS[config])
    norm = kw.pop("norm")
    x, state, out = inputs(n, seed), fresh_state(), []
    for k in range(steps):
        g = gradients(n, k, norm, seed)
        res, state, stats = step(ft, dict(x, g=g), state, **kw)
        x = {key: (res[key].astype(np.float32) if ft is np.float32 else res[key]) for key in "pmv"}
        out.append((res, state, stats, g))
    return out


# ---- the tolerance ----
ADAM_N, ADAM_STEPS = 2051, 5
ADAM_NORMS = (45.0, 2.3, 45.0, 4.5, 90.0)                   # clip active, inactive, active, inactive, active
ADAM_CASES = (dict(HYPER), dict(HYPER, weight_decay=0.01))
P_MAX = 4.0                                                  # the largest |p| of ADAM_CASES is above it (asserted)
TOL = {"p": 1.7e-6, "m": 1.4e-7, "v": 9.7e-9}               # 4 x the measured gaps: test_tolerances_are_derived recomputes them


@functools.lru_cache(maxsize=None)
def adam_runs():
    """Per case of ADAM_CASES the five steps in f32 (each step's f32 results are the next step's inputs), in float64
    without any rounding (carried in float64), and by the textbook formulas (carried in float64)."""
    out = []
    for kw in ADAM_CASES:
        x0 = inputs(ADAM_N)
        x32, x64, xt = dict(x0), {k: x0[k].astype(np.float64) for k in "pmv"}, {k: x0[k].astype(np.float64) for k in "pmv"}
        s32, s64, t = fresh_state(), fresh_state(), 0
        rows = []
        for k in range(ADAM_STEPS):
            g = gradients(ADAM_N, k, ADAM_NORMS[k])
            r32, s32, st32 = step(np.float32, dict(x32, g=g), s32, **kw)
            r64, s64, st64 = step(np.float64, dict(x64, g=g), s64, **kw)
            rt, t = textbook(dict(xt, g=g), t, **kw)
            x32, x64, xt = {q: r32[q] for q in "pmv"}, {q: r64[q] for q in "pmv"}, rt
            rows.append((r32, r64, rt, st32, st64))
        out.append(rows)
    return out


def measured_gaps():
    """{p, m, v: the largest |f32 restatement - unrounded restatement| over every step of every case of ADAM_CASES}."""
    gap = {k: 0.0 for k in "pmv"}
    for rows in adam_runs():
        for r32, r64, _, _, _ in rows:
            for k in "pmv":
                gap[k] = max(gap[k], float(np.abs(r32[k].astype(np.float64) - r64[k]).max()))
    return gap


# ---- tests: the contract ----
def test_tolerances_are_derived():
    gap = measured_gaps()
    print("optimiser, n = %d, %d steps, weight decay 0 and 0.01: largest |f32 - unrounded| " % (ADAM_N, ADAM_STEPS)
          + ", ".join(f"{k} {v:.3e}" for k, v in gap.items()) + "; TOL = 4 x, rounded up to two digits: " + ", ".join(f"{k} {v:.1e}" for k, v in TOL.items()))
    for k in "pmv":
        assert gap[k] > 0 and 4.0 * gap[k] <= TOL[k] <= 4.0 * gap[k] * 1.25, (k, gap[k], TOL[k])       # the constant is 4 x the gap, rounded up
    pmax = max(float(np.abs(rows[-1][1]["p"]).max()) for rows in adam_runs())
    assert pmax >= P_MAX, pmax
    # what the bound means: a step moves a parameter by up to lr = 1e-4; five steps of f32 rounding stay below 2 % of one step
    assert TOL["p"] < 0.02 * HYPER["lr"] * 1.0001


def test_the_restatement_is_adam():
    for kw, rows in zip(ADAM_CASES, adam_runs()):
        clips = [float(st32[1]) for _, _, _, st32, _ in rows]
        assert [c < 1 for c in clips] == [True, False, True, False, True], clips                    # both branches of the clip
        for k, (r32, r64, rt, st32, st64) in enumerate(rows):
            assert np.array_equal(st32, st64) and st32[3] == k + 1 and st32[2] == 0                # norm, clip and t are float64 in both
            for q in "pmv":
                exact = float(np.abs(r64[q] - rt[q]).max())
                err = float(np.abs(r32[q].astype(np.float64) - rt[q]).max())
                print(f"weight decay {kw['weight_decay']}, step {k + 1}, {q}: f32 restatement - textbook {err:.3e} (bound {TOL[q]:.1e}); unrounded restatement - textbook {exact:.3e}")
                # the same mathematics in float64: only the order of the sum of squares and pow against a running product differ
                assert exact <= 1e-12 * max(1.0, float(np.abs(rt[q]).max())), (q, exact)
                assert err <= TOL[q], (q, err)
    # the state's products are the powers, and the one-call forms agree with the carried ones on the first step
    _, s, _ = step(np.float32, dict(inputs(5), g=gradients(5, 0, 1.0)), fresh_state(), **HYPER)
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    assert s.tolist() == [b1, b2, 1.0, 0.0]
    x = dict(inputs(ADAM_N), g=gradients(ADAM_N, 0, ADAM_NORMS[0]))
    one, _ = textbook(x, 0, **HYPER)
    assert np.array_equal(one["p"], adam_runs()[0][0][2]["p"])
    r64, _, _ = step(np.float64, x, fresh_state(), **HYPER)
    assert np.array_equal(r64["p"], adam_runs()[0][0][1]["p"])


def test_the_sum_of_squares_has_the_stated_order():
    rng = np.random.default_rng(5)
    for n in SIZES + (ADAM_N,):
        g = rng.standard_normal(n).astype(np.float32)
        s, part = sum_squares(g)
        G = grid(n)
        assert part.shape == (G,) and G == {1: 1, 5: 1, 255: 1, 1025: 2, 2051: 3, SIZES[-1]: MAX_GRID}[n]
        exact = math.fsum((g.astype(np.float64) ** 2).tolist())
        assert abs(s - exact) <= n * 2.0 ** -52 * exact
        # element by element, as a lane sees it: workgroup b's partial from a plain loop over its quads
        b = G - 1
        lanes = []
        for lane in range(THREADS):
            acc, q = 0.0, b * THREADS + lane
            while VEC * q < n:
                for e in g[VEC * q:VEC * q + VEC]:
                    acc = acc + float(e) * float(e)
                q += G * THREADS
            lanes.append(acc)
        want = lanes[0]
        for a in lanes[1:]:
            want = want + a
        assert want == part[b], n
    assert grid(POLICY_FLAT) == MAX_GRID and grid(MAX_GRID * THREADS * VEC) == MAX_GRID and grid(MAX_GRID * THREADS * VEC - 4 * THREADS) == MAX_GRID - 1


def test_edge_inputs_in_the_restatement():
    n = 1025
    x = dict(inputs(n), g=gradients(n, 0, 20.0))
    warm, state, _ = step(np.float32, x, fresh_state(), **HYPER)
    x = dict(p=warm["p"], m=warm["m"], v=warm["v"])
    # a skipped step: everything but the skip count (and the zeroed gradients) is unchanged
    for bad, scale in ((np.inf, 1.0), (np.nan, 1.0), (-np.inf, 1.0), (1e30, 1e300)):
        g = np.array(gradients(n, 1, 20.0))
        g[77] = bad
        for zero in (True, False):
            res, new, stats = step(np.float32, dict(x, g=g), state, **dict(HYPER, grad_scale=scale, zero_grad=zero))
            assert all(np.array_equal(res[k].view(np.uint32), x[k].view(np.uint32)) for k in "pmv")
            assert new.tolist() == [state[0], state[1], 1.0, 1.0] and stats[2] == 1 and stats[3] == 1 and stats[1] == 0 and not np.isfinite(stats[0])
            assert (not res["g"].view(np.uint32).any()) if zero else np.array_equal(res["g"].view(np.uint32), g.view(np.uint32))
    assert np.isfinite(sum_squares(np.full(n, 1e30, np.float32))[0])                       # finite in the gradients' own scale: it overflows through grad_scale alone
    # an all-zero gradient from fresh moments: p unchanged, no NaN; with warm moments p still moves by its momentum
    z = dict(p=x["p"], g=np.zeros(n, np.float32), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    res, new, stats = step(np.float32, z, fresh_state(), **HYPER)
    assert np.array_equal(res["p"].view(np.uint32), x["p"].view(np.uint32)) and not res["m"].view(np.uint32).any() and not res["v"].view(np.uint32).any()
    assert stats.tolist() == [0.0, 1.0, 0.0, 1.0] and all(np.isfinite(res[k]).all() for k in "pmv")
    res, _, _ = step(np.float32, dict(x, g=np.zeros(n, np.float32)), state, **HYPER)
    assert np.isfinite(res["p"]).all() and (res["p"] != x["p"]).any()
    # padding: p = g = m = v = +0 stays +0, with weight decay too, and adds nothing to the norm
    pad = {k: np.concatenate([x.get(k, gradients(n, 1, 20.0)), np.zeros(75, np.float32)]) for k in "pgmv"}
    for wd in (0.0, 0.01):
        res, _, st = step(np.float32, pad, state, **dict(HYPER, weight_decay=wd))
        assert all(not res[k][n:].view(np.uint32).any() for k in "pmv")
    # trailing zeros that leave the grid as it is change no bit of the sum; zeros in between change only the order
    g = gradients(n, 2, 20.0)
    assert grid(n) == grid(n + 75) and sum_squares(g)[0] == sum_squares(np.concatenate([g, np.zeros(75, np.float32)]))[0]
    spread = np.zeros(3 * n, np.float32)
    spread[::3] = g
    a, b = sum_squares(g)[0], sum_squares(spread)[0]
    assert abs(a - b) <= n * 2.0 ** -52 * a
    # the clip is optax's: exactly max / gnorm above the limit, exactly 1 at or below it and when it is off
    for norm, mgn, want in ((20.0, 5.0, None), (2.0, 5.0, 1.0), (20.0, 0.0, 1.0), (20.0, -1.0, 1.0), (20.0, None, 1.0)):
        g = gradients(n, 3, norm)
        _, _, st = step(np.float32, dict(x, g=g), state, **dict(HYPER, max_grad_norm=mgn))
        assert st[1] == (5.0 / st[0] if want is None else want) and abs(st[0] - norm) < 1e-4 * norm


# ---- optim.flatten on the CPU ----
def test_flatten_on_cpu_tensors():
    from gpu_hideseek import optim
    assert (optim.THREADS, optim.VEC, optim.MAX_GRID, optim.STATE, optim.STATS, optim.PAD, optim.ALIGN) == (THREADS, VEC, MAX_GRID, STATE, STATS, PAD, 16)
    assert optim.DEFAULTS == HYPER and optim.fresh_state().tolist() == fresh_state().tolist() and optim.fresh_state().dtype == torch.float64
    g = torch.Generator().manual_seed(1)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3, 5), (64,), (1,), (7, 9, 2), (128,))]
    before = [p.detach().clone() for p in ps]
    ps[1].grad = torch.full((64,), 2.0)
    flat = optim.flatten([("a", ps[0]), ("b", ps[1]), ("c", ps[2]), ("d", ps[3]), ("e", ps[4])])
    lay = flat.layout()
    assert list(lay) == list("abcde") and lay == {"a": (0, 15, (3, 5)), "b": (64, 128, (64,)), "c": (128, 129, (1,)), "d": (192, 318, (7, 9, 2)), "e": (320, 448, (128,))}
    assert flat.params.shape == flat.grads.shape == (448,) and flat.params.dtype == torch.float32
    used = torch.zeros(448, dtype=torch.bool)
    for (name, (lo, hi, shape)), p, old in zip(lay.items(), ps, before):
        assert lo % PAD == 0 and p.data_ptr() == flat.params.data_ptr() + 4 * lo and p.grad.data_ptr() == flat.grads.data_ptr() + 4 * lo
        assert tuple(p.shape) == tuple(p.grad.shape) == shape and torch.equal(p.detach(), old) and p.is_contiguous() and isinstance(p, torch.nn.Parameter)
        assert torch.equal(flat.view(flat.params, name), p.detach())
        used[lo:hi] = True
    assert not flat.params[~used].any() and not flat.grads[~used].any() and bool((flat.grads[64:128] == 2).all()) and not flat.grads[:64].any()
    flat.params[0] = 7.0                                      # the views alias the buffer
    assert float(ps[0].detach()[0, 0]) == 7.0 and flat.detached() is None
    ps[3].grad = None
    assert flat.detached() == "d"
    flat.attach()
    assert flat.detached() is None
    assert list(optim.flatten([torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]).layout()) == ["0", "1"]
    for bad, what in (([], "no parameters"), ([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))], "float32"), ([ps[0], ps[0]], "twice"),
                      ([("a", ps[0]), ("a", ps[1])], "twice"), ([3.0], "parameters must be")):
        with pytest.raises(ValueError, match=what):
            optim.flatten(bad)


def test_flatten_the_policy_and_backward_fills_the_buffer():
    from gpu_hideseek import optim, policy as P
    net = P.make_policy(fused=False, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        net.critic_head.weight.copy_(0.05 * torch.randn(net.critic_head.weight.shape, generator=torch.Generator().manual_seed(4)))
    names = [k for k, _ in net.named_parameters()]
    flat = optim.flatten(net.named_parameters(), "cpu")
    lay = flat.layout()
    assert len(lay) == 24 and list(lay) == names and flat.params.numel() == POLICY_FLAT and all(lo % PAD == 0 for lo, _, _ in lay.values())
    assert sum(hi - lo for lo, hi, _ in lay.values()) == sum(p.numel() for p in net.parameters())
    n = 5
    rng = torch.Generator().manual_seed(6)
    state = tuple(tuple(0.5 * torch.randn(n, 256, generator=rng) for _ in range(2)) for _ in range(2))     # not zero: w_rec has a gradient
    total = None
    for _ in range(2):                                        # two backward passes accumulate in place: .grad stays the view
        logits, critic_logits, _ = net(None, torch.randn(n, 296, generator=rng), torch.randn(n, 296, generator=rng), state)
        (logits.sum() + critic_logits.square().sum()).backward()
        assert flat.detached() is None
        total = flat.grads.clone() if total is None else total
    assert all(p.grad.data_ptr() == flat.grads.data_ptr() + 4 * lay[k][0] for k, p in net.named_parameters())
    assert all(bool(flat.view(flat.grads, k).any()) for k in names) and not torch.equal(total, flat.grads)
    used = torch.zeros(POLICY_FLAT, dtype=torch.bool)
    for lo, hi, _ in lay.values():
        used[lo:hi] = True
    assert not flat.grads[~used].any() and not flat.params[~used].any()


# ---- the refusals of request() ----
def test_request_refuses_before_the_library_is_called():
    from gpu_hideseek import optim

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    n = 40
    good = dict(params=torch.zeros(n), grads=torch.zeros(n), m=torch.zeros(n), v=torch.zeros(n), state=optim.fresh_state())

    def call(**kw):
        a = dict(good, **kw)
        return optim.compute(Sim(), a.pop("params"), a.pop("grads"), a.pop("m"), a.pop("v"), a.pop("state"), **a)

    def off(by=1):
        t = torch.zeros(n + 8)[by:by + n]
        assert t.is_contiguous() and t.data_ptr() % 16
        return t

    for name in ("params", "grads", "m", "v"):
        for bad, what in ((torch.zeros(n, dtype=torch.float64), "dtype"), (torch.zeros(n, dtype=torch.bfloat16), "dtype"), (torch.zeros(n + 1), "shape"),
                          (torch.zeros(n, 1), "shape"), (torch.zeros(2 * n)[::2], "contiguous"), (off(1), "16-byte aligned"), (off(2), "16-byte aligned"),
                          (None, f"{name} must be a torch tensor")):
            with pytest.raises(ValueError, match=what):
                call(**{name: bad})
    for bad in (torch.zeros(0), torch.zeros(()), torch.zeros(2, 3)):
        with pytest.raises(ValueError, match="shape"):
            call(params=bad)
    for bad, what in ((torch.zeros(4), "dtype"), (torch.zeros(5, dtype=torch.float64), "shape"), (torch.zeros(8, dtype=torch.float64)[::2], "contiguous"), (None, "state must")):
        with pytest.raises(ValueError, match=what):
            call(state=bad)
    for bad, what in ((torch.zeros(4), "dtype"), (torch.zeros(3, dtype=torch.float64), "shape"), (2.0, "stats must")):
        with pytest.raises(ValueError, match=what):
            call(stats=bad)
    shared = torch.zeros(4 * n)
    names = ("params", "grads", "m", "v")
    for i, a in enumerate(names):                             # any two of the arrays
        for b in names[i + 1:]:
            with pytest.raises(ValueError, match=f"{b} overlaps {a}"):
                call(**{a: shared[:n], b: shared[8:8 + n]})
            with pytest.raises(ValueError, match=f"{b} overlaps {a}"):
                call(**{a: good[a], b: good[a]})
    both = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(ValueError, match="stats overlaps state"):
        call(state=both[:4], stats=both[2:6])
    with pytest.raises(ValueError, match="state overlaps m"):
        call(state=good["m"].view(torch.float64)[:4])
    nan, inf = float("nan"), float("inf")
    for key in ("lr", "eps", "weight_decay", "grad_scale", "max_grad_norm"):
        for bad in (nan, inf, -inf, "1"):
            with pytest.raises(ValueError, match=f"{key} must be"):
                call(**{key: bad})
    for key in ("lr", "eps", "weight_decay"):                 # finite as float64, not as the f32 the request carries
        with pytest.raises(ValueError, match=f"{key} must be finite"):
            call(**{key: 1e39})
    for key, bad, what in (("eps", 0.0, "eps must be above 0"), ("eps", -1e-8, "eps must be above 0"), ("eps", 1e-50, "eps must be above 0"),
                           ("lr", -1e-4, "lr must be at least 0"), ("weight_decay", -0.01, "weight_decay must be at least 0"),
                           ("grad_scale", 0.0, "grad_scale must be above 0"), ("grad_scale", -1.0, "grad_scale must be above 0")):
        with pytest.raises(ValueError, match=what):
            call(**{key: bad})
    for bad in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, 1.5), (nan, 0.999), (0.9, inf), (0.9,), 0.9, (0.9, 1 - 1e-9)):
        with pytest.raises(ValueError, match="betas must be"):
            call(betas=bad)
    for ok in (dict(), dict(lr=0.0, weight_decay=0.0, max_grad_norm=0.0), dict(max_grad_norm=None, stats=None), dict(betas=(0.0, 0.0), max_grad_norm=-1.0)):
        with pytest.raises(ValueError, match="on cpu"):       # well-formed tensors on the wrong device
            call(**ok)
    res, req = None, None
    with pytest.raises(ValueError, match="on cpu"):
        res, req = optim.request(0, *(good[k] for k in ("params", "grads", "m", "v", "state")))
    assert res is None and req is None


# ---- the header ----
CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "double": C.c_double}


def test_header_states_the_request(hideseek_lib):
    """include/hideseek.h declares the two entry points, the ctypes mirror agrees with it field by field in name and
    type, and the kernel's constants are the module's."""
    from gpu_hideseek import optim
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hideseek.h")).read()
    for name, value in (("HS_ADAM_MAX_GRID", MAX_GRID), ("HS_ADAM_STATE", STATE), ("HS_ADAM_STATS", STATS)):
        assert re.search(rf"{name} = (\d+)", src).group(1) == str(value), name
    assert re.search(r"int32_t hs_adam_step\(hs_sim \*\w*, const hs_adam_request \*\w*\);", src)
    assert re.search(r"int32_t hs_adam_step_async\(hs_sim \*\w*, void \*hip_stream, const hs_adam_request \*\w*\);", src)
    body = re.search(r"typedef struct hs_adam_request \{(.*?)\} hs_adam_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.replace("const", "").split()
        if words:
            for part in " ".join(words[1:]).split(","):
                part = part.strip()
                fields.append((part.lstrip("*").strip(), C.c_void_p if part.startswith("*") else CTYPES[words[0]]))
    assert fields == list(optim.HsAdamRequest._fields_), fields
    assert [f[0] for f in fields] == ["params", "grads", "m", "v", "n", "lr", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm", "grad_scale",
                                      "zero_grad", "state", "stats"]
    R = optim.HsAdamRequest
    assert C.sizeof(R) == 104 and R.n.offset == 32 and R.lr.offset == 40 and R.weight_decay.offset == 56 and R.max_grad_norm.offset == 64
    assert R.grad_scale.offset == 72 and R.zero_grad.offset == 80 and R.state.offset == 88 and R.stats.offset == 96
    lib = C.CDLL(hideseek_lib)
    assert hasattr(lib, "hs_adam_step") and hasattr(lib, "hs_adam_step_async")
    # the stated order and arithmetic, in the header's text
    for phrase in ("quad q = (trip * G + b) * 256 + lane", "gnorm = grad_scale * sqrt(sum)", "u = (m / bc1) / (sqrtf(v / bc2) + eps)",
                   "p = p - lr * (u + weight_decay * p)", "s = (float)(grad_scale * clip)", "{1, 1, 0, 0}"):
        assert phrase in src, phrase
    csrc = os.path.join(root, "marl-hideandseek_amd", "csrc")
    kernel, host = (open(os.path.join(csrc, f)).read() for f in ("hs_k_adam.h", "hideseek.hip"))
    for name, value in (("kAdamThreads", THREADS), ("kAdamVec", VEC), ("kAdamMaxGrid", MAX_GRID), ("kAdamState", STATE), ("kAdamStats", STATS)):
        assert int(re.search(rf"{name} = (\d+);", kernel).group(1)) == value, name
    assert "HS_ADAM_MAX_GRID == hs::kAdamMaxGrid" in host and "atomic" not in kernel.replace("No atomics", "")
    # every kernel of the file is a template, and the file is included after the other kernel headers
    assert len(re.findall(r"__global__", kernel)) == len(re.findall(r"template <int kThreads = kAdamThreads>\n__global__", kernel)) == 2
    includes = re.findall(r'#include "(hs_\w+\.h)"', host)
    assert includes[-2:] == ["hs_k_adam.h", "hs_core_probe.h"]        # behind it only the scalar core's probe table, which holds no kernel
    assert "__global__" not in open(os.path.join(csrc, "hs_core_probe.h")).read()
