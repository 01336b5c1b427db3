"""The entity encoder without a GPU (gpu_hideseek.entity_encoder, hs_entity_encode / hs_entity_encode_backward): a numpy
restatement of what include/hideseek.h states, forward and backward, once in f32 in the header's order and once in
float64; the backward against central differences of the float64 forward; entity_encoder.eager and its autograd gradient
against the restatement; the parameter layout; the tolerances the GPU tests use, derived from the two restatements on
the GPU tests' own cases; the refusals of request(); and the header.

The f32 restatement follows the header's order everywhere: the dot ascending in k, the butterfly over the channels, and
for the backward the rounds, halves, waves, workgroups and segments.  numpy has no fmaf: fmaf(x, w, z) is taken as the
f32 rounding of the float64 x * w + z.  The product of two f32 is exact in float64, the sum is rounded to float64 and then
to f32, which differs from the single rounding of fmaf only where the float64 sum falls within 2^-29 of its own ulp of an
f32 tie: rarely, and then by one ulp of one term.

Tolerances (printed by test_tolerances_are_derived; DESIGN.md quotes them), none a constant:
  features    per table (so per K) and E: 4 x (the project's margin, as in test_value_head_host) the largest deviation of
              the f32 restatement's features from the float64 one's over every case of that E, plus the rounding of the
              output dtype (ROUNDING: half an ulp relative, the smallest subnormal absolute).
  argmax      the value that the chosen entity has in the float64 restatement may lie below the float64 maximum by twice
              the feature tolerance: each of the two f32 values compared deviates by at most one.
  grad_params per case (n, E, gradient dtype) and table: 4 x the largest deviation of the f32 restatement's gradient
              block from the float64 restatement's, both evaluated with the f32 restatement's argmax.  It grows with n
              (more terms per sum) and with the size of the upstream gradient.
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

TABLES = (("self", 0, 45, 1), ("agents", 45, 14, 5), ("boxes", 115, 17, 9), ("ramps", 268, 14, 2))      # name, first column, K, entities
ROW, PARAM_ROWS, WAVES, MAX_GRID_BWD, SUM_SEGS = 296, 102, 4, 512, 8       # asserted against module and header below
EMBED_DIMS = (32, 64, 128)
EPS, SLOPE = 1e-6, 0.01
SEED = 0


def rows_per_block(E):
    return WAVES * (2 if E == 32 else 1)


def sizes(E):
    R = rows_per_block(E)
    return (1, R - 1, R, R + 1, 3 * R + 2)


BIG_E = 64
BIG = MAX_GRID_BWD * rows_per_block(BIG_E) + 3              # just past the backward grid cap: three rows take a second round
CASES = [(n, E, d) for E in EMBED_DIMS for n in sizes(E) for d in DTYPES] + [(BIG, BIG_E, "bfloat16")]


# ---- the contract, in the type `ft` ----
def fma(ft, x, w, z):
    if ft is np.float64:
        return x * w + z
    return (x.astype(np.float64) * w.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def chan_sum(p):
    """sum over the last axis (E channels) in the header's order; every lane ends with the same bits, lane 0's are taken."""
    E = p.shape[-1]
    s = p if E <= 64 else p[..., :64] + p[..., 64:]
    L = s.shape[-1]
    lane = np.arange(L)
    m = 1
    while m < L:
        s = s + s[..., lane ^ m]
        m <<= 1
    return s[..., 0]


def blocks(params, E):
    """{table index: (W [K, E], b, gamma, beta)} of a flat parameter array."""
    out, at = [], 0
    for _, _, K, _ in TABLES:
        out.append((params[at:at + K * E].reshape(K, E), params[at + K * E:at + (K + 1) * E], params[at + (K + 1) * E:at + (K + 2) * E],
                    params[at + (K + 2) * E:at + (K + 3) * E]))
        at += (K + 3) * E
    assert at == PARAM_ROWS * E == params.size
    return out


def entities(ft, rows, g):
    _, col, K, NE = TABLES[g]
    return np.asarray(rows)[:, col:col + NE * K].reshape(-1, NE, K).astype(ft)


def embed(ft, x, W, b, gamma, beta, eps):
    """z, mu, rstd, zhat, y of entities x [n, NE, K]."""
    n, NE, K = x.shape
    E = W.shape[1]
    z = np.broadcast_to(b, (n, NE, E)).astype(ft)
    for k in range(K):
        z = fma(ft, x[:, :, k, None], W[None, None, k, :], z)
    mu = chan_sum(z) / ft(E)
    d = z - mu[..., None]
    var = chan_sum(d * d) / ft(E)
    rstd = ft(1) / np.sqrt(var + eps)
    zhat = d * rstd[..., None]
    y = fma(ft, zhat, gamma, beta)
    assert y.dtype == ft and rstd.dtype == ft
    return rstd, zhat, y


def forward(ft, rows, params, E, eps=EPS, slope=SLOPE):
    """hs_entity_encode in float type `ft`: features [n, 4 E], argmax [n, 3, E] and the per-table activations a."""
    params = np.asarray(params).astype(ft)
    eps, slope = ft(np.float32(eps)), ft(np.float32(slope))
    feats, args, acts = [], [], []
    for g, blk in enumerate(blocks(params, E)):
        _, _, y = embed(ft, entities(ft, rows, g), *blk, eps)
        a = np.where(y >= 0, y, slope * y)
        j = a.argmax(1)                                     # the first index that attains the maximum
        feats.append(np.take_along_axis(a, j[:, None, :], 1)[:, 0, :])
        acts.append(a)
        if g:
            args.append(j.astype(np.uint8))
    return dict(features=np.concatenate(feats, 1), argmax=np.stack(args, 1), a=acts)


def backward(ft, rows, params, grad, argmax, E, eps=EPS, slope=SLOPE):
    """hs_entity_encode_backward in float type `ft`: grad_params [102 E], the sums in the header's order."""
    params = np.asarray(params).astype(ft)
    grad = np.asarray(grad).astype(ft)
    eps, slope = ft(np.float32(eps)), ft(np.float32(slope))
    n = grad.shape[0]
    R = rows_per_block(E)
    G = min(-(-n // R), MAX_GRID_BWD)
    S = G * R                                               # a row's place among the lanes' sums: row % S, in round row // S
    out = []
    for g, (W, b, gamma, beta) in enumerate(blocks(params, E)):
        _, _, K, NE = TABLES[g]
        x = entities(ft, rows, g)
        rstd, zhat, y = embed(ft, x, W, b, gamma, beta, eps)
        sel = np.ones((n, NE, E), bool) if g == 0 else np.asarray(argmax)[:, g - 1, None, :] == np.arange(NE)[None, :, None]
        dy = np.where(sel, grad[:, None, g * E:(g + 1) * E] * np.where(y >= 0, ft(1), slope), ft(0))
        h = gamma * dy
        mh, mhz = chan_sum(h) / ft(E), chan_sum(h * zhat) / ft(E)
        dz = rstd[..., None] * ((h - mh[..., None]) - zhat * mhz[..., None])
        acc = np.zeros((S, K + 3, E), ft)
        for t in range(-(-n // S)):
            r = slice(t * S, min(n, (t + 1) * S))
            m = r.stop - r.start
            for j in range(NE):
                acc[:m, :K] = fma(ft, x[r, j, :, None], dz[r, j, None, :], acc[:m, :K])
                acc[:m, K] = acc[:m, K] + dz[r, j]
                acc[:m, K + 1] = fma(ft, dy[r, j], zhat[r, j], acc[:m, K + 1])
                acc[:m, K + 2] = acc[:m, K + 2] + dy[r, j]
        acc = acc.reshape(G, WAVES, R // WAVES, K + 3, E)
        acc = acc[:, :, 0] if R == WAVES else acc[:, :, 0] + acc[:, :, 1]
        wg = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
        per = -(-G // SUM_SEGS)
        total = None
        for sg in range(SUM_SEGS):
            s = np.zeros((K + 3, E), ft)
            for blk in range(sg * per, min(G, sg * per + per)):
                s = s + wg[blk]
            total = s if total is None else total + s
        assert total.dtype == ft
        out.append(total.reshape(-1))
    return np.concatenate(out)


def table_slices(E):
    out, at = [], 0
    for _, _, K, _ in TABLES:
        out.append(slice(at, at + (K + 3) * E))
        at += (K + 3) * E
    return out


# ---- the inputs of the GPU tests ----
def draw_params(rng, E):
    """Parameters of a net some way into training: kernels of the initialiser's scale, every other part moved off its
    initial value."""
    p = np.zeros(PARAM_ROWS * E, np.float32)
    for W, b, gamma, beta in blocks(p, E):
        K = W.shape[0]
        W[:] = rng.standard_normal((K, E)) * np.sqrt(2.0 / max(K, E))
        b[:] = 0.1 * rng.standard_normal(E)
        gamma[:] = 1.0 + 0.2 * rng.standard_normal(E)
        beta[:] = 0.1 * rng.standard_normal(E)
    return p


def draw_rows(rng, n, dtype):
    """Rows as the pack writes them for an actor: values of order one, a third of the pooled entities masked to zero."""
    rows = rng.standard_normal((n, ROW)).astype(np.float32)
    for _, col, K, NE in TABLES[1:]:
        hidden = rng.random((n, NE)) < 1.0 / 3.0
        rows[:, col:col + NE * K] *= np.repeat(~hidden, K, axis=1)
    return to_dtype(rows, dtype)


@functools.lru_cache(maxsize=None)
def _inputs(n, E, dtype, seed):
    rng = np.random.default_rng([seed, n, E, DTYPES.index(dtype)])
    x = dict(rows=draw_rows(rng, n, dtype), params=draw_params(rng, E),
             grad=to_dtype(rng.standard_normal((n, 4 * E)).astype(np.float32) / np.float32(n), dtype))
    for v in x.values():
        v.setflags(write=False)
    return x


def inputs(n, E, dtype, seed=SEED):
    """A fresh dict of the (shared, read-only) arrays of a case: rows and the upstream gradient representable in `dtype`."""
    return dict(_inputs(n, E, dtype, seed))


@functools.lru_cache(maxsize=None)
def both(case):
    """(f32 restatement, float64 restatement) of a case: forward, and the backward with the f32 restatement's argmax.
    Computed once, shared, left unchanged."""
    n, E, _ = case
    x = inputs(*case)
    out = []
    f32 = forward(np.float32, x["rows"], x["params"], E)
    for ft, f in ((np.float32, f32), (np.float64, forward(np.float64, x["rows"], x["params"], E))):
        out.append(dict(f, grad_params=backward(ft, x["rows"], x["params"], x["grad"], f32["argmax"], E)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def feature_tolerance(E):
    """[4]: per table, 4 x the largest |f32 - float64| of a feature over the cases of this E."""
    dev = np.zeros(4)
    for case in CASES:
        if case[1] == E:
            r32, r64 = both(case)
            gap = np.abs(r32["features"].astype(np.float64) - r64["features"]).reshape(case[0], 4, E)
            dev = np.maximum(dev, gap.max((0, 2)))
    return 4.0 * dev


def feature_bound(want, E, dtype):
    """The bound on |got - want| of features [n, 4 E] stored in `dtype`."""
    rel, absolute = ROUNDING[dtype]
    return np.repeat(feature_tolerance(E), E)[None, :] + rel * np.abs(np.asarray(want, np.float64)) + absolute


@functools.lru_cache(maxsize=None)
def grad_tolerance(case):
    """[4]: per table, 4 x the largest |f32 - float64| of the gradient block of that table in this case."""
    r32, r64 = both(case)
    gap = np.abs(r32["grad_params"].astype(np.float64) - r64["grad_params"])
    return 4.0 * np.array([gap[s].max() for s in table_slices(case[1])])


def grad_bound(case):
    """The bound on |got - want| of grad_params [102 E] (float32 output: no rounding term)."""
    E = case[1]
    return np.concatenate([np.full(s.stop - s.start, t) for s, t in zip(table_slices(E), grad_tolerance(case))])


GAP = 2e-5              # 20 x the step of the central differences; above twice every feature tolerance (asserted)
SEPARATED_N = 5


def margins(rows, params, E):
    """(the smallest lead of a maximum over its runner-up, the smallest |y| of a chosen entity) in float64."""
    f = forward(np.float64, rows, params, E)
    lead = min(float((np.sort(a, 1)[:, -1] - np.sort(a, 1)[:, -2]).min()) for a in f["a"][1:])
    return lead, float(np.abs(f["features"]).min())


@functools.lru_cache(maxsize=None)
def separated(n, E):
    """Inputs (float32) whose runner-up trails every maximum, and whose chosen activations keep off the kink of the leaky
    ReLU, by more than GAP: the first of the seeds 0 .. 255 that gives them.  No entity is masked (masked ones tie)."""
    for seed in range(256):
        rng = np.random.default_rng([seed, n, E, 99])
        x = dict(rows=rng.standard_normal((n, ROW)).astype(np.float32), params=draw_params(rng, E),
                 grad=(rng.standard_normal((n, 4 * E)) / n).astype(np.float32))
        if min(margins(x["rows"], x["params"], E)) > GAP:
            return x
    raise AssertionError("no well-separated inputs among 256 seeds")


# ---- tests ----
def test_layout_tiles_the_parameters():
    from gpu_hideseek import entity_encoder as N
    from gpu_hideseek import policy_inputs as P
    assert N.PARAM_ROWS == PARAM_ROWS and N.EMBED_DIMS == EMBED_DIMS and N.MAX_GRID_BWD == MAX_GRID_BWD and N.SUM_SEGS == SUM_SEGS
    assert [(k, v[0], v[2][-1], int(np.prod(v[2][:-1]))) for k, v in P.TABLES.items()] == [tuple(t) for t in TABLES]
    for E in EMBED_DIMS:
        lay = N.param_layout(E)
        assert list(lay) == [t[0] for t in TABLES] and N.rows_per_block(E) == rows_per_block(E)
        at = 0
        for (name, _, K, _), sl in zip(TABLES, table_slices(E)):
            assert list(lay[name]) == ["kernel", "bias", "scale", "shift"] and sl.start == at
            for part, shape in (("kernel", (K, E)), ("bias", (E,)), ("scale", (E,)), ("shift", (E,))):
                lo, hi, sh = lay[name][part]
                assert lo == at and sh == shape and hi - lo == int(np.prod(shape))       # no gap, no overlap
                at = hi
            assert sl.stop == at
        assert at == PARAM_ROWS * E
        flat = torch.arange(PARAM_ROWS * E, dtype=torch.float32)
        v = N.views(flat, E)
        for g, (W, b, gamma, beta) in enumerate(blocks(flat.numpy(), E)):
            got = v[TABLES[g][0]]
            for a, t in ((W, got["kernel"]), (b, got["bias"]), (gamma, got["scale"]), (beta, got["shift"])):
                assert np.array_equal(a, t.numpy()) and t.data_ptr() == flat.data_ptr() + 4 * int(a.reshape(-1)[0])
    for bad in (16, 65, 64.0, True, None):
        with pytest.raises(ValueError, match="embed_dim"):
            N.param_layout(bad)


def test_init_params_follow_simplenet():
    from gpu_hideseek import entity_encoder as N
    for E in EMBED_DIMS:
        p = N.init_params(E, torch.Generator().manual_seed(1))
        assert p.dtype == torch.float32 and p.shape == (PARAM_ROWS * E,) and torch.equal(p, N.init_params(E, torch.Generator().manual_seed(1)))
        for name, parts in N.views(p, E).items():
            W = parts["kernel"].double()
            K = W.shape[0]
            gram = W @ W.T if K <= E else W.T @ W                     # orthogonal rows or columns, scaled by sqrt(2)
            assert torch.allclose(gram, 2.0 * torch.eye(min(K, E), dtype=torch.float64), atol=1e-5), name
            assert not parts["bias"].any() and not parts["shift"].any() and bool((parts["scale"] == 1).all())


def test_backward_is_the_gradient_of_the_forward():
    """Central differences of the float64 forward, on inputs where no argmax flips and no activation crosses the kink."""
    n, E, h = SEPARATED_N, 32, 1e-6
    x = separated(n, E)
    lead, off_kink = margins(x["rows"], x["params"], E)
    print(f"separated inputs: the runner-up trails by at least {lead:.3e}, chosen |y| at least {off_kink:.3e} (required {GAP:.0e})")
    assert lead > GAP and off_kink > GAP
    p64, g64 = x["params"].astype(np.float64), x["grad"].astype(np.float64)
    f0 = forward(np.float64, x["rows"], p64, E)
    got = backward(np.float64, x["rows"], p64, g64, f0["argmax"], E)

    def loss(p):
        f = forward(np.float64, x["rows"], p, E)
        assert np.array_equal(f["argmax"], f0["argmax"])              # no case is silently dropped: no flip at any probe
        return float((f["features"] * g64).sum())
    picks = np.concatenate([np.arange(s.start, s.stop, 41) for s in table_slices(E)] +
                           [np.arange(s.stop - 3 * E, s.stop, 5) for s in table_slices(E)])
    L, gmax, worst = abs(loss(p64)), float(np.abs(got).max()), 0.0
    # a central difference errs by the rounding of the two losses over 2 h and by h^2 f''' / 6, here taken as no more than
    # h times the largest gradient
    bound = 16 * 2.0 ** -52 * max(L, 1.0) / h + h * gmax
    for i in picks:
        q = p64.copy()
        q[i] += h
        up = loss(q)
        q[i] -= 2 * h
        fd = (up - loss(q)) / (2 * h)
        worst = max(worst, abs(fd - got[i]))
    print(f"{picks.size} parameters probed: largest |central difference - backward| = {worst:.3e} (bound {bound:.3e}, largest gradient {gmax:.3e})")
    assert worst <= bound and bound < 1e-3 * gmax


def test_eager_and_its_autograd_are_the_restatement():
    from gpu_hideseek import entity_encoder as N
    for E in EMBED_DIMS:
        n = SEPARATED_N
        x = separated(n, E)
        r64 = forward(np.float64, x["rows"], x["params"], E)
        g64 = backward(np.float64, x["rows"], x["params"], x["grad"], r64["argmax"], E)
        # float64 torch: the same mathematics in another order (eps and slope as the kernel sees them, rounded to f32)
        p = torch.tensor(x["params"], dtype=torch.float64, requires_grad=True)
        tables = {k: v.double() for k, v in __import__("gpu_hideseek").policy_inputs.views(torch.from_numpy(x["rows"])).items()}
        feats = []
        for name, t in tables.items():
            q = N.views(p, E)[name]
            a = torch.nn.functional.leaky_relu(torch.nn.functional.layer_norm(t @ q["kernel"] + q["bias"], (E,), q["scale"], q["shift"], float(np.float32(EPS))), float(np.float32(SLOPE)))
            feats.append(a if name == "self" else a.amax(-2))
        f = torch.cat(feats, -1)
        (f * torch.from_numpy(x["grad"]).double()).sum().backward()
        scale = float(np.abs(g64).max())
        err_f, err_g = float(np.abs(f.detach().numpy() - r64["features"]).max()), float(np.abs(p.grad.numpy() - g64).max())
        print(f"E = {E}: float64 torch vs restatement: features {err_f:.3e}, grad_params {err_g:.3e} (largest gradient {scale:.3e})")
        # float64 rounding through K <= 45 products, a LayerNorm and sums over n (4 + 16 entities) terms: 2^-52 x a few hundred
        assert err_f <= 2.0 ** -52 * 1024 and err_g <= 2.0 ** -52 * 1024 * max(scale, 1.0)
        # f32 eager: within the derived tolerances of the float64 restatement (float32 features: no rounding term), 4 x for
        # its own, different, order
        pe = torch.tensor(x["params"], requires_grad=True)
        fe = N.eager(torch.from_numpy(x["rows"]), pe, E)
        assert fe.dtype == torch.float32 and fe.shape == (n, 4 * E)
        (fe * torch.from_numpy(x["grad"])).sum().backward()
        assert (np.abs(fe.detach().numpy() - r64["features"]) <= 4 * feature_bound(r64["features"], E, "float32")).all()
        r32 = backward(np.float32, x["rows"], x["params"], x["grad"], r64["argmax"], E)
        tol = 4.0 * np.array([np.abs(r32.astype(np.float64) - g64)[s].max() for s in table_slices(E)])
        for s, t in zip(table_slices(E), tol):
            assert float(np.abs(pe.grad.numpy() - g64)[s].max()) <= 4 * t, (E, s)


def test_ties_go_to_the_first_entity_and_leave_the_gradient_alone():
    """Identical entities tie exactly; whichever of them takes the gradient, every parameter's gradient is the same."""
    E = 64
    x = inputs(7, E, "float32")
    rows = x["rows"].copy()
    _, col, K, _ = TABLES[2]
    rows[:, col + 5 * K:col + 6 * K] = rows[:, col + 2 * K:col + 3 * K] = 3.0 * rows[:, col + 2 * K:col + 3 * K]
    rows[0, 45:] = 0.0
    f = forward(np.float32, rows, x["params"], E)
    assert not f["argmax"][0].any()
    assert not (f["argmax"][:, 1] == 5).any() and (f["argmax"][:, 1] == 2).any()
    other = f["argmax"].copy()
    other[:, 1][other[:, 1] == 2] = 5
    a, b = (backward(np.float64, rows, x["params"], x["grad"], am, E) for am in (f["argmax"], other))
    assert np.abs(a - b).max() <= 2.0 ** -52 * 64 * np.abs(a).max()          # the same terms in another place of the sums


def test_zero_gradient_gives_plus_zero():
    n, E = 9, 32
    x = inputs(n, E, "float32")
    f = forward(np.float32, x["rows"], x["params"], E)
    for z in (np.zeros((n, 4 * E), np.float32), -np.zeros((n, 4 * E), np.float32)):
        g = backward(np.float32, x["rows"], x["params"], z, f["argmax"], E)
        assert not g.view(np.uint32).any()                            # +0 + (+-0) = +0 in every sum


def test_tolerances_are_derived():
    for E in EMBED_DIMS:
        ft = feature_tolerance(E)
        print(f"entity encoder, E = {E}: feature tolerance per table (4 x max f32-vs-f64) " + ", ".join(f"{t[0]} (K = {t[2]}) {v:.3e}" for t, v in zip(TABLES, ft)))
        # activations of magnitude up to ~4 after a LayerNorm: a few f32 ulps of the K-term dot, amplified by rstd
        assert (ft > 2.0 ** -24).all() and (2 * ft < GAP).all()
    for case in CASES:
        gt = grad_tolerance(case)
        r32, r64 = both(case)
        size = np.array([np.abs(r64["grad_params"][s]).max() for s in table_slices(case[1])])
        print(f"    n = {case[0]}, E = {case[1]}, {case[2]}: grad_params tolerance per table " + ", ".join(f"{v:.3e}" for v in gt) +
              f"; largest gradient {size.max():.3e}")
        assert (gt > 0).all() and (gt < 1e-4 * np.maximum(size, 1e-3)).all(), case
        assert (np.abs(r32["features"].astype(np.float64) - r64["features"]) <= feature_bound(r64["features"], case[1], "float32")).all()
    assert CASES[-1][0] == BIG == 2051 and len(CASES) == 46


def test_inputs_are_what_the_issue_describes():
    x = inputs(14, 64, "bfloat16")
    assert np.array_equal(to_dtype(x["rows"], "bfloat16"), x["rows"]) and np.array_equal(to_dtype(x["grad"], "bfloat16"), x["grad"])
    hidden = [(entities(np.float32, x["rows"], g) == 0).all(2).mean() for g in (1, 2, 3)]
    assert all(0.1 < h < 0.6 for h in hidden) and np.isfinite(x["params"]).all()
    f = forward(np.float32, x["rows"], x["params"], 64)
    assert f["argmax"].dtype == np.uint8 and f["argmax"].shape == (14, 3, 64) and f["argmax"].max() <= 8 and (f["argmax"][:, 1] > 4).any()
    assert len({n for n, E, _ in CASES if E == 64}) == 6 and {n for n, E, _ in CASES if E == 32} == {1, 7, 8, 9, 26}


def test_request_refuses_before_the_library_is_called():
    from gpu_hideseek import entity_encoder as N

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    n, E = 12, 64
    good = dict(rows=torch.zeros(n, ROW), params=torch.zeros(PARAM_ROWS * E))

    def call(**kw):
        a = dict(good, **kw)
        return N.compute(Sim(), a.pop("rows"), a.pop("params"), **a)

    def back(**kw):
        a = dict(dict(good, grad_features=torch.zeros(n, 4 * E), argmax=torch.zeros(n, 3, E, dtype=torch.uint8)), **kw)
        return N.compute_backward(Sim(), a.pop("rows"), a.pop("params"), a.pop("grad_features"), a.pop("argmax"), **a)

    for f in (call, back):
        for bad, what in ((torch.zeros(n, ROW - 1), "shape"), (torch.zeros(n * ROW), "shape"), (torch.zeros(0, ROW), "shape"),
                          (torch.zeros(n, ROW, dtype=torch.float64), "dtype"), (torch.zeros(ROW, n).t(), "contiguous"),
                          (torch.zeros(n, 2 * ROW)[:, :ROW], "contiguous"), (None, "rows")):
            with pytest.raises(ValueError, match=what):
                f(rows=bad)
        for bad, what in ((torch.zeros(PARAM_ROWS * E - 1), "shape"), (torch.zeros(PARAM_ROWS, E), "shape"), (torch.zeros(PARAM_ROWS * 32), "shape"),
                          (torch.zeros(PARAM_ROWS * E, dtype=torch.bfloat16), "dtype"), (torch.zeros(2 * PARAM_ROWS * E)[::2], "contiguous"),
                          (None, "params")):
            with pytest.raises(ValueError, match=what):
                f(params=bad)
        for bad in (16, 48, 256, 64.0, True):
            with pytest.raises(ValueError, match="embed_dim"):
                f(embed_dim=bad)
        for k in ("eps", "slope"):
            for v in (float("nan"), float("inf"), 1e39):
                with pytest.raises(ValueError, match=k):
                    f(**{k: v})
        for v in (0.0, -1e-6, 1e-50):
            with pytest.raises(ValueError, match="eps must be above 0"):
                f(eps=v)
        with pytest.raises(ValueError, match="on cpu"):               # well-formed tensors on the wrong device
            f()
    for name, bad, what in (("features", torch.zeros(n, 4 * E - 1), "shape"), ("features", torch.zeros(n + 1, 4 * E), "shape"),
                            ("features", torch.zeros(n, 4 * E, dtype=torch.float64), "dtype"), ("features", torch.zeros(n, 8 * E)[:, ::2], "contiguous"),
                            ("features", 3.0, "features"), ("argmax", torch.zeros(n, 3, E), "dtype"),
                            ("argmax", torch.zeros(n, 3 * E, dtype=torch.uint8), "shape"), ("argmax", "yes", "argmax")):
        with pytest.raises(ValueError, match=what):
            call(**{name: bad})
    with pytest.raises(ValueError, match="nothing to do"):
        call(features=None)
    with pytest.raises(ValueError, match="nothing to do"):
        call(features=False, argmax=False)
    with pytest.raises(ValueError, match="dtype"):
        call(dtype=torch.float64)
    shared = torch.zeros(n * 4 * E + n * ROW)
    with pytest.raises(ValueError, match="features overlaps rows"):
        call(rows=shared[:n * ROW].view(n, ROW), features=shared[n:n + n * 4 * E].view(n, 4 * E))
    with pytest.raises(ValueError, match="features overlaps params"):
        call(params=shared[:PARAM_ROWS * E], features=shared[8:8 + n * 4 * E].view(n, 4 * E))
    bytes_ = torch.zeros(n * 4 * E * 4 + 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="argmax overlaps features"):
        call(features=bytes_[:n * 4 * E * 4].view(torch.float32).view(n, 4 * E), argmax=bytes_[64:64 + n * 3 * E].view(n, 3, E))
    for name, bad, what in (("grad_features", torch.zeros(n, 4 * E - 1), "shape"), ("grad_features", torch.zeros(n, 4 * E, dtype=torch.float64), "dtype"),
                            ("grad_features", torch.zeros(n, 8 * E)[:, ::2], "contiguous"), ("grad_features", None, "grad_features"),
                            ("argmax", torch.zeros(n, 3, E, dtype=torch.int32), "dtype"), ("argmax", torch.zeros(n, 4, E, dtype=torch.uint8), "shape"),
                            ("argmax", None, "argmax"), ("grad_params", torch.zeros(PARAM_ROWS * E + 1), "shape"),
                            ("grad_params", torch.zeros(PARAM_ROWS * E, dtype=torch.float64), "dtype"), ("grad_params", None, "grad_params")):
        with pytest.raises(ValueError, match=what):
            back(**{name: bad})
    with pytest.raises(ValueError, match="grad_params overlaps params"):
        back(grad_params=good["params"])
    with pytest.raises(ValueError, match="grad_params overlaps grad_features"):
        back(grad_features=shared[:n * 4 * E].view(n, 4 * E), grad_params=shared[16:16 + PARAM_ROWS * E])


def test_header_states_the_requests(hideseek_lib):
    """include/hideseek.h declares the four entry points, the ctypes mirrors agree with it field by field, and the kernel's
    constants are the module's."""
    from gpu_hideseek import entity_encoder as N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hideseek.h")).read()
    assert re.search(r"HS_EMBED_PARAM_ROWS = (\d+)", src).group(1) == str(N.PARAM_ROWS) == str(PARAM_ROWS)
    assert re.search(r"HS_EMBED_MAX_GRID_BWD = (\d+)", src).group(1) == str(N.MAX_GRID_BWD) == str(MAX_GRID_BWD)
    assert re.search(r"HS_EMBED_SUM_SEGS = (\d+)", src).group(1) == str(N.SUM_SEGS) == str(SUM_SEGS)
    assert "#define HS_EMBED_ROWS_PER_WAVE(E) ((E) == 32 ? 2 : 1)" in src
    for fn, req in (("hs_entity_encode", "hs_entity_encode_request"), ("hs_entity_encode_backward", "hs_entity_encode_backward_request")):
        assert re.search(rf"int32_t {fn}\(hs_sim \*\w*, const {req} \*\w*\);", src)
        assert re.search(rf"int32_t {fn}_async\(hs_sim \*\w*, void \*hip_stream, const {req} \*\w*\);", src)
    for req, mirror in (("hs_entity_encode_request", N.HsEntityEncodeRequest), ("hs_entity_encode_backward_request", N.HsEntityEncodeBackwardRequest)):
        body = re.search(rf"typedef struct {req} \{{(.*?)\}} {req};", src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            if decl.strip():
                for word in ("const", "int32_t", "uint8_t", "float", "void"):
                    decl = re.sub(rf"\b{word}\b", "", decl)
                names += [part.split()[-1].lstrip("*") for part in decl.split(",")]
        assert names == [f[0] for f in mirror._fields_], names
    F, B = N.HsEntityEncodeRequest, N.HsEntityEncodeBackwardRequest
    assert C.sizeof(F) == 56 and F.n.offset == 16 and F.embed_dim.offset == 24 and F.eps.offset == 32 and F.features.offset == 40 and F.argmax.offset == 48
    assert C.sizeof(B) == 64 and B.grad_features.offset == 16 and B.argmax.offset == 24 and B.n.offset == 32 and B.grad_dtype.offset == 44
    assert B.eps.offset == 48 and B.grad_params.offset == 56
    lib = C.CDLL(hideseek_lib)
    for fn in ("hs_entity_encode", "hs_entity_encode_async", "hs_entity_encode_backward", "hs_entity_encode_backward_async"):
        assert hasattr(lib, fn)
    csrc = os.path.join(root, "marl-hideandseek_amd", "csrc")
    kernel, shared, host = (open(os.path.join(csrc, f)).read() for f in ("hs_k_embed.h", "hs_rows.h", "hideseek.hip"))
    assert '#include "hs_rows.h"' in kernel and "HS_EMBED_MAX_GRID_BWD == hs::kRowsMaxGridBwd && HS_EMBED_SUM_SEGS == hs::kRowsSumSegs" in host
    assert int(re.search(r"kRowsMaxGridBwd = (\d+);", shared).group(1)) == MAX_GRID_BWD
    assert int(re.search(r"kRowsSumSegs = (\d+),", shared).group(1)) == SUM_SEGS
    assert int(re.search(r"kEmbParamRows = (\d+);", kernel).group(1)) == PARAM_ROWS
    assert "kRowsWaves = kRowsThreads / 64" in shared and int(re.search(r"kRowsThreads = (\d+)", shared).group(1)) == 64 * WAVES == 64 * N.WAVES
    assert (N.DEFAULT_EPS, N.DEFAULT_SLOPE) == (EPS, SLOPE)
