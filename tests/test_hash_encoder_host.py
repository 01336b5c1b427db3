"""The SimHash encoder without a GPU (gpu_hideseek.hash_encoder, hs_hash_encode / hs_hash_encode_backward): a numpy
restatement of what include/hideseek.h states, forward and backward, once in f32 in the header's order and once in
float64; the near-tie rule for the bins and its cap on every input set the GPU tests use; the linearity the binned
backward rests on; hash_encoder.eager and its autograd gradient; the bounds the GPU tests use; the ABI; and the module
and the policy with fused=False.  tests/test_gpu_hash_encoder.py imports the restatement, the inputs and the bounds.

The f32 restatement follows the header's order everywhere: a lane's columns l, l + 64, ..., the butterfly over the 64
lanes, the LayerNorm's butterfly over 32 channels, and for the backward the rounds, halves, waves, workgroups and
segments.  fmaf is test_entity_encoder_host.fma (the f32 rounding of the float64 x * w + z, see there).

Bounds, none a constant and none taken from the device:
  bins        bit i of a row is NEAR A TIE where |y_i| < tau_i = 296 * 2^-23 * sum_k |proj[i][k] x_k| in float64: twice the
              standard n u bound (n = 296 terms, u = 2^-24) on the error of an f32 sum of 296 exactly representable
              products' roundings in any order, fmaf or not.  Outside that band every order gives the float64 sign.  A
              row with such a bit may land in any bin reachable by flipping its near-tie bits; at most NEAR_TIE_CAP = 1 %
              of a case's rows may be such rows.
  features    4 x (the project's margin, as in test_entity_encoder_host) the largest deviation of the f32 restatement's
              normalised table from the float64 one's over the parameter sets of the cases, plus the rounding of the
              output dtype (ROUNDING).
  grad_params per case and part (table, scale, shift): 4 x the largest deviation of the f32 restatement's gradient from
              the float64 one's, both with the same bins.  It grows with the depth of the sums.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_action_sampling_host import DTYPES, to_dtype
from test_entity_encoder_host import chan_sum, fma
from test_ppo_loss_host import ROUNDING

ROW, BITS, BINS, FEATURES, PARAMS = 296, 8, 256, 32, 10624          # asserted against module and header below
ROWS_PER_ROUND, WAVES, MAX_GRID_BWD, SUM_SEGS = 8, 4, 256, 8
PROJ, TABLE_END = BITS * ROW, BITS * ROW + BINS * FEATURES
EPS = 1e-6
SEED = 0
NEAR_TIE_CAP = 0.01
R = ROWS_PER_ROUND
BIG = MAX_GRID_BWD * R + R + 1                                  # past the backward's grid cap by one round plus one row
SIZES = (1, R - 1, R, R + 1, 257, 4099, BIG)
CASES = [(n, d) for n in SIZES for d in DTYPES]
PARTS = (("table", slice(PROJ, TABLE_END)), ("scale", slice(TABLE_END, TABLE_END + FEATURES)), ("shift", slice(TABLE_END + FEATURES, PARAMS)))


# ---- the contract, in the type `ft` ----
def parts(params):
    p = np.asarray(params)
    return p[:PROJ].reshape(BITS, ROW), p[PROJ:TABLE_END].reshape(BINS, FEATURES), p[TABLE_END:TABLE_END + FEATURES], p[TABLE_END + FEATURES:]


def project(ft, rows, proj):
    """y [n, 8]: in float64 any order will do; in f32 the header's: a lane's five columns ascending, then the butterfly."""
    x = np.asarray(rows).astype(ft)
    if ft is np.float64:
        return x @ np.asarray(proj).astype(ft).T
    xp, pp = np.zeros((x.shape[0], 320), ft), np.zeros((BITS, 320), ft)
    xp[:, :ROW], pp[:, :ROW] = x, proj
    xp, pp = xp.reshape(-1, 1, 5, 64), pp.reshape(1, BITS, 5, 64)
    acc = np.zeros((x.shape[0], BITS, 64), ft)
    for j in range(5):
        nxt = fma(ft, xp[:, :, j], pp[:, :, j], acc)
        acc = nxt if j < 4 else np.where(np.arange(64) < ROW - 256, nxt, acc)          # lanes 40 .. 63 own no fifth column
    return chan_sum(acc)


def bins_of(y):
    return ((y > 0).astype(np.int64) << np.arange(BITS)).sum(-1).astype(np.uint8)


def near_ties(rows, proj):
    """[n, 8] bool: the bits whose float64 projection lies inside the band an f32 sum cannot resolve."""
    x, p = np.asarray(rows).astype(np.float64), np.asarray(proj).astype(np.float64)
    tau = ROW * 2.0 ** -23 * (np.abs(x)[:, None, :] * np.abs(p)[None]).sum(-1)
    return np.abs(x @ p.T) < tau


def norm_table(ft, params, eps=EPS):
    """(that [256, 32], rstd [256], T [256, 32]) of the table's LayerNorm."""
    _, table, gamma, beta = (a.astype(ft) for a in parts(params))
    eps = ft(np.float32(eps))
    mu = chan_sum(table) / ft(FEATURES)
    d = table - mu[:, None]
    var = chan_sum(d * d) / ft(FEATURES)
    rstd = ft(1) / np.sqrt(var + eps)
    that = d * rstd[:, None]
    T = fma(ft, that, gamma, beta)
    assert T.dtype == ft and rstd.dtype == ft
    return that, rstd, T


def forward(ft, rows, params, eps=EPS):
    """hs_hash_encode in float type `ft`: y [n, 8], bin [n] uint8, the normalised table T and features [n, 32]."""
    y = project(ft, rows, parts(params)[0])
    b = bins_of(y)
    T = norm_table(ft, params, eps)[2]
    return dict(y=y, bin=b, T=T, features=T[b])


def binned(ft, bins, grad):
    """G [256, 32]: the rows' gradients summed per bin in the header's order."""
    g, b = np.asarray(grad).astype(ft), np.asarray(bins).astype(np.int64)
    n = g.shape[0]
    if ft is np.float64:
        G = np.zeros((BINS, FEATURES), ft)
        np.add.at(G, b, g)
        return G
    W = min(-(-n // R), MAX_GRID_BWD)
    S = W * R
    acc = np.zeros((W, WAVES, BINS, FEATURES), ft)
    wg, wave = np.arange(S) // R, np.arange(S) % R // 2
    for t in range(-(-n // S)):
        for s in (0, 1):
            r = t * S + np.arange(s, S, 2)                  # one row per (workgroup, wave): no slice is hit twice
            r = r[r < n]
            k = r - t * S
            acc[wg[k], wave[k], b[r]] = acc[wg[k], wave[k], b[r]] + g[r]
    per_wg = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    per = -(-W // SUM_SEGS)
    total = None
    for sg in range(SUM_SEGS):
        s = np.zeros((BINS, FEATURES), ft)
        for w in range(sg * per, min(W, sg * per + per)):
            s = s + per_wg[w]
        total = s if total is None else total + s
    assert total.dtype == ft
    return total


def table_backward(ft, G, params, eps=EPS):
    """grad_params [10624] from the bins' sums G: the LayerNorm's backward per bin, +0 for a bin whose G is all zero,
    d gamma and d beta over 8 segments of 32 bins."""
    gamma = parts(params)[2].astype(ft)
    that, rstd, _ = norm_table(ft, params, eps)
    h = gamma * G
    mh, mhz = chan_sum(h) / ft(FEATURES), chan_sum(h * that) / ft(FEATURES)
    dt = rstd[:, None] * ((h - mh[:, None]) - that * mhz[:, None])
    dt = np.where((G != 0).any(1)[:, None], dt, ft(0))
    dgamma, dbeta = np.zeros((SUM_SEGS, FEATURES), ft), np.zeros((SUM_SEGS, FEATURES), ft)
    for i in range(BINS // SUM_SEGS):
        b = np.arange(SUM_SEGS) * (BINS // SUM_SEGS) + i
        dgamma = fma(ft, G[b], that[b], dgamma)
        dbeta = dbeta + G[b]
    out = np.zeros(PARAMS, ft)
    out[PROJ:TABLE_END] = dt.reshape(-1)
    for sl, segs in ((PARTS[1][1], dgamma), (PARTS[2][1], dbeta)):
        s = segs[0]
        for k in range(1, SUM_SEGS):
            s = s + segs[k]
        out[sl] = s
    return out


def backward(ft, bins, grad, params, eps=EPS):
    """hs_hash_encode_backward in float type `ft`."""
    return table_backward(ft, binned(ft, bins, grad), params, eps)


def per_row_backward(bins, grad, params, eps=EPS):
    """The float64 gradient the long way: every row's LayerNorm backward on its own, then summed."""
    _, _, gamma, _ = (a.astype(np.float64) for a in parts(params))
    that, rstd, _ = norm_table(np.float64, params, eps)
    out = np.zeros(PARAMS)
    dt = out[PROJ:TABLE_END].reshape(BINS, FEATURES)
    for b, g in zip(np.asarray(bins).astype(np.int64), np.asarray(grad).astype(np.float64)):
        h = gamma * g
        dt[b] += rstd[b] * ((h - h.mean()) - that[b] * (h * that[b]).mean())
        out[PARTS[1][1]] += g * that[b]
        out[PARTS[2][1]] += g
    return out


# ---- the inputs of the GPU tests ----
def draw_params(rng):
    """Parameters some way into training: a standard-normal projection, a table of the initialiser's scale, scale and
    shift moved off their initial values."""
    p = np.zeros(PARAMS, np.float32)
    p[:PROJ] = rng.standard_normal(PROJ)
    p[PROJ:TABLE_END] = rng.standard_normal(BINS * FEATURES) * np.sqrt(2.0 / BINS)
    p[PARTS[1][1]] = 1.0 + 0.2 * rng.standard_normal(FEATURES)
    p[PARTS[2][1]] = 0.1 * rng.standard_normal(FEATURES)
    return p


def draw_rows(rng, n, dtype):
    """Rows as the pack writes them for an actor: values of order one, a third of the pooled entities masked to zero."""
    rows = rng.standard_normal((n, ROW)).astype(np.float32)
    for col, K, NE in ((45, 14, 5), (115, 17, 9), (268, 14, 2)):
        hidden = rng.random((n, NE)) < 1.0 / 3.0
        rows[:, col:col + NE * K] *= np.repeat(~hidden, K, axis=1)
    return to_dtype(rows, dtype)


@functools.lru_cache(maxsize=None)
def _inputs(n, dtype, seed):
    rng = np.random.default_rng([seed, n, 4242, DTYPES.index(dtype)])
    x = dict(rows=draw_rows(rng, n, dtype), params=draw_params(rng),
             grad=to_dtype(rng.standard_normal((n, FEATURES)).astype(np.float32) / np.float32(n), dtype))
    for v in x.values():
        v.setflags(write=False)
    return x


def inputs(n, dtype, seed=SEED):
    """A fresh dict of the (shared, read-only) arrays of a case: rows and the upstream gradient representable in `dtype`."""
    return dict(_inputs(n, dtype, seed))


@functools.lru_cache(maxsize=None)
def exact_inputs():
    """A projection of +-unit vectors on 8 columns and 256 + 3 rows: row b < 256 spells bin b with the signs of those
    columns (everything else in it is noise the projection does not see); then an all-zero row, a row with a NaN in a
    projected column (0 * NaN is NaN, so it clears every bit, not only that column's), and a row whose y_3 is exactly 0
    while the other bits are set."""
    rng = np.random.default_rng([SEED, 77])
    cols = np.array([3, 44, 45, 64, 114, 200, 255, 295])         # one in every lane group, the first and the last table
    sign = np.array([1, -1, 1, 1, -1, 1, -1, 1], np.float32)
    p = draw_params(rng)
    proj = np.zeros((BITS, ROW), np.float32)
    proj[np.arange(BITS), cols] = sign
    p[:PROJ] = proj.reshape(-1)
    rows = rng.standard_normal((BINS + 3, ROW)).astype(np.float32)
    bit = (np.arange(BINS)[:, None] >> np.arange(BITS)) & 1
    mag = 0.5 + rng.random((BINS, BITS)).astype(np.float32)
    rows[:BINS, cols] = np.where(bit == 1, mag, -mag) * sign
    rows[BINS] = 0.0
    rows[BINS + 1, cols] = sign
    rows[BINS + 1, cols[5]] = np.nan
    rows[BINS + 2, cols] = sign
    rows[BINS + 2, cols[3]] = 0.0
    want = np.concatenate([np.arange(BINS), [0, 0, 255 - 8]]).astype(np.uint8)
    for a in (p, rows, want):
        a.setflags(write=False)
    return dict(rows=rows, params=p, bin=want)


def same_rows(n=4099, dtype="float32"):
    """n copies of one row: the deepest sum a single bin can get."""
    x = inputs(n, dtype)
    return dict(x, rows=np.repeat(np.asarray(x["rows"])[:1], n, axis=0))


def check_bins(got, rows, params, tag=""):
    """The near-tie rule: `got` [n] equals the float64 bins outside the near-tie rows, a near-tie row differs from its
    float64 bin in near-tie bits only, and at most NEAR_TIE_CAP of the rows are near-tie rows.  Returns how many are."""
    proj = parts(params)[0]
    want = bins_of(project(np.float64, rows, proj))
    near = near_ties(rows, proj)
    loose = (near.astype(np.int64) << np.arange(BITS)).sum(-1)
    n_near = int(near.any(1).sum())
    diff = np.asarray(got).astype(np.int64) ^ want.astype(np.int64)
    print(f"{tag}: {n_near} of {len(want)} rows near a tie (cap {NEAR_TIE_CAP * len(want):.2f}), {int((diff != 0).sum())} bins differ from float64's")
    assert n_near <= NEAR_TIE_CAP * len(want), (tag, n_near)
    assert not (diff & ~loose).any(), (tag, "a bit outside the near-tie band differs", np.flatnonzero(diff & ~loose)[:8])
    return n_near


@functools.lru_cache(maxsize=None)
def feature_tolerance():
    """4 x the largest |f32 - float64| of the normalised table over the parameter sets the GPU tests use."""
    sets = [inputs(n, d)["params"] for n, d in CASES] + [exact_inputs()["params"]]
    return 4.0 * max(float(np.abs(norm_table(np.float32, p)[2].astype(np.float64) - norm_table(np.float64, p)[2]).max()) for p in sets)


def feature_bound(want, dtype):
    """The bound on |got - want| of features [n, 32] stored in `dtype`, `want` the float64 LayerNorm of table[bin]."""
    rel, absolute = ROUNDING[dtype]
    return feature_tolerance() + rel * np.abs(np.asarray(want, np.float64)) + absolute


def grad_tolerance(bins, grad, params, eps=EPS):
    """[3]: per part, 4 x the largest |f32 - float64| of the restatement's gradient with these bins."""
    gap = np.abs(backward(np.float32, bins, grad, params, eps).astype(np.float64) - backward(np.float64, bins, grad, params, eps))
    return 4.0 * np.array([gap[sl].max() for _, sl in PARTS])


def grad_bound(bins, grad, params, eps=EPS):
    """The bound on |got - want| of grad_params [10624] (float32 output: no rounding term; the proj range: 0)."""
    out = np.zeros(PARAMS)
    for (_, sl), t in zip(PARTS, grad_tolerance(bins, grad, params, eps)):
        out[sl] = t
    return out


# ---- tests ----
def test_constants_and_layout():
    from gpu_hideseek import hash_encoder as N
    from gpu_hideseek import policy_inputs as P
    assert (N.BITS, N.BINS, N.FEATURES, N.PARAMS) == (BITS, BINS, FEATURES, PARAMS) == (8, 256, 32, 8 * 296 + 256 * 32 + 64)
    assert (N.ROWS_PER_ROUND, N.MAX_GRID_BWD, N.SUM_SEGS, N.DEFAULT_EPS) == (ROWS_PER_ROUND, MAX_GRID_BWD, SUM_SEGS, EPS) and P.ROW == ROW
    assert [v[0] for v in P.TABLES.values()] == [0, 45, 115, 268]            # self, agents, boxes, ramps: HashNet's concatenation
    lay = N.param_layout()
    assert list(lay) == ["proj", "table", "scale", "shift"]
    at = 0
    for part, shape in (("proj", (BITS, ROW)), ("table", (BINS, FEATURES)), ("scale", (FEATURES,)), ("shift", (FEATURES,))):
        lo, hi, sh = lay[part]
        assert lo == at and sh == shape and hi - lo == int(np.prod(shape))
        at = hi
    assert at == PARAMS and [lay[k][:2] for k, _ in PARTS] == [(sl.start, sl.stop) for _, sl in PARTS]
    flat = torch.arange(PARAMS, dtype=torch.float32)
    for a, t in zip(parts(flat.numpy()), N.views(flat).values()):
        assert np.array_equal(a, t.numpy()) and t.data_ptr() == flat.data_ptr() + 4 * int(a.reshape(-1)[0])
    with pytest.raises(ValueError, match="shape"):
        N.views(torch.zeros(PARAMS + 1))


def test_init_params():
    from gpu_hideseek import hash_encoder as N
    p = N.init_params(torch.Generator().manual_seed(1))
    assert p.dtype == torch.float32 and p.shape == (PARAMS,) and torch.equal(p, N.init_params(torch.Generator().manual_seed(1)))
    v = N.views(p)
    assert abs(float(v["proj"].std()) - 1.0) < 0.05 and abs(float(v["proj"].mean())) < 0.05
    assert abs(float(v["table"].std()) / np.sqrt(2.0 / BINS) - 1.0) < 0.05
    assert bool((v["scale"] == 1).all()) and not v["shift"].any()


def test_the_f32_order_flips_no_bit_outside_the_band_and_the_cap_holds():
    """Every input set of the GPU tests: the float64 reference alone stays within the cap, and the f32 restatement in the
    header's order obeys the rule the device is held to."""
    worst = 0.0
    for case in CASES:
        x = inputs(*case)
        f32 = forward(np.float32, x["rows"], x["params"])
        near = check_bins(f32["bin"], x["rows"], x["params"], case)
        worst = max(worst, near / case[0])
    print(f"largest share of near-tie rows over the cases: {worst:.4%}")
    e = exact_inputs()
    assert check_bins(forward(np.float32, e["rows"], e["params"])["bin"], e["rows"], e["params"], "exact") == 0
    s = same_rows()
    assert check_bins(forward(np.float32, s["rows"], s["params"])["bin"], s["rows"], s["params"], "same rows") == 0
    assert SIZES == (1, 7, 8, 9, 257, 4099, 2057) and len(CASES) == 21


def test_exact_bins_and_the_zero_rule():
    e = exact_inputs()
    for ft in (np.float32, np.float64):
        f = forward(ft, e["rows"], e["params"])
        assert np.array_equal(f["bin"], e["bin"]) and set(f["bin"][:BINS]) == set(range(BINS))
        assert not f["y"][BINS].any() and np.isnan(f["y"][BINS + 1]).all() and f["y"][BINS + 2, 3] == 0
    assert not near_ties(e["rows"][:BINS + 1], parts(e["params"])[0]).any()


def test_a_near_tie_row_may_only_move_within_its_band():
    x = inputs(257, "float32")
    rows, params = np.array(x["rows"]), np.array(x["params"])
    y = project(np.float64, rows, parts(params)[0])
    want = bins_of(y)
    with pytest.raises(AssertionError, match="outside the near-tie band"):
        check_bins(want ^ np.uint8(4) * (np.arange(257) == 5), rows, params)
    # a row built to sit on a tie of bit 0: the component along proj[0] removed in float64, then rounded to f32
    p0 = parts(params)[0][0].astype(np.float64)
    rows[5] = (rows[5].astype(np.float64) - y[5, 0] / (p0 @ p0) * p0).astype(np.float32)
    assert near_ties(rows, parts(params)[0])[5, 0]
    want = bins_of(project(np.float64, rows, parts(params)[0]))
    more = np.concatenate([rows[5:6]] * 3 + [rows])               # one or two of 257 rows are within the cap; three more are not
    with pytest.raises(AssertionError, match="more"):
        check_bins(bins_of(project(np.float64, more, parts(params)[0])), more, params, "more")
    assert check_bins(want ^ np.uint8(1) * (np.arange(257) == 5), rows, params) >= 1


def test_the_binned_backward_is_the_sum_of_the_rows_backwards_and_autograd():
    """Linearity, in float64: per-row LayerNorm backwards summed == the backward of the binned sums == torch autograd
    through hash_encoder.eager."""
    from gpu_hideseek import hash_encoder as N
    n = 257
    x = inputs(n, "float32")
    bins = forward(np.float64, x["rows"], x["params"])["bin"]
    assert len(set(bins)) > 100 and len(set(bins)) < BINS           # visited and unvisited bins
    a, b = backward(np.float64, bins, x["grad"], x["params"]), per_row_backward(bins, x["grad"], x["params"])
    scale = np.abs(a).max()
    assert np.abs(a - b).max() <= 2.0 ** -52 * 64 * n * scale
    p = torch.from_numpy(np.array(x["params"])).double().requires_grad_()
    rows = torch.from_numpy(np.array(x["rows"]))
    assert np.array_equal(N.eager_bins(rows, p.detach()).numpy(), bins.astype(np.int64))
    f = N.eager(rows, p)
    assert f.dtype == torch.float64 and f.shape == (n, FEATURES)
    assert np.abs(f.detach().numpy() - forward(np.float64, x["rows"], x["params"])["features"]).max() < 1e-12
    (f * torch.from_numpy(np.array(x["grad"])).double()).sum().backward()
    g = p.grad.numpy()
    assert not g[:PROJ].any() and np.abs(g - a).max() <= 2.0 ** -52 * 64 * n * scale
    unvisited = np.setdiff1d(np.arange(BINS), bins)
    assert not a[PROJ:TABLE_END].reshape(BINS, FEATURES)[unvisited].any()
    # the f32 restatement: the same within its own bound, +0 where nothing was added
    g32 = backward(np.float32, bins, x["grad"], x["params"])
    assert (np.abs(g32 - a) <= grad_bound(bins, x["grad"], x["params"])).all()
    assert not g32[:PROJ].view(np.uint32).any() and not g32[PROJ:TABLE_END].reshape(BINS, FEATURES)[unvisited].view(np.uint32).any()
    for z in (np.zeros((n, FEATURES), np.float32), -np.zeros((n, FEATURES), np.float32)):
        neg = np.array(x["params"])
        neg[PARTS[1][1]][::2] *= -1                                # a negative scale must not turn +0 into -0
        assert not backward(np.float32, bins, z, neg).view(np.uint32).any()


def test_bounds_are_derived():
    ft = feature_tolerance()
    print(f"hash encoder: feature tolerance (4 x max f32-vs-f64 of the normalised table) {ft:.3e}")
    assert 2.0 ** -24 < ft < 1e-5                                 # a LayerNorm over 32 channels of values up to ~4: a few f32 ulps
    for case in CASES + [("same", "float32")]:
        x = same_rows() if case[0] == "same" else inputs(*case)
        bins = forward(np.float64, x["rows"], x["params"])["bin"]
        gt = grad_tolerance(bins, x["grad"], x["params"])
        g64 = backward(np.float64, bins, x["grad"], x["params"])
        size = np.array([np.abs(g64[sl]).max() for _, sl in PARTS])
        print(f"    {case}: grad_params tolerance per part " + ", ".join(f"{k} {v:.3e}" for (k, _), v in zip(PARTS, gt)) + f"; largest gradient {size.max():.3e}")
        # (a sum of a few short terms is exact in f32 in every order: the shift's tolerance may be 0, and the device has to
        # be exact there too)
        assert gt[0] > 0 and (gt < 1e-4 * np.maximum(size, 1e-3)).all(), case


def test_request_refuses_before_the_library_is_called():
    from gpu_hideseek import hash_encoder as N

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    n = 12
    good = dict(rows=torch.zeros(n, ROW), params=torch.zeros(PARAMS))

    def call(**kw):
        a = dict(good, **kw)
        return N.compute(Sim(), a.pop("rows"), a.pop("params"), **a)

    def back(**kw):
        a = dict(dict(bin=torch.zeros(n, dtype=torch.uint8), grad_features=torch.zeros(n, FEATURES), params=good["params"]), **kw)
        return N.compute_backward(Sim(), a.pop("bin"), a.pop("grad_features"), a.pop("params"), **a)

    for bad, what in ((torch.zeros(n, ROW - 1), "shape"), (torch.zeros(0, ROW), "shape"), (torch.zeros(n, ROW, dtype=torch.float64), "dtype"),
                      (torch.zeros(ROW, n).t(), "contiguous"), (None, "rows")):
        with pytest.raises(ValueError, match=what):
            call(rows=bad)
    off = torch.zeros(n * ROW + 8)
    first = -(off.data_ptr() // 4) % 4 + 1                            # one element past a 16-byte boundary
    with pytest.raises(ValueError, match="16-byte aligned"):
        call(rows=off[first:first + n * ROW].view(n, ROW))
    for f in (call, back):
        for bad, what in ((torch.zeros(PARAMS - 1), "shape"), (torch.zeros(PARAMS, dtype=torch.bfloat16), "dtype"), (torch.zeros(2 * PARAMS)[::2], "contiguous"),
                          (None, "params")):
            with pytest.raises(ValueError, match=what):
                f(params=bad)
        for v in (float("nan"), float("inf"), 1e39):
            with pytest.raises(ValueError, match="eps"):
                f(eps=v)
        for v in (0.0, -1e-6, 1e-50):
            with pytest.raises(ValueError, match="eps must be above 0"):
                f(eps=v)
        with pytest.raises(ValueError, match="on cpu"):               # well-formed tensors on the wrong device
            f()
    for name, bad, what in (("features", torch.zeros(n, FEATURES - 1), "shape"), ("features", torch.zeros(n, FEATURES, dtype=torch.float64), "dtype"),
                            ("features", None, "features"), ("features", False, "features"), ("bin", torch.zeros(n), "dtype"),
                            ("bin", torch.zeros(n, 1, dtype=torch.uint8), "shape"), ("dtype", torch.float64, "dtype")):
        with pytest.raises(ValueError, match=what):
            call(**{name: bad})
    shared = torch.zeros(n * ROW + n * FEATURES)
    with pytest.raises(ValueError, match="features overlaps rows"):
        call(rows=shared[:n * ROW].view(n, ROW), features=shared[n:n + n * FEATURES].view(n, FEATURES))
    for name, bad, what in (("bin", torch.zeros(n, dtype=torch.int32), "dtype"), ("bin", None, "bin"), ("grad_features", torch.zeros(n + 1, FEATURES), "shape"),
                            ("grad_features", torch.zeros(n, FEATURES, dtype=torch.float64), "dtype"), ("grad_features", None, "grad_features"),
                            ("grad_params", torch.zeros(PARAMS + 1), "shape"), ("grad_params", None, "grad_params")):
        with pytest.raises(ValueError, match=what):
            back(**{name: bad})
    with pytest.raises(ValueError, match="grad_params overlaps params"):
        back(grad_params=good["params"])


def test_header_states_the_requests(hideseek_lib):
    """include/hideseek.h declares the four entry points, the ctypes mirrors agree with it field by field, the library and
    the build's symbol list have them, and the kernels use no atomic."""
    from gpu_hideseek import hash_encoder as N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hideseek.h")).read()
    for name, v in (("HS_HASH_BITS", BITS), ("HS_HASH_BINS", BINS), ("HS_HASH_FEATURES", FEATURES), ("HS_HASH_ROWS_PER_ROUND", ROWS_PER_ROUND),
                    ("HS_HASH_MAX_GRID_BWD", MAX_GRID_BWD), ("HS_HASH_SUM_SEGS", SUM_SEGS)):
        assert re.search(rf"{name} = (\d+)", src).group(1) == str(v), name
    assert "HS_HASH_PARAMS = 8 * 296 + 256 * 32 + 32 + 32" in src and 8 * 296 + 256 * 32 + 32 + 32 == PARAMS
    assert re.search(r"HS_EMBED_SUM_SEGS = (\d+)", src).group(1) == str(SUM_SEGS)
    for fn, req in (("hs_hash_encode", "hs_hash_encode_request"), ("hs_hash_encode_backward", "hs_hash_encode_backward_request")):
        assert re.search(rf"int32_t {fn}\(hs_sim \*\w*, const {req} \*\w*\);", src)
        assert re.search(rf"int32_t {fn}_async\(hs_sim \*\w*, void \*hip_stream, const {req} \*\w*\);", src)
    for req, mirror in (("hs_hash_encode_request", N.HsHashEncodeRequest), ("hs_hash_encode_backward_request", N.HsHashEncodeBackwardRequest)):
        body = re.search(rf"typedef struct {req} \{{(.*?)\}} {req};", src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            if decl.strip():
                for word in ("const", "int32_t", "uint8_t", "float", "void"):
                    decl = re.sub(rf"\b{word}\b", "", decl)
                names += [part.split()[-1].lstrip("*") for part in decl.split(",")]
        assert names == [f[0] for f in mirror._fields_], names
    F, B = N.HsHashEncodeRequest, N.HsHashEncodeBackwardRequest
    assert C.sizeof(F) == 48 and (F.rows.offset, F.params.offset, F.n.offset, F.rows_dtype.offset, F.features_dtype.offset, F.eps.offset,
                                  F.features.offset, F.bin.offset) == (0, 8, 16, 20, 24, 28, 32, 40)
    assert C.sizeof(B) == 48 and (B.bin.offset, B.grad_features.offset, B.params.offset, B.n.offset, B.grad_dtype.offset, B.eps.offset,
                                  B.reserved.offset, B.grad_params.offset) == (0, 8, 16, 24, 28, 32, 36, 40)
    host = open(os.path.join(root, "marl-hideandseek_amd", "csrc", "hideseek.hip")).read()
    assert "sizeof(hs_hash_encode_request) == 48" in host and "sizeof(hs_hash_encode_backward_request) == 48" in host
    symbols = ("hs_hash_encode", "hs_hash_encode_async", "hs_hash_encode_backward", "hs_hash_encode_backward_async")
    lib = C.CDLL(hideseek_lib)
    entry = open(os.path.join(root, "__graft_entry__.py")).read()
    for fn in symbols:
        assert hasattr(lib, fn) and f'"{fn}"' in entry, fn
    kernel = open(os.path.join(root, "marl-hideandseek_amd", "csrc", "hs_k_hash.h")).read()
    assert "atomic" not in kernel.lower()
    assert int(re.search(r"kHashMaxGridBwd = (\d+);", kernel).group(1)) == MAX_GRID_BWD and "kHashSub = 2, kHashRows = kRowsWaves * kHashSub" in kernel


def test_the_module_and_the_policy_without_kernels():
    """fused=False, sim=None: shapes, dtypes, the three kinds' flat lengths, load_policy's choice, and the refusal."""
    from gpu_hideseek import evaluate, hash_encoder, optim, policy
    assert policy.ENCODERS == ("simple", "attention", "hash")
    enc = hash_encoder.HashEncoder(generator=torch.Generator().manual_seed(0))
    assert [(k, tuple(p.shape), p.dtype) for k, p in enc.named_parameters()] == [("params", (PARAMS,), torch.float32)] and not list(enc.buffers())
    assert {k: tuple(v.shape) for k, v in enc.named_views().items()} == {"proj": (BITS, ROW), "table": (BINS, FEATURES), "scale": (FEATURES,), "shift": (FEATURES,)}
    n, T = 5, 3
    rng = np.random.default_rng(5)
    lengths = {}
    for kind in policy.ENCODERS:
        length = 0
        for p in policy.make_policy(encoder=kind, fused=False).parameters():
            length = -(-(length + p.numel()) // optim.PAD) * optim.PAD
        lengths[kind] = length
    assert len(set(lengths.values())) == 3, lengths
    for dtype in (torch.float32, torch.bfloat16):
        net = policy.make_policy(dtype, fused=False, generator=torch.Generator().manual_seed(0), encoder="hash")
        assert net.encoder == "hash" and not hasattr(net.actor, "mlp") and net.actor.core.w_in.shape[-2:] in ((FEATURES, 1024), (1024, FEATURES))
        actor, critic = (torch.from_numpy(rng.standard_normal((T, n, ROW)).astype(np.float32)).to(dtype) for _ in range(2))
        state = net.init_state(n, "cpu")
        logits, crit, state2 = net(None, actor[0], critic[0], state, clear=torch.zeros(n, dtype=torch.int32))
        assert logits.shape == (n, 19) and crit.shape == (n, 255) and logits.dtype == dtype and crit.dtype == dtype
        assert state2[0][0].shape == (n, 256) and state2[0][0].dtype == dtype and state2[0][1].dtype == torch.float32
        ls, cs, _ = net.sequence(None, actor, critic, state, torch.zeros(T, n, dtype=torch.int32))
        assert ls.shape == (T, n, 19) and cs.shape == (T, n, 255) and ls.dtype == dtype and torch.isfinite(ls.float()).all()
        assert float((ls[0].float() - logits.float()).detach().abs().max()) < (1e-6 if dtype == torch.float32 else 2e-3)     # the GEMMs' shapes differ
        ls.float().sum().backward()
        g = hash_encoder.views(net.actor.encoder.params.grad)
        assert not g["proj"].any() and g["table"].any() and g["shift"].any()
    flat = optim.flatten(net.named_parameters(), "cpu")
    state = {"params": flat.params.detach().clone(), "optimizer": {"layout": flat.layout()}, "normaliser": None}
    assert state["params"].shape == (lengths["hash"],)
    got, norm = evaluate.load_policy(state, torch.bfloat16, "cpu")
    assert got.encoder == "hash" and norm is None and torch.equal(got.actor.encoder.params, net.actor.encoder.params)
    for make in (policy.make_policy, policy.Backbone):
        with pytest.raises(ValueError, match="encoder must be one of"):
            make(encoder="hashes")
    with pytest.raises(ValueError, match="channels must be 32"):     # the width that feeds the LSTM is the encoder's, not free
        policy.Backbone(encoder="hash", channels=256)
    bb = policy.Backbone(encoder="hash", channels=FEATURES, hidden=64, generator=torch.Generator().manual_seed(0))
    assert bb.kind == "hash" and bb.core.hidden == 64 and [k for k, _ in bb.named_parameters()] == ["encoder.params", "core.w_in", "core.w_rec", "core.cell_params"]
    with pytest.raises(ValueError, match="encoder must be None or one of"):
        evaluate.load_policy(state, encoder="simhash")
