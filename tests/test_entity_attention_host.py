"""The attention core of the entity self-attention encoder without a GPU (gpu_hideseek.entity_attention, hs_entity_attend /
hs_entity_attend_backward): a numpy restatement of what include/hideseek.h states, forward and backward, once in f32 in
the header's orders and once in float64; the float64 one against torch's scaled_dot_product_attention (an independent
implementation), its backward against autograd through that function and against central differences; the properties
the header promises (only self valid gives v_0, NaN in masked keys changes nothing, masked keys get +0, p sums to 1); the
tolerances the GPU tests use, derived from the two restatements on the GPU tests' own cases; the refusals of request();
the header; and AttentionEncoder(fused=False) on the CPU.

expf is the device library's and is not pinned bit for bit, so the f32 restatement is not the kernel's bits: the GPU is
compared with it within the tolerance.

Tolerances (printed by test_tolerances_are_derived; DESIGN.md quotes them), none a constant: per case (n, E, dtype) and
per output (out, grad_qkv) 4 x (the project's margin, as in test_value_head_host) the largest deviation of the f32
restatement from the float64 one, plus the rounding of the output's dtype (ROUNDING: half an ulp relative, the smallest
subnormal absolute).
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from test_lstm_cell_host import DTYPES, ROUNDING, to_dtype

S, HEADS, WAVES, MAX_GRID = 17, 4, 4, 2048                                 # asserted against module and header below
EMBED_DIMS = (64, 128)
SEED = 0
SIZES = (1, 3, 5, 37)                                                      # one row; a partial round; one row past a round; ten workgroups
BIG_FWD = (MAX_GRID * WAVES + 3, 64, "float32")                            # past the sweep of 2048 workgroups: forward only
CASES = [(n, E, d) for E in EMBED_DIMS for n in SIZES for d in DTYPES]
OUTPUTS = ("out", "grad_qkv")
CHUNK = 512                                                                # rows restated at a time (memory)


# ---- the contract, in the type `ft` ----
def dot(a, b):
    """The header's dot over the last axis (a head's D channels): four parts of P = D / 4 adjacent channels, each added in
    ascending order from its first product, then the butterfly xor 1, xor 2; every part ends with the same bits."""
    prod = a * b
    P = prod.shape[-1] // 4
    q = prod.reshape(prod.shape[:-1] + (4, P))
    t = q[..., 0]
    for c in range(1, P):
        t = t + q[..., c]
    t = t + t[..., [1, 0, 3, 2]]
    t = t + t[..., [2, 3, 0, 1]]
    return t[..., 0]


def valid_keys(key_mask, n):
    v = np.ones((n, S), bool) if key_mask is None else np.asarray(key_mask) != 0
    v = v.copy()
    v[:, 0] = True
    return v


def probs(ft, q, k, valid):
    """p [n, H, i, j] of q, k [n, S, H, D] in `ft`: 0 at the masked keys, by selects."""
    D = q.shape[-1]
    scale = ft(1) / np.sqrt(ft(D))
    vj = valid[:, None, None, :]
    with np.errstate(all="ignore"):
        s = dot(q.transpose(0, 2, 1, 3)[:, :, :, None, :], k.transpose(0, 2, 1, 3)[:, :, None, :, :]) * scale      # [n, H, i, j]
        m = s[..., 0]
        for j in range(1, S):
            m = np.where(vj[..., j], np.maximum(m, s[..., j]), m)
        e = np.where(vj, np.exp(s - m[..., None]), ft(0))
        l = e[..., 0]
        for j in range(1, S):
            l = np.where(vj[..., j], l + e[..., j], l)
        p = np.where(vj, e / l[..., None], ft(0))
    assert p.dtype == ft
    return p


def weighted(ft, w, x, take):
    """((+0 + w_0 x_0) + w_1 x_1) + ... over axis r: w [n, H, a, r], x [n, r, H, D], take [n, r] (or None: all) -> [n, a, H, D]."""
    n, H, A, R = w.shape
    acc = np.zeros((n, A, H, x.shape[-1]), ft)
    with np.errstate(all="ignore"):
        for r in range(R):
            term = acc + w[:, :, :, r].transpose(0, 2, 1)[..., None] * x[:, r][:, None]
            acc = term if take is None else np.where(take[:, r][:, None, None, None], term, acc)
    return acc


def _forward(ft, qkv, key_mask):
    qkv = np.asarray(qkv).astype(ft)
    n = qkv.shape[0]
    valid = valid_keys(key_mask, n)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    p = probs(ft, q, k, valid)
    return dict(out=weighted(ft, p, v, valid).reshape(n, S, -1), p=p)


def _backward(ft, qkv, key_mask, grad_out):
    qkv = np.asarray(qkv).astype(ft)
    n, D = qkv.shape[0], qkv.shape[-1]
    scale = ft(1) / np.sqrt(ft(D))
    valid = valid_keys(key_mask, n)
    vj = valid[:, None, None, :]
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    g = np.asarray(grad_out).astype(ft).reshape(n, S, HEADS, D)
    p = probs(ft, q, k, valid)
    with np.errstate(all="ignore"):
        dp = dot(g.transpose(0, 2, 1, 3)[:, :, :, None, :], v.transpose(0, 2, 1, 3)[:, :, None, :, :])             # [n, H, i, j]
        t = np.zeros(dp.shape[:-1], ft)
        for j in range(S):
            t = np.where(vj[..., j], t + p[..., j] * dp[..., j], t)
        ds = np.where(vj, p * (dp - t[..., None]), ft(0))
    dq = weighted(ft, ds, k, valid) * scale
    pT, dsT = p.transpose(0, 1, 3, 2), ds.transpose(0, 1, 3, 2)                                                # [n, H, j, i]
    on = valid[:, :, None, None]
    dv = np.where(on, weighted(ft, pT, g, None), ft(0))
    dk = np.where(on, weighted(ft, dsT, q, None) * scale, ft(0))
    out = np.stack([dq, dk, dv], 2)
    assert out.dtype == ft and out.shape == qkv.shape
    return dict(grad_qkv=out)


def _chunked(f, n, *arrays):
    parts = [f(*[None if a is None else a[i:i + CHUNK] for a in arrays]) for i in range(0, n, CHUNK)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def forward(ft, qkv, key_mask=None):
    """hs_entity_attend in float type `ft`: out [n, 17, E] (not yet rounded to a narrow dtype) and p [n, H, i, j]."""
    return _chunked(functools.partial(_forward, ft), len(qkv), qkv, key_mask)


def backward(ft, qkv, key_mask, grad_out):
    """hs_entity_attend_backward in float type `ft`: grad_qkv with the shape of qkv."""
    return _chunked(functools.partial(_backward, ft), len(qkv), qkv, key_mask, grad_out)


# ---- the inputs of the GPU tests ----
SPECIAL = {1: "all valid", 2: "all-zero bytes", 3: "only self"}            # rows r with r % 7 in SPECIAL


@functools.lru_cache(maxsize=None)
def _inputs(n, E, dtype, seed):
    rng = np.random.default_rng([seed, n, E, DTYPES.index(dtype), 9])
    D = E // HEADS
    mask = (rng.random((n, S)) < 0.5).astype(np.uint8) * rng.integers(1, 256, (n, S)).astype(np.uint8)         # any nonzero byte counts
    for r in range(n):
        if r % 7 == 1:
            mask[r] = 1
        elif r % 7 == 2:
            mask[r] = 0
        elif r % 7 == 3:
            mask[r] = 0
            mask[r, 0] = 1
    x = dict(qkv=to_dtype(rng.standard_normal((n, S, 3, HEADS, D)), dtype), key_mask=mask, grad_out=to_dtype(rng.standard_normal((n, S, E)), dtype))
    for v in x.values():
        v.setflags(write=False)
    return x


def inputs(n, E, dtype, seed=SEED):
    """A fresh dict of the (shared, read-only) arrays of a case: qkv and grad_out N(0, 1) and representable in `dtype`,
    key_mask about half valid with the special rows of SPECIAL."""
    return dict(_inputs(n, E, dtype, seed))


def run(ft, x, mask=True):
    km = x["key_mask"] if mask else None
    out = forward(ft, x["qkv"], km)
    out.update(backward(ft, x["qkv"], km, x["grad_out"]))
    return out


@functools.lru_cache(maxsize=None)
def both(case, mask=True):
    """(f32 restatement, float64 restatement) of a case, forward and backward (BIG_FWD: forward).  Computed once, shared,
    left unchanged."""
    x = inputs(*case)
    if case == BIG_FWD:
        return tuple(forward(ft, x["qkv"], x["key_mask"] if mask else None) for ft in (np.float32, np.float64))
    return run(np.float32, x, mask), run(np.float64, x, mask)


def gaps(r32, r64):
    return {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in OUTPUTS if k in r32}


def tolerance(case, mask=True):
    """{output: 4 x the largest |f32 - float64| of it in this case}."""
    return {k: 4.0 * v for k, v in gaps(*both(case, mask)).items()}


def bound(name, want, case, tol=None, mask=True):
    """The bound on |got - want| of output `name` of a case: the derived tolerance plus the rounding of the case's dtype
    (out and grad_qkv are stored in it)."""
    tol = tolerance(case, mask) if tol is None else tol
    rel, absolute = ROUNDING[case[2]]
    return tol[name] + rel * np.abs(np.asarray(want, np.float64)) + absolute


# ---- the encoder: the allowance for the GEMMs' dtype and order ----
ENCODER = dict(n=37, E=64, out=64)


def encoder_net(fused, device="cpu", E=None, out=None):
    """AttentionEncoder with the parameters every test of the module shares: seeded, and biases, scales and shifts off
    their initial 0 / 1 / 0 so that their gradients matter."""
    from gpu_hideseek import entity_attention as A
    net = A.AttentionEncoder(E or ENCODER["E"], out or ENCODER["out"], fused=fused, generator=torch.Generator().manual_seed(11))
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for layer in (*net.tokens.values(), net.residual, net.project):
            v = layer.named_views()
            Cn = layer.channels
            v["bias"].copy_(0.1 * torch.randn(Cn, generator=g))
            v["scale"].copy_(1.0 + 0.2 * torch.randn(Cn, generator=g))
            v["shift"].copy_(0.1 * torch.randn(Cn, generator=g))
        net.b_qkv.copy_(0.1 * torch.randn(net.b_qkv.shape, generator=g))
    return net.to(device)


def synthetic_rows(n, seed=5):
    """Rows [n, 296] N(0, 1) with about a third of the agents, boxes and ramps exactly zero (masked out)."""
    from gpu_hideseek import entity_attention as A
    from gpu_hideseek.policy_inputs import TABLES
    rng = np.random.default_rng([SEED, seed])
    rows = rng.standard_normal((n, 296)).astype(np.float32)
    for name, _, count, K in A.table_tokens():
        if name == "self":
            continue
        lo = TABLES[name][0]
        for e in range(count):
            gone = rng.random(n) < 0.35
            rows[gone, lo + e * K:lo + (e + 1) * K] = 0.0
    return rows


def encoder_eager(ft, rows, weight, device="cpu", masked=True, **kw):
    """AttentionEncoder(fused=False) and its autograd in torch dtype `ft`: features and every parameter's gradient of
    loss = sum(features * weight) + 0.5 * mean(features^2), as float64 numpy."""
    net = encoder_net(False, device, **kw).to(ft)
    f = net(None, torch.from_numpy(np.array(rows)).to(device).to(ft), ft, masked)
    (f * torch.from_numpy(np.array(weight)).to(device).to(ft)).sum().add(0.5 * (f ** 2).mean()).backward()
    out = {"features": f.detach()}
    out.update({k: p.grad for k, p in net.named_parameters()})
    return {k: v.double().cpu().numpy() for k, v in out.items()}


def encoder_allowance(rows, weight, masked=True, **kw):
    """({quantity: 4 x the largest |torch f32 - torch float64| of it on the CPU}, the float64 results): the rule of
    tests/test_gpu_policy.py, on the rows and parameters given."""
    f32, f64 = (encoder_eager(ft, rows, weight, masked=masked, **kw) for ft in (torch.float32, torch.float64))
    return {k: 4.0 * float(np.abs(f32[k] - f64[k]).max()) for k in f64}, f64


# ---- tests: the kernel's contract ----
def _sdpa(qkv, key_mask):
    """torch's scaled_dot_product_attention in float64 on the CPU, with a boolean mask: [n, S, E]."""
    n = qkv.shape[0]
    q, k, v = (qkv[:, :, c].permute(0, 2, 1, 3) for c in range(3))                                             # [n, H, S, D]
    valid = torch.from_numpy(valid_keys(key_mask, n))
    out = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=valid[:, None, None, :])
    return out.permute(0, 2, 1, 3).reshape(n, S, -1)


def test_float64_restatement_is_torchs_attention_and_its_autograd():
    for E in EMBED_DIMS:
        case = (37, E, "float32")
        x = inputs(*case)
        r64 = both(case)[1]
        qkv = torch.from_numpy(np.array(x["qkv"])).double().requires_grad_()
        out = _sdpa(qkv, x["key_mask"])
        (out * torch.from_numpy(np.array(x["grad_out"])).double()).sum().backward()
        for k, t in (("out", out), ("grad_qkv", qkv.grad)):
            err = float(np.abs(t.detach().numpy() - r64[k]).max())
            limit = 2.0 ** -52 * 1024 * max(float(np.abs(r64[k]).max()), 1.0)      # the same mathematics in another order, in float64
            print(f"E = {E}: {k}: largest |torch sdpa float64 - restatement| = {err:.3e} (bound {limit:.3e})")
            assert err <= limit, (E, k)


def test_backward_is_the_gradient_of_the_forward():
    """Central differences of the float64 forward; softmax attention is smooth, so nothing has to be kept clear of."""
    n, E, h = 3, 64, 1e-6
    x = inputs(5, E, "float32")
    qkv, km, w = x["qkv"][:n].astype(np.float64), x["key_mask"][:n], x["grad_out"][:n].astype(np.float64)
    got = backward(np.float64, qkv, km, w)["grad_qkv"]

    def loss(v):
        return float((forward(np.float64, v, km)["out"] * w).sum())
    L, flat, gmax, worst = abs(loss(qkv)), got.reshape(-1), float(np.abs(got).max()), 0.0
    picks = np.arange(0, flat.size, 7)
    limit = 16 * 2.0 ** -52 * max(L, 1.0) / h + h * max(gmax, 1.0)
    for i in picks:
        v = qkv.copy()
        v.reshape(-1)[i] += h
        up = loss(v)
        v.reshape(-1)[i] -= 2 * h
        worst = max(worst, abs((up - loss(v)) / (2 * h) - flat[i]))
    print(f"{picks.size} probed: largest |central difference - backward| = {worst:.3e} (bound {limit:.3e}, largest gradient {gmax:.3e})")
    assert worst <= limit and limit < 1e-3 * gmax
    assert (km[1] == 1).all() and not km[2].any()                            # an all-valid and an all-zero-bytes row were probed


def test_properties_of_the_restatement():
    for E, dtype in ((64, "float32"), (128, "bfloat16")):
        x = inputs(37, E, dtype)
        D = E // HEADS
        valid = valid_keys(x["key_mask"], 37)
        assert valid[2].sum() == 1 and valid[3].sum() == 1 and valid[1].all() and 0.3 < valid[:, 1:].mean() < 0.7
        r = run(np.float32, x)
        # only self valid: out_i = v_0, bit for bit (p = e / e = 1, +0 + 1 * v = v)
        for row in (2, 3):
            v0 = x["qkv"][row, 0, 2].reshape(E)
            assert np.array_equal(r["out"][row].view(np.uint32), np.broadcast_to(v0, (S, E)).view(np.uint32)), (E, row)
        # NaN and Inf in the masked keys' k and v change nothing
        bad = np.array(x["qkv"])
        gone = ~valid
        bad[:, :, 1][gone] = np.nan
        bad[:, :, 2][gone] = np.inf
        rb = run(np.float32, dict(x, qkv=bad))
        assert np.array_equal(rb["out"].view(np.uint32), r["out"].view(np.uint32))
        assert np.array_equal(rb["grad_qkv"].view(np.uint32), r["grad_qkv"].view(np.uint32)) and np.isfinite(rb["grad_qkv"]).all()
        # masked keys: dk and dv exactly +0; the valid ones are not all zero
        g = r["grad_qkv"]
        assert not g[:, :, 1:][gone].view(np.uint32).any() and g[:, :, 1:][valid].any() and g[:, :, 0][gone].any()
        # every p row sums to 1 within n roundings of f32 on 17 terms of at most 1
        p = r["p"]
        assert p.shape == (37, HEADS, S, S) and float(np.abs(p.astype(np.float64).sum(-1) - 1).max()) <= 17 * 2.0 ** -24 and (p >= 0).all()
        assert not p[np.broadcast_to(gone[:, None, None, :], p.shape)].any()
        # a zero grad_out: grad_qkv all +0
        z = backward(np.float32, x["qkv"], x["key_mask"], np.zeros_like(x["grad_out"]))["grad_qkv"]
        assert not z.view(np.uint32).any()
        # the null mask is the all-valid mask
        full = forward(np.float32, x["qkv"], None)["out"]
        assert np.array_equal(full, forward(np.float32, x["qkv"], np.ones((37, S), np.uint8))["out"]) and np.array_equal(full[1], r["out"][1])
        assert D in (16, 32)


def test_tolerances_are_derived():
    for case in CASES + [BIG_FWD]:
        for mask in (True, False):
            if case == BIG_FWD and not mask:
                continue
            tol = tolerance(case, mask)
            print(f"attention core, n = {case[0]}, E = {case[1]}, {case[2]}, {'masked' if mask else 'null mask'}: " + ", ".join(f"{k} {v:.3e}" for k, v in tol.items()))
            r32, r64 = both(case, mask)
            # out is a convex combination of N(0, 1) values and the gradients sums of 17 products: a few f32 ulps of values below 10
            assert 0 < tol["out"] < 1e-4 and 0 < tol.get("grad_qkv", 1e-6) < 1e-3, case
            for k in tol:
                assert (np.abs(r32[k].astype(np.float64) - r64[k]) <= bound(k, r64[k], case, mask=mask)).all(), (case, k)
    assert len(CASES) == 24 and BIG_FWD[0] == 8195


def test_inputs_are_what_the_issue_describes():
    x = inputs(37, 128, "bfloat16")
    assert np.array_equal(to_dtype(x["qkv"], "bfloat16"), x["qkv"]) and np.array_equal(to_dtype(x["grad_out"], "bfloat16"), x["grad_out"])
    assert x["qkv"].shape == (37, S, 3, HEADS, 32) and x["key_mask"].dtype == np.uint8 and 0.9 < x["qkv"].std() < 1.1
    p = both((37, 128, "bfloat16"))[1]["p"]
    top = p.max(-1)
    assert 0.15 < float(np.median(top)) < 0.9                                # neither flat (1 / 17) nor one-hot
    kinds = {r % 7 for r in range(37)}
    assert set(SPECIAL) <= kinds and (x["key_mask"] > 1).any()


def test_eager_and_its_autograd_are_the_restatement():
    from gpu_hideseek import entity_attention as A
    for E in EMBED_DIMS:
        case = (5, E, "float32")
        x = inputs(*case)
        r64 = both(case)[1]
        for ft in (torch.float64, torch.float32):
            qkv = torch.from_numpy(np.array(x["qkv"])).to(ft).requires_grad_()
            out = A.eager(qkv, torch.from_numpy(np.array(x["key_mask"])))
            assert out.dtype == ft and out.shape == (5, S, E)
            (out * torch.from_numpy(np.array(x["grad_out"])).to(ft)).sum().backward()
            for k, t in dict(out=out, grad_qkv=qkv.grad).items():
                err = np.abs(t.detach().double().numpy() - r64[k])
                if ft is torch.float64:
                    assert err.max() <= 2.0 ** -52 * 1024 * max(float(np.abs(r64[k]).max()), 1.0), (E, k)
                else:
                    assert (err <= 4.0 * bound(k, r64[k], case)).all(), (E, k, float(err.max()))
        assert A.eager(torch.from_numpy(np.array(x["qkv"])).bfloat16()).dtype == torch.float32
        # NaN in a masked key does not reach eager's output either
        bad = np.array(x["qkv"])
        bad[:, :, 1:][~valid_keys(x["key_mask"], 5)] = np.nan
        assert torch.equal(A.eager(torch.from_numpy(bad), torch.from_numpy(np.array(x["key_mask"]))), A.eager(torch.from_numpy(np.array(x["qkv"])), torch.from_numpy(np.array(x["key_mask"]))))


def test_constants_and_tokens():
    from gpu_hideseek import entity_attention as A
    from gpu_hideseek.policy_inputs import TABLES
    assert (A.TOKENS, A.HEADS, A.EMBED_DIMS, A.ALIGN, A.ROWS_PER_ROUND, A.MAX_GRID) == (S, HEADS, EMBED_DIMS, 16, WAVES, MAX_GRID)
    toks = A.table_tokens()
    assert [t[0] for t in toks] == list(TABLES) == ["self", "agents", "boxes", "ramps"] and [t[1:] for t in toks] == [(0, 1, 45), (1, 5, 14), (6, 9, 17), (15, 2, 14)]


def test_request_refuses_before_the_library_is_called():
    from gpu_hideseek import entity_attention as A

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    n, E = 6, 64
    D = E // HEADS
    good = dict(qkv=torch.zeros(n, S, 3, HEADS, D), key_mask=torch.ones(n, S, dtype=torch.uint8))

    def call(**kw):
        a = dict(good, **kw)
        return A.compute(Sim(), a.pop("qkv"), a.pop("key_mask"), **a)

    def back(**kw):
        a = dict(dict(good, grad_out=torch.zeros(n, S, E)), **kw)
        return A.compute_backward(Sim(), a.pop("qkv"), a.pop("key_mask"), a.pop("grad_out"), **a)

    def off(shape, dtype=torch.float32, by=1):
        """A contiguous view that starts `by` elements into its allocation: not 16-byte aligned."""
        size = int(np.prod(shape))
        t = torch.zeros(size + 8, dtype=dtype)[by:by + size].view(shape)
        assert t.is_contiguous() and t.data_ptr() % 16
        return t
    qs = (n, S, 3, HEADS, D)
    for f in (call, back):
        for bad, what in ((torch.zeros(n, S, 3, HEADS, 8), "shape"), (torch.zeros(n, S, 3, HEADS, 64), "shape"), (torch.zeros(n, S, 3 * E), "shape"),
                          (torch.zeros(n, S - 1, 3, HEADS, D), "shape"), (torch.zeros(n, S, 3, 2, 2 * D), "shape"), (torch.zeros(0, S, 3, HEADS, D), "shape"),
                          (torch.zeros(qs, dtype=torch.float64), "dtype"), (torch.zeros(n, S, 3, HEADS, 2 * D)[..., :D], "contiguous"), (None, "qkv must"),
                          (off(qs), "16-byte aligned"), (off(qs, torch.bfloat16, 3), "16-byte aligned"), (off(qs, torch.float16, 4), "16-byte aligned")):
            with pytest.raises(ValueError, match=what):
                f(qkv=bad)
        for bad, what in ((torch.ones(n, S + 1, dtype=torch.uint8), "shape"), (torch.ones(n + 1, S, dtype=torch.uint8), "shape"), (torch.ones(n, S, dtype=torch.bool), "dtype"),
                          (torch.ones(n, S), "dtype"), (torch.ones(n, 2 * S, dtype=torch.uint8)[:, ::2], "contiguous"), (3, "key_mask must")):
            with pytest.raises(ValueError, match=what):
                f(key_mask=bad)
        with pytest.raises(ValueError, match="on cpu"):               # well-formed tensors on the wrong device
            f()
        with pytest.raises(ValueError, match="on cpu"):
            f(key_mask=None)
    os_ = (n, S, E)
    for bad, what in ((torch.zeros(n, S, E - 1), "shape"), (torch.zeros(n, S * E), "shape"), (torch.zeros(os_, dtype=torch.float64), "dtype"),
                      (torch.zeros(n, S, 2 * E)[..., ::2], "contiguous"), (3.0, "out must"), (off(os_), "16-byte aligned"), (off(os_, torch.bfloat16), "16-byte aligned")):
        with pytest.raises(ValueError, match=what):
            call(out=bad)
    for none in (None, False):
        with pytest.raises(ValueError, match="nothing to do"):
            call(out=none)
    with pytest.raises(ValueError, match="out_dtype"):
        call(out_dtype=torch.float64)
    shared = torch.zeros(n * S * 4 * E + 64)
    with pytest.raises(ValueError, match="out overlaps qkv"):
        call(qkv=shared[:n * S * 3 * E].view(qs), out=shared[E:E + n * S * E].view(os_))
    with pytest.raises(ValueError, match="out overlaps key_mask"):
        call(key_mask=shared.view(torch.uint8)[:n * S].view(n, S), out=shared[:n * S * E].view(os_))
    for name, bad, what in (("grad_out", torch.zeros(n, S, E + 1), "shape"), ("grad_out", torch.zeros(os_, dtype=torch.float64), "dtype"),
                            ("grad_out", torch.zeros(n, S, 2 * E)[..., ::2], "contiguous"), ("grad_out", None, "grad_out"), ("grad_out", off(os_), "16-byte aligned"),
                            ("grad_qkv", torch.zeros(n + 1, S, 3, HEADS, D), "shape"), ("grad_qkv", torch.zeros(qs, dtype=torch.float16), "dtype"),
                            ("grad_qkv", off(qs), "16-byte aligned"), ("grad_qkv", 2, "grad_qkv")):
        with pytest.raises(ValueError, match=what):
            back(**{name: bad})
    with pytest.raises(ValueError, match="nothing to do"):
        back(grad_qkv=None)
    with pytest.raises(ValueError, match="grad_qkv overlaps qkv"):
        back(grad_qkv=good["qkv"])
    with pytest.raises(ValueError, match="grad_qkv overlaps grad_out"):
        back(grad_out=shared[:n * S * E].view(os_), grad_qkv=shared[16:16 + n * S * 3 * E].view(qs))


def test_header_mirror_and_symbols_agree(hideseek_lib):
    """include/hideseek.h declares the four entry points, the ctypes mirrors agree with it field by field, and the kernel's
    constants are the module's."""
    from gpu_hideseek import entity_attention as A
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hideseek.h")).read()
    for name, value in (("HS_ATTEND_TOKENS", S), ("HS_ATTEND_HEADS", HEADS), ("HS_ATTEND_ROWS_PER_ROUND", WAVES), ("HS_ATTEND_MAX_GRID", MAX_GRID)):
        assert re.search(rf"{name} = (\d+)", src).group(1) == str(value), name
    assert "HS_ATTEND_MAX_ROWS = 1 << 24" in src and A.MAX_ROWS == 1 << 24
    pairs = (("hs_entity_attend", "hs_entity_attend_request", A.HsEntityAttendRequest),
             ("hs_entity_attend_backward", "hs_entity_attend_backward_request", A.HsEntityAttendBackwardRequest))
    for fn, req, mirror in pairs:
        assert re.search(rf"int32_t {fn}\(hs_sim \*\w*, const {req} \*\w*\);", src)
        assert re.search(rf"int32_t {fn}_async\(hs_sim \*\w*, void \*hip_stream, const {req} \*\w*\);", src)
        body = re.search(rf"typedef struct {req} \{{(.*?)\}} {req};", src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            if decl.strip():
                for word in ("const", "int32_t", "uint8_t", "float", "void"):
                    decl = re.sub(rf"\b{word}\b", "", decl)
                names += [part.split()[-1].lstrip("*") for part in decl.split(",")]
        assert names == [f[0] for f in mirror._fields_], names
    F, B = A.HsEntityAttendRequest, A.HsEntityAttendBackwardRequest
    assert C.sizeof(F) == 40 and F.key_mask.offset == 8 and F.n.offset == 16 and F.out_dtype.offset == 28 and F.out.offset == 32
    assert C.sizeof(B) == 48 and B.grad_out.offset == 16 and B.n.offset == 24 and B.grad_dtype.offset == 36 and B.grad_qkv.offset == 40
    lib = C.CDLL(hideseek_lib)
    for fn in ("hs_entity_attend", "hs_entity_attend_async", "hs_entity_attend_backward", "hs_entity_attend_backward_async"):
        assert hasattr(lib, fn)
    entry = open(os.path.join(root, "__graft_entry__.py")).read()
    assert all(f'"{fn}"' in entry for fn, _, _ in pairs) and all(f'"{fn}_async"' in entry for fn, _, _ in pairs)
    csrc = os.path.join(root, "marl-hideandseek_amd", "csrc")
    kernel, host = (open(os.path.join(csrc, f)).read() for f in ("hs_k_attend.h", "hideseek.hip"))
    assert re.search(r"kAttendTokens = (\d+),", kernel).group(1) == str(S) and re.search(r"kAttendHeads = (\d+);", kernel).group(1) == str(HEADS)
    assert "HS_ATTEND_MAX_GRID == hs::kRowsMaxGrid" in host and "HS_ATTEND_ROWS_PER_ROUND == hs::kRowsWaves" in host and "atomic" not in kernel.lower().replace("no atomics", "")


# ---- the encoder on the CPU, with eager pieces ----
def test_encoder_shapes_and_parameters():
    from gpu_hideseek import entity_attention as A
    net = A.AttentionEncoder(generator=torch.Generator().manual_seed(1))
    assert (net.embed, net.out, net.heads, net.fused) == (128, 256, 4, True) and isinstance(net, torch.nn.Module)
    shapes = {k: tuple(p.shape) for k, p in net.named_parameters()}
    assert shapes == {"w_qkv": (128, 384), "b_qkv": (384,), "tokens.self.weight": (45, 128), "tokens.self.params": (384,), "tokens.agents.weight": (14, 128),
                      "tokens.agents.params": (384,), "tokens.boxes.weight": (17, 128), "tokens.boxes.params": (384,), "tokens.ramps.weight": (14, 128),
                      "tokens.ramps.params": (384,), "residual.weight": (128, 128), "residual.params": (384,), "project.weight": (128, 256), "project.params": (768,)}
    w = net.tokens["boxes"].weight.detach()                                 # orthogonal with gain sqrt(2): the columns of [17, 128]^T
    assert torch.allclose(w @ w.t(), 2.0 * torch.eye(17), atol=1e-4) and net.residual.slope == 1.0 and not net.b_qkv.any()
    net.fused = False
    assert not net.fused and not net.tokens["self"].fused
    rows = torch.from_numpy(synthetic_rows(7))
    for masked in (True, False):
        f = net(None, rows, None, masked)
        assert f.shape == (7, 256) and f.dtype == torch.float32 and torch.isfinite(f).all()
    assert net(None, rows.bfloat16(), None, True).dtype == torch.bfloat16
    for kw, what in ((dict(embed=96), "embed"), (dict(heads=8), "heads"), (dict(out=100), "channels")):
        with pytest.raises(ValueError, match=what):
            A.AttentionEncoder(**kw)


def test_encoder_works_many_rows_in_pieces(monkeypatch):
    """Rows beyond what one dense call can index: the features are those of the pieces, and so are the gradients."""
    from gpu_hideseek import entity_attention as A
    rows = torch.from_numpy(synthetic_rows(11)).double()
    outs = []
    for limit in (A.INDEX_LIMIT, 4 * S * ENCODER["E"] + 1):                  # whole, and four rows at a time (three pieces)
        monkeypatch.setattr(A, "INDEX_LIMIT", limit)
        net = encoder_net(False).double()
        f = net(None, rows, None, True)
        f.square().sum().backward()
        outs.append((f.detach(), net.w_qkv.grad.clone()))
    assert outs[0][0].shape == (11, ENCODER["out"]) and torch.equal(outs[0][0], outs[1][0])
    assert float((outs[0][1] - outs[1][1]).abs().max()) <= 2.0 ** -52 * 64 * float(outs[0][1].abs().max())


def test_encoder_ignores_masked_entities():
    """masked=True: the features are those of a hand composition in which every masked-out entity's token is replaced by
    noise before the QKV GEMM and left out of the pool, and they differ from masked=False on the same rows."""
    from gpu_hideseek import entity_attention as A
    from gpu_hideseek import mlp as M
    from gpu_hideseek.policy_inputs import TABLES
    n = 9
    net = encoder_net(False).double()
    rows = torch.from_numpy(synthetic_rows(n)).double()
    got = net(None, rows, None, True).detach()
    mask = net.key_mask(rows)
    want = np.ones((n, S), np.uint8)
    for name, first, count, K in A.table_tokens()[1:]:
        lo = TABLES[name][0]
        for e in range(count):
            want[:, first + e] = (rows[:, lo + e * K:lo + (e + 1) * K] != 0).any(1).numpy()
    assert np.array_equal(mask.numpy(), want) and mask.dtype == torch.uint8 and 0.2 < 1 - want[:, 1:].mean() < 0.5
    xs = []
    for name, _, count, K in A.table_tokens():
        lo, hi, _ = TABLES[name]
        xs.append(net.tokens[name](None, rows[:, lo:hi].reshape(n * count, K)).reshape(n, count, -1))
    x = torch.cat(xs, 1)
    valid = mask.bool()
    x = torch.where(valid[..., None], x, 3.0 * torch.randn(x.shape, dtype=x.dtype, generator=torch.Generator().manual_seed(4)))
    qkv = (x @ net.w_qkv + net.b_qkv).reshape(n, S, 3, HEADS, -1)
    y = M.eager((x + A.eager(qkv, mask) @ net.residual.weight).reshape(n * S, -1), net.residual.params, net.residual.eps, 1.0).reshape(n, S, -1)
    pooled = torch.stack([y[r][valid[r]].mean(0) for r in range(n)])
    hand = net.project(None, pooled).detach()
    assert float((got - hand).abs().max()) <= 2.0 ** -52 * 4096 * max(float(hand.abs().max()), 1.0)
    assert float((got - net(None, rows, None, False).detach()).abs().max()) > 1e-3


def test_encoder_backward_is_the_gradient():
    """A central difference through the whole encoder in float64, masked and not."""
    n, h = 5, 1e-6
    rows, weight = synthetic_rows(n), np.random.default_rng([SEED, 6]).standard_normal((n, ENCODER["out"]))
    for masked in (True, False):
        f64 = encoder_eager(torch.float64, rows, weight, masked=masked)

        def loss(net):
            f = net(None, torch.from_numpy(rows).double(), torch.float64, masked)
            return float((f * torch.from_numpy(weight)).sum().add(0.5 * (f ** 2).mean()))
        for name in ("w_qkv", "b_qkv", "tokens.boxes.weight", "tokens.self.params", "residual.weight", "residual.params", "project.weight"):
            net = encoder_net(False).double()
            p = dict(net.named_parameters())[name]
            grad, flat = f64[name].reshape(-1), p.detach().reshape(-1)
            gmax, worst = float(np.abs(grad).max()), 0.0
            with torch.no_grad():
                for i in range(0, flat.numel(), max(1, flat.numel() // 12)):
                    old = float(flat[i])
                    flat[i] = old + h
                    up = loss(net)
                    flat[i] = old - h
                    worst = max(worst, abs((up - loss(net)) / (2 * h) - grad[i]))
                    flat[i] = old
            print(f"masked {masked}: {name}: largest |central difference - autograd| = {worst:.3e} (largest gradient {gmax:.3e})")
            assert gmax > 0 and worst <= 1e-5 * max(gmax, 1.0), (masked, name)


# ---- the policy with and without the new argument ----
def test_the_default_policy_is_what_it_was():
    """make_policy() with no new argument: the 24 parameter names, the flat length of tests/test_optim_host.py, and the bits
    of a composition written out here piece by piece in the order the backbones have always drawn from the generator."""
    from gpu_hideseek import entity_encoder, mlp, optim, policy as P, recurrent
    net = P.make_policy(fused=False, generator=torch.Generator().manual_seed(3))
    names = [k for k, _ in net.named_parameters()]
    per = ["encoder.params", "mlp.layers.0.weight", "mlp.layers.0.params", "mlp.layers.1.weight", "mlp.layers.1.params", "mlp.layers.2.weight",
           "mlp.layers.2.params", "core.w_in", "core.w_rec", "core.cell_params"]
    assert names == ["actor." + k for k in per] + ["critic." + k for k in per] + ["actor_head.weight", "actor_head.bias", "critic_head.weight", "critic_head.bias"]
    assert net.encoder == "simple" and optim.flatten(net.named_parameters(), "cpu").params.numel() == 1532992
    g = torch.Generator().manual_seed(3)
    want = []
    for _ in ("actor", "critic"):
        pieces = (entity_encoder.EntityEncoder(64, generator=g), mlp.MLP(256, 256, 3, generator=g), recurrent.LSTMCore(256, 256, generator=g))
        want += [p for piece in pieces for p in piece.parameters()]
    head = torch.empty(19, 256)
    torch.nn.init.orthogonal_(head, gain=0.01, generator=g)
    want += [head, torch.zeros(19), torch.zeros(255, 256), torch.zeros(255)]
    same = P.make_policy(fused=False, generator=torch.Generator().manual_seed(3), encoder="simple")
    for k, a, b, c in zip(names, net.parameters(), want, same.parameters()):
        assert a.shape == b.shape and torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), k
        assert torch.equal(a.detach().view(torch.int32), c.detach().view(torch.int32)), k
    att = P.make_policy(fused=False, generator=torch.Generator().manual_seed(3), encoder="attention")
    assert att.encoder == "attention" and att.actor.masked and not att.critic.masked and att.actor.core.hidden == net.actor.core.hidden == 256
    assert [k for k, _ in att.named_parameters()][-4:] == names[-4:] and not any(".mlp." in k for k, _ in att.named_parameters())
    with pytest.raises(ValueError, match="encoder"):
        P.Backbone(encoder="hash")
    # one step and a chunk on the CPU with eager pieces: the shapes of the simple policy's
    rows = torch.from_numpy(synthetic_rows(6)).reshape(2, 3, 296)
    state = att.init_state(3, "cpu")
    lg, cl, state2 = att(None, rows[0], rows[0], state)
    seq = att.sequence(None, rows, rows, state)
    assert lg.shape == (3, 19) and cl.shape == (3, 255) and seq[0].shape == (2, 3, 19) and torch.allclose(seq[0][0], lg, atol=1e-6)
