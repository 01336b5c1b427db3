"""Action sampling without a GPU (gpu_hideseek.action_sampling, hs_sample_actions): a numpy restatement of what
include/hideseek.h states — Threefry in uint32, the f32 head arithmetic, and the same in float64 — the tolerances the
GPU tests use, derived from the two on the GPU tests' own logits, the cap on draws near a CDF edge, the refusals of
request(), and the header.

Tolerances (printed by test_tolerances_are_derived; DESIGN.md quotes them): each is 4 x the largest deviation of the f32
restatement from the float64 one over every case of CASES.  The deviation of a CDF edge is |c_i / S - cdf64_i| plus 2^-24,
the bound on the relative rounding of the f32 product u * S that the draw compares with c_i."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

HEADS = 5
BUCKETS = ((5, 5, 5, 2, 2), (11, 11, 11, 2, 2))
DTYPES = ("float32", "bfloat16", "float16")
# (worlds, agents per world): one partial block; 36 rows; a partial last block and a partial octet of worlds
SHAPES = ((1, 4), (9, 4), (301, 6))
STRIDED = 40                      # the strided width (>= 37)
SEED, COUNTER = (0x5EED, 7), 3    # the key of the GPU tests' draws
CASES = [(w * a, b, d) for (w, a) in SHAPES for b in BUCKETS for d in DTYPES]
NEAR_EDGE_CAP = 1e-3


# ---- Threefry-2x32-20 and the uniforms, in uint32 ----
def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def threefry2x32(k0, k1, c0, c1):
    k0, k1, c0, c1 = (np.asarray(v, dtype=np.uint32) for v in (k0, k1, c0, c1))
    with np.errstate(over="ignore"):
        ks = (k0, k1, np.uint32(0x1BD11BDA) ^ k0 ^ k1)
        x0, x1 = c0 + ks[0], c1 + ks[1]
        rot = ((13, 15, 26, 6), (17, 29, 16, 24))
        for block in range(5):
            for r in rot[block % 2]:
                x0 = x0 + x1
                x1 = _rotl(x1, r) ^ x0
            x0 = x0 + ks[(block + 1) % 3]
            x1 = x1 + ks[(block + 2) % 3] + np.uint32(block + 1)
    return x0, x1


def uniforms(seed, counter, global_rows):
    """u [rows, 5] f32 of the global agent rows: k = threefry(seed, g, counter), u_h from threefry(k, h, 0)."""
    g = np.asarray(global_rows, dtype=np.uint32)
    k0, k1 = threefry2x32(seed[0], seed[1], g, counter)
    h = np.arange(HEADS, dtype=np.uint32)
    x0, x1 = threefry2x32(k0[:, None], k1[:, None], h[None, :], 0)
    return ((x0 ^ x1) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


# ---- the logits of the GPU tests ----
def to_dtype(x, dtype):
    """f32 values rounded to nearest even into `dtype`, as f32 again (what the kernel's exact widening gives back)."""
    x = np.asarray(x, dtype=np.float32)
    if dtype == "float32":
        return x
    if dtype == "float16":
        return x.astype(np.float16).astype(np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000          # bf16 (no NaN among the logits)
    return b.astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def logits_of(rows, buckets, dtype, seed=0):
    """[rows, L] f32: ~N(0, 2), 2 % of the entries +-30, 5 % -inf but never a whole head; rounded to `dtype`."""
    rng = np.random.default_rng([seed, rows, sum(buckets), DTYPES.index(dtype)])
    L = sum(buckets)
    x = rng.normal(0.0, 2.0, size=(rows, L)).astype(np.float32)
    big = rng.random((rows, L)) < 0.02
    x[big] = np.where(rng.random((rows, L)) < 0.5, np.float32(30), np.float32(-30))[big]
    off = np.concatenate([[0], np.cumsum(buckets)])
    mask = rng.random((rows, L)) < 0.05
    keep = rng.integers(0, 1 << 30, size=(rows, HEADS))
    for h, K in enumerate(buckets):                              # one bucket of every head is never masked
        mask[np.arange(rows), off[h] + keep[:, h] % K] = False
    x[mask] = -np.inf
    x = to_dtype(x, dtype)
    x.setflags(write=False)
    return x


def heads_of(x, buckets):
    off = np.concatenate([[0], np.cumsum(buckets)])
    return [x[:, off[h]:off[h + 1]] for h in range(HEADS)]


# ---- one head, in the kernel's f32 order or in float64 ----
def head_tables(l, ft):
    """(c [R,K] running sums, S, lp [R,K] log-prob of every bucket, entropy [R]) of a head's logits l in type `ft`."""
    l = l.astype(ft)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = l - l.max(1, keepdims=True)
        e = np.exp(d)
        t = np.where(e == 0, ft(0), e * d)
        c, T = np.empty_like(e), t[:, 0].copy()
        c[:, 0] = e[:, 0]
        for i in range(1, l.shape[1]):
            c[:, i] = c[:, i - 1] + e[:, i]
            T = T + t[:, i]
        S = c[:, -1]
        logS = np.log(S)
        lp = d - logS[:, None]
        ent = logS - T / S
    assert c.dtype == ft and lp.dtype == ft and ent.dtype == ft
    return c, S, lp, ent, e


def draw_f32(l, u):
    """The restatement's draw of a head: smallest a with u S < c_a in f32, else the last bucket with e > 0."""
    c, S, _, _, e = head_tables(l, np.float32)
    t = (u * S).astype(np.float32)
    hit = t[:, None] < c
    last = l.shape[1] - 1 - np.argmax((e > 0)[:, ::-1], axis=1)
    return np.where(hit.any(1), hit.argmax(1), last).astype(np.int32)


def sum5(x):
    """(((x0 + x1) + x2) + x3) + x4 in the type of x."""
    return (((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]) + x[:, 4]


def reference64(x, buckets, action):
    """float64: (cdf [5 x [R,K]], head_log_prob [R,5] at `action`, log_prob [R], entropy [R], probability of `action`)."""
    R = x.shape[0]
    cdf, hlp, ent, p = [], np.empty((R, HEADS)), np.empty((R, HEADS)), np.empty((R, HEADS))
    for h, l in enumerate(heads_of(x, buckets)):
        c, S, lp, e_h, e = head_tables(l, np.float64)
        cdf.append(c / S[:, None])
        hlp[:, h] = lp[np.arange(R), action[:, h]]
        p[:, h] = (e / S[:, None])[np.arange(R), action[:, h]]
        ent[:, h] = e_h
    return cdf, hlp, hlp.sum(1), ent.sum(1), p


def near_edge(cdf, u, tol):
    """[R] bool per head list: u within tol of an interior CDF edge."""
    return np.stack([(np.abs(c[:, :-1] - u[:, h:h + 1].astype(np.float64)) <= tol).any(1) for h, c in enumerate(cdf)], 1)


@functools.lru_cache(maxsize=None)
def tolerances():
    """{"cdf", "head_log_prob", "log_prob", "entropy"}: 4 x the largest f32-vs-f64 deviation over CASES."""
    dev = dict(cdf=0.0, head_log_prob=0.0, log_prob=0.0, entropy=0.0)
    for rows, buckets, dtype in CASES:
        x = logits_of(rows, buckets, dtype)
        u = uniforms(SEED, COUNTER, np.arange(rows))
        lp32, lp64, e32, e64, acts = [], [], [], [], []
        for h, l in enumerate(heads_of(x, buckets)):
            c, S, lp, ent, e = head_tables(l, np.float32)
            c6, S6, lp6, ent6, _ = head_tables(l, np.float64)
            dev["cdf"] = max(dev["cdf"], float(np.abs(c.astype(np.float64) / S.astype(np.float64)[:, None] - c6 / S6[:, None]).max()))
            live = e > 0                                         # a bucket of probability 0 has log_prob -inf in both
            dev["head_log_prob"] = max(dev["head_log_prob"], float(np.abs(lp.astype(np.float64)[live] - lp6[live]).max()))
            lp32.append(lp), lp64.append(lp6), e32.append(ent), e64.append(ent6)
            least = np.where(live, lp, np.inf).argmin(1)         # the least likely live bucket: the largest magnitudes
            acts.append((draw_f32(l, u[:, h]), l.argmax(1), least))
        r = np.arange(rows)
        for pick in range(3):                                    # row sums at the drawn, the greedy and the least likely action
            a32 = np.stack([lp32[h][r, acts[h][pick]] for h in range(HEADS)], 1)
            a64 = np.stack([lp64[h][r, acts[h][pick]] for h in range(HEADS)], 1)
            dev["log_prob"] = max(dev["log_prob"], float(np.abs(sum5(a32).astype(np.float64) - a64.sum(1)).max()))
        dev["entropy"] = max(dev["entropy"], float(np.abs(sum5(np.stack(e32, 1)).astype(np.float64) - np.stack(e64, 1).sum(1)).max()))
    dev["cdf"] += 2.0 ** -24
    assert all(np.isfinite(v) and v > 0 for v in dev.values()), dev
    return {k: 4.0 * v for k, v in dev.items()}


# ---- tests ----
def test_uniforms_are_the_core_headers_threefry(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(11)
    out = (C.c_uint32 * 2)()
    for _ in range(60):
        seed = tuple(int(v) for v in rng.integers(0, 1 << 32, size=2))
        counter = int(rng.integers(0, 1 << 32))
        g = rng.integers(0, 1 << 32, size=5).astype(np.uint32)
        g[0] = 0xFFFFFFFF
        u = uniforms(seed, counter, g)
        for i, gi in enumerate(g):
            L.hsref_threefry(seed[0], seed[1], int(gi), counter, out)
            k = (out[0], out[1])
            for h in range(HEADS):
                L.hsref_threefry(k[0], k[1], h, 0, out)
                want = np.float32((out[0] ^ out[1]) >> 8) * np.float32(2.0 ** -24)
                assert u[i, h] == want and 0.0 <= u[i, h] < 1.0, (seed, counter, gi, h)


def test_logits_are_what_the_issue_describes():
    for rows, buckets, dtype in CASES:
        x = logits_of(rows, buckets, dtype)
        assert x.shape == (rows, sum(buckets)) and not np.isnan(x).any() and not np.isposinf(x).any()
        assert np.array_equal(to_dtype(x, dtype), x)             # representable in the narrow type
        for l in heads_of(x, buckets):
            assert np.isfinite(l).any(1).all()                   # never a whole head masked
    x = logits_of(1806, BUCKETS[1], "float32")
    assert 0.03 < np.isneginf(x).mean() < 0.06 and 0.01 < (np.abs(x) == 30).mean() < 0.03
    assert 1.8 < x[np.isfinite(x) & (np.abs(x) != 30)].std() < 2.2


def test_tolerances_are_derived():
    tol = tolerances()
    print("action sampling tolerances (4 x max f32-vs-f64 deviation): " + ", ".join(f"{k} {v:.3e}" for k, v in tol.items()))
    # f32 arithmetic on logits up to 30 apart: between an ulp of a probability and a few thousand ulps of 60
    assert 4 * 2.0 ** -24 < tol["cdf"] < 1e-5
    for k in ("head_log_prob", "log_prob", "entropy"):
        assert 2.0 ** -24 < tol[k] < 1e-3, (k, tol[k])


def test_f32_restatement_meets_its_own_tolerances_and_few_draws_are_near_an_edge():
    tol = tolerances()
    near = total = 0
    for rows, buckets, dtype in CASES:
        x = logits_of(rows, buckets, dtype)
        u = uniforms(SEED, COUNTER, np.arange(rows))
        act = np.stack([draw_f32(l, u[:, h]) for h, l in enumerate(heads_of(x, buckets))], 1)
        cdf, hlp, lp, ent, p = reference64(x, buckets, act)
        assert (p > 0).all()
        for h, c in enumerate(cdf):
            r = np.arange(rows)
            lo = np.where(act[:, h] > 0, c[r, np.maximum(act[:, h] - 1, 0)], 0.0)
            assert ((lo - tol["cdf"] <= u[:, h]) & (u[:, h] < c[r, act[:, h]] + tol["cdf"])).all()
        ne = near_edge(cdf, u, tol["cdf"])
        near, total = near + int(ne.sum()), total + ne.size
        assert ne.sum() < NEAR_EDGE_CAP * ne.size, (rows, buckets, dtype, int(ne.sum()))
    print(f"draws within the CDF tolerance of an edge: {near} of {total}")
    assert near < NEAR_EDGE_CAP * total


def test_request_refuses_before_the_library_is_called():
    from gpu_hideseek import action_sampling as A

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    R, L = 32, 19
    good = torch.zeros(R, L)
    for bad, what in ((torch.zeros(R, L - 1), "shape"), (torch.zeros(R + 1, L), "shape"), (torch.zeros(R * L), "shape"),
                      (torch.zeros(R, 2, L), "shape"), (torch.zeros(R, L, dtype=torch.float64), "dtype"),
                      (torch.zeros(R, L, dtype=torch.int32), "dtype"), (torch.zeros(L, R).t(), "stride"),
                      (torch.zeros(R, 2 * L)[:, ::2], "stride"), (torch.zeros(R * L).as_strided((R, L), (L - 1, 1)), "stride")):
        with pytest.raises(ValueError, match=what):
            A.sample(Sim(), bad)
    with pytest.raises(ValueError, match="shape"):                # wide enough for [5,5,5,2,2] only
        A.sample(Sim(), good, buckets=BUCKETS[1])
    with pytest.raises(ValueError, match="on cpu"):               # a well-formed tensor on the wrong device
        A.sample(Sim(), good)
    with pytest.raises(ValueError, match="on cpu"):
        A.sample(Sim(), torch.zeros(R, STRIDED)[:, :L], log_prob=True)
    for buckets in ((5, 5, 5, 2, 0), (17, 5, 5, 2, 2), (5, 5, 5, 2), (5, 5, 5, 2, 2, 2), (16, 16, 16, 16, 16)):
        with pytest.raises(ValueError, match="buckets"):
            A.sample(Sim(), torch.zeros(R, 80), buckets=buckets)
    with pytest.raises(ValueError, match="mode"):
        A.sample(Sim(), good, mode="sample")
    with pytest.raises(ValueError, match="nothing to do"):
        A.sample(Sim(), good, mode="evaluate")
    with pytest.raises(ValueError, match="nothing to do"):
        A.sample(Sim(), good, mode="evaluate", action=torch.zeros(R, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match="evaluate"):
        A.sample(Sim(), good, mode="evaluate", action=True, log_prob=True)
    with pytest.raises(ValueError, match="seed"):
        A.sample(Sim(), good, seed=(1, 2, 3))
    with pytest.raises(ValueError):
        A.sample(Sim(), [[0.0] * L] * R)


def test_header_states_the_request(hideseek_lib):
    """include/hideseek.h declares both entry points and the enums, and the ctypes mirror agrees with it."""
    from gpu_hideseek import action_sampling as A
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hideseek.h")).read()
    for name, value in (("HS_SAMPLE_HEADS", A.HEADS), ("HS_SAMPLE_MAX_BUCKETS", A.MAX_BUCKETS), ("HS_SAMPLE_MAX_LOGITS", A.MAX_LOGITS),
                        ("HS_SAMPLE_DRAW", A.MODES["draw"]), ("HS_SAMPLE_GREEDY", A.MODES["greedy"]),
                        ("HS_SAMPLE_EVALUATE", A.MODES["evaluate"]), ("HS_SAMPLE_ZERO_INACTIVE", A.ZERO_INACTIVE)):
        assert re.search(rf"{name} = (\d+)", src).group(1) == str(value), name
    assert re.search(r"int32_t hs_sample_actions\(hs_sim \*\w*, const hs_sample_request \*\w*\);", src)
    assert re.search(r"int32_t hs_sample_actions_async\(hs_sim \*\w*, void \*hip_stream, const hs_sample_request \*\w*\);", src)
    R = A.HsSampleRequest
    assert C.sizeof(R) == 88 and R.buckets.offset == 16 and R.mode.offset == 36 and R.seed.offset == 44
    assert R.counter.offset == 52 and R.action.offset == 56 and R.head_log_prob.offset == 80
    lib = C.CDLL(hideseek_lib)
    assert hasattr(lib, "hs_sample_actions") and hasattr(lib, "hs_sample_actions_async")
