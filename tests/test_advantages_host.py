"""The contract of hs_compute_gae (include/hideseek.h) restated in numpy, and what can be checked of it without a GPU:
first principles in float64, the distance of the f32 restatement from float64, masked steps, the refusals of
gpu_hideseek.advantages.request and the agreement of the ctypes mirror with the header.  tests/test_gpu_advantages.py
compares the kernel with gae_f32 bit for bit on the inputs made here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, LAMBDA = 0.998, 0.95                       # scripts/jax_train.py:152-153
DTYPES = ("float32", "bfloat16", "float16")
F = np.float32


def gae_f32(reward, done, value, bootstrap, mask, gamma, lam):
    """The contract, every operation an explicit IEEE f32 operation in the stated order, selects where it says select.
    reward [T, R] f32, done [T, R] integers, value [T, R] and bootstrap [R] f32 (narrow values already widened), mask
    [T, R] f32 or None.  Returns (advantage, returns), [T, R] f32."""
    reward, value, bootstrap = np.asarray(reward), np.asarray(value), np.asarray(bootstrap)
    assert reward.dtype == F and value.dtype == F and bootstrap.dtype == F
    T, R = reward.shape
    g = F(gamma)
    gl = g * F(lam)
    assert type(gl) is F
    zero = np.zeros(R, F)
    carry, vn = zero, bootstrap
    adv, ret = np.empty((T, R), F), np.empty((T, R), F)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            v, r = value[t], reward[t]
            active = np.ones(R, bool) if mask is None else np.asarray(mask[t]) != 0
            ended = np.asarray(done[t]) != 0
            delta = np.where(ended, r - v, (r + g * vn) - v)
            run = np.where(ended, delta, delta + gl * carry)
            a = np.where(active, run, zero)
            rt = np.where(active, run + v, zero)
            assert a.dtype == F and rt.dtype == F
            adv[t], ret[t] = a, rt
            carry, vn = a, v
    return adv, ret


def gae_f64(reward, done, value, bootstrap, mask, gamma, lam):
    """The same recurrence in float64 (gamma and lambda as given)."""
    reward, value, vn = np.asarray(reward, np.float64), np.asarray(value, np.float64), np.asarray(bootstrap, np.float64)
    T, R = reward.shape
    carry = np.zeros(R)
    adv, ret = np.empty((T, R)), np.empty((T, R))
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            v, r = value[t], reward[t]
            active = np.ones(R, bool) if mask is None else np.asarray(mask[t]) != 0
            ended = np.asarray(done[t]) != 0
            delta = np.where(ended, r - v, (r + gamma * vn) - v)
            run = np.where(ended, delta, delta + (gamma * lam) * carry)
            adv[t], ret[t] = np.where(active, run, 0.0), np.where(active, run + v, 0.0)
            carry, vn = adv[t], v
    return adv, ret


def round_to(x, dtype):
    """f32 array x rounded to `dtype` (a torch dtype name) and widened back."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, F)).to(getattr(torch, dtype)).float().numpy()


def inputs(T, rows, dtype="float32", masked=True, seed=0, p_done=0.1):
    """A rollout to test on: values ~ 5 N(0, 1) rounded to `dtype`, rewards from {-1, 0, 1} with a few large ones, dones
    Bernoulli(p_done) (a few of them 7 rather than 1), and, if masked, masks drawn per episode segment (constant from
    the step after a done to the next done, as the simulator produces them), about a quarter inactive, with NaN in
    reward and value at every inactive step.  dict of reward, done, value, bootstrap, mask (None if not masked)."""
    rng = np.random.default_rng([seed, T, rows, DTYPES.index(dtype), int(masked)])
    value = round_to(5.0 * rng.standard_normal((T, rows)), dtype)
    bootstrap = round_to(5.0 * rng.standard_normal(rows), dtype)
    reward = rng.integers(-1, 2, size=(T, rows)).astype(F)
    big = rng.random((T, rows)) < 0.02
    reward[big] = (rng.standard_normal(int(big.sum())) * 100.0).astype(F)
    done = (rng.random((T, rows)) < p_done).astype(np.int32)
    done[(done != 0) & (rng.random((T, rows)) < 0.25)] = 7
    mask = None
    if masked:
        seg = np.zeros((T, rows), np.int64)                       # dones before t: the episode segment step t is in
        seg[1:] = np.cumsum(done[:-1] != 0, axis=0)
        live = rng.random((T + 1, rows)) >= 0.25                   # one draw per (segment, row)
        mask = live[seg, np.arange(rows)[None, :]].astype(F)
        reward[mask == 0] = np.nan
        value[mask == 0] = np.nan
    return dict(reward=reward, done=done, value=value, bootstrap=bootstrap, mask=mask)


def bits(x):
    return np.ascontiguousarray(x, F).view(np.int32)


def _plain(T=40, rows=17, seed=1):
    """An unmasked segment with no done, float64."""
    x = inputs(T, rows, masked=False, seed=seed)
    x["done"][:] = 0
    return x


def test_lambda_one_is_the_discounted_return():
    x = _plain()
    T = x["reward"].shape[0]
    _, ret = gae_f64(x["reward"], x["done"], x["value"], x["bootstrap"], None, GAMMA, 1.0)
    r, b = x["reward"].astype(np.float64), x["bootstrap"].astype(np.float64)
    for t in range(T):
        want = sum(GAMMA ** k * r[t + k] for k in range(T - t)) + GAMMA ** (T - t) * b
        scale = np.abs(r[t:]).sum(0) + np.abs(b) + 2 * np.abs(x["value"]).max()
        assert (np.abs(ret[t] - want) <= 4 * T * 2.0 ** -53 * scale).all(), t


def test_lambda_zero_is_the_td_error_and_gamma_zero_is_reward_minus_value():
    x = _plain()
    r, v = x["reward"].astype(np.float64), x["value"].astype(np.float64)
    vn = np.concatenate([v[1:], x["bootstrap"][None].astype(np.float64)])
    adv, ret = gae_f64(x["reward"], x["done"], x["value"], x["bootstrap"], None, GAMMA, 0.0)
    assert np.array_equal(adv, (r + GAMMA * vn) - v) and np.array_equal(ret, adv + v)
    adv, _ = gae_f64(x["reward"], x["done"], x["value"], x["bootstrap"], None, 0.0, LAMBDA)
    assert np.array_equal(adv, r - v)
    # and the f32 restatement, bit for bit
    adv32, _ = gae_f32(x["reward"], x["done"], x["value"], x["bootstrap"], None, GAMMA, 0.0)
    vn32 = np.concatenate([x["value"][1:], x["bootstrap"][None]])
    assert np.array_equal(bits(adv32), bits((x["reward"] + F(GAMMA) * vn32) - x["value"]))
    adv32, _ = gae_f32(x["reward"], x["done"], x["value"], x["bootstrap"], None, 0.0, LAMBDA)
    assert np.array_equal(bits(adv32), bits(x["reward"] - x["value"]))


@pytest.mark.parametrize("restatement", [gae_f32, gae_f64])
def test_a_done_cuts_the_rollout(restatement):
    T, rows, cut = 23, 9, 11
    x = _plain(T, rows, seed=2)
    x["done"][cut] = 1
    base = restatement(x["reward"], x["done"], x["value"], x["bootstrap"], None, GAMMA, LAMBDA)
    for poison in (1000.0, np.nan, np.inf):
        y = {k: (None if v is None else v.copy()) for k, v in x.items()}
        y["reward"][cut + 1:] = poison
        y["value"][cut + 1:] = poison
        y["bootstrap"][:] = poison
        got = restatement(y["reward"], y["done"], y["value"], y["bootstrap"], None, GAMMA, LAMBDA)
        for a, b in zip(base, got):
            assert np.array_equal(a[:cut + 1], b[:cut + 1]) and np.isfinite(b[:cut + 1]).all(), poison
        assert not np.array_equal(base[0][cut + 1:], got[0][cut + 1:], equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_f32_restatement_is_close_to_float64(dtype):
    """A sanity check of the restatement, not a GPU tolerance: a step adds at most four roundings of 2^-24 relative to a
    quantity no larger than M = max|reward| + 2 max|value| + max|advantage|, and the recurrence carries them with a
    factor gamma lambda < 1, so the distance stays within T 2^-23 M."""
    for T, rows in ((40, 301), (67, 36)):
        x = inputs(T, rows, dtype, masked=True, seed=3)
        a32, r32 = gae_f32(x["reward"], x["done"], x["value"], x["bootstrap"], x["mask"], GAMMA, LAMBDA)
        a64, r64 = gae_f64(x["reward"], x["done"], x["value"], x["bootstrap"], x["mask"], float(F(GAMMA)), float(F(LAMBDA)))
        M = np.nanmax(np.abs(x["reward"])) + 2 * np.nanmax(np.abs(x["value"])) + np.abs(a64).max()
        err = max(np.abs(a32 - a64).max(), np.abs(r32 - r64).max())
        print(f"{dtype} T={T} rows={rows}: max |f32 - f64| = {err:.3e}, bound {T * 2.0 ** -23 * M:.3e}")
        assert err <= T * 2.0 ** -23 * M


def test_masked_steps_are_positive_zero_and_nan_stays_out():
    for dtype in DTYPES:
        x = inputs(67, 301, dtype, masked=True, seed=4)
        off = x["mask"] == 0
        assert 0.15 < off.mean() < 0.35 and np.isnan(x["reward"][off]).all() and np.isnan(x["value"][off]).all()
        assert not np.isnan(x["reward"][~off]).any() and (x["done"] != 0).any()
        # constant between dones: a change of the mask from t to t + 1 needs a done at t
        change = x["mask"][1:] != x["mask"][:-1]
        assert change.any() and (x["done"][:-1][change] != 0).all()
        for fn in (gae_f32, gae_f64):
            adv, ret = fn(x["reward"], x["done"], x["value"], x["bootstrap"], x["mask"], GAMMA, LAMBDA)
            assert np.isfinite(adv).all() and np.isfinite(ret).all()
            assert not adv[off].any() and not ret[off].any() and not np.signbit(adv[off]).any() and not np.signbit(ret[off]).any()
        adv, ret = gae_f32(x["reward"], x["done"], x["value"], x["bootstrap"], x["mask"], GAMMA, LAMBDA)
        assert np.array_equal(bits(ret[~off]), bits(adv[~off] + x["value"][~off]))


class _Sim:
    num_worlds, agents_per_world, gpu_id = 6, 4, 0


def test_request_refuses_before_the_library_is_called():
    import torch
    from gpu_hideseek import advantages as A
    T, R = 5, 24
    r, d, v, b = torch.zeros(T, R), torch.zeros(T, R, dtype=torch.int32), torch.zeros(T, R), torch.zeros(R)

    def call(rewards=r, dones=d, values=v, bootstrap=b, **kw):
        return A.compute(_Sim(), rewards, dones, values, bootstrap, **kw)

    bad = [
        (dict(rewards=torch.zeros(T, R + 1)), "rewards.*shape"), (dict(rewards=torch.zeros(T * R)), "rewards.*shape"),
        (dict(rewards=torch.zeros(T, R, dtype=torch.float64)), "rewards.*dtype"), (dict(rewards=[[0.0] * R] * T), "rewards"),
        (dict(dones=torch.zeros(T + 1, R, dtype=torch.int32)), "dones.*shape"), (dict(dones=torch.zeros(T, R)), "dones.*dtype"),
        (dict(dones=torch.zeros(T, R, dtype=torch.int64)), "dones.*dtype"),
        (dict(values=torch.zeros(T, 4, 6)), "values.*shape"), (dict(values=torch.zeros(T, R, dtype=torch.int32)), "values.*dtype"),
        (dict(values=torch.zeros(R, T).t()), "values.*not contiguous"), (dict(rewards=torch.zeros(T, 2 * R)[:, ::2]), "rewards.*not contiguous"),
        (dict(bootstrap=torch.zeros(R + 1)), "bootstrap.*shape"), (dict(bootstrap=torch.zeros(T, R)), "bootstrap.*shape"),
        (dict(bootstrap=torch.zeros(R, dtype=torch.bfloat16)), "bootstrap.*dtype"), (dict(bootstrap=torch.zeros(2 * R)[::2]), "bootstrap.*not contiguous"),
        (dict(mask=torch.zeros(T, R - 1)), "mask.*shape"), (dict(mask=torch.zeros(T, R, dtype=torch.int32)), "mask.*dtype"),
        (dict(mask=torch.zeros(T, R, 2)[:, :, 0]), "mask.*not contiguous"),
        (dict(advantages=torch.zeros(T, R + 1)), "advantages.*shape"), (dict(returns=torch.zeros(T, R, dtype=torch.float16)), "returns.*dtype"),
        (dict(returns=torch.zeros(R, T).t()), "returns.*not contiguous"), (dict(advantages=3), "advantages"),
        (dict(moments=torch.zeros(4, dtype=torch.float64)), "moments.*shape"), (dict(moments=torch.zeros(5)), "moments.*dtype"),
        (dict(rewards=torch.zeros(0, R), dones=torch.zeros(0, R, dtype=torch.int32), values=torch.zeros(0, R)), "rewards.*T = 0"),
        (dict(rewards=torch.zeros(4097, R)), "rewards.*T = 4097"),
        (dict(gamma=1.5), "gamma"), (dict(gamma=-0.1), "gamma"), (dict(gamma=float("inf")), "gamma"),
        (dict(gae_lambda=float("nan")), "gae_lambda"), (dict(gae_lambda=1.01), "gae_lambda"),
        (dict(advantages=None, returns=None), "nothing to do"), (dict(advantages=False, returns=None, moments=None), "nothing to do"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            call(**kw)
    # well formed, on the wrong device: every accepted shape gets as far as the device check
    for shape in ((T, R), (T, R, 1), (T, 6, 4)):
        with pytest.raises(ValueError, match="rewards must be on cuda:0: it is on cpu"):
            call(rewards=r.reshape(shape), dones=d.reshape(shape), values=v.reshape(shape), mask=torch.ones(shape),
                 bootstrap=b.reshape(shape[1:]), moments=None)


def test_moments_to_mean_std():
    import torch
    from gpu_hideseek import advantages as A
    a, r = np.array([1.0, -2.0, 4.0]), np.array([0.5, 0.25, 8.0])
    m = torch.tensor([a.sum(), (a * a).sum(), r.sum(), (r * r).sum(), 3.0], dtype=torch.float64)
    out = A.moments_to_mean_std(m)
    assert float(out["count"]) == 3.0
    for name, x in (("advantages", a), ("returns", r)):
        mean, std = out[name]
        assert abs(float(mean) - x.mean()) < 1e-12 and abs(float(std) - x.std()) < 1e-12
    none = A.moments_to_mean_std(torch.zeros(5, dtype=torch.float64))
    assert float(none["advantages"][0]) == 0.0 and float(none["returns"][1]) == 0.0
    with pytest.raises(ValueError, match="moments"):
        A.moments_to_mean_std(torch.zeros(4))


def test_header_mirror_and_symbols_agree(hideseek_lib):
    from gpu_hideseek import advantages as A
    src = open(os.path.join(ROOT, "include", "hideseek.h")).read()
    flat = " ".join(src.split())
    assert "int32_t hs_compute_gae(hs_sim *sim, const hs_gae_request *req);" in flat
    assert "int32_t hs_compute_gae_async(hs_sim *sim, void *hip_stream, const hs_gae_request *req);" in flat
    enums = dict(re.findall(r"(HS_GAE_[A-Z_]+) = (\d+)", src))
    assert enums == {"HS_GAE_MAX_STEPS": "4096", "HS_GAE_MOMENTS": "5"}
    assert A.MAX_STEPS == 4096 and A.MOMENTS == 5
    # the fields of the struct in the header, in order, are the mirror's
    body = re.search(r"typedef struct hs_gae_request \{(.*?)\} hs_gae_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in A.HsGaeRequest._fields_]
    want = dict(reward=0, done=8, value=16, bootstrap=24, mask=32, value_dtype=40, steps=44, gamma=48, advantage=56,
                returns=64, moments=72)
    want["lambda"] = 52
    assert C.sizeof(A.HsGaeRequest) == 80
    assert {n: getattr(A.HsGaeRequest, n).offset for n in want} == want
    L = C.CDLL(hideseek_lib)
    assert hasattr(L, "hs_compute_gae") and hasattr(L, "hs_compute_gae_async")
