"""The observation normaliser, the parts that need no GPU (gpu_hideseek.policy_inputs.ObsNormaliser, hs_obs_norm_update,
hs_pack_policy_inputs_normalized): the header mirror, a numpy restatement of both contracts (norm_update: the f64 fold in
the stated order; norm_rows: the f32 (x - mu) * inv, mask, cast — independent of the product;
tests/test_gpu_obs_normaliser.py holds the kernels to them bit for bit), properties of that restatement, and the
refusals that Python makes before the library is involved."""
import numpy as np
import pytest
import torch

ROW = 296
STATE = 2 * ROW + 1
SKIP = (0, 14)


def fresh_state():
    return np.zeros(STATE, np.float64)


def table_of(state, eps):
    """float32 [592] mu | inv of a state, by the contract: mu = m1 / N, v = m2 / N - mu * mu clamped by select,
    inv = 1 / sqrt(v + eps); +0 and 1 for a skipped column or N == 0."""
    m1, m2, N = state[:ROW], state[ROW:2 * ROW], state[2 * ROW]
    mu, inv = np.zeros(ROW, np.float32), np.ones(ROW, np.float32)
    if N > 0:
        with np.errstate(all="ignore"):
            mean = m1 / N
            v = m2 / N - mean * mean
            v = np.where(v < 0, np.float64(0.0), v)
            mu = mean.astype(np.float32)
            inv = (np.float64(1.0) / np.sqrt(v + np.float64(eps))).astype(np.float32)
        for c in SKIP:
            mu[c], inv[c] = 0.0, 1.0
    return np.concatenate([mu, inv])


def norm_update(state, moments, decay, eps):
    """(new state, table) of hs_obs_norm_update: `moments` [K, 593] f64 is one batch, summed in index order starting
    from the first vector; two products and one addition per running moment."""
    moments = np.asarray(moments, np.float64).reshape(-1, STATE)
    s = moments[0].copy()
    for k in range(1, len(moments)):
        s = s + moments[k]
    n = s[2 * ROW]
    state = state.copy()
    if n > 0:
        decay = np.float64(decay)
        a = np.float64(1.0) - decay
        with np.errstate(all="ignore"):
            state[:ROW] = decay * state[:ROW] + a * (s[:ROW] / n)
            state[ROW:2 * ROW] = decay * state[ROW:2 * ROW] + a * (s[ROW:2 * ROW] / n)
            state[2 * ROW] = decay * state[2 * ROW] + a
    return state, table_of(state, eps)


def entity_mask(vis):
    """[R, 296] f32: 1 in columns 0-44, the visibility mask of the column's entity in columns 45-295; `vis` is the three
    masks (agents [R, 5], boxes [R, 9], ramps [R, 2])."""
    R = vis[0].shape[0]
    cols = [np.ones((R, 45), np.float32)]
    for m, w in zip(vis, (14, 17, 14)):
        cols.append(np.repeat(m.reshape(R, -1).astype(np.float32), w, axis=1))
    out = np.concatenate(cols, 1)
    assert out.shape == (R, ROW)
    return out


def norm_rows(critic_f32, table, vis=None, dtype=torch.float32):
    """The normalised rows as a torch CPU tensor of `dtype`: y = (x - mu) * inv in f32, unfused, on the un-normalised f32
    critic rows; the actor (vis given) multiplies columns 45-295 by the masks after that; the cast comes last."""
    x = np.asarray(critic_f32, np.float32)
    mu, inv = table[:ROW].astype(np.float32), table[ROW:].astype(np.float32)
    with np.errstate(all="ignore"):
        d = x - mu[None, :]
        y = d * inv[None, :]
        if vis is not None:
            y[:, 45:] = y[:, 45:] * entity_mask(vis)[:, 45:]
    assert y.dtype == np.float32
    return torch.from_numpy(y).to(dtype)


def batch_moments(x, m):
    x, m = np.asarray(x, np.float64), np.asarray(m, np.float64).reshape(-1, 1)
    return np.concatenate([(m * x).sum(0), (m * x * x).sum(0), [m.sum()]])


def _batch(seed, R=50):
    rng = np.random.default_rng(seed)
    x = rng.normal(2.0, 3.0, size=(R, ROW)).astype(np.float32)
    m = (rng.random(R) < 0.8).astype(np.float32)
    return x, m


def test_header_states_the_contract(hideseek_lib):
    """The ctypes mirror of hs_obs_norm_request, the constants and the skip list agree with include/hideseek.h."""
    import ctypes as C
    import os
    import re
    from gpu_hideseek import policy_inputs as P
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hideseek.h")).read()

    def const(name):
        return int(re.search(rf"\b{name} = (\d+)", src).group(1))
    assert const("HS_NORM_STATE") == P.NORM_STATE == STATE == const("HS_PACK_MOMENTS") == P.MOMENTS
    assert const("HS_NORM_TABLE") == P.NORM_TABLE == 2 * const("HS_PACK_ROW")
    assert const("HS_NORM_MAX_MOMENTS") == P.NORM_MAX_MOMENTS == 4096
    skipped = sorted(int(v) for v in re.findall(r"\bHS_NORM_SKIP_\w+ = (\d+)", src))
    assert skipped == sorted(P.LAYOUT[n][0] for n in P.NORM_SKIP) == list(SKIP)
    assert P.NORM_SKIP == ("prep_counter", "self_type") and all(P.LAYOUT[n][1] - P.LAYOUT[n][0] == 1 for n in P.NORM_SKIP)
    R = P.HsObsNormRequest
    assert C.sizeof(R) == 48
    assert [getattr(R, f).offset for f in ("moments", "num_moments", "decay", "eps", "state", "table")] == [0, 8, 16, 24, 32, 40]
    struct = re.search(r"typedef struct hs_obs_norm_request \{(.*?)\} hs_obs_norm_request;", src, re.S).group(1)
    assert re.findall(r"(\w+);", struct) == ["moments", "num_moments", "decay", "eps", "state", "table"]
    assert C.sizeof(P.HsPackRequest) == 40                                      # hs_pack_request itself did not change
    L = C.CDLL(hideseek_lib)
    for sym in ("hs_obs_norm_update", "hs_obs_norm_update_async", "hs_pack_policy_inputs_normalized",
                "hs_pack_policy_inputs_normalized_async"):
        assert hasattr(L, sym), sym


def test_decay_zero_gives_the_batch_mean_and_biased_variance():
    x, m = _batch(0)
    mom = batch_moments(x, m)
    state, table = norm_update(fresh_state(), mom, 0.0, 1e-5)
    n = mom[2 * ROW]
    assert state[2 * ROW] == 1.0
    assert np.array_equal(state[:ROW], mom[:ROW] / n) and np.array_equal(state[ROW:2 * ROW], mom[ROW:2 * ROW] / n)
    sel = x[m > 0].astype(np.float64)
    keep = np.ones(ROW, bool)
    keep[list(SKIP)] = False
    assert np.allclose(table[:ROW][keep], sel.mean(0)[keep], rtol=1e-6, atol=0)
    assert np.allclose(table[ROW:][keep], 1.0 / np.sqrt(sel.var(0) + 1e-5)[keep], rtol=1e-6, atol=0)
    # exactly: the mean is the f32 of s1 / n, the variance that of s2 / n - mean^2
    mean = mom[:ROW] / n
    assert np.array_equal(table[:ROW][keep], mean.astype(np.float32)[keep])
    assert np.array_equal(table[ROW:][keep], (1.0 / np.sqrt(mom[ROW:2 * ROW] / n - mean * mean + 1e-5)).astype(np.float32)[keep])


def test_fresh_state_gives_the_identity_table_and_the_identity_rows():
    table = table_of(fresh_state(), 1e-5)
    assert np.array_equal(table.view(np.int32), np.concatenate([np.zeros(ROW, np.float32), np.ones(ROW, np.float32)]).view(np.int32))
    x, _ = _batch(1)
    x[3, 50] = -0.0
    x[4, 60] = np.float32(1e-41)                                                # a subnormal keeps its bits too
    assert np.array_equal(norm_rows(x, table).numpy().view(np.int32), x.view(np.int32))
    state, table = norm_update(fresh_state(), batch_moments(x, np.zeros(len(x))), 0.9, 1e-5)
    assert not state.any() and np.array_equal(table, table_of(fresh_state(), 1e-5))


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9, 0.99999])
def test_identical_batches_give_the_batch_mean_for_any_decay(decay):
    x, m = _batch(2)
    mom = batch_moments(x, m)
    state = fresh_state()
    sel = x[m > 0].astype(np.float64)
    for k in range(1, 6):
        state, table = norm_update(state, mom, decay, 1e-5)
        # the bias correction: N = 1 - decay^k, each fold rounding three times at magnitude <= 1
        assert abs(state[2 * ROW] - (1.0 - decay ** k)) <= 4 * k * 2.0 ** -52
        mean = state[:ROW] / state[2 * ROW]
        var = state[ROW:2 * ROW] / state[2 * ROW] - mean * mean
        assert np.allclose(mean, sel.mean(0), rtol=1e-11, atol=1e-11), k
        assert np.allclose(var, sel.var(0), rtol=1e-9, atol=1e-9), k


def test_a_zero_count_batch_changes_nothing():
    x, m = _batch(3)
    state, table = norm_update(fresh_state(), batch_moments(x, m), 0.9, 1e-5)
    zero = batch_moments(x, np.zeros(len(x)))
    zero[:2 * ROW] = 7.0                                                        # whatever the sums hold, the count decides
    again, table2 = norm_update(state, np.stack([zero, zero]), 0.9, 1e-5)
    assert np.array_equal(again.view(np.int64), state.view(np.int64))
    assert np.array_equal(table2.view(np.int32), table.view(np.int32))           # and the table is rewritten from it


def test_k_vectors_are_one_batch():
    parts = [batch_moments(*_batch(10 + k)) for k in range(5)]
    total = parts[0].copy()
    for p in parts[1:]:
        total = total + p
    start, _ = norm_update(fresh_state(), batch_moments(*_batch(4)), 0.9, 1e-5)
    a, ta = norm_update(start, np.stack(parts), 0.99, 1e-5)
    b, tb = norm_update(start, total, 0.99, 1e-5)
    assert np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(ta.view(np.int32), tb.view(np.int32))
    c, _ = norm_update(start, np.stack(parts[::-1]), 0.99, 1e-5)                # the order is part of the contract
    assert np.allclose(a, c, rtol=1e-13, atol=0)


def test_a_constant_column_and_the_clamp():
    x, m = _batch(5)
    x[:, 20] = 3.25                                                             # exact in f32, its square too
    x[:, 0], x[:, 14] = 0.5, 1.0
    eps = 1e-5
    state, table = norm_update(fresh_state(), batch_moments(x, m), 0.0, eps)
    assert table[20] == np.float32(3.25) and table[ROW + 20] == np.float32(1.0 / np.sqrt(eps))
    y = norm_rows(x, table).numpy()
    assert (y[:, 20] == 0).all()
    assert np.array_equal(y[:, [0, 14]], x[:, [0, 14]])                         # the skipped columns pass through
    # a computed variance below zero is clamped by a select: m2 / N < mu^2
    state = fresh_state()
    state[2 * ROW] = 1.0
    state[30], state[ROW + 30] = 2.0, 3.0
    assert table_of(state, eps)[ROW + 30] == np.float32(1.0 / np.sqrt(eps))


def test_the_mask_comes_after_the_normalisation_and_before_the_cast():
    rng = np.random.default_rng(6)
    R = 9
    x = rng.normal(size=(R, ROW)).astype(np.float32)
    vis = [rng.integers(0, 2, (R, n)).astype(np.float32) for n in (5, 9, 2)]
    state, table = norm_update(fresh_state(), batch_moments(x, np.ones(R)), 0.0, 1e-5)
    crit, act = norm_rows(x, table).numpy(), norm_rows(x, table, vis).numpy()
    mask = entity_mask(vis)
    assert np.array_equal(act[:, :45], crit[:, :45])
    assert np.array_equal(act[mask == 1], crit[mask == 1]) and (act[mask == 0] == 0).all()
    assert ((mask[:, 45:] == 0).any() and (np.signbit(act[mask == 0]) == np.signbit(crit[mask == 0])).all())     # y * 0 keeps the sign
    b = norm_rows(x, table, vis, torch.bfloat16)
    assert b.dtype == torch.bfloat16 and torch.equal(b, torch.from_numpy(act).to(torch.bfloat16))


def test_python_refusals_come_before_the_library():
    from gpu_hideseek import policy_inputs as P

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    for kw in (dict(decay=1.0), dict(decay=-0.1), dict(decay=float("nan")), dict(eps=0.0), dict(eps=-1.0),
               dict(eps=float("inf")), dict(eps=float("nan"))):
        with pytest.raises(ValueError, match="decay|eps"):
            P.ObsNormaliser(0, **kw)
    R = 32
    out = torch.zeros(R, ROW)                                                   # on the CPU: refused too, but after the table
    for bad, what in ((torch.zeros(591), "shape"), (torch.zeros(2, 296), "shape"), (torch.zeros(592, dtype=torch.float64), "dtype"),
                      (torch.zeros(2 * 592)[::2], "contiguous"), (torch.zeros(592), "on cpu")):
        with pytest.raises(ValueError, match=what):
            P.norm_table(bad, 0)
    for bad in ("yes", 3, [torch.zeros(592)]):
        with pytest.raises(ValueError, match="normaliser"):
            P.norm_table(bad, 0)
    with pytest.raises(ValueError):
        P.pack(Sim(), actor=out, normaliser=torch.zeros(592))
    # the host's table of a state follows the same formula as the restatement
    x, m = _batch(7)
    state, table = norm_update(fresh_state(), batch_moments(x, m), 0.9, 1e-5)
    assert np.array_equal(P.table_of_state(state, 1e-5).view(np.int32), table.view(np.int32))
    assert np.array_equal(P.table_of_state(fresh_state(), 1e-5).view(np.int32), table_of(fresh_state(), 1e-5).view(np.int32))
