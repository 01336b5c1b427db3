"""The observation normaliser on the GPU (policy_inputs.ObsNormaliser, hs_obs_norm_update, csrc/hs_k_norm.h;
pack_policy_inputs(normaliser=...), hs_pack_policy_inputs_normalized): the update bit for bit against the numpy
restatement of tests/test_obs_normaliser_host.py, the normalised rows bit for bit against that restatement applied to the
GPU's own un-normalised f32 critic rows and visibility masks, a rollout loop on one side stream, and the refusals of the
C ABI."""
import ctypes as C

import numpy as np
import pytest

from test_obs_normaliser_host import ROW, STATE, fresh_state, norm_rows, norm_update, table_of

pytestmark = pytest.mark.gpu

EPS = 1e-5
# (worlds, agents per team): 164 rows = five blocks and a partial one; 32 772 rows = 1 024 workgroups, the first of
# which takes a second (partial) row block
SIZES = {"partial": (41, 2), "second-block": (5462, 3)}
NEG_ZERO = (0, 5)                       # (row, column): a -0 written into the self_data export


def _sim(n, agents, seed=0):
    import gpu_hideseek
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=0, rand_seed=seed, min_hiders=agents,
        max_hiders=agents, min_seekers=agents, max_seekers=agents, num_pbt_policies=1)


def _drive(sim, steps, seed=0):
    import torch
    act = sim.action_tensor().to_torch()
    g = torch.Generator(device=act.device).manual_seed(seed)
    for _ in range(steps):
        act[:, 0:2] = torch.randint(-5, 5, (act.shape[0], 2), device=act.device, dtype=torch.int32, generator=g)
        sim.step()


def _bits(t):
    import torch
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _vis(sim):
    R = sim.num_worlds * sim.agents_per_world
    return [getattr(sim, n + "_tensor")().to_torch().reshape(R, -1).cpu().numpy()
            for n in ("visible_agents_mask", "visible_boxes_mask", "visible_ramps_mask")]


@pytest.fixture(scope="module")
def worlds():
    """Per size: a simulator after 30 steps with a -0 in its exports, its un-normalised f32 critic rows and masks, the
    moments of that state, a table from a real update and a crafted one.  Shared and left unchanged by the tests."""
    import torch
    from gpu_hideseek import policy_inputs as P
    made = {}

    def get(size):
        if size not in made:
            n, agents = SIZES[size]
            sim = _sim(n, agents)
            sim.init()
            _drive(sim, 30)
            sim.self_data_tensor().to_torch().reshape(n * 2 * agents, -1)[NEG_ZERO[0], NEG_ZERO[1] - 1] = -0.0
            raw = sim.pack_policy_inputs(critic=True, moments=True)
            norm = P.ObsNormaliser(0, decay=0.9, eps=EPS)
            norm.update(sim, raw["moments"])
            crafted = norm.table.clone()
            crafted[NEG_ZERO[1]], crafted[ROW + NEG_ZERO[1]] = 0.0, 2.0 ** 20         # the -0 keeps its sign through * 2^20
            crafted[ROW + 115:ROW + 268] = 2.0 ** 20                                  # the boxes: masked entities among them
            made[size] = dict(sim=sim, rows=n * 2 * agents, critic=raw["critic"].cpu().numpy(), moments=raw["moments"],
                              vis=_vis(sim), tables={"updated": norm.table, "crafted": crafted}, norm=norm)
        return made[size]
    yield get
    for w in made.values():
        w["sim"].close()


@pytest.fixture(scope="module")
def rollout_moments():
    """[40, 593] moments of 40 consecutive steps after 30 steps, from real pack_policy_inputs(moments=True) calls."""
    import torch
    sim = _sim(24, 3, seed=2)
    sim.init()
    _drive(sim, 30)
    mom = torch.empty(40, STATE, dtype=torch.float64, device="cuda")
    for t in range(40):
        _drive(sim, 1, seed=100 + t)
        sim.pack_policy_inputs(moments=mom[t])
    yield sim, mom
    sim.close()


def _update_on_gpu(sim, state, moments, decay, eps=EPS):
    import torch
    from gpu_hideseek import policy_inputs as P
    norm = P.ObsNormaliser(0, decay=decay, eps=eps)
    norm.state.copy_(torch.from_numpy(state))
    norm.table.fill_(-7.0)                       # the table is always rewritten
    norm.update(sim, moments)
    return norm.state.cpu().numpy(), norm.table.cpu().numpy()


def _ulps32(a, b):
    a, b = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max())


def _check_update(sim, state, moments, decay, tag, eps=EPS):
    got_s, got_t = _update_on_gpu(sim, state, moments, decay, eps)
    want_s, want_t = norm_update(state, moments.cpu().numpy(), decay, eps)
    bad = np.flatnonzero(got_s.view(np.int64) != want_s.view(np.int64))
    assert not len(bad), (tag, "state", len(bad), int(bad[0]), got_s[bad[0]], want_s[bad[0]])
    print(f"{tag}: table max difference {_ulps32(got_t, want_t)} f32 ulp")
    bad = np.flatnonzero(got_t.view(np.int32) != want_t.view(np.int32))
    assert not len(bad), (tag, "table", len(bad), int(bad[0]), got_t[bad[0]], want_t[bad[0]])
    return got_s, got_t


@pytest.mark.parametrize("decay", [0.0, 0.9, 0.99999])
@pytest.mark.parametrize("k", [1, 3, 40])
def test_update_equals_the_restatement_bit_for_bit(rollout_moments, k, decay):
    sim, mom = rollout_moments
    assert float(mom[:, 2 * ROW].min()) > 0 and bool(mom.isfinite().all())
    fresh = fresh_state()
    s1, t1 = _check_update(sim, fresh, mom[:k], decay, ("fresh", k, decay))
    assert s1[2 * ROW] == 1.0 - decay and t1[0] == 0 and t1[ROW] == 1 and t1[14] == 0 and t1[ROW + 14] == 1
    assert (t1[ROW:] > 0).all() and np.isfinite(t1).all()
    # from a non-trivial state: another batch on top, and a single vector [593]
    s2, t2 = _check_update(sim, s1, mom[40 - k:], decay, ("second", k, decay))
    _check_update(sim, s2, mom[7], decay, ("vector", k, decay))
    # a second identical call from the same inputs gives the same bits
    again_s, again_t = _update_on_gpu(sim, s1, mom[40 - k:], decay)
    assert np.array_equal(again_s.view(np.int64), s2.view(np.int64)) and np.array_equal(again_t.view(np.int32), t2.view(np.int32))


def test_update_zero_count_clamp_and_the_longest_batch(rollout_moments):
    import torch
    sim, mom = rollout_moments
    start, table = _check_update(sim, fresh_state(), mom[:3], 0.9, "start")
    # a zero-count batch: the state keeps its bits, the table is rewritten from it
    zero = mom[:2].clone()
    zero[:, 2 * ROW] = 0.0
    s, t = _check_update(sim, start, zero, 0.9, "zero count")
    assert np.array_equal(s.view(np.int64), start.view(np.int64)) and np.array_equal(t.view(np.int32), table.view(np.int32))
    s, t = _check_update(sim, fresh_state(), zero, 0.9, "zero count, fresh")
    assert not s.any() and np.array_equal(t.view(np.int32), table_of(fresh_state(), EPS).view(np.int32))
    # a computed variance below zero: s2 / n < (s1 / n)^2 in every column
    neg = torch.zeros(1, STATE, dtype=torch.float64, device="cuda")
    neg[0, :ROW], neg[0, ROW:2 * ROW], neg[0, 2 * ROW] = 2.0 * 50, 3.0 * 50, 50.0
    s, t = _check_update(sim, fresh_state(), neg, 0.0, "clamp")
    assert t[ROW + 20] == np.float32(1.0 / np.sqrt(EPS)) and t[20] == 2.0
    # the most vectors the request takes, with another eps
    many = mom.repeat(103, 1)[:4096].contiguous()
    _check_update(sim, start, many, 0.99999, "4096 vectors", eps=1e-2)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("size", list(SIZES))
def test_normalised_rows_equal_the_restatement_bit_for_bit(worlds, size, dtype):
    import torch
    w = worlds(size)
    sim, dt = w["sim"], getattr(torch, dtype)
    assert np.signbit(w["critic"][NEG_ZERO]) and w["critic"][NEG_ZERO] == 0
    hidden = sum(int((m == 0).sum()) for m in w["vis"])
    assert hidden > 0
    plain = sim.pack_policy_inputs(actor=True, critic=True, dtype=dt)
    for tname, table in w["tables"].items():
        tab = table.cpu().numpy()
        want = {"critic": norm_rows(w["critic"], tab, None, dt), "actor": norm_rows(w["critic"], tab, w["vis"], dt)}
        for names in (("actor",), ("critic",), ("actor", "critic")):
            for moments in (False, True):
                out = sim.pack_policy_inputs(moments=moments or None, dtype=dt, normaliser=table, **{n: True for n in names})
                assert set(out) == set(names) | ({"moments"} if moments else set())
                for n in names:
                    got = out[n].cpu()
                    assert got.dtype == dt and got.shape == (w["rows"], ROW)
                    bad = (_bits(got) != _bits(want[n])).nonzero()
                    assert not len(bad), (size, dtype, tname, names, moments, n, len(bad), bad[0].tolist(),
                                          float(got[tuple(bad[0])]), float(want[n][tuple(bad[0])]))
                    # prep_counter and self_type are untouched
                    assert torch.equal(_bits(out[n][:, [0, 14]]), _bits(plain[n][:, [0, 14]]))
                if moments:                      # the moments are those of the raw rows
                    assert torch.equal(_bits(out["moments"]), _bits(w["moments"]))
        if tname == "crafted":                   # -0 * 2^20 keeps its sign; a masked box is +-0, not the big value
            c = want["critic"].float().numpy()
            assert c[NEG_ZERO] == 0 and np.signbit(c[NEG_ZERO])
            assert np.abs(c[:, 115:268]).max() > 2.0 ** 10


def test_fresh_table_is_the_identity_and_the_normaliser_object(worlds):
    import torch
    from gpu_hideseek import policy_inputs as P
    w = worlds("partial")
    sim = w["sim"]
    fresh = P.ObsNormaliser(0)
    assert fresh.decay == 0.99999 and fresh.eps == 1e-5 and not bool(fresh.state.any())
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        plain = sim.pack_policy_inputs(actor=True, critic=True, moments=True, dtype=dt)
        out = sim.pack_policy_inputs(actor=True, critic=True, moments=True, dtype=dt, normaliser=fresh)
        for k in ("actor", "critic", "moments"):
            assert torch.equal(_bits(out[k]), _bits(plain[k])), (dt, k)
    assert float(plain["critic"][NEG_ZERO]) == 0 and bool(torch.signbit(plain["critic"][NEG_ZERO]))
    # the object and its table are the same argument
    a = sim.pack_policy_inputs(critic=True, normaliser=w["norm"])["critic"]
    b = sim.pack_policy_inputs(critic=True, normaliser=w["norm"].table)["critic"]
    assert torch.equal(_bits(a), _bits(b)) and not torch.equal(_bits(a), _bits(plain["critic"].float()))
    # a row of a [T, 593] buffer is 8-byte aligned: accepted as the moments output, with or without a normaliser
    buf = torch.zeros(2, STATE, dtype=torch.float64, device="cuda")
    assert buf[1].data_ptr() % 16 == 8
    assert torch.equal(_bits(sim.pack_policy_inputs(moments=buf[1])["moments"]), _bits(w["moments"]))
    assert not bool(buf[0].any())
    # moments alone with a normaliser: those of the raw rows
    m = sim.pack_policy_inputs(moments=True, normaliser=w["norm"])
    assert set(m) == {"moments"} and torch.equal(_bits(m["moments"]), _bits(w["moments"]))
    # mean_var, state_dict, load_state_dict, reset
    mean, var, N = w["norm"].mean_var()
    state = w["norm"].state.cpu().numpy()
    assert mean.dtype == var.dtype == torch.float64 and mean.is_cuda and float(N) == state[2 * ROW] > 0
    mu = state[:ROW] / state[2 * ROW]
    assert np.allclose(mean.cpu().numpy(), mu, rtol=1e-14, atol=0)
    assert np.allclose(var.cpu().numpy(), np.maximum(state[ROW:2 * ROW] / state[2 * ROW] - mu * mu, 0), rtol=1e-12, atol=1e-14)
    m0, v0, n0 = fresh.mean_var()
    assert float(n0) == 0 and not bool(m0.any()) and not bool(v0.any())
    d = w["norm"].state_dict()
    assert d["state"].device.type == "cpu" and d["decay"] == 0.9 and d["eps"] == EPS
    other = P.ObsNormaliser(0)
    other.load_state_dict(d)
    assert other.decay == 0.9 and other.eps == EPS
    assert torch.equal(_bits(other.state), _bits(w["norm"].state)) and torch.equal(_bits(other.table), _bits(w["norm"].table))
    other.reset()
    assert torch.equal(_bits(other.state), _bits(fresh.state)) and torch.equal(_bits(other.table), _bits(fresh.table))


def test_stream_form_and_rollout_slot(worlds):
    import torch
    w = worlds("partial")
    sim, R, table = w["sim"], w["rows"], w["tables"]["updated"]
    blocking = sim.pack_policy_inputs(actor=True, critic=True, moments=True, dtype=torch.bfloat16, normaliser=table)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = sim.pack_policy_inputs(actor=True, critic=True, moments=True, dtype=torch.bfloat16, normaliser=table, stream=side)
    raw = sim.pack_policy_inputs(critic=True, dtype=torch.bfloat16, normaliser=table, stream=side.cuda_stream)      # a raw handle
    side.synchronize()
    for k in ("actor", "critic", "moments"):
        assert torch.equal(_bits(got[k]), _bits(blocking[k])), k
    assert torch.equal(_bits(raw["critic"]), _bits(blocking["critic"]))
    # a slot of a rollout buffer; the other slots keep their sentinel
    buf = torch.full((4, R, ROW), -7.0, dtype=torch.bfloat16, device="cuda")
    res = sim.pack_policy_inputs(actor=buf[2], normaliser=table)
    assert res["actor"].data_ptr() == buf[2].data_ptr()
    assert torch.equal(_bits(buf[2]), _bits(blocking["actor"])) and bool((buf[[0, 1, 3]] == -7.0).all())


def test_two_handles_against_one_and_sharded(worlds):
    import torch
    import gpu_hideseek
    from gpu_hideseek import policy_inputs as P
    table = worlds("partial")["tables"]["updated"]
    kw = dict(sim_flags=0, rand_seed=3, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0], 40, **kw)
    one = gpu_hideseek.HideAndSeekSimulator(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=40, **kw)
    ss.init()
    one.init()
    for _ in range(3):
        ss.step()
        one.step()
    whole = one.pack_policy_inputs(actor=True, critic=True, moments=True, dtype=torch.bfloat16, normaliser=table)
    norms = [P.ObsNormaliser(0), P.ObsNormaliser(0)]
    for n in norms:
        n.table.copy_(table)
    for arg in (table, norms):                   # one table for all shards of its device, or one normaliser per shard
        res = ss.pack_policy_inputs(actor=True, critic=True, moments=True, dtype=torch.bfloat16, normaliser=arg)
        assert len(res) == 2
        for k in ("actor", "critic"):
            assert torch.equal(_bits(torch.cat([r[k] for r in res])), _bits(whole[k])), k
    with pytest.raises(ValueError, match="per shard"):
        ss.pack_policy_inputs(actor=True, normaliser=[table])
    # the shards' moments stacked are one batch: the count is that of the single handle, the state agrees closely
    stacked = torch.stack([r["moments"] for r in res])
    a, b = P.ObsNormaliser(0, decay=0.9), P.ObsNormaliser(0, decay=0.9)
    a.update(ss.shards[0], stacked)
    b.update(one, whole["moments"])
    want, _ = norm_update(fresh_state(), stacked.cpu().numpy(), 0.9, 1e-5)
    assert np.array_equal(a.state.cpu().numpy().view(np.int64), want.view(np.int64))
    assert float(stacked[:, 2 * ROW].sum()) == float(whole["moments"][2 * ROW]) == 160
    assert torch.allclose(a.state, b.state, rtol=1e-12, atol=1e-12)
    ss.close()
    one.close()


def test_a_rollout_loop_on_one_side_stream():
    import torch
    from gpu_hideseek import policy_inputs as P
    sim = _sim(48, 3, seed=4)
    sim.init()
    R = 48 * 6
    norm = P.ObsNormaliser(0, decay=0.9, eps=EPS)
    rounds = 10
    mom = torch.zeros(rounds, STATE, dtype=torch.float64, device="cuda")
    rows = torch.empty(rounds, R, ROW, dtype=torch.bfloat16, device="cuda")
    tables = torch.empty(rounds, 2 * ROW, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for r in range(rounds):                  # nothing in here waits for the device
            for _ in range(4):
                sim.step_async(side.cuda_stream)
            tables[r].copy_(norm.table)
            sim.pack_policy_inputs(actor=rows[r], moments=mom[r], normaliser=norm, stream=side)
            norm.update(sim, mom[r], stream=side)
    side.synchronize()
    state, m = fresh_state(), mom.cpu().numpy()
    for r in range(rounds):
        assert np.array_equal(tables[r].cpu().numpy().view(np.int32), table_of(state, EPS).view(np.int32)), r    # the table the pack read
        state, table = norm_update(state, m[r], 0.9, EPS)
    assert m[:, 2 * ROW].min() == R
    assert np.array_equal(norm.state.cpu().numpy().view(np.int64), state.view(np.int64))
    assert np.array_equal(norm.table.cpu().numpy().view(np.int32), table.view(np.int32))
    # the last round's rows are the restatement of the raw rows under the table of the round before
    raw = sim.pack_policy_inputs(critic=True)["critic"].cpu().numpy()
    want = norm_rows(raw, tables[rounds - 1].cpu().numpy(), _vis(sim), torch.bfloat16)
    assert torch.equal(_bits(rows[rounds - 1].cpu()), _bits(want))
    sim.close()


def test_the_c_abi_refuses_and_writes_nothing(worlds):
    import torch
    from gpu_hideseek import policy_inputs as P
    from gpu_hideseek._native import load
    INVALID = 1
    sim = worlds("partial")["sim"]
    L, h = sim._L, sim._h
    K = 3
    mom = torch.full((K * STATE + 8,), 1.0, dtype=torch.float64, device="cuda")
    state = torch.full((STATE + 8,), -7.0, dtype=torch.float64, device="cuda")
    table = torch.full((2 * ROW + 8,), -7.0, device="cuda")
    m, s, t = mom.data_ptr(), state.data_ptr(), table.data_ptr()
    nan, inf = float("nan"), float("inf")

    def refused(rc, what):
        assert rc == INVALID, what
        msg = load().hs_last_error().decode()
        assert what in msg, (what, msg)
        torch.cuda.synchronize()
        assert bool((state == -7).all()) and bool((table == -7).all()) and bool((mom == 1).all()), what

    def update(*fields):
        req = P.HsObsNormRequest(*fields)
        return L.hs_obs_norm_update(h, C.byref(req)), L.hs_obs_norm_update_async(h, None, C.byref(req))
    for fields, what in (((None, K, 0.9, EPS, s, t), "null moments"), ((m, K, 0.9, EPS, None, t), "null state"),
                         ((m, K, 0.9, EPS, s, None), "null table"), ((m, 0, 0.9, EPS, s, t), "num_moments"),
                         ((m, -1, 0.9, EPS, s, t), "num_moments"), ((m, 4097, 0.9, EPS, s, t), "num_moments"),
                         ((m, K, 1.0, EPS, s, t), "decay"), ((m, K, -0.1, EPS, s, t), "decay"), ((m, K, nan, EPS, s, t), "decay"),
                         ((m, K, 0.9, 0.0, s, t), "eps"), ((m, K, 0.9, -EPS, s, t), "eps"), ((m, K, 0.9, inf, s, t), "eps"),
                         ((m, K, 0.9, nan, s, t), "eps"), ((m, K, 0.9, EPS, s, t + 4), "table must be 16-byte aligned"),
                         ((m, K, 0.9, EPS, s, t + 8), "table must be 16-byte aligned"),
                         ((m, K, 0.9, EPS, m + 8 * (K * STATE - 1), t), "state overlaps moments"),
                         ((m, K, 0.9, EPS, m + 8 * 5, t), "state overlaps moments"),
                         ((m, K, 0.9, EPS, s, m + 16 * 7), "table overlaps moments"),
                         ((m, K, 0.9, EPS, s, m + 8 * (K * STATE - 1)), "table overlaps moments"),
                         ((m + 4, K, 0.9, EPS, s, t), "moments and state must be 8-byte aligned"),
                         ((m, K, 0.9, EPS, s + 4, t), "moments and state must be 8-byte aligned"),
                         ((m, K, 0.9, EPS, s, s + 16), "table overlaps state"),
                         ((m, K, 0.9, EPS, s, s + 8 * (STATE - 1)), "table overlaps state")):
        for rc in update(*fields):
            refused(rc, what)
    for rc in (L.hs_obs_norm_update(h, None), L.hs_obs_norm_update_async(h, None, None)):
        refused(rc, "null request")
    # the accepted call does write, and only its own ranges
    ok = P.HsObsNormRequest(m, K, 0.9, EPS, s, t)
    assert L.hs_obs_norm_update(h, C.byref(ok)) == 0
    assert bool((state[:STATE] != -7).all()) and bool((state[STATE:] == -7).all())
    assert bool((table[:2 * ROW] != -7).all()) and bool((table[2 * ROW:] == -7).all())
    state.fill_(-7.0)
    table.fill_(-7.0)
    # a state that starts where the moments end, and a table that starts where that state ends, are no overlap
    adj = torch.full((K * STATE + STATE + 1 + ROW + 8,), 1.0, dtype=torch.float64, device="cuda")     # (+1: the table on 16 bytes)
    a0 = adj.data_ptr()
    ts = a0 + 8 * (K * STATE + STATE)
    ts += ts % 16
    assert a0 % 16 == 0 and ts - (a0 + 8 * (K * STATE + STATE)) in (0, 8)
    touching = P.HsObsNormRequest(a0, K, 0.9, EPS, a0 + 8 * K * STATE, ts)
    assert L.hs_obs_norm_update(h, C.byref(touching)) == 0
    assert bool((adj[:K * STATE] == 1).all()) and bool((adj[K * STATE:K * STATE + STATE - 1] == 0.9 * 1 + (1 - 0.9) * (K / K)).all())
    assert bool((adj[(ts - a0) // 8 + ROW:] == 1).all())

    # the normalised pack: the table, then everything hs_pack_policy_inputs refuses
    R = sim.num_worlds * sim.agents_per_world
    out = torch.full((R * ROW + 8,), -7.0, device="cuda")
    good = torch.zeros(2 * ROW + 8, device="cuda")

    def pack(req, tp):
        r = C.byref(req) if req is not None else None
        return (L.hs_pack_policy_inputs_normalized(h, r, tp), L.hs_pack_policy_inputs_normalized_async(h, None, r, tp))

    def pack_refused(rc, what):
        assert rc == INVALID, what
        assert what in load().hs_last_error().decode(), what
        torch.cuda.synchronize()
        assert bool((out == -7).all()), what
    f32 = P.HsPackRequest(out.data_ptr(), 1, None, 0, None)
    for req, tp, what in ((f32, None, "null table"), (f32, good.data_ptr() + 4, "table must be 16-byte aligned"),
                          (f32, good.data_ptr() + 8, "table must be 16-byte aligned"), (None, good.data_ptr(), "null request"),
                          (P.HsPackRequest(None, 0, None, 0, None), good.data_ptr(), "every output is null"),
                          (P.HsPackRequest(out.data_ptr(), 7, None, 0, None), good.data_ptr(), "dtype"),
                          (P.HsPackRequest(out.data_ptr() + 4, 1, None, 0, None), good.data_ptr(), "16-byte aligned")):
        for rc in pack(req, tp):
            pack_refused(rc, what)
    other = _sim(4, 2)                                                          # before hs_init, inside an open step
    req4 = P.HsPackRequest(out.data_ptr(), 1, None, 0, None)
    rcs = (L.hs_pack_policy_inputs_normalized(other._h, C.byref(req4), good.data_ptr()),
           L.hs_obs_norm_update(other._h, C.byref(P.HsObsNormRequest(m, K, 0.9, EPS, s, t))))
    assert rcs == (INVALID, INVALID) and "before hs_init" in load().hs_last_error().decode()
    other.init()
    other.step_begin()
    rcs = (L.hs_pack_policy_inputs_normalized_async(other._h, None, C.byref(req4), good.data_ptr()),
           L.hs_obs_norm_update_async(other._h, None, C.byref(P.HsObsNormRequest(m, K, 0.9, EPS, s, t))))
    assert rcs == (INVALID, INVALID) and "open step" in load().hs_last_error().decode()
    other.step_end()
    other.close()
    from lockstep import EXT_SKIP_OBSERVATIONS                                 # no observations: unsupported, as the plain pack
    import gpu_hideseek
    skip = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=sim.num_worlds, sim_flags=EXT_SKIP_OBSERVATIONS,
        rand_seed=0, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    skip.init()
    rcs = (L.hs_pack_policy_inputs_normalized(skip._h, C.byref(req4), good.data_ptr()),
           L.hs_pack_policy_inputs_normalized_async(skip._h, None, C.byref(req4), good.data_ptr()))
    assert rcs == (3, 3) and "HS_FLAG_EXT_SKIP_OBSERVATIONS" in load().hs_last_error().decode()
    with pytest.raises(NotImplementedError):
        skip.pack_policy_inputs(actor=out[:R * ROW].view(R, ROW), normaliser=good[:2 * ROW])
    skip.close()
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((state == -7).all()) and bool((table == -7).all())
    # Python's own refusals on the device
    with pytest.raises(ValueError, match="16-byte"):
        sim.pack_policy_inputs(critic=True, normaliser=good[1:1 + 2 * ROW])
    norm = P.ObsNormaliser(0)
    for bad, what in ((torch.zeros(592, dtype=torch.float64, device="cuda"), "shape"), (torch.zeros(593, device="cuda"), "dtype"),
                      (torch.zeros(593, dtype=torch.float64), "on cpu"), (torch.zeros(4097, 593, dtype=torch.float64, device="cuda"), "shape"),
                      (torch.zeros(2, 2 * 593, dtype=torch.float64, device="cuda")[:, :593], "contiguous")):
        with pytest.raises(ValueError, match=what):
            norm.update(sim, bad)
    assert not bool(norm.state.any())
