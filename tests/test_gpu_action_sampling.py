"""Action sampling on the GPU (sim.sample_actions, hs_sample_actions, csrc/hs_k_sample.h) against the numpy restatement
and the float64 reference of tests/test_action_sampling_host.py, with that file's derived tolerances: the draws, the exact
cases, greedy, evaluate, keying, shard invariance, the in-place path into a step, zero_inactive, the stream form and the
refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import test_action_sampling_host as H
from test_action_sampling_host import BUCKETS, COUNTER, DTYPES, HEADS, SEED, SHAPES, STRIDED

pytestmark = pytest.mark.gpu

TEAMS = {4: ((2, 2), (2, 2)), 6: ((3, 3), (3, 3))}


def _sim(worlds, agents=4, seed=0, flags=0, world_offset=0, teams=None):
    import gpu_hideseek
    hiders, seekers = teams or TEAMS[agents]
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=flags, rand_seed=seed,
        min_hiders=hiders[0], max_hiders=hiders[1], min_seekers=seekers[0], max_seekers=seekers[1], num_pbt_policies=1,
        world_offset=world_offset)
    return sim


@pytest.fixture(scope="module")
def sims():
    """Initialised simulators by (worlds, agents per world), shared by the tests that only need rows to sample for."""
    made = {}

    def get(worlds, agents=4):
        if (worlds, agents) not in made:
            made[worlds, agents] = _sim(worlds, agents)
            made[worlds, agents].init()
        return made[worlds, agents]
    yield get
    for s in made.values():
        s.close()


def _dev(x, dtype="float32", width=None):
    """The logits x [R, L] (numpy f32, representable in dtype) on the device; width: inside a [R, width] buffer of NaN."""
    import torch
    t = torch.from_numpy(np.array(x, dtype=np.float32)).to(getattr(torch, dtype)).cuda()
    if width is None:
        return t
    buf = torch.full((x.shape[0], width), float("nan"), dtype=t.dtype, device="cuda")
    buf[:, :x.shape[1]] = t
    return buf[:, :x.shape[1]]


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


ALL = dict(action=True, log_prob=True, entropy=True, head_log_prob=True)


def _check_against_f64(x, buckets, out, tag, u=None):
    """Every output of a call within the derived tolerances of float64 at the GPU's own action; with u: the draws too."""
    tol = H.tolerances()
    act = out["action"]
    R = x.shape[0]
    assert act.dtype == np.int32 and act.shape == (R, HEADS) and (act >= 0).all() and (act < np.array(buckets)).all(), tag
    cdf, hlp, lp, ent, p = H.reference64(x, buckets, act)
    assert (p > 0).all(), (tag, "a bucket of probability 0 was chosen", np.argwhere(p == 0)[:3].tolist())
    if u is not None:
        r = np.arange(R)
        for h, c in enumerate(cdf):
            lo = np.where(act[:, h] > 0, c[r, np.maximum(act[:, h] - 1, 0)], 0.0)
            ok = (lo - tol["cdf"] <= u[:, h]) & (u[:, h] < c[r, act[:, h]] + tol["cdf"])
            assert ok.all(), (tag, h, np.argwhere(~ok)[:3].tolist())
        ne = H.near_edge(cdf, u, tol["cdf"])
        assert ne.sum() < H.NEAR_EDGE_CAP * ne.size, (tag, int(ne.sum()))
    for name, want in (("head_log_prob", hlp), ("log_prob", lp), ("entropy", ent)):
        got = out[name]
        assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all(), (tag, name)
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"{tag} {name}: max error {err:.3e} (tolerance {tol[name]:.3e})")
        assert err <= tol[name], (tag, name, err, tol[name])
    assert np.array_equal(H.sum5(out["head_log_prob"]).view(np.int32), out["log_prob"].view(np.int32)), tag


@pytest.mark.parametrize("buckets", BUCKETS, ids=lambda b: f"k{b[0]}")
@pytest.mark.parametrize("dtype", DTYPES)
def test_draws_are_the_right_ones(sims, dtype, buckets):
    for worlds, agents in SHAPES:
        sim, rows = sims(worlds, agents), worlds * agents
        x = H.logits_of(rows, buckets, dtype)
        u = H.uniforms(SEED, COUNTER, np.arange(rows))
        outs = []
        for width in (None, STRIDED):
            lg = _dev(x, dtype, width)
            assert lg.stride(0) == (width or sum(buckets))
            out = _np(sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=COUNTER, **ALL))
            _check_against_f64(x, buckets, out, (rows, dtype, buckets[0], width), u)
            outs.append(out)
        for k in outs[0]:                                        # the stride changes nothing
            assert np.array_equal(outs[0][k].view(np.int32), outs[1][k].view(np.int32)), (rows, k)
        # the f32 restatement draws the same action wherever u is not next to an edge
        want = np.stack([H.draw_f32(l, u[:, h]) for h, l in enumerate(H.heads_of(x, buckets))], 1)
        far = ~H.near_edge(H.reference64(x, buckets, want)[0], u, H.tolerances()["cdf"])
        assert np.array_equal(outs[0]["action"][far], want[far])


def test_one_live_bucket_is_exact(sims):
    worlds, agents = SHAPES[2]
    sim, rows = sims(worlds, agents), worlds * agents
    rng = np.random.default_rng(3)
    for buckets in BUCKETS:
        x = np.full((rows, sum(buckets)), -np.inf, dtype=np.float32)
        idx = np.stack([rng.integers(0, K, size=rows) for K in buckets], 1).astype(np.int32)
        off = np.concatenate([[0], np.cumsum(buckets)])
        for h in range(HEADS):
            x[np.arange(rows), off[h] + idx[:, h]] = 0.0
        for mode in ("draw", "greedy"):
            out = _np(sim.sample_actions(_dev(x), buckets=buckets, mode=mode, seed=SEED, counter=1, **ALL))
            assert np.array_equal(out["action"], idx), (buckets, mode)
            for k in ("log_prob", "entropy", "head_log_prob"):     # +0.0, bit for bit
                assert not out[k].view(np.int32).any(), (buckets, mode, k)


def test_a_masked_last_bucket_is_never_drawn(sims):
    """Equal logits with the last one (or two) buckets at -inf, over 16 counters: among the 144 480 uniforms per bucket
    set are ones within 2^-12 of 1, and those rows draw the last live bucket, never a masked one.  (The fall-back of
    the draw, "no index has u S < c_a", cannot be reached by a finite head: u <= 1 - 2^-24, and the f32 product of that
    with S is below S for every S.  The kernel keeps the guard; this test pins what it guards.)"""
    worlds, agents = SHAPES[2]
    sim, rows = sims(worlds, agents), worlds * agents
    top = 0
    for buckets in BUCKETS:
        for masked in (1, 2):
            x = np.zeros((rows, sum(buckets)), dtype=np.float32)
            heads = H.heads_of(x, buckets)
            live = [K - (masked if K > masked else 0) for K in buckets]
            for h, K in enumerate(buckets):
                heads[h][:, live[h]:] = -np.inf
            lg = _dev(x)
            for counter in range(16):
                act = sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=counter, action=True)["action"].cpu().numpy()
                assert (act < np.array(live)).all() and (act >= 0).all(), (buckets, masked, counter)
                u = H.uniforms(SEED, counter, np.arange(rows))
                hot = u >= 1.0 - 2.0 ** -12
                top += int(hot.sum())
                assert np.array_equal(act[hot], np.broadcast_to(np.array(live) - 1, act.shape)[hot])
    assert top >= 20


def test_greedy_is_the_first_maximum(sims):
    worlds, agents = SHAPES[2]
    sim, rows = sims(worlds, agents), worlds * agents
    rng = np.random.default_rng(4)
    for buckets in BUCKETS:
        x = rng.integers(-1, 2, size=(rows, sum(buckets))).astype(np.float32)          # ties in almost every head
        x[rng.random(x.shape) < 0.2] = -np.inf
        for h, l in enumerate(H.heads_of(x, buckets)):
            l[np.isneginf(l).all(1), -1] = 1.0
        x[:8] = 0.5                                                                    # all equal: index 0
        want = np.stack([l.argmax(1) for l in H.heads_of(x, buckets)], 1).astype(np.int32)
        assert (np.stack([(l == l.max(1, keepdims=True)).sum(1) for l in H.heads_of(x, buckets)], 1) > 1).mean() > 0.3
        for dtype in DTYPES:
            out = _np(sim.sample_actions(_dev(x, dtype, STRIDED), buckets=buckets, mode="greedy", **ALL))
            assert np.array_equal(out["action"], want), (buckets, dtype)
            _check_against_f64(x, buckets, out, ("greedy", buckets[0], dtype))


def test_evaluate_returns_what_the_draw_returned(sims):
    import torch
    worlds, agents = SHAPES[2]
    sim, rows = sims(worlds, agents), worlds * agents
    for buckets in BUCKETS:
        lg = _dev(H.logits_of(rows, buckets, "bfloat16"), "bfloat16")
        drawn = sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=5, **ALL)
        act = drawn["action"].clone()
        ev = sim.sample_actions(lg, buckets=buckets, mode="evaluate", action=act, log_prob=True, entropy=True, head_log_prob=True)
        assert ev["action"].data_ptr() == act.data_ptr() and torch.equal(act, drawn["action"])
        for k in ("log_prob", "entropy", "head_log_prob"):
            assert _same(ev[k], drawn[k]), (buckets, k)
        # in place: the simulator's own action tensor is read and left as it is
        mine = sim.action_tensor().to_torch()
        mine.copy_(act)
        ev = sim.sample_actions(lg, buckets=buckets, mode="evaluate", log_prob=True)
        assert torch.equal(mine, act) and _same(ev["log_prob"], drawn["log_prob"]) and ev["action"].data_ptr() == mine.data_ptr()
        # out-of-range actions are clamped for the lookup, and not rewritten
        wild = act.clone()
        wild[::3] = 99
        wild[1::3] = -3
        clamped = torch.minimum(wild.clamp(min=0), torch.tensor(buckets, dtype=torch.int32, device="cuda") - 1)
        keep = wild.clone()
        a = sim.sample_actions(lg, buckets=buckets, mode="evaluate", action=wild, log_prob=True, entropy=True)
        b = sim.sample_actions(lg, buckets=buckets, mode="evaluate", action=clamped, log_prob=True, entropy=True)
        assert torch.equal(wild, keep) and _same(a["log_prob"], b["log_prob"]) and _same(a["entropy"], b["entropy"])


def test_determinism_and_keying(sims):
    worlds, agents = SHAPES[2]
    sim, rows = sims(worlds, agents), worlds * agents
    buckets = BUCKETS[0]
    lg = _dev(H.logits_of(rows, buckets, "float32"))
    base = _np(sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=COUNTER, **ALL))
    again = _np(sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=COUNTER, **ALL))
    for k in base:
        assert np.array_equal(base[k].view(np.int32), again[k].view(np.int32)), k
    for kw in (dict(seed=SEED, counter=COUNTER + 1), dict(seed=(SEED[0] + 1, SEED[1]), counter=COUNTER),
               dict(seed=(SEED[0], SEED[1] + 1), counter=COUNTER)):
        other = _np(sim.sample_actions(lg, buckets=buckets, action=True, **kw))["action"]
        assert (other != base["action"]).any(1).mean() > 1 / 3, kw
        want = H.uniforms(kw["seed"], kw["counter"], np.arange(rows))
        x = H.logits_of(rows, buckets, "float32")
        _check_against_f64(x, buckets, dict(_np(sim.sample_actions(lg, buckets=buckets, **ALL, **kw))), ("keying", kw["counter"]), want)
    # a wider tensor passed whole (W > L) and a strided view of it read the same columns
    wide = _dev(H.logits_of(rows, buckets, "float32"), "float32", STRIDED)
    whole = wide._base if wide._base is not None else wide
    for t in (wide, whole):
        got = _np(sim.sample_actions(t, buckets=buckets, seed=SEED, counter=COUNTER, **ALL))
        for k in base:
            assert np.array_equal(base[k].view(np.int32), got[k].view(np.int32)), k


def test_shards_draw_what_one_handle_draws():
    import gpu_hideseek
    buckets = BUCKETS[1]
    x = H.logits_of(64, buckets, "float16", seed=1)
    one = _sim(16)
    one.init()
    want = _np(one.sample_actions(_dev(x, "float16"), buckets=buckets, seed=SEED, counter=9, **ALL))
    one.close()
    halves = [_sim(8, world_offset=0), _sim(8, world_offset=8)]
    for i, s in enumerate(halves):
        s.init()
        got = _np(s.sample_actions(_dev(x[32 * i:32 * i + 32], "float16"), buckets=buckets, seed=SEED, counter=9, **ALL))
        for k in want:
            assert np.array_equal(got[k].view(np.int32), want[k][32 * i:32 * i + 32].view(np.int32)), (i, k)
        s.close()
    _check_against_f64(x[32:], buckets, got, "offset 8", H.uniforms(SEED, 9, 32 + np.arange(32)))
    # the same through ShardedSimulator, whose shards carry the offsets
    kw = dict(sim_flags=0, rand_seed=0, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0], 16, **kw)
    ss.init()
    res = ss.sample_actions([_dev(x[:32], "float16"), _dev(x[32:], "float16")], buckets=buckets, seed=SEED, counter=9,
                            log_prob=True, entropy=True, head_log_prob=True)
    assert len(res) == 2
    for i, (shard, r) in enumerate(zip(ss.shards, res)):
        assert r["action"].data_ptr() == shard.action_tensor().to_torch().data_ptr()
        r = _np(r)
        for k in want:
            assert np.array_equal(r[k].view(np.int32), want[k][32 * i:32 * i + 32].view(np.int32)), (i, k)
    ss.step()
    ss.close()


def _exports(sim):
    import gpu_hideseek
    return {n: getattr(sim, n + "_tensor")().to_torch().clone() for n in gpu_hideseek._EXPORTS if n not in ("depth", "rgb")}


def _rollout(how, steps=20, worlds=64):
    """`steps` steps of a 3+3 simulator driven by sampled actions; how: "in place", "buffer" or "interleaved"."""
    import torch
    sim = _sim(worlds, 6, seed=5, flags=13)
    sim.init()
    rows, buckets = worlds * 6, BUCKETS[1]
    mine = sim.action_tensor().to_torch()
    buf = torch.empty(rows, HEADS, dtype=torch.int32, device="cuda")
    for t in range(steps):
        lg = _dev(H.logits_of(rows, buckets, "float32", seed=100 + t))
        if how == "in place":
            out = sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=t, log_prob=True)
            assert out["action"].data_ptr() == mine.data_ptr()
        else:
            sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=t, action=buf, log_prob=True)
            mine.copy_(buf)
        sim.step()
        if how == "interleaved":                                 # sampler calls that must leave the simulator alone
            other = torch.empty_like(buf)
            sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=1000 + t, action=other, entropy=True)
            sim.sample_actions(lg, buckets=buckets, mode="greedy", action=other, zero_inactive=True)
            sim.sample_actions(lg, buckets=buckets, mode="evaluate", action=other, log_prob=True)
            sim.sample_actions(lg, buckets=buckets, mode="evaluate", head_log_prob=True)
    out = _exports(sim)
    sim.close()
    return out


def test_in_place_sampling_feeds_the_step_and_side_calls_change_nothing():
    import torch
    runs = {how: _rollout(how) for how in ("in place", "buffer", "interleaved")}
    assert int((runs["buffer"]["action"] != 0).sum()) > 0
    for how in ("in place", "interleaved"):
        for name, want in runs["buffer"].items():
            assert _same(runs[how][name], want), (how, name)


def test_zero_inactive_zeroes_the_inactive_rows():
    import torch
    worlds = 64
    sim = _sim(worlds, flags=13, seed=5, teams=((1, 3), (1, 3)))
    sim.init()
    sim.step()
    rows, buckets = worlds * sim.agents_per_world, BUCKETS[0]
    assert sim.agents_per_world == 6
    live = sim.self_mask_tensor().to_torch().reshape(rows) != 0
    assert 0 < int(live.sum()) < rows
    lg = _dev(H.logits_of(rows, buckets, "float32", seed=2))
    for mode in ("greedy", "draw"):
        plain = sim.sample_actions(lg, buckets=buckets, mode=mode, seed=SEED, counter=2, **ALL)
        zeroed = sim.sample_actions(lg, buckets=buckets, mode=mode, seed=SEED, counter=2, zero_inactive=True, **ALL)
        for k in plain:
            assert _same(zeroed[k][live], plain[k][live]), (mode, k)
            assert not _bits(zeroed[k][~live]).any(), (mode, k)
        assert bool((plain["action"][~live] != 0).any())
    # in place (the draw again), and scoring a stored action
    sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=2, zero_inactive=True)
    assert torch.equal(sim.action_tensor().to_torch(), zeroed["action"])
    ev = sim.sample_actions(lg, buckets=buckets, mode="evaluate", action=plain["action"], log_prob=True, entropy=True,
                            zero_inactive=True)
    assert not _bits(ev["log_prob"][~live]).any() and not _bits(ev["entropy"][~live]).any()
    assert _same(ev["log_prob"][live], plain["log_prob"][live])
    sim.close()


def test_the_stream_form_equals_the_blocking_form(sims):
    import torch
    worlds, agents = SHAPES[2]
    sim, rows = sims(worlds, agents), worlds * agents
    buckets = BUCKETS[1]
    lg = _dev(H.logits_of(rows, buckets, "bfloat16"), "bfloat16", STRIDED)
    blocking = sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=4, **ALL)
    side = torch.cuda.Stream()
    ev = torch.cuda.Event()
    ev.record()
    side.wait_event(ev)
    got = sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=4, stream=side, **ALL)
    raw = sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=4, stream=side.cuda_stream, log_prob=True)     # in place
    side.synchronize()
    for k in blocking:
        assert _same(got[k], blocking[k]), k
    assert _same(raw["log_prob"], blocking["log_prob"]) and torch.equal(raw["action"], blocking["action"])
    assert raw["action"].data_ptr() == sim.action_tensor().to_torch().data_ptr()
    # a slot of a rollout buffer; the other slots keep their sentinel
    buf = torch.full((3, rows), -7.0, device="cuda")
    abuf = torch.full((3, rows, HEADS), -7, dtype=torch.int32, device="cuda")
    res = sim.sample_actions(lg, buckets=buckets, seed=SEED, counter=4, action=abuf[1], log_prob=buf[1])
    assert res["log_prob"].data_ptr() == buf[1].data_ptr() and _same(buf[1], blocking["log_prob"])
    assert torch.equal(abuf[1], blocking["action"]) and bool((buf[[0, 2]] == -7).all()) and bool((abuf[[0, 2]] == -7).all())


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import action_sampling as A
    from lockstep import EXT_SKIP_OBSERVATIONS
    INVALID, UNSUPPORTED = 1, 3
    worlds, rows, buckets = 16, 64, BUCKETS[0]
    L = sum(buckets)
    lg = torch.zeros(rows * L + 8, device="cuda")
    lgh = torch.zeros(rows * L + 8, dtype=torch.bfloat16, device="cuda")
    act = torch.full((rows * HEADS + 8,), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((rows + 8,), -7.0, device="cuda")
    ent = torch.full((rows + 8,), -7.0, device="cuda")
    hlp = torch.full((rows * HEADS + 8,), -7.0, device="cuda")

    def req(logits=lg.data_ptr(), dtype=1, stride=L, b=buckets, mode=0, flags=0, action=act.data_ptr(), log_prob=lp.data_ptr(),
            entropy=ent.data_ptr(), head=hlp.data_ptr()):
        return A.HsSampleRequest(logits, dtype, stride, (C.c_int32 * HEADS)(*b), mode, flags, (C.c_uint32 * 2)(1, 2), 3,
                                 action, log_prob, entropy, head)

    def untouched(sim=None):
        torch.cuda.synchronize()
        mine = True if sim is None else bool((sim.action_tensor().to_torch() == -7).all())
        return mine and all(bool((t == -7).all()) for t in (act, lp, ent, hlp))

    def call(sim, r, stream=False):
        p = C.byref(r) if r is not None else None
        if stream:
            return sim._L.hs_sample_actions_async(sim._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p)
        return sim._L.hs_sample_actions(sim._h, p)

    sim = _sim(worlds)
    assert call(sim, req()) == INVALID and "before hs_init" in sim._L.hs_last_error().decode() and untouched()
    sim.init()
    sim.action_tensor().to_torch().fill_(-7)
    bad = {
        "null request": None, "null logits": req(logits=None), "dtype i32": req(dtype=0), "dtype u8": req(dtype=2), "dtype 7": req(dtype=7),
        "mode": req(mode=3), "mode -1": req(mode=-1), "flag bit": req(flags=2), "flag bits": req(flags=0x80000001),
        "bucket 0": req(b=(5, 5, 0, 2, 2), stride=40), "bucket 17": req(b=(17, 5, 5, 2, 2), stride=40),
        "65 logits": req(b=(16, 16, 16, 16, 1), stride=80), "stride": req(stride=L - 1), "stride 0": req(stride=0),
        "logits f32 +2": req(logits=lg.data_ptr() + 2), "logits bf16 +1": req(logits=lgh.data_ptr() + 1, dtype=3),
        "action +2": req(action=act.data_ptr() + 2), "log_prob +1": req(log_prob=lp.data_ptr() + 1),
        "entropy +2": req(entropy=ent.data_ptr() + 2), "head +3": req(head=hlp.data_ptr() + 3),
        "evaluate, no output": req(mode=2, log_prob=None, entropy=None, head=None),
        "evaluate in place, no output": req(mode=2, action=None, log_prob=None, entropy=None, head=None),
    }
    for what, r in bad.items():
        for stream in (False, True):
            assert call(sim, r, stream) == INVALID, what
    assert untouched(sim)
    sim.step_begin()
    for stream in (False, True):
        assert call(sim, req(), stream) == INVALID and "open step" in sim._L.hs_last_error().decode()
    sim.step_end()
    assert untouched()                                            # (the step itself may rewrite the simulator's own actions)
    # bf16 logits two bytes past a 4-byte boundary are aligned to their element; the accepted call does write
    assert call(sim, req(logits=lgh.data_ptr() + 2, dtype=3, action=None)) == 0
    assert not untouched() and not bool((sim.action_tensor().to_torch() == -7).any())
    sim.close()

    skip = _sim(worlds, flags=EXT_SKIP_OBSERVATIONS)
    skip.init()
    for t in (act, lp, ent, hlp):
        t.fill_(-7)
    for stream in (False, True):
        assert call(skip, req(flags=1), stream) == UNSUPPORTED
    assert untouched()
    assert call(skip, req()) == 0 and not untouched()             # without the flag it works under skip-observations
    skip.close()
