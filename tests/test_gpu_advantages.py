"""GAE on the GPU (sim.compute_advantages, hs_compute_gae, csrc/hs_k_gae.h) against the numpy restatement of
tests/test_advantages_host.py, bit for bit: shapes and dtypes, crafted done patterns, edge parameters, the outputs that
were not asked for, the moments, shard invariance, a rollout of the simulator itself, the stream form and the refusals
of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import test_advantages_host as H
from test_advantages_host import DTYPES, GAMMA, LAMBDA, bits, gae_f32

pytestmark = pytest.mark.gpu

SHAPES = ((1, 4), (6, 6), (301, 6))               # (worlds, agents per world): 4, 36 and 1 806 rows
STEPS = (1, 2, 7, 40, 67)
TEAMS = {4: ((2, 2), (2, 2)), 6: ((3, 3), (3, 3))}


def _sim(worlds, agents=4, seed=0, flags=0, world_offset=0):
    import gpu_hideseek
    hiders, seekers = TEAMS[agents]
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=flags, rand_seed=seed,
        min_hiders=hiders[0], max_hiders=hiders[1], min_seekers=seekers[0], max_seekers=seekers[1], num_pbt_policies=1,
        world_offset=world_offset)


@pytest.fixture(scope="module")
def sims():
    """Initialised simulators by (worlds, agents per world), shared by the tests that only need a handle of that many rows."""
    made = {}

    def get(worlds, agents=4):
        if (worlds, agents) not in made:
            made[worlds, agents] = _sim(worlds, agents)
            made[worlds, agents].init()
        return made[worlds, agents]
    yield get
    for s in made.values():
        s.close()


def _dev(x, dtype="float32"):
    """Inputs of H.inputs on the device; value and bootstrap in `dtype` (they are representable in it)."""
    import torch
    out = {}
    for k, v in x.items():
        if v is None:
            out[k] = None
        else:
            t = torch.from_numpy(np.ascontiguousarray(v)).cuda()
            out[k] = t.to(getattr(torch, dtype)) if k in ("value", "bootstrap") else t
    return out


def _call(sim, d, **kw):
    return sim.compute_advantages(d["reward"], d["done"], d["value"], d["bootstrap"], mask=d["mask"], **kw)


def _want(x, gamma=GAMMA, lam=LAMBDA):
    return gae_f32(x["reward"], x["done"], x["value"], x["bootstrap"], x["mask"], gamma, lam)


def _check(out, x, tag, gamma=GAMMA, lam=LAMBDA):
    """advantages and returns of a call equal gae_f32 bit for bit, and returns == advantages + value where active."""
    adv, ret = out["advantages"].cpu().numpy(), out["returns"].cpu().numpy()
    wa, wr = _want(x, gamma, lam)
    assert adv.dtype == np.float32 and adv.shape == wa.shape and ret.shape == wr.shape, tag
    for name, got, want in (("advantages", adv, wa), ("returns", ret, wr)):
        ne = bits(got) != bits(want)
        assert not ne.any(), (tag, name, int(ne.sum()), np.argwhere(ne)[:3].tolist())
    assert np.isfinite(adv).all() and np.isfinite(ret).all(), tag
    on = np.ones(adv.shape, bool) if x["mask"] is None else x["mask"] != 0
    assert np.array_equal(bits(ret[on]), bits(adv[on] + x["value"][on])), tag
    assert not bits(adv[~on]).any() and not bits(ret[~on]).any(), tag


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bit_parity(sims, dtype, masked):
    for worlds, agents in SHAPES:
        sim, rows = sims(worlds, agents), worlds * agents
        for T in STEPS:
            x = H.inputs(T, rows, dtype, masked, seed=10)
            _check(_call(sim, _dev(x, dtype)), x, (rows, T, dtype, masked))


def test_accepted_shapes_give_the_same_bits(sims):
    import torch
    worlds, agents = SHAPES[1]
    sim, rows, T = sims(worlds, agents), worlds * agents, 7
    x = H.inputs(T, rows, "bfloat16", True, seed=11)
    d = _dev(x, "bfloat16")
    flat = _call(sim, d)
    _check(flat, x, "flat")
    for shape in ((T, rows, 1), (T, worlds, agents)):
        e = {k: v.reshape(shape if k != "bootstrap" else shape[1:]) for k, v in d.items()}
        out = _call(sim, e)
        assert tuple(out["advantages"].shape) == shape and tuple(out["returns"].shape) == shape
        for k in ("advantages", "returns"):
            assert torch.equal(out[k].reshape(T, rows).view(torch.int32), flat[k].view(torch.int32)), (shape, k)


@pytest.mark.parametrize("pattern", ["none", "all", "first", "last"])
def test_crafted_done_patterns(sims, pattern):
    worlds, agents = SHAPES[1]
    sim, rows, T = sims(worlds, agents), worlds * agents, 7
    for dtype in DTYPES:
        x = H.inputs(T, rows, dtype, masked=False, seed=12)
        x["done"][:] = 0
        if pattern == "all":
            x["done"][:] = 1
        elif pattern == "first":
            x["done"][0] = 1
        elif pattern == "last":
            x["done"][T - 1] = 1
            x["bootstrap"][:] = np.nan                    # the bootstrap must not matter
        out = _call(sim, _dev(x, dtype))
        _check(out, x, (pattern, dtype))                  # (_check requires finite outputs)
        if pattern == "all":
            assert np.array_equal(bits(out["advantages"].cpu().numpy()), bits(x["reward"] - x["value"]))


@pytest.mark.parametrize("gamma,lam", [(1.0, 1.0), (0.0, 0.95), (0.998, 0.0), (0.998, 0.95)])
def test_edge_parameters(sims, gamma, lam):
    worlds, agents = SHAPES[2]
    sim, rows = sims(worlds, agents), worlds * agents
    for dtype, masked, T in (("float32", True, 40), ("float16", False, 67)):
        x = H.inputs(T, rows, dtype, masked, seed=13)
        _check(_call(sim, _dev(x, dtype), gamma=gamma, gae_lambda=lam), x, (gamma, lam, dtype), gamma, lam)


def test_only_requested_outputs_are_written(sims):
    import torch
    worlds, agents = SHAPES[1]
    sim, rows, T = sims(worlds, agents), worlds * agents, 40
    x = H.inputs(T, rows, "float32", True, seed=14)
    d = _dev(x)
    both = _call(sim, d)
    _check(both, x, "both")
    for name, other in (("advantages", "returns"), ("returns", "advantages")):
        buf = torch.full((3, T, rows), -7.0, device="cuda")          # the output in the middle, canaries on both sides
        mom = torch.full((7,), -7.0, dtype=torch.float64, device="cuda")
        out = _call(sim, d, **{name: buf[1], other: None})
        assert set(out) == {name} and out[name].data_ptr() == buf[1].data_ptr()
        assert torch.equal(buf[1].view(torch.int32), both[name].view(torch.int32)), name
        assert bool((buf[[0, 2]] == -7).all()) and bool((mom == -7).all()), name
    # moments alone: neither tensor is written
    buf = torch.full((2, T, rows), -7.0, device="cuda")
    out = _call(sim, d, advantages=None, returns=None, moments=True)
    assert set(out) == {"moments"} and bool((buf == -7).all())
    want = _call(sim, d, moments=True)["moments"]
    assert torch.equal(out["moments"].view(torch.int64), want.view(torch.int64))


def test_moments(sims):
    import torch
    from gpu_hideseek import advantages as A
    for (worlds, agents), T, dtype, masked in ((SHAPES[2], 67, "float32", True), (SHAPES[2], 40, "bfloat16", False),
                                               (SHAPES[0], 1, "float16", True), (SHAPES[1], 7, "float32", True)):
        sim, rows = sims(worlds, agents), worlds * agents
        x = H.inputs(T, rows, dtype, masked, seed=15)
        d = _dev(x, dtype)
        plain = _call(sim, d)
        out = _call(sim, d, moments=True)
        again = _call(sim, d, moments=True)
        _check(out, x, ("moments", rows, T))
        m = out["moments"].cpu().numpy()
        assert m.dtype == np.float64 and m.shape == (5,)
        assert np.array_equal(m.view(np.int64), again["moments"].cpu().numpy().view(np.int64))            # the same bits every call
        assert torch.equal(out["advantages"].view(torch.int32), plain["advantages"].view(torch.int32))   # moments change nothing
        assert torch.equal(out["returns"].view(torch.int32), plain["returns"].view(torch.int32))
        on = np.ones((T, rows), bool) if x["mask"] is None else x["mask"] != 0
        assert m[4] == float(on.sum())
        # against numpy's float64 sum of the GPU's own outputs: n 2^-53 sum |term|, the worst case of reordering a sum
        adv, ret = out["advantages"].cpu().numpy().astype(np.float64)[on], out["returns"].cpu().numpy().astype(np.float64)[on]
        n = T * rows
        for i, term in enumerate((adv, adv * adv, ret, ret * ret)):
            bound = n * 2.0 ** -53 * np.abs(term).sum()
            err = abs(m[i] - term.sum())
            print(f"rows={rows} T={T} moments[{i}] = {m[i]:.17g}: |gpu - numpy| = {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (rows, T, i, err, bound)
        stats = A.moments_to_mean_std(out["moments"])
        if on.any():
            assert abs(float(stats["advantages"][0]) - adv.mean()) <= 1e-9 * (1 + np.abs(adv).max())
            assert abs(float(stats["returns"][1]) - ret.std()) <= 1e-6 * (1 + np.abs(ret).max())


def test_shards_compute_what_one_handle_computes():
    import gpu_hideseek
    import torch
    T, rows = 40, 24
    x = H.inputs(T, rows, "float16", True, seed=16)
    one = _sim(6)
    one.init()
    d = _dev(x, "float16")
    want = _call(one, d)
    _check(want, x, "one handle")
    one.close()

    def half(i):
        return {k: (None if v is None else v[..., 12 * i:12 * i + 12].contiguous()) for k, v in d.items()}
    for i, s in enumerate((_sim(3, world_offset=0), _sim(3, world_offset=3))):
        s.init()
        got = _call(s, half(i))
        for k in ("advantages", "returns"):
            assert torch.equal(got[k].view(torch.int32), want[k][:, 12 * i:12 * i + 12].contiguous().view(torch.int32)), (i, k)
        s.close()
    kw = dict(sim_flags=0, rand_seed=0, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0], 6, **kw)
    ss.init()
    assert [s.num_worlds for s in ss.shards] == [3, 3]
    halves = [half(0), half(1)]
    res = ss.compute_advantages(*[[h[k] for h in halves] for k in ("reward", "done", "value", "bootstrap")],
                                mask=[h["mask"] for h in halves], moments=True)
    assert len(res) == 2
    for i, r in enumerate(res):
        for k in ("advantages", "returns"):
            assert torch.equal(r[k].view(torch.int32), want[k][:, 12 * i:12 * i + 12].contiguous().view(torch.int32)), (i, k)
        assert float(r["moments"][4]) == float((x["mask"][:, 12 * i:12 * i + 12] != 0).sum())
    ss.close()


def test_a_rollout_of_the_simulator_itself():
    import torch
    worlds, T, before = 6, 40, 220
    sim = _sim(worlds, 6, seed=3)                      # episode length on: every world resets at step 240
    sim.init()
    rows = worlds * sim.agents_per_world
    action = sim.action_tensor().to_torch()
    g = torch.Generator(device="cuda").manual_seed(0)
    high = torch.tensor([11, 11, 11, 2, 2], device="cuda")
    rew = torch.empty(T, rows, device="cuda")
    done = torch.empty(T, rows, dtype=torch.int32, device="cuda")
    mask = torch.empty(T, rows, device="cuda")
    for t in range(before + T):
        action.copy_((torch.rand(rows, 5, device="cuda", generator=g) * high).to(torch.int32))
        sim.step()
        if t >= before:
            rew[t - before].copy_(sim.reward_tensor().to_torch().reshape(rows))
            done[t - before].copy_(sim.done_tensor().to_torch().reshape(rows))
            mask[t - before].copy_(sim.self_mask_tensor().to_torch().reshape(rows))
    assert bool((done != 0).any()) and not bool((done != 0).all()), "the window must contain the reset of step 240"
    rng = np.random.default_rng(17)
    x = dict(reward=rew.cpu().numpy(), done=done.cpu().numpy(), mask=mask.cpu().numpy(),
             value=(5.0 * rng.standard_normal((T, rows))).astype(np.float32),
             bootstrap=(5.0 * rng.standard_normal(rows)).astype(np.float32))
    d = dict(reward=rew, done=done, mask=mask, value=torch.from_numpy(x["value"]).cuda(), bootstrap=torch.from_numpy(x["bootstrap"]).cuda())
    _check(_call(sim, d), x, "simulator")
    sim.close()


def test_the_stream_form_equals_the_blocking_form(sims):
    import torch
    worlds, agents = SHAPES[2]
    sim, rows, T = sims(worlds, agents), worlds * agents, 40
    x = H.inputs(T, rows, "bfloat16", True, seed=18)
    d = _dev(x, "bfloat16")
    blocking = _call(sim, d, moments=True)
    _check(blocking, x, "blocking")
    side = torch.cuda.Stream()
    ev = torch.cuda.Event()
    ev.record()
    side.wait_event(ev)
    got = _call(sim, d, moments=True, stream=side)
    raw = _call(sim, d, stream=side.cuda_stream)
    side.synchronize()
    for k in ("advantages", "returns"):
        assert torch.equal(got[k].view(torch.int32), blocking[k].view(torch.int32)), k
        assert torch.equal(raw[k].view(torch.int32), blocking[k].view(torch.int32)), k
    assert torch.equal(got["moments"].view(torch.int64), blocking["moments"].view(torch.int64))


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import advantages as A
    from lockstep import EXT_SKIP_OBSERVATIONS
    INVALID = 1
    worlds, rows, T = 4, 16, 5
    n = T * rows
    x = H.inputs(T, rows, "float32", True, seed=19)
    rew = torch.zeros(n + 8, device="cuda")
    rew[:n] = torch.from_numpy(x["reward"]).reshape(n)
    don = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    don[:n] = torch.from_numpy(x["done"]).reshape(n)
    val = torch.zeros(n + 8, device="cuda")
    val[:n] = torch.from_numpy(x["value"]).reshape(n)
    valh = torch.zeros(n + 8, dtype=torch.bfloat16, device="cuda")
    boot = torch.zeros(rows + 8, device="cuda")
    boot[:rows] = torch.from_numpy(x["bootstrap"])
    booth = torch.zeros(rows + 8, dtype=torch.bfloat16, device="cuda")
    msk = torch.ones(n + 8, device="cuda")
    msk[:n] = torch.from_numpy(x["mask"]).reshape(n)
    adv = torch.full((n + 8,), -7.0, device="cuda")
    ret = torch.full((n + 8,), -7.0, device="cuda")
    mom = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    ab = torch.full((n + rows,), -7.0, device="cuda")          # an advantage whose last element is the bootstrap's first
    inputs = [t.clone() for t in (rew, don, val, boot, msk)]

    def req(reward=rew.data_ptr(), done=don.data_ptr(), value=val.data_ptr(), bootstrap=boot.data_ptr(), mask=msk.data_ptr(),
            dtype=1, steps=T, gamma=GAMMA, lam=LAMBDA, advantage=adv.data_ptr(), returns=ret.data_ptr(), moments=mom.data_ptr()):
        return A.HsGaeRequest(reward, done, value, bootstrap, mask, dtype, steps, gamma, lam, advantage, returns, moments)

    def untouched():
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((rew, don, val, boot, msk), inputs))
        return same and all(bool((t == -7).all()) for t in (adv, ret, mom, ab))

    def call(sim, r, stream=False):
        p = C.byref(r) if r is not None else None
        if stream:
            return sim._L.hs_compute_gae_async(sim._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p)
        return sim._L.hs_compute_gae(sim._h, p)

    def message(sim):
        return sim._L.hs_last_error().decode()

    sim = _sim(worlds)
    for stream in (False, True):
        assert call(sim, req(), stream) == INVALID and "before hs_init" in message(sim)
    assert untouched()
    sim.init()
    bad = {
        "null request": (None, "null request"), "null reward": (req(reward=None), "null reward"), "null done": (req(done=None), "null done"),
        "null value": (req(value=None), "null value"), "null bootstrap": (req(bootstrap=None), "null bootstrap"),
        "no output": (req(advantage=None, returns=None, moments=None), "every output is null"),
        "dtype i32": (req(dtype=0), "dtype"), "dtype u8": (req(dtype=2), "dtype"), "dtype 7": (req(dtype=7), "dtype"),
        "steps 0": (req(steps=0), "steps"), "steps -1": (req(steps=-1), "steps"), "steps 4097": (req(steps=4097), "steps"),
        "gamma 1.5": (req(gamma=1.5), "gamma"), "gamma -0": (req(gamma=-0.001), "gamma"), "gamma nan": (req(gamma=float("nan")), "gamma"),
        "gamma inf": (req(gamma=float("inf")), "gamma"), "lambda nan": (req(lam=float("nan")), "lambda"), "lambda 2": (req(lam=2.0), "lambda"),
        "lambda -inf": (req(lam=float("-inf")), "lambda"),
        "reward +2": (req(reward=rew.data_ptr() + 2), "aligned"), "done +1": (req(done=don.data_ptr() + 1), "aligned"),
        "mask +2": (req(mask=msk.data_ptr() + 2), "aligned"), "value f32 +2": (req(value=val.data_ptr() + 2), "aligned"),
        "value bf16 +1": (req(value=valh.data_ptr() + 1, bootstrap=booth.data_ptr(), dtype=3), "aligned"),
        "bootstrap f16 +1": (req(value=valh.data_ptr(), bootstrap=booth.data_ptr() + 1, dtype=4), "aligned"),
        "advantage +2": (req(advantage=adv.data_ptr() + 2), "aligned"), "returns +1": (req(returns=ret.data_ptr() + 1), "aligned"),
        "moments +4": (req(moments=mom.data_ptr() + 4), "moments must be 8-byte aligned"),
        "advantage is reward": (req(advantage=rew.data_ptr()), "advantage overlaps reward"),
        "returns in value": (req(returns=val.data_ptr() + 16), "returns overlaps value"),
        "advantage on done": (req(advantage=don.data_ptr() + 8), "advantage overlaps done"),
        "returns on mask": (req(returns=msk.data_ptr()), "returns overlaps mask"),
        "advantage ends in bootstrap": (req(advantage=ab.data_ptr(), bootstrap=ab.data_ptr() + 4 * (n - 1)), "advantage overlaps bootstrap"),
        "returns is advantage": (req(returns=adv.data_ptr()), "returns overlaps advantage"),
        "returns into advantage": (req(returns=adv.data_ptr() + 16), "returns overlaps advantage"),
        "moments in returns": (req(moments=ret.data_ptr() + 8), "moments overlaps returns"),
        "moments in reward": (req(moments=rew.data_ptr()), "moments overlaps reward"),
    }
    for what, (r, msg) in bad.items():
        for stream in (False, True):
            assert call(sim, r, stream) == INVALID, what
            assert msg in message(sim), (what, message(sim))
    assert untouched()
    sim.step_begin()
    for stream in (False, True):
        assert call(sim, req(), stream) == INVALID and "open step" in message(sim)
    sim.step_end()
    assert untouched()
    # neighbours that only touch are accepted, as are bf16 values two bytes past a 4-byte boundary; the call does write
    assert call(sim, req(value=valh.data_ptr() + 2, bootstrap=booth.data_ptr() + 2, dtype=3)) == 0
    assert not untouched()
    for t in (adv, ret):
        t.fill_(-7)
    both = torch.full((2 * n,), -7.0, device="cuda")
    assert call(sim, req(advantage=both.data_ptr(), returns=both.data_ptr() + 4 * n)) == 0
    want_a, want_r = gae_f32(x["reward"], x["done"], x["value"], x["bootstrap"], x["mask"], GAMMA, LAMBDA)
    got = both.cpu().numpy()
    assert np.array_equal(bits(got[:n]), bits(want_a.reshape(n))) and np.array_equal(bits(got[n:]), bits(want_r.reshape(n)))
    sim.close()

    skip = _sim(worlds, flags=EXT_SKIP_OBSERVATIONS)          # it reads no export: it works without observations
    skip.init()
    both.fill_(-7)
    assert call(skip, req(advantage=both.data_ptr(), returns=both.data_ptr() + 4 * n)) == 0
    assert np.array_equal(bits(both.cpu().numpy()[:n]), bits(want_a.reshape(n)))
    skip.close()
