"""Policy inputs on the GPU (sim.pack_policy_inputs, hs_pack_policy_inputs, csrc/hs_k_pack.h): f32 rows bit for bit
against the numpy restatement of tests/test_policy_inputs_host.py applied to the ORACLE's tensors, bf16 / f16 rows bit for
bit against torch's own concatenation and cast on the same device, one launch against separate calls, the stream form,
rollout slots, deterministic moments, refusals, and an unaffected step path."""
import numpy as np
import pytest

import lockstep
from lockstep import EXT_SKIP_OBSERVATIONS, Pair, bits
from test_policy_inputs_host import CONFIGS, ENTITIES, ROW, moments_of, obs_of, pack_rows

pytestmark = pytest.mark.gpu


def _pair(cfg, worlds=256, seed=5, **kw):
    flags, hiders, seekers, kind = CONFIGS[cfg]
    return Pair(worlds, flags=flags, seed=seed, hiders=hiders, seekers=seekers, **kw), kind


def _sim(n, seed=0, flags=0, hiders=(2, 2), seekers=(2, 2)):
    import gpu_hideseek
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=flags, rand_seed=seed,
        min_hiders=hiders[0], max_hiders=hiders[1], min_seekers=seekers[0], max_seekers=seekers[1], num_pbt_policies=1)


def _drive(sim, steps, seed=0):
    import torch
    act = sim.action_tensor().to_torch()
    g = torch.Generator(device=act.device).manual_seed(seed)
    for _ in range(steps):
        act[:, 0:2] = torch.randint(-5, 5, (act.shape[0], 2), device=act.device, dtype=torch.int32, generator=g)
        sim.step()


def torch_rows(sim, actor, dtype):
    """The packed rows composed from the simulator's own exports with torch ops on its device."""
    import torch
    t = {n: getattr(sim, n + "_tensor")().to_torch() for n in lockstep.OBS}
    R = t["prep_counter"].shape[0]
    prep = t["prep_counter"].reshape(R, 1).to(torch.float32)
    # (a tensor divisor: torch turns division by a Python scalar into a multiplication by its reciprocal)
    cols = [prep / torch.full_like(prep, 96.0), t["self_data"].reshape(R, -1),
            t["self_type"].reshape(R, 1).to(torch.float32), t["lidar"].reshape(R, -1)]
    for d, m in ENTITIES:
        x = t[d].reshape(R, t[m].reshape(R, -1).shape[1], -1)
        cols.append((x * t[m].reshape(R, -1, 1) if actor else x).reshape(R, -1))
    return torch.cat(cols, 1).to(dtype)


def _bits16(x):
    import torch
    return x.view(torch.int16) if x.dtype != torch.float32 else x.view(torch.int32)


def _check_f32(p, tag):
    ref = obs_of(p.ref)
    out = p.sim.pack_policy_inputs(actor=True, critic=True)
    for name, actor in (("critic", False), ("actor", True)):
        got, want = out[name].cpu().numpy(), pack_rows(ref, actor)
        assert got.dtype == np.float32 and got.shape == want.shape
        bad = np.argwhere(bits(got) != bits(want))
        assert not len(bad), (tag, name, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_f32_rows_equal_the_restatement_of_the_oracle(cfg):
    p, kind = _pair(cfg)
    draw, cols = lockstep.stream(kind)
    _check_f32(p, (cfg, 0))
    assert (pack_rows(obs_of(p.ref), False)[:, 0].max() > 0)          # inside the preparation phase: column 0 is live
    for s in range(241):
        p.step(draw(s, p.rows), cols)
        if s + 1 in (1, 96, 130, 241):
            _check_f32(p, (cfg, s + 1))
    if cfg == "var":
        assert (p.ref.tensor("self_mask") == 0).any()


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_narrow_rows_equal_torch_on_the_device(cfg):
    import torch
    p, kind = _pair(cfg)
    p.drive(130, kind, every=130, names=lockstep.OBS, bodies=False, walls=False)
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        out = p.sim.pack_policy_inputs(actor=True, critic=True, dtype=dtype)
        for name, actor in (("critic", False), ("actor", True)):
            want = torch_rows(p.sim, actor, dtype)
            assert out[name].dtype == dtype and torch.equal(_bits16(out[name]), _bits16(want)), (cfg, dtype, name)
    # f16 subnormals are kept, not flushed
    h = p.sim.pack_policy_inputs(critic=True, dtype=torch.float16)["critic"]
    sub = (h != 0) & (h.abs() < 2.0 ** -14)
    assert int(sub.sum()) > 0


def test_one_launch_equals_separate_calls_stream_form_and_rollout_slot():
    import torch
    p, kind = _pair("3+3")
    p.drive(100, kind, every=100, names=lockstep.OBS, bodies=False, walls=False)
    sim, R = p.sim, p.rows
    one = sim.pack_policy_inputs(actor=True, critic=True, moments=True, dtype=torch.bfloat16)
    a = sim.pack_policy_inputs(actor=True, dtype=torch.bfloat16)["actor"]
    c = sim.pack_policy_inputs(critic=True, dtype=torch.bfloat16)["critic"]
    m = sim.pack_policy_inputs(moments=True)["moments"]
    assert torch.equal(one["actor"].view(torch.int16), a.view(torch.int16))
    assert torch.equal(one["critic"].view(torch.int16), c.view(torch.int16))
    assert m.dtype == torch.float64 and torch.equal(one["moments"].view(torch.int64), m.view(torch.int64))
    # mixed dtypes in one launch
    mix = sim.pack_policy_inputs(actor=torch.empty(R, ROW, dtype=torch.float16, device="cuda"),
                                 critic=torch.empty(R, ROW, dtype=torch.float32, device="cuda"))
    assert torch.equal(mix["actor"].view(torch.int16), torch_rows(sim, True, torch.float16).view(torch.int16))
    assert torch.equal(mix["critic"].view(torch.int32), torch_rows(sim, False, torch.float32).view(torch.int32))

    # the stream form on a side stream, ordered after the step by an event
    p.step(lockstep.stream(kind)[0](0, p.rows))
    side = torch.cuda.Stream()
    ev = torch.cuda.Event()
    ev.record()
    side.wait_event(ev)
    got = sim.pack_policy_inputs(actor=True, critic=True, moments=True, dtype=torch.bfloat16, stream=side)
    side.synchronize()
    blocking = sim.pack_policy_inputs(actor=True, critic=True, moments=True, dtype=torch.bfloat16)
    raw = sim.pack_policy_inputs(critic=True, dtype=torch.bfloat16, stream=side.cuda_stream)      # a raw handle
    side.synchronize()
    for k in ("actor", "critic"):
        assert torch.equal(got[k].view(torch.int16), blocking[k].view(torch.int16)), k
    assert torch.equal(got["moments"].view(torch.int64), blocking["moments"].view(torch.int64))
    assert torch.equal(raw["critic"].view(torch.int16), blocking["critic"].view(torch.int16))

    # a slot of a rollout buffer; the other slots keep their sentinel
    buf = torch.full((4, R, ROW), -7.0, dtype=torch.bfloat16, device="cuda")
    res = sim.pack_policy_inputs(actor=buf[2])
    assert res["actor"].data_ptr() == buf[2].data_ptr()
    assert torch.equal(buf[2].view(torch.int16), blocking["actor"].view(torch.int16))
    assert bool((buf[[0, 1, 3]] == -7.0).all())


def _moment_terms(t):
    x = pack_rows(t, False).astype(np.float64)
    m = t["self_mask"].reshape(-1, 1).astype(np.float64)
    return np.concatenate([np.abs(m * x).sum(0), (m * x * x).sum(0), [m.sum()]])


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_moments_are_deterministic_and_close_to_f64_sums(cfg):
    import torch
    outs = []
    for _ in range(2):                           # two fresh simulators with the same seed
        p, kind = _pair(cfg)
        p.drive(130, kind, every=130, names=lockstep.OBS, bodies=False, walls=False)
        m1 = p.sim.pack_policy_inputs(moments=True)["moments"]
        m2 = p.sim.pack_policy_inputs(moments=True, critic=True, dtype=torch.float16)["moments"]
        assert torch.equal(m1.view(torch.int64), m2.view(torch.int64))
        outs.append(m1.cpu().numpy())
        ref = obs_of(p.ref)
        p.sim.close()
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64))
    want, mag = moments_of(ref), _moment_terms(ref)
    R = ref["self_mask"].shape[0]
    bound = 2 * R * 2.0 ** -53 * mag
    err = np.abs(outs[0] - want)
    print(f"{cfg}: moments max error / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert (err <= bound).all(), (np.argmax(err - bound), err.max())
    assert outs[0][592] == float((ref["self_mask"] > 0).sum())
    if cfg == "var":
        assert outs[0][592] < R


def test_the_size_users_run():
    import torch
    sim = _sim(16000, hiders=(3, 3), seekers=(3, 3))
    sim.init()
    _drive(sim, 20)
    assert sim.agents_per_world == 6
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        out = sim.pack_policy_inputs(actor=True, critic=True, dtype=dtype)
        for name, actor in (("actor", True), ("critic", False)):
            want = torch_rows(sim, actor, dtype)
            assert out[name].shape == (96000, ROW) and torch.equal(_bits16(out[name]), _bits16(want)), (dtype, name)
            del want
    t = {n: getattr(sim, n + "_tensor")().to_torch().cpu().numpy() for n in lockstep.OBS}
    got = sim.pack_policy_inputs(moments=True)["moments"].cpu().numpy()
    assert (np.abs(got - moments_of(t)) <= 2 * 96000 * 2.0 ** -53 * _moment_terms(t)).all()
    sim.close()


def test_refusals_leave_the_outputs_untouched():
    import torch
    R = 64 * 4

    def sentinel(dtype=torch.float32, dev="cuda"):
        return torch.full((R, ROW), -7.0, dtype=dtype, device=dev)

    def untouched(t):
        torch.cuda.synchronize()
        return bool((t == -7.0).all())

    sim = _sim(64)
    out = sentinel()
    with pytest.raises(ValueError, match="before hs_init"):
        sim.pack_policy_inputs(actor=out)
    assert untouched(out)
    sim.init()
    sim.step_begin()
    with pytest.raises(ValueError, match="open step"):
        sim.pack_policy_inputs(actor=out)
    with pytest.raises(ValueError, match="open step"):
        sim.pack_policy_inputs(actor=out, stream=torch.cuda.current_stream())
    sim.step_end()
    assert untouched(out)
    # misaligned: a tensor offset by one element
    flat = torch.full((R * ROW + 8,), -7.0, device="cuda")
    off = flat[1:1 + R * ROW].view(R, ROW)
    with pytest.raises(ValueError, match="16-byte"):
        sim.pack_policy_inputs(critic=off)
    from gpu_hideseek import policy_inputs as P
    from gpu_hideseek._native import check
    import ctypes as C
    for req in (P.HsPackRequest(off.data_ptr(), 1, None, 0, None), P.HsPackRequest(None, 0, off.data_ptr(), 1, None),
                P.HsPackRequest(out.data_ptr(), 2, None, 0, None), P.HsPackRequest(out.data_ptr(), 7, None, 0, None),
                P.HsPackRequest(None, 0, None, 0, None)):
        with pytest.raises(ValueError):          # the library's own checks: alignment, dtype code, nothing requested
            check(sim._L.hs_pack_policy_inputs(sim._h, C.byref(req)))
    with pytest.raises(ValueError):
        check(sim._L.hs_pack_policy_inputs(sim._h, None))
    assert untouched(flat) and untouched(out)
    # wrong dtype, wrong device
    for bad in (sentinel(torch.float64), sentinel(torch.int32), sentinel(dev="cpu")):
        with pytest.raises(ValueError):
            sim.pack_policy_inputs(actor=bad)
        assert bool((bad == -7).all())
    sim.pack_policy_inputs(actor=out)            # and the accepted call does write
    assert not untouched(out)
    sim.close()

    skip = _sim(64, flags=EXT_SKIP_OBSERVATIONS)
    skip.init()
    out = sentinel()
    with pytest.raises(NotImplementedError):
        skip.pack_policy_inputs(actor=out)
    assert untouched(out)
    skip.close()


def test_the_step_path_is_unaffected():
    import torch
    p, kind = _pair("3+3", worlds=64)
    draw, cols = lockstep.stream(kind)
    buf = torch.empty(2, p.rows, ROW, dtype=torch.bfloat16, device="cuda")
    for s in range(40):
        p.step(draw(s, p.rows), cols)
        p.sim.pack_policy_inputs(actor=buf[0], critic=buf[1], moments=True)
        p.check(f"step {s}")


def test_sharded_pack_on_one_device():
    import torch
    import gpu_hideseek
    kw = dict(sim_flags=0, rand_seed=3, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0], 40, **kw)
    ss.init()
    ss.step()
    res = ss.pack_policy_inputs(actor=True, critic=True, moments=True, dtype=torch.bfloat16)
    assert len(res) == 2
    for shard, r in zip(ss.shards, res):
        for name, actor in (("actor", True), ("critic", False)):
            assert torch.equal(r[name].view(torch.int16), torch_rows(shard, actor, torch.bfloat16).view(torch.int16))
        assert float(r["moments"][592]) == shard.num_worlds * 4
    ss.close()
