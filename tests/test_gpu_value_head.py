"""The two-hot symlog critic head on the GPU (sim.value_head, hs_twohot_value, csrc/hs_k_twohot.h) against the numpy
restatement of tests/test_value_head_host.py within the tolerances derived there: sizes around the block of samples and
past the grid cap, bin sets, dtypes, masks; +0 for inactive samples holding NaN; strided and unaligned logits against the
aligned call, bit for bit; determinism and position independence; the outputs that were not asked for; the decode into a
rollout buffer of a live simulator; loss_coef, grad_scale and the count; the sum with ppo_loss against the textbook
total loss; the autograd face; the stream form, the shards and the refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import test_value_head_host as H
from test_value_head_host import BIG, BINS, CASES, DTYPES, ROUNDING, SIZES, STAT_NAMES, f32, twohot

pytestmark = pytest.mark.gpu

STRIDED = 264


def _sim(worlds=6, agents=6, seed=0, flags=0):
    import gpu_hideseek
    k = agents // 2
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=flags, rand_seed=seed,
        min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=1)


@pytest.fixture(scope="module")
def sim():
    """One initialised handle of 6 x 6 rows: n is not tied to it."""
    s = _sim()
    s.init()
    yield s
    s.close()


def _dev(x, dtype="float32"):
    """The inputs of H.inputs on the device; logits in `dtype` (they are representable in it)."""
    import torch
    d = {k: (None if x[k] is None else torch.from_numpy(np.array(x[k])).cuda()) for k in ("returns", "mask")}
    d["logits"] = torch.from_numpy(np.array(x["logits"])).cuda().to(getattr(torch, dtype))
    d.update(bins=x["logits"].shape[1], lo=x["lo"], hi=x["hi"])
    return d


def _call(sim, d, **kw):
    a = dict(d, **kw)
    return sim.value_head(a.pop("logits"), a.pop("returns"), **a)


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype.is_floating_point and t.element_size() < 8 else t.detach().cpu().numpy()


def _bits(t):
    import torch
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _check(out, x, r32, dtype, tag):
    """Parity with the f32 restatement within the derived tolerances; +0 where the contract says so; the statistics."""
    n, B = x["logits"].shape
    tol = H.tolerances(n)
    on = r32["active"]
    if "value" in out:
        v, want = _np(out["value"]).reshape(-1).astype(np.float64), r32["value"].astype(np.float64)
        bound = H.value_bound(want, tol["y"], dtype)
        fits = np.abs(want) + bound < 65504.0 if dtype == "float16" else np.ones(n, bool)      # beyond it float16 rounds to inf
        err = np.abs(v - want)
        print(f"{tag}: value: largest |got - want| / (1 + |want|) = {float((err[fits] / (1 + np.abs(want[fits]))).max(initial=0)):.3e} (tol_y {tol['y']:.3e})")
        assert np.isfinite(v[fits]).all() and (err[fits] <= bound[fits]).all(), (tag, "value", float((err - bound)[fits].max()))
        assert ((v[~fits] == np.sign(want[~fits]) * np.inf) | (err[~fits] <= bound[~fits])).all(), (tag, "float16 overflow")
        assert not _bits(out["value"]).cpu().numpy().reshape(-1)[~on].any(), (tag, "inactive samples get +0")
    if "grad_logits" in out:
        g, want = _np(out["grad_logits"])[:, :B].astype(np.float64), r32["grad_logits"].astype(np.float64)
        rel, absolute = ROUNDING[dtype]
        err, bound = np.abs(g - want), tol["grad_logits"] + rel * np.abs(want) + absolute
        print(f"{tag}: grad_logits: largest |got - want| = {float(err.max()):.3e} (tolerance {tol['grad_logits']:.3e})")
        assert np.isfinite(g).all() and (err <= bound).all(), (tag, "grad_logits", float((err - bound).max()))
        assert not _bits(out["grad_logits"][:, :B]).cpu().numpy()[~on].any(), (tag, "inactive samples get +0")
    if "stats" in out:
        s, want = out["stats"].cpu().numpy(), r32["stats"]
        assert s.dtype == np.float64 and s.shape == (6,)
        assert s[5] == want[5] == r32["cnt"], (tag, "cnt is exact")
        cnt = max(r32["cnt"], 1)
        for q, name in enumerate(STAT_NAMES):
            dev, bound = abs(s[q] - want[q]), tol["stat_" + name] * cnt + H.summation_slack(r32["per"][name][on])
            assert dev <= bound, (tag, "stats", name, dev, bound)


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bins", BINS, ids=lambda b: f"B{b[0]}")
def test_parity_with_the_restatement(sim, bins, dtype, masked):
    import torch
    for n in SIZES:
        case = (n, bins, dtype, masked)
        x = H.inputs(*case)
        r32, _ = H.both(case)
        d = _dev(x, dtype)
        out = _call(sim, d)
        assert set(out) == {"value", "grad_logits", "stats", "coefficients"}
        assert out["value"].dtype == out["grad_logits"].dtype == getattr(torch, dtype) and out["value"].shape == (n,)
        _check(out, x, r32, dtype, case)
        dec = _call(sim, dict(d, returns=None), value_dtype=torch.float32)          # the rollout's decode: the same values
        assert set(dec) == {"value", "coefficients"}
        _check(dec, x, r32, "float32", (case, "decode"))
        assert torch.equal(_bits(dec["value"].to(out["value"].dtype)), _bits(out["value"]))


def test_past_the_grid_cap(sim):
    from gpu_hideseek import value_head as V
    assert BIG == V.MAX_GRID * V.ROWS_PER_BLOCK + V.ROWS_PER_BLOCK + 1
    case = CASES[-1]
    assert case[0] == BIG
    x = H.inputs(*case)
    r32, _ = H.both(case)
    _check(_call(sim, _dev(x, case[2])), x, r32, case[2], case)


def test_nan_in_inactive_samples_reaches_nothing(sim):
    import torch
    for dtype, bins in (("float32", BINS[2]), ("float16", BINS[1])):
        x = H.inputs(1806, bins, dtype, True)
        off = torch.from_numpy(x["mask"] == 0).cuda()
        assert np.isnan(x["logits"]).any() and np.isnan(x["returns"]).any()        # some are planted in the case itself
        d = _dev(x, dtype)
        clean = dict(d, logits=d["logits"].clone(), returns=d["returns"].clone())
        clean["logits"][off] = 0.5
        clean["returns"][off] = 2.0
        dirty = dict(d, logits=d["logits"].clone(), returns=d["returns"].clone())
        dirty["logits"][off] = float("nan")
        dirty["returns"][off] = float("nan")
        a, b = _call(sim, clean), _call(sim, dirty)
        for k in ("value", "grad_logits", "stats"):
            assert not torch.isnan(b[k]).any().item(), k
            assert torch.equal(_bits(a[k]), _bits(b[k])), (dtype, k)
        assert not _bits(b["value"])[off].any().item() and not _bits(b["grad_logits"])[off].any().item()


def test_strided_and_unaligned_logits_give_the_aligned_bits(sim):
    import torch
    for bins, dtype, n in ((BINS[2], "bfloat16", 1806), (BINS[2], "float32", 33), (BINS[1], "float16", 1806)):
        B = bins[0]
        x = H.inputs(n, bins, dtype, True)
        d = _dev(x, dtype)
        dt = d["logits"].dtype
        assert d["logits"].data_ptr() % 16 == 0
        ref = _call(sim, d)
        # strided: rows of W = 264 elements, NaN in the padding of the logits and of a preallocated gradient
        wide = torch.full((n, STRIDED), float("nan"), dtype=dt, device="cuda")
        wide[:, :B] = d["logits"]
        gwide = torch.full((n, STRIDED), float("nan"), dtype=dt, device="cuda")
        out = _call(sim, dict(d, logits=wide[:, :B]), grad_logits=gwide[:, :B])
        for k in ("value", "grad_logits", "stats"):
            assert torch.equal(_bits(out[k]), _bits(ref[k])), (bins, dtype, "strided", k)
        assert torch.isnan(gwide[:, B:]).all().item(), "the padding of a strided gradient is not written"
        auto = _call(sim, dict(d, logits=wide[:, :B]))                              # an allocated gradient is as wide, its padding 0
        assert auto["grad_logits"].shape == (n, B) and torch.equal(_bits(auto["grad_logits"]), _bits(ref["grad_logits"]))
        # a base offset by one row: with B = 255 of 2 bytes that is 510 bytes, not a multiple of 16
        flat = torch.zeros((n + 1) * B, dtype=dt, device="cuda")
        gflat = torch.full(((n + 1) * B,), -7.0, dtype=dt, device="cuda")
        lg, gl = flat[B:].view(n, B), gflat[B:].view(n, B)
        lg.copy_(d["logits"])
        assert B % 8 == 0 or lg.data_ptr() % 16 != 0
        out = _call(sim, dict(d, logits=lg), grad_logits=gl)
        for k in ("value", "grad_logits", "stats"):
            assert torch.equal(_bits(out[k]), _bits(ref[k])), (bins, dtype, "offset by a row", k)
        assert bool((gflat[:B] == -7).all())


def test_determinism_position_and_unrequested_outputs(sim):
    import torch
    n, bins = 1806, BINS[2]
    B = bins[0]
    x = H.inputs(n, bins, "bfloat16", True)
    d = _dev(x, "bfloat16")
    first, again = _call(sim, d), _call(sim, d)
    for k in ("value", "grad_logits", "stats"):
        assert torch.equal(_bits(first[k]), _bits(again[k])), k
    perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
    moved = _call(sim, dict(d, logits=d["logits"][perm].contiguous(), returns=d["returns"][perm].contiguous(), mask=d["mask"][perm].contiguous()))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n, device="cuda")
    for k in ("value", "grad_logits"):
        assert torch.equal(_bits(moved[k][inv]), _bits(first[k])), k
    assert moved["stats"][5].item() == first["stats"][5].item()
    # the same value bits for a sample at another position of a batch of another size (the decode has no count in it)
    sub = torch.arange(40, 40 + 77, device="cuda")
    small = _call(sim, dict(d, logits=d["logits"][sub].contiguous(), returns=None, mask=d["mask"][sub].contiguous()))
    assert torch.equal(_bits(small["value"]), _bits(first["value"][sub]))
    # only what is requested is written
    val = torch.full((n + 2,), -7.0, dtype=torch.bfloat16, device="cuda")
    gl = torch.full((n + 2, B), -7.0, dtype=torch.bfloat16, device="cuda")
    st = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    out = _call(sim, d, value=val[1:n + 1], grad_logits=False, stats=False)
    assert set(out) == {"value", "coefficients"} and bool((gl == -7).all()) and bool((st == -7).all())
    assert torch.equal(_bits(val[1:n + 1]), _bits(first["value"])) and bool((val[[0, n + 1]] == -7).all())
    val.fill_(-7)
    out = _call(sim, d, value=None, grad_logits=gl[1:n + 1], stats=False)
    assert set(out) == {"grad_logits", "coefficients"} and bool((val == -7).all()) and bool((st == -7).all())
    assert torch.equal(_bits(gl[1:n + 1]), _bits(first["grad_logits"])) and bool((gl[[0, n + 1]] == -7).all())
    gl.fill_(-7)
    out = _call(sim, d, value=None, grad_logits=False, stats=st[1:7])
    assert set(out) == {"stats", "coefficients"} and bool((val == -7).all()) and bool((gl == -7).all())
    assert torch.equal(_bits(st[1:7]), _bits(first["stats"])) and st[0].item() == -7 and st[7].item() == -7


def test_decode_into_a_rollout_buffer_of_a_live_simulator():
    import torch
    worlds, agents, T = 6, 6, 5
    s = _sim(worlds, agents, seed=3)
    s.init()
    rows = worlds * agents
    g = torch.Generator(device="cuda").manual_seed(1)
    Wc = torch.randn(296, 255, device="cuda", generator=g) * 0.2
    obs = torch.empty(rows, 296, device="cuda")
    values = torch.full((T, rows), -7.0, dtype=torch.bfloat16, device="cuda")
    rew, done = torch.empty(T, rows, device="cuda"), torch.empty(T, rows, dtype=torch.int32, device="cuda")
    tol = H.tolerances(rows)
    for t in range(T):
        s.pack_policy_inputs(actor=obs)
        logits = (obs @ Wc).to(torch.bfloat16)
        out = s.value_head(logits, value=values[t])
        assert set(out) == {"value", "coefficients"} and out["value"].data_ptr() == values[t].data_ptr()
        want = twohot(np.float32, dict(logits=logits.float().cpu().numpy(), lo=-20.0, hi=20.0, returns=None, mask=None))["value"]
        got = values[t].float().cpu().numpy().astype(np.float64)
        assert (np.abs(got - want) <= H.value_bound(want, tol["y"], "bfloat16")).all(), t
        assert bool((values[t + 1:] == -7).all())
        s.step()
        rew[t].copy_(s.reward_tensor().to_torch().reshape(rows))
        done[t].copy_(s.done_tensor().to_torch().reshape(rows))
    assert values.float().abs().max().item() > 0
    gae = s.compute_advantages(rew, done, values, values[-1].clone())             # the buffer is what compute_advantages takes
    assert gae["advantages"].shape == (T, rows) and torch.isfinite(gae["returns"]).all().item()
    s.close()


def test_coefficients_and_the_count_scale_the_gradient(sim):
    import torch
    n, bins = 1806, BINS[2]
    x = H.inputs(n, bins, "float32", True)
    d = _dev(x)
    none = _call(sim, d, mask=torch.zeros(n, device="cuda"))
    for k in ("value", "grad_logits", "stats"):
        assert not _bits(none[k]).any().item(), k
    one = _call(sim, d)
    two = _call(sim, d, grad_scale=2.0)
    half = _call(sim, d, loss_coef=0.5)
    assert torch.equal(_bits(two["grad_logits"]), _bits(2 * one["grad_logits"]))
    assert torch.equal(_bits(half["grad_logits"]), _bits(0.5 * one["grad_logits"]))
    for o in (two, half):
        assert torch.equal(_bits(o["stats"]), _bits(one["stats"])) and torch.equal(_bits(o["value"]), _bits(one["value"]))
    # without the mask the count is n: on the samples active under the mask the gradient is cnt / n of the masked one
    every = dict(d, mask=None, logits=torch.nan_to_num(d["logits"]), returns=torch.nan_to_num(d["returns"]))
    full = _call(sim, every)
    on = torch.from_numpy(x["mask"] != 0).cuda()
    cnt = int(on.sum())
    assert full["stats"][5].item() == n and one["stats"][5].item() == cnt
    ratio = full["grad_logits"][on].double() * n - one["grad_logits"][on].double() * cnt
    assert ratio.abs().max().item() <= 2.0 ** -22 * (1 + 2.0 ** -20)     # |p - t| <= 1; w and the product round once on each side
    r32 = twohot(np.float32, x, loss_coef=0.5, grad_scale=2.0)
    both = _call(sim, d, loss_coef=0.5, grad_scale=2.0)
    _check(both, x, r32, "float32", "coefficients")


def test_adds_to_the_gradient_of_the_textbook_total_loss(sim):
    """ppo_loss without a value term and value_head under the same mask: their gradients are those of
    policy loss - entropy_coef entropy + value_coef cross-entropy, by torch autograd in float64."""
    import torch
    import test_ppo_loss_host as P
    from gpu_hideseek import value_head as V
    n, buckets, bins = 1806, P.BUCKETS[0], BINS[2]
    px = P.inputs(n, buckets, "float32", True, "none")
    vx = dict(H.inputs(n, bins, "float32", False), mask=px["mask"])
    mask = torch.from_numpy(np.array(px["mask"])).cuda()
    pd = {k: torch.from_numpy(np.array(px[k])).cuda() for k in ("logits", "action", "old_log_prob", "advantage")}
    pol = sim.ppo_loss(pd["logits"], pd["action"], pd["old_log_prob"], pd["advantage"], buckets=buckets, mask=mask)
    val = _call(sim, dict(_dev(vx), mask=mask), loss_coef=P.VALUE_COEF)
    assert pol["stats"][6].item() == val["stats"][5].item()
    # float64 autograd of the total: the two networks' logits are separate leaves, so the policy terms give d / d logits
    # (over the live buckets, as the kernel defines it) and value_coef x the masked mean cross-entropy d / d critic logits
    pol64 = torch.from_numpy(P.autograd64(px, live_only=True)[0])
    m64 = torch.from_numpy((px["mask"] != 0).astype(np.float64))
    lc = torch.tensor(np.asarray(vx["logits"], np.float64), requires_grad=True)
    ce = -(V.twohot(torch.tensor(np.asarray(vx["returns"], np.float64)), *bins) * torch.log_softmax(lc, dim=1)).sum(1)
    (float(f32(P.VALUE_COEF)) * (ce * m64).sum() / m64.sum()).backward()
    ptol, vtol = P.tolerances(n), H.tolerances(n)
    ne = P.near_edge(P.ppo(np.float64, px), ptol)
    assert ne.sum() <= P.NEAR_EDGE_CAP * n
    assert float((pol["grad_logits"].double().cpu() - pol64).abs()[~ne].max()) <= ptol["grad_logits"]
    assert float((val["grad_logits"].double().cpu() - lc.grad).abs().max()) <= vtol["grad_logits"]
    fused = V.stats_to_metrics(val["stats"])["value_loss"].item()
    assert abs(fused - float((ce.detach() * m64).sum() / m64.sum())) <= vtol["stat_ce"]


def test_the_autograd_face(sim):
    import torch
    from gpu_hideseek import value_head as V
    n, bins = 1806, BINS[2]
    x = H.inputs(n, bins, "float32", True)
    d = _dev(x)
    torch.manual_seed(0)
    feat = torch.randn(n, 16, device="cuda")
    critic = torch.nn.Linear(16, 255).cuda()
    params = list(critic.parameters())

    def forward():
        for q in params:
            q.grad = None
        return critic(feat)

    logits = forward()
    out = sim.value_head(logits.detach(), d["returns"], mask=d["mask"], loss_coef=0.5)
    loss = V.attach(logits, out)
    assert loss.dtype == torch.float64 and loss.shape == ()
    assert loss.item() == 0.5 * V.stats_to_metrics(out["stats"])["value_loss"].item()
    loss.backward()
    fused = [q.grad.clone() for q in params]
    logits = forward()
    torch.autograd.backward([logits], [out["grad_logits"]])
    for a, b in zip(fused, params):
        assert torch.equal(a, b.grad)                       # the path with no extra op hands on the same gradient
    logits = forward()
    on = d["mask"] != 0
    eager = 0.5 * V.eager_loss(logits[on], d["returns"][on], None, *bins)
    eager.backward()
    tol = H.tolerances(n)
    assert abs(eager.item() - loss.item()) <= 2 * tol["stat_ce"]
    # a parameter gradient is a sum over the rows of (output gradient x feature); every output gradient is within the
    # gradient tolerance of the exact one on both sides
    colsum = float(feat.abs().sum(0).max())
    for a, b, bound in zip(fused, params, (2 * tol["grad_logits"] * colsum, 2 * tol["grad_logits"] * n)):
        err, size = float((a - b.grad).abs().max()), float(b.grad.abs().max())
        print(f"parameter {tuple(a.shape)}: |fused - eager| = {err:.3e} (bound {bound:.3e}, largest gradient {size:.3e})")
        assert err <= bound and 10 * bound < size


def test_the_stream_form_and_the_shards(sim):
    import gpu_hideseek
    import torch
    n, bins = 1806, BINS[2]
    x = H.inputs(n, bins, "bfloat16", True)
    d = _dev(x, "bfloat16")
    blocking = _call(sim, d)
    side = torch.cuda.Stream()
    ev = torch.cuda.Event()
    ev.record()
    side.wait_event(ev)
    got = _call(sim, d, stream=side)
    done = torch.cuda.Event()
    done.record(side)
    raw = _call(sim, d, stream=side.cuda_stream)
    torch.cuda.current_stream().wait_event(done)
    first = {k: got[k].clone() for k in ("value", "grad_logits", "stats")}        # ordered after the first call by the event
    side.synchronize()
    for k in ("value", "grad_logits", "stats"):
        assert torch.equal(_bits(first[k]), _bits(blocking[k])) and torch.equal(_bits(raw[k]), _bits(blocking[k])), k
    kw = dict(sim_flags=0, rand_seed=0, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0], 6, **kw)
    ss.init()
    cut = 1000
    halves = [{k: (v[:cut] if isinstance(v, torch.Tensor) else v) for k, v in d.items()},
              {k: (v[cut:] if isinstance(v, torch.Tensor) else v) for k, v in d.items()}]
    singles = [_call(sim, h) for h in halves]
    res = ss.value_head([h["logits"] for h in halves], [h["returns"] for h in halves], mask=[h["mask"] for h in halves],
                        bins=bins[0], lo=bins[1], hi=bins[2])
    assert len(res) == 2
    for r, one in zip(res, singles):
        for k in ("value", "grad_logits", "stats"):
            assert torch.equal(_bits(r[k]), _bits(one[k])), k
    dec = ss.value_head([h["logits"] for h in halves], mask=[h["mask"] for h in halves])
    for r, one in zip(dec, singles):
        assert set(r) == {"value", "coefficients"} and torch.equal(_bits(r["value"]), _bits(one["value"]))
    ss.close()


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import value_head as V
    INVALID = 1
    n, bins = 48, BINS[2]
    B = bins[0]
    x = H.inputs(n, bins, "float32", True, seed=23)
    pad = 8

    def buf(a, dtype=None):
        t = torch.zeros(a.size + pad, dtype=dtype or torch.from_numpy(np.array(a)).dtype, device="cuda")
        t[:a.size] = torch.from_numpy(np.array(a)).reshape(-1).to(t.dtype)
        return t
    lg, ret, msk = buf(x["logits"]), buf(x["returns"]), buf(x["mask"])
    lgh = torch.zeros(n * B + pad, dtype=torch.bfloat16, device="cuda")
    val = torch.full((n + pad,), -7.0, device="cuda")
    valh = torch.full((n + pad,), -7.0, dtype=torch.float16, device="cuda")
    gl = torch.full((n * B + pad,), -7.0, device="cuda")
    st = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    ins = (lg, ret, msk)
    saved = [t.clone() for t in ins]

    def req(logits=lg.data_ptr(), returns=ret.data_ptr(), mask=msk.data_ptr(), n=n, ldt=1, lstride=B, bins=B, lo=bins[1], hi=bins[2], coef=1.0,
            scale=1.0, vdt=1, gdt=1, gstride=B, value=val.data_ptr(), grad_logits=gl.data_ptr(), stats=st.data_ptr()):
        return V.HsTwohotRequest(logits, returns, mask, n, ldt, lstride, bins, lo, hi, coef, scale, vdt, gdt, gstride, 0, value, grad_logits, stats)

    def untouched():
        torch.cuda.synchronize()
        same = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ins, saved))
        return same and all(bool((t == -7).all()) for t in (val, valh, gl, st))

    def call(s, r, stream=False):
        p = C.byref(r) if r is not None else None
        if stream:
            return s._L.hs_twohot_value_async(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p)
        return s._L.hs_twohot_value(s._h, p)

    def message(s):
        return s._L.hs_last_error().decode()

    s = _sim(4, 4)
    for stream in (False, True):
        assert call(s, req(), stream) == INVALID and "before hs_init" in message(s)
    assert untouched()
    s.init()
    nan, inf = float("nan"), float("inf")
    bad = {
        "null request": (None, "null request"), "null logits": (req(logits=None), "null logits"),
        "no output": (req(value=None, grad_logits=None, stats=None), "every output is null"),
        "gradient without returns": (req(returns=None, stats=None), "without returns"),
        "stats without returns": (req(returns=None, grad_logits=None), "without returns"),
        "logits dtype": (req(ldt=0), "dtype"), "value dtype": (req(vdt=2), "dtype"), "grad dtype": (req(gdt=7), "dtype"),
        "bins 1": (req(bins=1), "bins"), "bins 0": (req(bins=0), "bins"), "bins 257": (req(bins=257, lstride=257, gstride=257), "bins"),
        "logits stride": (req(lstride=B - 1), "logits_stride"), "grad stride": (req(gstride=B - 1), "grad_stride"),
        "lo nan": (req(lo=nan), "lo and hi"), "hi inf": (req(hi=inf), "lo and hi"), "lo = hi": (req(lo=2.0, hi=2.0), "lo and hi"),
        "lo > hi": (req(lo=20.0, hi=-20.0), "lo and hi"), "coef nan": (req(coef=nan), "finite"), "scale -inf": (req(scale=-inf), "finite"),
        "n 0": (req(n=0), "n must"), "n -1": (req(n=-1), "n must"), "n x stride": (req(n=2 ** 23, lstride=256), "n must"),
        "n x grad stride": (req(n=2 ** 23, gstride=256), "n must"),
        "returns +2": (req(returns=ret.data_ptr() + 2), "aligned"), "mask +1": (req(mask=msk.data_ptr() + 1), "aligned"),
        "logits f32 +2": (req(logits=lg.data_ptr() + 2), "aligned"), "logits bf16 +1": (req(logits=lgh.data_ptr() + 1, ldt=3), "aligned"),
        "value +2": (req(value=val.data_ptr() + 2), "aligned"), "value f16 +1": (req(value=valh.data_ptr() + 1, vdt=4), "aligned"),
        "grad_logits +2": (req(grad_logits=gl.data_ptr() + 2), "aligned"), "stats +4": (req(stats=st.data_ptr() + 4), "8-byte aligned"),
        "grad_logits is logits": (req(grad_logits=lg.data_ptr()), "grad_logits overlaps logits"),
        "value is returns": (req(value=ret.data_ptr()), "value overlaps returns"),
        "value on mask": (req(value=msk.data_ptr() + 8), "value overlaps mask"),
        "grad_logits in value": (req(grad_logits=val.data_ptr() + 4, n=2), "grad_logits overlaps value"),
        "stats in grad_logits": (req(stats=gl.data_ptr() + 8), "stats overlaps grad_logits"),
        "stats in value": (req(stats=val.data_ptr() + 8), "stats overlaps value"),
    }
    for what, (r, msg) in bad.items():
        for stream in (False, True):
            assert call(s, r, stream) == INVALID, what
            assert msg in message(s), (what, message(s))
    assert untouched()
    s.step_begin()
    for stream in (False, True):
        assert call(s, req(), stream) == INVALID and "open step" in message(s)
    s.step_end()
    assert untouched()
    assert call(s, req()) == 0                                   # the call does write
    assert not untouched()
    want = twohot(np.float32, x)
    tol = H.tolerances(n)
    got = gl.cpu().numpy()[:n * B].reshape(n, B).astype(np.float64)
    assert (np.abs(got - want["grad_logits"]) <= tol["grad_logits"]).all()
    assert st[5].item() == want["cnt"] and bool((gl[n * B:] == -7).all()) and bool((val[n:] == -7).all())
    assert call(s, req(returns=None, grad_logits=None, stats=None, value=valh.data_ptr(), vdt=4)) == 0       # the decode alone
    assert bool((valh[n:] == -7).all()) and not bool((valh[:n] == -7).any())
    s.close()
