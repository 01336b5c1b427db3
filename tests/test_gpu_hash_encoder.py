"""The SimHash encoder on the GPU (sim.hash_encode / hash_encode_backward, hs_hash_encode, csrc/hs_k_hash.h) against the
numpy restatement of tests/test_hash_encoder_host.py within the bounds derived there: sizes around the rows a workgroup
takes per round and past the backward's grid cap in every dtype; the bins under the near-tie rule; crafted exact bins, the
all-zero row, the NaN and the exact zero; the features; the backward with the deepest single-bin sum, every bin once, +0
for empty bins, the projection and a zero gradient; determinism, position independence, the stream form and the shards,
bit for bit; the refusals of the C ABI; live rows of a stepped simulator, actor against critic; the module under Adam."""
import ctypes as C

import numpy as np
import pytest

import test_hash_encoder_host as H
from test_hash_encoder_host import BINS, BITS, CASES, DTYPES, FEATURES, PARAMS, PROJ, ROW, SIZES, TABLE_END

pytestmark = pytest.mark.gpu


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
    import torch
    dt = getattr(torch, dtype)
    out = dict(rows=torch.from_numpy(np.array(x["rows"])).cuda().to(dt), params=torch.from_numpy(np.array(x["params"])).cuda())
    if "grad" in x:
        out["grad"] = torch.from_numpy(np.array(x["grad"])).cuda().to(dt)
    return out


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype.is_floating_point else t.detach().cpu().numpy()


def _bits(t):
    import torch
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _check_forward(out, rows, params, dtype, tag, eps=H.EPS):
    """The bins under the near-tie rule (with its cap), the features within the derived bound of the float64 LayerNorm of
    table[device bin].  Returns the device's bins."""
    got_bin = _np(out["bin"])
    assert got_bin.dtype == np.uint8 and got_bin.shape == (len(rows),)
    H.check_bins(got_bin, rows, params, tag)
    want = H.norm_table(np.float64, params, eps)[2][got_bin]
    got = _np(out["features"]).astype(np.float64)
    err, bound = np.abs(got - want), H.feature_bound(want, dtype)
    print(f"{tag}: features: largest |got - want| = {float(err.max()):.3e} (tolerance {H.feature_tolerance():.3e})")
    assert got.shape == (len(rows), FEATURES) and np.isfinite(got).all() and (err <= bound).all(), (tag, float((err - bound).max()))
    return got_bin


def _check_backward(gp, bins, grad, params, tag, eps=H.EPS):
    """grad_params within the derived bound of the float64 restatement fed the device's bins; the projection's range and
    the table rows of bins without rows +0 by bit pattern."""
    want = H.backward(np.float64, bins, grad, params, eps)
    got = _np(gp).astype(np.float64)
    err, bound = np.abs(got - want), H.grad_bound(bins, grad, params, eps)
    f32 = H.backward(np.float32, bins, grad, params, eps)
    print(f"{tag}: grad_params: largest |got - want| = {float(err.max()):.3e} (tolerances {H.grad_tolerance(bins, grad, params, eps)}, largest gradient "
          f"{float(np.abs(want).max()):.3e}); {int((_np(gp) != f32).sum())} of {PARAMS} differ from the f32 restatement")
    assert gp.dtype.is_floating_point and gp.element_size() == 4 and gp.shape == (PARAMS,) and np.isfinite(got).all()
    assert (err <= bound).all(), (tag, float((err - bound).max()))
    raw = _bits(gp).cpu().numpy()
    empty = np.setdiff1d(np.arange(BINS), np.asarray(bins))
    assert not raw[:PROJ].any() and not raw[PROJ:TABLE_END].reshape(BINS, FEATURES)[empty].any(), (tag, "a -0 or a value where +0 belongs")


@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_with_the_restatement(sim, dtype):
    import torch
    from gpu_hideseek import hash_encoder as N
    assert SIZES == (1, N.ROWS_PER_ROUND - 1, N.ROWS_PER_ROUND, N.ROWS_PER_ROUND + 1, 257, 4099, N.MAX_GRID_BWD * N.ROWS_PER_ROUND + N.ROWS_PER_ROUND + 1)
    for n in SIZES:
        case = (n, dtype)
        assert case in CASES
        x = H.inputs(*case)
        d = _dev(x, dtype)
        out = sim.hash_encode(d["rows"], d["params"], bin=True)
        assert set(out) == {"features", "bin"} and out["features"].dtype == getattr(torch, dtype) and out["features"].shape == (n, FEATURES)
        bins = _check_forward(out, x["rows"], x["params"], dtype, case)
        res = sim.hash_encode_backward(out["bin"], d["grad"], d["params"])
        assert set(res) == {"grad_params"}
        _check_backward(res["grad_params"], bins, x["grad"], x["params"], case)


def test_exact_bins_zero_nan_and_every_bin_once(sim):
    import torch
    e = H.exact_inputs()
    for dtype in DTYPES:
        rows = H.to_dtype(np.array(e["rows"]), dtype)                     # rounding keeps every sign and the zeros
        d = _dev(dict(rows=rows, params=e["params"]), dtype)
        out = sim.hash_encode(d["rows"], d["params"], bin=True)
        got = _np(out["bin"])
        assert np.array_equal(got, e["bin"]), (dtype, np.flatnonzero(got != e["bin"]))
        assert sorted(got[:BINS]) == list(range(BINS)) and tuple(got[BINS:]) == (0, 0, 247)
        assert not H.near_ties(rows[:BINS + 1], H.parts(e["params"])[0]).any()      # no row left out
        want = H.norm_table(np.float64, e["params"])[2][e["bin"]]
        assert (np.abs(_np(out["features"]).astype(np.float64) - want) <= H.feature_bound(want, dtype)).all(), dtype
        # every bin once: 256 sums of one term
        rng = np.random.default_rng(9)
        grad = H.to_dtype(rng.standard_normal((BINS, FEATURES)).astype(np.float32), dtype)
        gp = sim.hash_encode_backward(out["bin"][:BINS].contiguous(), torch.from_numpy(grad).cuda().to(d["rows"].dtype), d["params"])["grad_params"]
        _check_backward(gp, e["bin"][:BINS], grad, e["params"], ("every bin once", dtype))


def test_the_deepest_single_bin_sum_and_zero_gradients(sim):
    import torch
    x = H.same_rows()
    n = len(x["rows"])
    d = _dev(x)
    out = sim.hash_encode(d["rows"], d["params"], bin=True)
    bins = _np(out["bin"])
    assert n == 4099 and len(set(bins)) == 1 and bins[0] == H.forward(np.float64, x["rows"][:1], x["params"])["bin"][0]
    gp = torch.full((PARAMS,), -7.0, device="cuda")
    sim.hash_encode_backward(out["bin"], d["grad"], d["params"], grad_params=gp)
    _check_backward(gp, bins, x["grad"], x["params"], "4099 identical rows")
    for dtype in DTYPES:
        xx = H.inputs(257, dtype)
        dd = _dev(xx, dtype)
        dd["params"][H.PARTS[1][1]][::2] *= -1                          # a negative scale must not turn +0 into -0
        b = sim.hash_encode(dd["rows"], dd["params"], bin=True)["bin"]
        for zero in (torch.zeros_like(dd["grad"]), -torch.zeros_like(dd["grad"])):
            gp.fill_(-7.0)
            sim.hash_encode_backward(b, zero, dd["params"], grad_params=gp)
            assert not _bits(gp).any().item(), dtype


def test_bit_for_bit(sim):
    import gpu_hideseek
    import torch
    for dtype in DTYPES:
        n = 4099 if dtype == "bfloat16" else 257
        d = _dev(H.inputs(n, dtype), dtype)
        first, again = sim.hash_encode(d["rows"], d["params"], bin=True), sim.hash_encode(d["rows"], d["params"], bin=True)
        for k in ("features", "bin"):
            assert torch.equal(_bits(first[k]), _bits(again[k])), (dtype, k)
        g1 = sim.hash_encode_backward(first["bin"], d["grad"], d["params"])["grad_params"]
        g2 = sim.hash_encode_backward(first["bin"], d["grad"], d["params"])["grad_params"]
        assert torch.equal(_bits(g1), _bits(g2)), dtype
        # a row at another index of a batch of another size
        perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
        moved = sim.hash_encode(d["rows"][perm].contiguous(), d["params"], bin=True)
        for k in ("features", "bin"):
            assert torch.equal(_bits(moved[k]), _bits(first[k][perm])), (dtype, k)
        for cut in (slice(3, 4), slice(8, 19), slice(1, 256)):
            sub = sim.hash_encode(d["rows"][cut].contiguous(), d["params"], bin=True)
            for k in ("features", "bin"):
                assert torch.equal(_bits(sub[k]), _bits(first[k][cut])), (dtype, k, cut)
        # the element type of the rows does not matter either: the same values as float32 give the same bins
        wide = sim.hash_encode(d["rows"].float(), d["params"], bin=True, dtype=d["rows"].dtype)
        for k in ("features", "bin"):
            assert torch.equal(_bits(wide[k]), _bits(first[k])), (dtype, k, "as float32")
        assert set(sim.hash_encode(d["rows"], d["params"])) == {"features"}
        # the stream form
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        got = sim.hash_encode(d["rows"], d["params"], bin=True, stream=side)
        gs = sim.hash_encode_backward(got["bin"], d["grad"], d["params"], stream=side.cuda_stream)["grad_params"]
        side.synchronize()
        for k in ("features", "bin"):
            assert torch.equal(_bits(got[k]), _bits(first[k])), (dtype, k, "stream")
        assert torch.equal(_bits(gs), _bits(g1))
    # the shards [0, 0]: each the call on its own piece
    kw = dict(sim_flags=0, rand_seed=0, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0], 6, **kw)
    ss.init()
    cuts = [slice(0, 104), slice(104, n)]
    parts = [d["rows"][c].contiguous() for c in cuts]
    res = ss.hash_encode(parts, d["params"], bin=True)
    assert len(res) == 2
    for r, c in zip(res, cuts):
        for k in ("features", "bin"):
            assert torch.equal(_bits(r[k]), _bits(first[k][c])), k
    back = ss.hash_encode_backward([r["bin"] for r in res], [d["grad"][c].contiguous() for c in cuts], [d["params"]] * 2)
    for b, c in zip(back, cuts):
        one = sim.hash_encode_backward(first["bin"][c].contiguous(), d["grad"][c].contiguous(), d["params"])["grad_params"]
        assert torch.equal(_bits(b["grad_params"]), _bits(one))
    ss.close()
    # another eps: within the bounds of its own restatement
    x = H.inputs(257, "float32")
    d = _dev(x)
    out = sim.hash_encode(d["rows"], d["params"], bin=True, eps=1e-3)
    want = H.norm_table(np.float64, x["params"], 1e-3)[2][_np(out["bin"])]
    assert (np.abs(_np(out["features"]) - want) <= H.feature_bound(want, "float32")).all()
    assert not torch.equal(out["features"], sim.hash_encode(d["rows"], d["params"])["features"])
    _check_backward(sim.hash_encode_backward(out["bin"], d["grad"], d["params"], eps=1e-3)["grad_params"], _np(out["bin"]), x["grad"], x["params"], "eps", 1e-3)


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import hash_encoder as N
    INVALID = 1
    n = 9
    x = H.inputs(n, "float32")
    pad = 16
    rows = torch.zeros(n * ROW + pad, device="cuda")
    rows[:n * ROW] = torch.from_numpy(np.array(x["rows"])).reshape(-1)
    params = torch.zeros(PARAMS + pad, device="cuda")
    params[:PARAMS] = torch.from_numpy(np.array(x["params"]))
    grad = torch.zeros(n * FEATURES + pad, device="cuda")
    grad[:n * FEATURES] = torch.from_numpy(np.array(x["grad"])).reshape(-1)
    feat = torch.full((n * FEATURES + pad,), -7.0, device="cuda")
    feat_h = torch.full((n * FEATURES + pad,), -7.0, dtype=torch.float16, device="cuda")
    bins = torch.full((n + pad,), 77, dtype=torch.uint8, device="cuda")
    gp = torch.full((PARAMS + pad,), -7.0, device="cuda")
    ins = (rows, params, grad)
    saved = [t.clone() for t in ins]
    assert rows.data_ptr() % 16 == 0

    def fwd(rows=rows.data_ptr(), params=params.data_ptr(), n=n, rdt=1, fdt=1, eps=1e-6, features=feat.data_ptr(), bin=bins.data_ptr()):
        return N.HsHashEncodeRequest(rows, params, n, rdt, fdt, eps, features, bin)

    def bwd(bin=bins.data_ptr(), grad_features=grad.data_ptr(), params=params.data_ptr(), n=n, gdt=1, eps=1e-6, grad_params=gp.data_ptr()):
        return N.HsHashEncodeBackwardRequest(bin, grad_features, params, n, gdt, eps, 0, grad_params)

    def untouched():
        torch.cuda.synchronize()
        same = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ins, saved))
        return same and all(bool((t == -7).all()) for t in (feat, feat_h, gp)) and bool((bins == 77).all())

    def call(s, r, stream=False):
        fn = "hs_hash_encode_backward" if isinstance(r, N.HsHashEncodeBackwardRequest) else "hs_hash_encode"
        if stream:
            return getattr(s._L, fn + "_async")(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(r))
        return getattr(s._L, fn)(s._h, C.byref(r))

    def message(s):
        return s._L.hs_last_error().decode()

    s = _sim(4, 4)
    for r in (fwd(), bwd()):
        for stream in (False, True):
            assert call(s, r, stream) == INVALID and "before hs_init" in message(s)
    assert untouched()
    s.init()
    for fn in ("hs_hash_encode", "hs_hash_encode_backward"):
        assert getattr(s._L, fn)(s._h, None) == INVALID and "null request" in message(s)
        assert getattr(s._L, fn + "_async")(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), None) == INVALID and "null request" in message(s)
    nan, inf = float("nan"), float("inf")
    bad = {}
    for name, make in (("forward", fwd), ("backward", bwd)):
        bad.update({
            (name, "null params"): (make(params=None), "null params"), (name, "n 0"): (make(n=0), "n must"), (name, "n -1"): (make(n=-1), "n must"),
            (name, "n x 296"): (make(n=2 ** 23), "n must"), (name, "eps nan"): (make(eps=nan), "eps must"), (name, "eps 0"): (make(eps=0.0), "eps must"),
            (name, "eps < 0"): (make(eps=-1e-6), "eps must"), (name, "eps inf"): (make(eps=inf), "eps must"),
            (name, "params +2"): (make(params=params.data_ptr() + 2), "4-byte aligned"),
        })
    bad.update({
        "null rows": (fwd(rows=None), "null rows"), "null features": (fwd(features=None), "null features"), "rows dtype": (fwd(rdt=2), "dtype"),
        "features dtype": (fwd(fdt=0), "dtype"), "rows +4": (fwd(rows=rows.data_ptr() + 4), "16-byte aligned"),
        "rows +8 bf16": (fwd(rows=rows.data_ptr() + 8, rdt=3), "16-byte aligned"),
        "features +2": (fwd(features=feat.data_ptr() + 2), "aligned"), "features f16 +1": (fwd(features=feat_h.data_ptr() + 1, fdt=4), "aligned"),
        "features is rows": (fwd(features=rows.data_ptr()), "features overlaps rows"),
        "features in params": (fwd(features=params.data_ptr() + 64), "features overlaps params"),
        "bin in rows": (fwd(bin=rows.data_ptr() + 3), "bin overlaps rows"), "bin in features": (fwd(bin=feat.data_ptr() + 5), "bin overlaps features"),
        "null bin": (bwd(bin=None), "null bin"), "null grad_features": (bwd(grad_features=None), "null grad_features"),
        "null grad_params": (bwd(grad_params=None), "null grad_params"), "grad dtype": (bwd(gdt=9), "dtype"),
        "grad_features +2": (bwd(grad_features=grad.data_ptr() + 2), "aligned"), "grad_params +1": (bwd(grad_params=gp.data_ptr() + 1), "4-byte aligned"),
        "grad_params is params": (bwd(grad_params=params.data_ptr()), "grad_params overlaps params"),
        "grad_params in grad_features": (bwd(grad_params=grad.data_ptr() + 4), "grad_params overlaps"),
        "grad_params on bin": (bwd(grad_params=bins.data_ptr()), "grad_params overlaps"),
    })
    for what, (r, msg) in bad.items():
        for stream in (False, True):
            assert call(s, r, stream) == INVALID, what
            assert msg in message(s), (what, message(s))
    assert untouched()
    s.step_begin()
    for r in (fwd(), bwd()):
        for stream in (False, True):
            assert call(s, r, stream) == INVALID and "open step" in message(s)
    s.step_end()
    assert untouched()
    assert call(s, fwd()) == 0                                   # the calls do write, and only their own ranges
    assert not untouched() and bool((feat[n * FEATURES:] == -7).all()) and bool((bins[n:] == 77).all())
    got = _check_forward(dict(features=feat[:n * FEATURES].view(n, FEATURES), bin=bins[:n]), x["rows"], x["params"], "float32", "C ABI")
    assert call(s, bwd()) == 0
    torch.cuda.synchronize()
    assert bool((gp[PARAMS:] == -7).all()) and not bool((gp[:PARAMS] == -7).any())
    _check_backward(gp[:PARAMS], got, x["grad"], x["params"], "C ABI")
    assert call(s, fwd(features=feat_h.data_ptr(), fdt=4, bin=None)) == 0
    assert bool((feat_h[n * FEATURES:] == -7).all()) and not bool((feat_h[:n * FEATURES] == -7).any())
    s.close()


def test_live_rows_actor_and_critic():
    import torch
    worlds, agents, T = 6, 6, 3
    s = _sim(worlds, agents, seed=3)
    s.init()
    rows = worlds * agents
    params = H.inputs(rows, "float32")["params"]
    dparams = torch.from_numpy(np.array(params)).cuda()
    differ = 0
    for dtype in (torch.float32, torch.bfloat16):
        actor, critic = torch.empty(rows, ROW, device="cuda", dtype=dtype), torch.empty(rows, ROW, device="cuda", dtype=dtype)
        buf = torch.full((T, 2, rows, FEATURES), -7.0, device="cuda", dtype=dtype)
        for t in range(T):
            for _ in range(4):
                s.step()
            s.pack_policy_inputs(actor=actor, critic=critic)
            got = []
            for i, r in enumerate((actor, critic)):
                out = s.hash_encode(r, dparams, features=buf[t, i], bin=True)
                assert out["features"].data_ptr() == buf[t, i].data_ptr()
                got.append(_check_forward(out, _np(r), params, str(dtype).replace("torch.", ""), ("live", dtype, t, i)))
            assert bool((buf[t + 1:] == -7).all())
            differ += int((got[0] != got[1]).sum())
    assert differ > 0, "the actor's masked rows and the critic's rows never fell into different bins"
    s.close()


def test_the_module_under_adam(sim):
    """HashEncoder under optim.Adam, three steps: the rows of visited bins move, the rows of unvisited bins and the
    projection keep their bits."""
    import torch
    from gpu_hideseek import hash_encoder as N
    from gpu_hideseek import optim
    n = 257
    x = H.inputs(n, "float32")
    enc = N.HashEncoder().cuda()
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(np.array(x["params"])))
    opt = optim.Adam(sim, enc.named_parameters(), lr=1e-2)
    rows, w = torch.from_numpy(np.array(x["rows"])).cuda(), torch.from_numpy(np.array(x["grad"])).cuda()
    before = enc.params.detach().clone()
    visited = np.unique(_np(sim.hash_encode(rows, enc.params.detach(), bin=True)["bin"]))
    assert 100 < len(visited) < BINS
    for step in range(3):
        opt.zero_grad()
        feats = enc(sim, rows)
        assert feats.requires_grad and feats.shape == (n, FEATURES)
        ((feats * w).sum() + 0.5 * (feats ** 2).mean()).backward()
        g = N.views(enc.params.grad)
        assert not _bits(g["proj"]).any().item() and g["table"].any().item()
        opt.step()
    a, b = N.views(enc.params.detach()), N.views(before)
    assert torch.equal(_bits(a["proj"]), _bits(b["proj"]))
    moved = (a["table"] != b["table"]).any(1).cpu().numpy()
    assert moved[visited].all() and not moved[np.setdiff1d(np.arange(BINS), visited)].any()
    unvisited = torch.from_numpy(np.setdiff1d(np.arange(BINS), visited)).cuda()
    assert torch.equal(_bits(a["table"][unvisited]), _bits(b["table"][unvisited]))
    assert (a["scale"] != b["scale"]).any().item() and (a["shift"] != b["shift"]).any().item() and torch.isfinite(enc.params).all().item()
    assert BITS == 8
