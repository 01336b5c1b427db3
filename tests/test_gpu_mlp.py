"""The dense layer after its GEMM on the GPU (sim.dense_norm_act / dense_norm_act_backward, hs_dense_norm_act,
csrc/hs_k_dense.h) against the numpy restatement of tests/test_mlp_host.py within the tolerances derived there: one row,
a partial round, one row past a round, past the backward's sweep and (forward only) past the forward's; every channel
count and dtype; the f32 y bit for bit; determinism, position independence, exact zeros for a zero gradient, a constant
row, dead channels, other slopes and another eps; only the requested outputs; the stream form and the shards; the
refusals of the C ABI; and the torch modules against their eager form under autograd."""
import ctypes as C

import numpy as np
import pytest

import test_mlp_host as H
from test_mlp_host import BIG_FWD, CHANNELS, DTYPES, PARAM_ROWS, SIZES

pytestmark = pytest.mark.gpu


def _sim(worlds=6, agents=6, seed=0):
    import gpu_hideseek
    k = agents // 2
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=0, rand_seed=seed,
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
    t = {k: torch.from_numpy(np.array(v)).cuda() for k, v in x.items()}
    for k in ("z", "grad_y"):
        t[k] = t[k].to(dt)
    return t


def _np(t):
    return t.detach().float().cpu().numpy()


def _bits(t):
    import torch
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _fwd(sim, d, **kw):
    return sim.dense_norm_act(d["z"], d["params"], **kw)


def _bwd(sim, d, **kw):
    return sim.dense_norm_act_backward(d["z"], d["params"], d["grad_y"], **kw)


def _check(got, want, names, case, tag, tol=None):
    """Every output within its derived bound of the f32 restatement (want: H.run(np.float32, ...))."""
    for k in names:
        g, w = _np(got[k]).astype(np.float64), want[k].astype(np.float64)
        err, limit = np.abs(g - w), H.bound(k, w, case, tol)
        print(f"{tag}: {k}: largest |got - want| = {float(err.max()):.3e}, largest excess over the bound {float((err - limit).max()):.3e}, "
              f"{int((g != w).sum())} of {g.size} differ")
        assert g.shape == w.shape and np.isfinite(g).all() and (err <= limit).all(), (tag, k, float((err - limit).max()))


def _same_f32(got, want, tag):
    """No expf or tanhf is involved: the f32 y is the restatement's bit for bit."""
    g, w = got.detach().cpu().numpy(), np.asarray(want)
    assert g.dtype == w.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32)), (tag, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("channels", CHANNELS)
def test_parity_with_the_restatement(sim, channels, dtype):
    import torch
    for n in SIZES:
        case = (n, channels, dtype)
        d = _dev(H.inputs(*case), dtype)
        want = H.both(case)[0]
        out = _fwd(sim, d)
        assert set(out) == {"y"} and out["y"].dtype == getattr(torch, dtype) and out["y"].shape == (n, channels)
        _check(out, want, ("y",), case, case)
        if dtype == "float32":
            _same_f32(out["y"], want["y"], case)
        else:                                                                   # a narrow z with an f32 y: the same bits again
            _same_f32(_fwd(sim, d, y_dtype=torch.float32)["y"], want["y"], case)
        res = _bwd(sim, d)
        assert set(res) == {"grad_z", "grad_params"} and res["grad_z"].dtype == getattr(torch, dtype) and res["grad_params"].shape == (PARAM_ROWS * channels,)
        _check(res, want, ("grad_z", "grad_params"), case, case)


def test_past_the_forward_sweep(sim):
    n, channels, dtype = BIG_FWD
    x = H.inputs(*BIG_FWD)
    want = H.forward(np.float32, x["z"], x["params"], channels)
    out = _fwd(sim, _dev(x, dtype))
    _check(out, want, ("y",), BIG_FWD, BIG_FWD)
    _same_f32(out["y"], want["y"], BIG_FWD)


def test_determinism_and_position(sim):
    import torch
    for channels, dtype, n in ((64, "float32", 14), (128, "bfloat16", 14), (256, "bfloat16", 2051), (512, "float16", 14)):
        d = _dev(H.inputs(n, channels, dtype), dtype)
        first, again = _fwd(sim, d), _fwd(sim, d)
        assert torch.equal(_bits(first["y"]), _bits(again["y"])), (channels, dtype)
        g1, g2 = _bwd(sim, d), _bwd(sim, d)
        for k in ("grad_z", "grad_params"):
            assert torch.equal(_bits(g1[k]), _bits(g2[k])), (channels, dtype, k)
        # a row at another index of a batch of another size: the same y and the same grad_z
        perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
        moved = {k: (v[perm].contiguous() if k != "params" else v) for k, v in d.items()}
        assert torch.equal(_bits(_fwd(sim, moved)["y"]), _bits(first["y"][perm])), (channels, dtype)
        assert torch.equal(_bits(_bwd(sim, moved, grad_params=None)["grad_z"]), _bits(g1["grad_z"][perm])), (channels, dtype)
        sub = {k: (v[4:7].contiguous() if k != "params" else v) for k, v in d.items()}
        assert torch.equal(_bits(_fwd(sim, sub)["y"]), _bits(first["y"][4:7]))
        assert torch.equal(_bits(_bwd(sim, sub)["grad_z"]), _bits(g1["grad_z"][4:7]))


def test_zero_gradients_constant_rows_and_dead_channels(sim):
    import torch
    for channels, dtype in ((64, "float32"), (256, "bfloat16"), (512, "float16")):
        n = 14
        x = H.inputs(n, channels, dtype)
        d = _dev(x, dtype)
        # an all-zero grad_y: grad_params all +0, grad_z zero
        gp = torch.full((PARAM_ROWS * channels,), -7.0, device="cuda")
        res = _bwd(sim, dict(d, grad_y=torch.zeros_like(d["grad_y"])), grad_params=gp)
        assert not _bits(gp).any().item() and not (res["grad_z"] != 0).any().item(), (channels, dtype)
        # a constant row (var = 0): exactly leaky(beta), and finite gradients
        z = np.array(x["z"])
        z[2] = 1.5
        p = np.array(x["params"])
        p[:channels] = 0.25
        c = _dev(dict(x, z=z, params=p), dtype)
        beta = p[2 * channels:]
        y = _fwd(sim, c, y_dtype=torch.float32)["y"]
        _same_f32(y[2], np.where(beta > 0, beta, np.float32(H.SLOPE) * beta), (channels, dtype, "constant row"))
        back = _bwd(sim, c)
        assert torch.isfinite(back["grad_z"].float()).all().item() and torch.isfinite(back["grad_params"]).all().item()
        want = H.run(np.float32, dict(x, z=z, params=p), channels)
        tol = {k: 4.0 * v for k, v in H.gaps(want, H.run(np.float64, dict(x, z=z, params=p), channels), channels).items()}
        _check(back, want, ("grad_z", "grad_params"), (n, channels, dtype), (channels, dtype, "constant row"), tol)
        # channels with gamma = beta = 0: +0, in the first and in the last lane's piece
        p = np.array(x["params"])
        dead = [1, channels - 1]
        for ch in dead:
            p[channels + ch] = p[2 * channels + ch] = 0.0
        y = _fwd(sim, _dev(dict(x, params=p), dtype))["y"]
        assert not _bits(y)[:, dead].any().item() and bool((y != 0).any())


def test_other_slopes_and_another_eps(sim):
    import torch
    channels, dtype, n = 256, "bfloat16", 14
    x = H.inputs(n, channels, dtype)
    d = _dev(x, dtype)
    base = _fwd(sim, d)["y"]
    for kw in (dict(slope=0.0), dict(slope=0.2), dict(slope=1.0), dict(eps=1e-2), dict(eps=1e-3, slope=0.5)):
        r32, r64 = H.run(np.float32, x, channels, **kw), H.run(np.float64, x, channels, **kw)
        tol = {k: 4.0 * v for k, v in H.gaps(r32, r64, channels).items()}
        out = _fwd(sim, d, **kw)
        assert not torch.equal(_bits(out["y"]), _bits(base)), kw
        _check(out, r32, ("y",), (n, channels, dtype), kw, tol)
        _same_f32(_fwd(sim, d, y_dtype=torch.float32, **kw)["y"], r32["y"], kw)
        _check(_bwd(sim, d, **kw), r32, ("grad_z", "grad_params"), (n, channels, dtype), kw, tol)


def test_only_what_is_requested_is_written(sim):
    import torch
    channels, dtype, n = 128, "float16", 9
    d = _dev(H.inputs(n, channels, dtype), dtype)
    full = _bwd(sim, d)
    one = _bwd(sim, d, grad_z=None)
    assert set(one) == {"grad_params"} and torch.equal(_bits(one["grad_params"]), _bits(full["grad_params"]))
    other = _bwd(sim, d, grad_params=None)
    assert set(other) == {"grad_z"} and torch.equal(_bits(other["grad_z"]), _bits(full["grad_z"]))
    # preallocated outputs: a slot of a larger buffer is written, its neighbours are not
    buf = torch.full((3, n, channels), -7.0, dtype=torch.float32, device="cuda")
    out = _fwd(sim, d, y=buf[1])
    assert out["y"].data_ptr() == buf[1].data_ptr() and bool((buf[0] == -7).all()) and bool((buf[2] == -7).all()) and not bool((buf[1] == -7).any())
    assert torch.equal(_bits(buf[1]), _bits(_fwd(sim, d, y_dtype=torch.float32)["y"]))
    gbuf = torch.full((2, n, channels), -7.0, dtype=torch.float16, device="cuda")
    _bwd(sim, d, grad_z=gbuf[0], grad_params=None)
    assert torch.equal(_bits(gbuf[0]), _bits(full["grad_z"])) and bool((gbuf[1] == -7).all())


def test_the_stream_form_and_the_shards(sim):
    import gpu_hideseek
    import torch
    channels, dtype, n = 256, "bfloat16", 14
    d = _dev(H.inputs(n, channels, dtype), dtype)
    blocking, gb = _fwd(sim, d), _bwd(sim, d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = _fwd(sim, d, stream=side)
    gs = _bwd(sim, d, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(_bits(got["y"]), _bits(blocking["y"]))
    for k in ("grad_z", "grad_params"):
        assert torch.equal(_bits(gs[k]), _bits(gb[k])), k
    kw = dict(sim_flags=0, rand_seed=0, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0, 0], 6, **kw)
    ss.init()
    cuts = [slice(0, 5), slice(5, 9), slice(9, n)]
    part = lambda k: [d[k][c].contiguous() for c in cuts]                   # noqa: E731
    res = ss.dense_norm_act(part("z"), d["params"])
    assert len(res) == 3
    for r, c in zip(res, cuts):
        assert torch.equal(_bits(r["y"]), _bits(blocking["y"][c]))
    back = ss.dense_norm_act_backward(part("z"), [d["params"]] * 3, part("grad_y"))
    for b, c in zip(back, cuts):
        one = _bwd(sim, {k: (v[c].contiguous() if k != "params" else v) for k, v in d.items()})
        for k in ("grad_z", "grad_params"):
            assert torch.equal(_bits(b[k]), _bits(one[k])), k
        assert torch.equal(_bits(b["grad_z"]), _bits(gb["grad_z"][c]))
    ss.close()


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import mlp as M
    INVALID = 1
    n, channels = 9, 64
    case = (n, channels, "float32")
    x = H.inputs(*case)
    pad = 16

    def padded(a, dtype=torch.float32, fill=None):
        a = np.array(a)
        t = torch.zeros(a.size + pad, dtype=dtype, device="cuda") if fill is None else torch.full((a.size + pad,), fill, dtype=dtype, device="cuda")
        if fill is None:
            t[:a.size] = torch.from_numpy(a).reshape(-1).to(dtype)
        return t
    z, params, gy = padded(x["z"]), padded(x["params"]), padded(x["grad_y"])
    z_h = torch.zeros(n * channels + pad, dtype=torch.bfloat16, device="cuda")
    y, gz, gp = padded(np.zeros(n * channels), fill=-7.0), padded(np.zeros(n * channels), fill=-7.0), padded(np.zeros(PARAM_ROWS * channels), fill=-7.0)
    y_h = padded(np.zeros(n * channels), torch.float16, -7.0)
    ins, outs = (z, params, gy), (y, gz, gp, y_h)
    saved = [t.clone() for t in ins]
    P = lambda t: t.data_ptr()                                              # noqa: E731
    assert all(P(t) % 16 == 0 for t in ins + outs + (z_h,))

    def fwd(z=P(z), params=P(params), n=n, channels=channels, zdt=1, ydt=1, eps=1e-6, slope=0.01, y=P(y)):
        return M.HsDenseNormActRequest(z, params, n, channels, zdt, ydt, eps, slope, y)

    def bwd(z=P(z), params=P(params), grad_y=P(gy), n=n, channels=channels, zdt=1, ydt=1, eps=1e-6, slope=0.01, grad_z=P(gz), grad_params=P(gp)):
        return M.HsDenseNormActBackwardRequest(z, params, grad_y, n, channels, zdt, ydt, eps, slope, grad_z, grad_params)

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ins, saved)) and all(bool((t == -7).all()) for t in outs)

    def call(s, r, stream=False):
        fn = "hs_dense_norm_act_backward" if isinstance(r, M.HsDenseNormActBackwardRequest) else "hs_dense_norm_act"
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
    for fn in ("hs_dense_norm_act", "hs_dense_norm_act_backward"):
        assert getattr(s._L, fn)(s._h, None) == INVALID and "null request" in message(s)
        assert getattr(s._L, fn + "_async")(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), None) == INVALID and "null request" in message(s)
    nan, inf = float("nan"), float("inf")
    bad = {}
    for name, make in (("forward", fwd), ("backward", bwd)):
        bad.update({
            (name, "null z"): (make(z=None), "null z"), (name, "null params"): (make(params=None), "null params"),
            (name, "z dtype"): (make(zdt=2), "z dtype"), (name, "y dtype"): (make(ydt=0), "y dtype"), (name, "y dtype 5"): (make(ydt=5), "y dtype"),
            (name, "C 32"): (make(channels=32), "channels must"), (name, "C 0"): (make(channels=0), "channels must"),
            (name, "C 192"): (make(channels=192), "channels must"), (name, "C 1024"): (make(channels=1024), "channels must"),
            (name, "n 0"): (make(n=0), "n must"), (name, "n -1"): (make(n=-1), "n must"), (name, "n x C"): (make(n=2 ** 22, channels=512), "n must"),
            (name, "eps nan"): (make(eps=nan), "eps must"), (name, "eps 0"): (make(eps=0.0), "eps must"), (name, "eps < 0"): (make(eps=-1e-6), "eps must"),
            (name, "eps inf"): (make(eps=inf), "eps must"), (name, "slope nan"): (make(slope=nan), "slope must"), (name, "slope inf"): (make(slope=inf), "slope must"),
            (name, "slope < 0"): (make(slope=-0.01), "slope must"), (name, "slope > 1"): (make(slope=1.5), "slope must"),
            (name, "z +4"): (make(z=P(z) + 4), "z must be 16-byte aligned"), (name, "z +8"): (make(z=P(z) + 8), "z must be 16-byte aligned"),
            (name, "z bf16 +2"): (make(z=P(z_h) + 2, zdt=3), "z must be 16-byte aligned"), (name, "params +2"): (make(params=P(params) + 2), "4-byte aligned"),
        })
    bad.update({
        "no output": (fwd(y=None), "every output is null"), "y +4": (fwd(y=P(y) + 4), "16-byte aligned"), "y f16 +2": (fwd(y=P(y_h) + 2, ydt=4), "16-byte aligned"),
        "y is z": (fwd(y=P(z)), "y overlaps z"), "y in z": (fwd(y=P(z) + 64), "y overlaps z"), "y on params": (fwd(y=P(params)), "y overlaps params"),
        "null grad_y": (bwd(grad_y=None), "null grad_y"), "no gradient out": (bwd(grad_z=None, grad_params=None), "every output is null"),
        "grad_y +8": (bwd(grad_y=P(gy) + 8), "16-byte aligned"), "grad_z +4": (bwd(grad_z=P(gz) + 4), "16-byte aligned"),
        "grad_params +2": (bwd(grad_params=P(gp) + 2), "4-byte aligned"),
        "grad_z is z": (bwd(grad_z=P(z)), "grad_z overlaps z"), "grad_z in grad_y": (bwd(grad_z=P(gy) + 16), "grad_z overlaps grad_y"),
        "grad_params is params": (bwd(grad_params=P(params)), "grad_params overlaps params"),
        "grad_params in grad_y": (bwd(grad_params=P(gy) + 8), "grad_params overlaps grad_y"),
        "grad_params in grad_z": (bwd(grad_params=P(gz) + 16), "grad_params overlaps grad_z"),
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
    want = H.both(case)[0]
    assert call(s, fwd()) == 0 and call(s, bwd()) == 0           # the calls do write, and only their own ranges
    torch.cuda.synchronize()
    for t, k, size in ((y, "y", n * channels), (gz, "grad_z", n * channels), (gp, "grad_params", PARAM_ROWS * channels)):
        assert bool((t[size:] == -7).all()) and not bool((t[:size] == -7).any()), k
        _check({k: t[:size].view(want[k].shape)}, want, (k,), case, "C ABI")
    assert call(s, fwd(y=P(y_h), ydt=4)) == 0
    torch.cuda.synchronize()
    assert bool((y_h[n * channels:] == -7).all()) and not bool((y_h[:n * channels] == -7).any())
    s.close()


def test_the_modules_against_their_eager_form(sim):
    """DenseNormAct and MLP(fused=True) against fused=False under autograd: both within the allowance for float32 GEMMs
    in another order (4 x torch f32 against float64 on the CPU, test_mlp_host.module_allowance) of the float64 result."""
    import torch
    from gpu_hideseek import mlp as M
    allow, f64 = H.module_allowance()
    x = {k: torch.from_numpy(np.array(v)).cuda() for k, v in H.module_inputs().items()}
    fused = H.module_net(True, "cuda")
    y = fused(sim, x["x"])
    assert y.shape == (H.MODULE["n"], H.MODULE["C"]) and y.requires_grad and y.dtype == torch.float32
    (y * x["weight"]).sum().add(0.5 * (y ** 2).mean()).backward()
    got = {"y": y}
    got.update({k: p.grad for k, p in fused.named_parameters()})
    eager = H.module_eager(torch.float32, "cuda")                           # fused=False on the device
    assert set(got) == set(eager) == set(f64)
    for k in f64:
        ef, ee = float(np.abs(_np(got[k]).astype(np.float64) - f64[k]).max()), float(np.abs(eager[k] - f64[k]).max())
        print(f"MLP module: {k}: fused {ef:.3e}, eager on the device {ee:.3e} from float64 (allowance {allow[k]:.3e}, largest value {float(np.abs(f64[k]).max()):.3e})")
        assert ef <= allow[k] and ee <= allow[k], k
    # one layer alone, and the switch: the same module computes eager() on the same parameters
    layer = fused.layers[0]
    a = layer(sim, x["x"])
    layer.fused = False
    b = layer(None, x["x"])
    layer.fused = True
    assert torch.equal(b, M.eager(x["x"] @ layer.weight, layer.params, layer.eps, layer.slope)) and a.shape == b.shape and not torch.equal(a, torch.zeros_like(a))
    # bf16: the GEMM and y in bf16, the gradient of the input too
    xb = x["x"].bfloat16().requires_grad_()
    yb = fused(sim, xb)
    yb.float().sum().backward()
    assert yb.dtype == torch.bfloat16 and xb.grad.dtype == torch.bfloat16 and torch.isfinite(yb.float()).all().item() and torch.isfinite(xb.grad.float()).all().item()
    assert isinstance(M.MLP(8, 64, 1), torch.nn.Module)
