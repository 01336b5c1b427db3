"""The recurrent core on the GPU (sim.lstm_cell / lstm_cell_backward, hs_lstm_cell, csrc/hs_k_lstm.h) against the numpy
restatement of tests/test_lstm_cell_host.py within the tolerances derived there: one row, a partial round, one row past a
round, past the backward's sweep and (forward only) past the forward's; every hidden size and dtype; with and without
clear and the optional gradients; determinism, position independence, exact zeros for cleared rows and for zero
gradients, bit for bit; the done export of a stepped simulator as clear; the torch module against the eager sequence and
under Adam; the stream form, the shards, another eps, and the refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import test_lstm_cell_host as H
from test_lstm_cell_host import BACKWARD_OUTPUTS, BIG_FWD, DTYPES, FORWARD_OUTPUTS, HIDDEN, PARAM_ROWS, SIZES

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
    t = {k: torch.from_numpy(np.array(v)).cuda() for k, v in x.items()}
    for k in ("gates", "grad_y", "grad_h_next"):
        t[k] = t[k].to(dt)
    return t


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype.is_floating_point else t.detach().cpu().numpy()


def _bits(t):
    import torch
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _fwd(sim, d, clear=True, **kw):
    return sim.lstm_cell(d["gates"], d["c_prev"], d["params"], clear=d["clear"] if clear else None, **kw)


def _bwd(sim, d, clear=True, grad_h=True, grad_c=True, **kw):
    return sim.lstm_cell_backward(d["gates"], d["c_prev"], d["params"], d["grad_y"], clear=d["clear"] if clear else None,
                                  grad_h_next=d["grad_h_next"] if grad_h else None, grad_c_next=d["grad_c_next"] if grad_c else None, **kw)


def _check(got, want, names, case, tag, tol=None):
    """Every output within its derived bound of the f32 restatement (want: H.run(np.float32, ...))."""
    for k in names:
        g, w = _np(got[k]).astype(np.float64), want[k].astype(np.float64)
        err, limit = np.abs(g - w), H.bound(k, w, case, tol)
        print(f"{tag}: {k}: largest |got - want| = {float(err.max()):.3e}, largest excess over the bound {float((err - limit).max()):.3e}, "
              f"{int((g != w).sum())} of {g.size} differ")
        assert g.shape == w.shape and np.isfinite(g).all() and (err <= limit).all(), (tag, k, float((err - limit).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hidden", HIDDEN)
def test_parity_with_the_restatement(sim, hidden, dtype):
    import torch
    for n in SIZES:
        case = (n, hidden, dtype)
        d = _dev(H.inputs(*case), dtype)
        want = H.both(case)[0]
        out = _fwd(sim, d)
        assert set(out) == set(FORWARD_OUTPUTS) and out["y"].dtype == out["h_next"].dtype == getattr(torch, dtype) and out["c_next"].dtype == torch.float32
        _check(out, want, FORWARD_OUTPUTS, case, case)
        res = _bwd(sim, d)
        assert set(res) == set(BACKWARD_OUTPUTS) and res["grad_gates"].dtype == getattr(torch, dtype) and res["grad_cell_params"].shape == (PARAM_ROWS * hidden,)
        _check(res, want, BACKWARD_OUTPUTS, case, case)


def test_past_the_forward_sweep(sim):
    n, hidden, dtype = BIG_FWD
    x = H.inputs(*BIG_FWD)
    d = _dev(x, dtype)
    want = H.forward(np.float32, x["gates"], x["c_prev"], x["params"], x["clear"], hidden)
    _check(_fwd(sim, d), want, FORWARD_OUTPUTS, BIG_FWD, BIG_FWD)


@pytest.mark.parametrize("hidden,dtype", [(64, "bfloat16"), (256, "float32"), (512, "float16")])
def test_null_options(sim, hidden, dtype):
    """Without clear, without grad_h_next, without grad_c_next: within the tolerances of the case (the same arithmetic on
    the same inputs, fewer terms), and bit for bit what explicit zeros give."""
    import torch
    case = (5, hidden, dtype)
    x = H.inputs(*case)
    d = _dev(x, dtype)
    for opts in (dict(clear=False), dict(grad_h=False), dict(grad_c=False), dict(clear=False, grad_h=False, grad_c=False)):
        want = H.run(np.float32, x, hidden, **opts)
        if "clear" in opts:
            _check(_fwd(sim, d, clear=False), want, FORWARD_OUTPUTS, case, (case, opts))
        got = _bwd(sim, d, **opts)
        _check(got, want, BACKWARD_OUTPUTS, case, (case, opts))
        z = dict(d, clear=torch.zeros_like(d["clear"]) if "clear" in opts else d["clear"],
                 grad_h_next=torch.zeros_like(d["grad_h_next"]) if "grad_h" in opts else d["grad_h_next"],
                 grad_c_next=torch.zeros_like(d["grad_c_next"]) if "grad_c" in opts else d["grad_c_next"])
        explicit = _bwd(sim, z)
        for k in BACKWARD_OUTPUTS:
            assert torch.equal(_bits(got[k]), _bits(explicit[k])), (case, opts, k)
    # only what is requested is written
    only = sim.lstm_cell(d["gates"], d["c_prev"], d["params"], clear=d["clear"], y=None, h_next=None)
    assert set(only) == {"c_next"} and torch.equal(_bits(only["c_next"]), _bits(_fwd(sim, d)["c_next"]))
    one = _bwd(sim, d, grad_gates=None, grad_c_prev=None)
    assert set(one) == {"grad_cell_params"} and torch.equal(_bits(one["grad_cell_params"]), _bits(_bwd(sim, d)["grad_cell_params"]))
    assert set(_bwd(sim, d, grad_cell_params=None)) == {"grad_gates", "grad_c_prev"}


def test_determinism_position_and_cleared_rows(sim):
    import torch
    for hidden, dtype, n in ((64, "float32", 14), (128, "bfloat16", 14), (256, "bfloat16", 2051), (512, "float16", 14)):
        d = _dev(H.inputs(n, hidden, dtype), dtype)
        first, again = _fwd(sim, d), _fwd(sim, d)
        for k in FORWARD_OUTPUTS:
            assert torch.equal(_bits(first[k]), _bits(again[k])), (hidden, dtype, k)
        g1, g2 = _bwd(sim, d), _bwd(sim, d)
        for k in BACKWARD_OUTPUTS:
            assert torch.equal(_bits(g1[k]), _bits(g2[k])), (hidden, dtype, k)
        # cleared rows: h_next and c_next exactly +0, y what it is without the clear
        rows = d["clear"] != 0
        assert bool(rows.any()) and not bool(rows.all())
        assert not _bits(first["h_next"])[rows].any().item() and not _bits(first["c_next"])[rows].any().item()
        free = _fwd(sim, d, clear=False)
        assert torch.equal(_bits(free["y"]), _bits(first["y"])) and bool((free["h_next"][rows] != 0).any())
        assert torch.equal(_bits(free["h_next"][~rows]), _bits(first["h_next"][~rows]))
        # a row at another index of a batch of another size: the same outputs and the same per-row gradients
        perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
        moved = {k: (v[perm].contiguous() if k != "params" else v) for k, v in d.items()}
        mf, mb = _fwd(sim, moved), _bwd(sim, moved, grad_cell_params=None)
        for k in FORWARD_OUTPUTS:
            assert torch.equal(_bits(mf[k]), _bits(first[k][perm])), (hidden, dtype, k)
        for k in ("grad_gates", "grad_c_prev"):
            assert torch.equal(_bits(mb[k]), _bits(g1[k][perm])), (hidden, dtype, k)
        sub = {k: (v[3:6].contiguous() if k != "params" else v) for k, v in d.items()}
        sf, sb = _fwd(sim, sub), _bwd(sim, sub)
        for k in FORWARD_OUTPUTS:
            assert torch.equal(_bits(sf[k]), _bits(first[k][3:6])), (hidden, dtype, k)
        assert torch.equal(_bits(sb["grad_gates"]), _bits(g1["grad_gates"][3:6]))


def test_zero_gradients_give_plus_zero(sim):
    import torch
    for hidden, dtype in ((64, "float32"), (256, "bfloat16"), (512, "float16")):
        n = 14
        d = _dev(H.inputs(n, hidden, dtype), dtype)
        gp = torch.full((PARAM_ROWS * hidden,), -7.0, device="cuda")
        z = dict(d, grad_y=torch.zeros_like(d["grad_y"]), grad_h_next=torch.zeros_like(d["grad_h_next"]), grad_c_next=torch.zeros_like(d["grad_c_next"]))
        for kw in (dict(), dict(grad_h=False, grad_c=False)):
            res = _bwd(sim, z, grad_cell_params=gp.fill_(-7.0), **kw)
            assert not _bits(gp).any().item(), (hidden, dtype)
            assert not (res["grad_gates"] != 0).any().item() and not (res["grad_c_prev"] != 0).any().item()


def test_the_done_export_as_clear():
    """A stepped simulator's done export (every world resets at step 240) clears the carried state of its rows."""
    import torch
    worlds, agents, hidden = 6, 6, 256
    s = _sim(worlds, agents, seed=3)
    s.init()
    rows = worlds * agents
    x = H.inputs(rows, hidden, "bfloat16")
    d = _dev(x, "bfloat16")
    seen = set()
    for step in range(241):
        s.step()
        if step < 238:
            continue
        done = s.done_tensor().to_torch()
        assert done.dtype == torch.int32 and done.numel() == rows
        flat = done.reshape(rows)
        for clear in (done, flat):                              # [rows, 1] as exported, or flattened
            out = s.lstm_cell(d["gates"], d["c_prev"], d["params"], clear=clear)
            want = H.forward(np.float32, x["gates"], x["c_prev"], x["params"], flat.cpu().numpy(), hidden)
            _check(out, want, FORWARD_OUTPUTS, (rows, hidden, "bfloat16"), ("done", step), tol=_tol(x, hidden, flat))
            ended = flat != 0
            assert not _bits(out["h_next"])[ended].any().item() and not _bits(out["c_next"])[ended].any().item()
            assert bool((out["h_next"][~ended] != 0).any()) or bool(ended.all())
        seen.add(bool((flat != 0).any()))
    assert seen == {False, True}, "the window must contain steps with and without an episode's end"
    s.close()


def _tol(x, hidden, clear):
    """4 x the f32-vs-float64 gap of the forward on these inputs with this clear (the rule of the host file)."""
    cl = clear.cpu().numpy()
    f32, f64 = (H.forward(ft, x["gates"], x["c_prev"], x["params"], cl, hidden) for ft in (np.float32, np.float64))
    return {k: 4.0 * float(np.abs(f32[k].astype(np.float64) - f64[k]).max()) for k in FORWARD_OUTPUTS}


def test_the_module_against_the_eager_sequence_and_under_adam(sim):
    import torch
    from gpu_hideseek import recurrent as N
    T, n, F, hidden = (H.SEQ[k] for k in "TnFH")
    allow, f64 = H.sequence_allowance()
    x = {k: torch.from_numpy(np.array(v)).cuda() for k, v in H.sequence_inputs().items()}
    core = N.LSTMCore(F, hidden).cuda()
    assert [tuple(p.shape) for p in core.parameters()] == [(F, 4 * hidden), (hidden, 4 * hidden), (PARAM_ROWS * hidden,)]
    with torch.no_grad():
        core.w_in.copy_(x["w_in"]); core.w_rec.copy_(x["w_rec"]); core.cell_params.copy_(x["cell_params"])

    def loss_of(ys):
        return (ys * x["weight"]).sum() + 0.5 * (ys ** 2).mean()
    ys, (h, c) = core.sequence(sim, x["xs"], (x["h0"], x["c0"]), x["clears"])
    assert ys.shape == (T, n, hidden) and ys.requires_grad and h.dtype == c.dtype == torch.float32
    loss_of(ys).backward()
    fused = {"ys": ys, "w_in": core.w_in.grad, "w_rec": core.w_rec.grad, "cell_params": core.cell_params.grad}
    eager = H.sequence_eager(torch.float32, "cuda")                         # the same composition in plain torch on the device
    cleared = x["clears"][1] != 0
    for k in ("ys", "w_in", "w_rec", "cell_params"):
        ef, ee = float(np.abs(_np(fused[k]).astype(np.float64) - f64[k]).max()), float(np.abs(eager[k] - f64[k]).max())
        print(f"module sequence: {k}: fused {ef:.3e}, eager on the device {ee:.3e} from float64 (allowance {allow[k]:.3e}, largest value {float(np.abs(f64[k]).max()):.3e})")
        assert ef <= allow[k] and ee <= allow[k], k
    # a few Adam steps on the fused path: the loss decreases
    opt = torch.optim.Adam(core.parameters(), lr=3e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        ys, _ = core.sequence(sim, x["xs"], (x["h0"], x["c0"]), x["clears"])
        loss = 0.5 * ((ys - x["weight"]) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("module under Adam:", losses)
    assert all(np.isfinite(losses)) and all(b < a for a, b in zip(losses, losses[1:]))
    # bf16 GEMMs and state: the module runs and carries a bf16 h
    state = core.init_state(n, "cuda", torch.bfloat16)
    y, (h, c) = core(sim, x["xs"][0], state, x["clears"][1])
    assert y.dtype == h.dtype == torch.bfloat16 and c.dtype == torch.float32 and not h[cleared].any().item() and torch.isfinite(y.float()).all().item()


def test_the_stream_form_the_shards_and_another_eps(sim):
    import gpu_hideseek
    import torch
    hidden, dtype, n = 256, "bfloat16", 14
    x = H.inputs(n, hidden, dtype)
    d = _dev(x, dtype)
    blocking, gb = _fwd(sim, d), _bwd(sim, d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = _fwd(sim, d, stream=side)
    gs = _bwd(sim, d, stream=side.cuda_stream)
    side.synchronize()
    for k in FORWARD_OUTPUTS:
        assert torch.equal(_bits(got[k]), _bits(blocking[k])), k
    for k in BACKWARD_OUTPUTS:
        assert torch.equal(_bits(gs[k]), _bits(gb[k])), k
    kw = dict(sim_flags=0, rand_seed=0, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0, 0], 6, **kw)
    ss.init()
    cuts = [slice(0, 5), slice(5, 9), slice(9, n)]
    part = lambda k: [d[k][c].contiguous() for c in cuts]                   # noqa: E731
    res = ss.lstm_cell(part("gates"), part("c_prev"), d["params"], clear=part("clear"))
    assert len(res) == 3
    for r, c in zip(res, cuts):
        for k in FORWARD_OUTPUTS:
            assert torch.equal(_bits(r[k]), _bits(blocking[k][c])), k
    back = ss.lstm_cell_backward(part("gates"), part("c_prev"), [d["params"]] * 3, part("grad_y"), clear=part("clear"), grad_h_next=part("grad_h_next"),
                                 grad_c_next=part("grad_c_next"))
    for b, c in zip(back, cuts):
        one = _bwd(sim, {k: (v[c].contiguous() if k != "params" else v) for k, v in d.items()})
        for k in BACKWARD_OUTPUTS:
            assert torch.equal(_bits(b[k]), _bits(one[k])), k
        assert torch.equal(_bits(b["grad_gates"]), _bits(gb["grad_gates"][c]))
    ss.close()
    # another eps: within the tolerances of its own restatement (the rule of the host file on the same inputs)
    eps = 1e-2
    r32, r64 = H.run(np.float32, x, hidden, eps), H.run(np.float64, x, hidden, eps)
    tol = {k: 4.0 * v for k, v in H._gaps(r32, r64, hidden).items()}
    out = _fwd(sim, d, eps=eps)
    assert not torch.equal(_bits(out["y"]), _bits(blocking["y"]))
    _check(out, r32, FORWARD_OUTPUTS, (n, hidden, dtype), "eps", tol)
    _check(_bwd(sim, d, eps=eps), r32, BACKWARD_OUTPUTS, (n, hidden, dtype), "eps", tol)


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import recurrent as N
    INVALID = 1
    n, hidden = 9, 64
    case = (n, hidden, "float32")
    x = H.inputs(*case)
    pad = 16

    def padded(a, dtype=torch.float32, fill=None):
        a = np.array(a)
        t = torch.zeros(a.size + pad, dtype=dtype, device="cuda") if fill is None else torch.full((a.size + pad,), fill, dtype=dtype, device="cuda")
        if fill is None:
            t[:a.size] = torch.from_numpy(a).reshape(-1).to(dtype)
        return t
    gates, cprev, params = padded(x["gates"]), padded(x["c_prev"]), padded(x["params"])
    clear = padded(x["clear"], torch.int32)
    gy, gh, gc = padded(x["grad_y"]), padded(x["grad_h_next"]), padded(x["grad_c_next"])
    gates_h = torch.zeros(n * 4 * hidden + pad, dtype=torch.bfloat16, device="cuda")
    y, hn, cn = (padded(np.zeros(n * hidden), fill=-7.0) for _ in range(3))
    y_h = padded(np.zeros(n * hidden), torch.float16, -7.0)
    gg, gcp, gp = padded(np.zeros(n * 4 * hidden), fill=-7.0), padded(np.zeros(n * hidden), fill=-7.0), padded(np.zeros(PARAM_ROWS * hidden), fill=-7.0)
    ins = (gates, cprev, params, clear, gy, gh, gc)
    outs = (y, hn, cn, y_h, gg, gcp, gp)
    saved = [t.clone() for t in ins]
    P = lambda t: t.data_ptr()                                              # noqa: E731

    def fwd(gates=P(gates), c_prev=P(cprev), cell_params=P(params), clear=P(clear), n=n, hidden=hidden, gdt=1, ydt=1, eps=1e-6, y=P(y), h_next=P(hn), c_next=P(cn)):
        return N.HsLstmCellRequest(gates, c_prev, cell_params, clear, n, hidden, gdt, ydt, eps, 0, y, h_next, c_next)

    def bwd(gates=P(gates), c_prev=P(cprev), cell_params=P(params), clear=P(clear), grad_y=P(gy), grad_h_next=P(gh), grad_c_next=P(gc), n=n, hidden=hidden,
            gdt=1, ydt=1, eps=1e-6, grad_gates=P(gg), grad_c_prev=P(gcp), grad_cell_params=P(gp)):
        return N.HsLstmCellBackwardRequest(gates, c_prev, cell_params, clear, grad_y, grad_h_next, grad_c_next, n, hidden, gdt, ydt, eps, 0, grad_gates,
                                           grad_c_prev, grad_cell_params)

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ins, saved)) and all(bool((t == -7).all()) for t in outs)

    def call(s, r, stream=False):
        fn = "hs_lstm_cell_backward" if isinstance(r, N.HsLstmCellBackwardRequest) else "hs_lstm_cell"
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
    for fn in ("hs_lstm_cell", "hs_lstm_cell_backward"):
        assert getattr(s._L, fn)(s._h, None) == INVALID and "null request" in message(s)
        assert getattr(s._L, fn + "_async")(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), None) == INVALID and "null request" in message(s)
    nan, inf = float("nan"), float("inf")
    bad = {}
    for name, make in (("forward", fwd), ("backward", bwd)):
        bad.update({
            (name, "null gates"): (make(gates=None), "null gates"), (name, "null c_prev"): (make(c_prev=None), "null c_prev"),
            (name, "null cell_params"): (make(cell_params=None), "null cell_params"), (name, "gates dtype"): (make(gdt=2), "gates dtype"),
            (name, "y dtype"): (make(ydt=0), "y dtype"), (name, "H 32"): (make(hidden=32), "hidden must"), (name, "H 0"): (make(hidden=0), "hidden must"),
            (name, "H 192"): (make(hidden=192), "hidden must"), (name, "H 1024"): (make(hidden=1024), "hidden must"),
            (name, "n 0"): (make(n=0), "n must"), (name, "n -1"): (make(n=-1), "n must"), (name, "n x 4 H"): (make(n=2 ** 20, hidden=512), "n must"),
            (name, "eps nan"): (make(eps=nan), "eps must"), (name, "eps 0"): (make(eps=0.0), "eps must"), (name, "eps < 0"): (make(eps=-1e-6), "eps must"),
            (name, "eps inf"): (make(eps=inf), "eps must"), (name, "gates +2"): (make(gates=P(gates) + 2), "aligned"),
            (name, "gates bf16 +1"): (make(gates=P(gates_h) + 1, gdt=3), "aligned"), (name, "c_prev +2"): (make(c_prev=P(cprev) + 2), "4-byte aligned"),
            (name, "cell_params +1"): (make(cell_params=P(params) + 1), "4-byte aligned"), (name, "clear +2"): (make(clear=P(clear) + 2), "4-byte aligned"),
        })
    bad.update({
        "no output": (fwd(y=None, h_next=None, c_next=None), "every output is null"), "y +2": (fwd(y=P(y) + 2), "aligned"),
        "y f16 +1": (fwd(y=P(y_h) + 1, ydt=4), "aligned"), "h_next +2": (fwd(h_next=P(hn) + 2), "aligned"), "c_next +1": (fwd(c_next=P(cn) + 1), "4-byte aligned"),
        "y is gates": (fwd(y=P(gates)), "y overlaps gates"), "h_next in c_prev": (fwd(h_next=P(cprev) + 64), "h_next overlaps c_prev"),
        "c_next in params": (fwd(c_next=P(params) + 8), "c_next overlaps"), "y on clear": (fwd(y=P(clear)), "y overlaps"),
        "h_next in y": (fwd(h_next=P(y) + 4), "h_next overlaps y"), "c_next is h_next": (fwd(c_next=P(hn)), "c_next overlaps h_next"),
        "null grad_y": (bwd(grad_y=None), "null grad_y"), "no gradient out": (bwd(grad_gates=None, grad_c_prev=None, grad_cell_params=None), "every output is null"),
        "grad_y +2": (bwd(grad_y=P(gy) + 2), "aligned"), "grad_h_next +2": (bwd(grad_h_next=P(gh) + 2), "aligned"), "grad_gates +2": (bwd(grad_gates=P(gg) + 2), "aligned"),
        "grad_c_next +2": (bwd(grad_c_next=P(gc) + 2), "4-byte aligned"), "grad_c_prev +1": (bwd(grad_c_prev=P(gcp) + 1), "4-byte aligned"),
        "grad_cell_params +2": (bwd(grad_cell_params=P(gp) + 2), "4-byte aligned"),
        "grad_gates is gates": (bwd(grad_gates=P(gates)), "grad_gates overlaps gates"), "grad_c_prev in grad_y": (bwd(grad_c_prev=P(gy) + 4), "grad_c_prev overlaps grad_y"),
        "grad_cell_params is cell_params": (bwd(grad_cell_params=P(params)), "grad_cell_params overlaps cell_params"),
        "grad_cell_params in grad_h_next": (bwd(grad_cell_params=P(gh) + 8), "grad_cell_params overlaps grad_h_next"),
        "grad_gates on grad_c_next": (bwd(grad_gates=P(gc)), "grad_gates overlaps"),
        "grad_c_prev in grad_gates": (bwd(grad_c_prev=P(gg) + 16), "grad_c_prev overlaps grad_gates"),
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
    for t, k, size in ((y, "y", n * hidden), (hn, "h_next", n * hidden), (cn, "c_next", n * hidden), (gg, "grad_gates", n * 4 * hidden),
                       (gcp, "grad_c_prev", n * hidden), (gp, "grad_cell_params", PARAM_ROWS * hidden)):
        assert bool((t[size:] == -7).all()) and not bool((t[:size] == -7).any()), k
        _check({k: t[:size].view(want[k].shape)}, want, (k,), case, "C ABI")
    assert call(s, fwd(y=P(y_h), ydt=4, h_next=None, c_next=None, clear=None)) == 0
    assert bool((y_h[n * hidden:] == -7).all()) and not bool((y_h[:n * hidden] == -7).any())
    s.close()
