"""The entity encoder on the GPU (sim.encode_entities / encode_entities_backward, hs_entity_encode,
csrc/hs_k_embed.h) against the numpy restatement of tests/test_entity_encoder_host.py within the tolerances derived
there: sizes around the rows a workgroup takes per round and past the backward's grid cap, every embed_dim and dtype; the
argmax; crafted exact ties; +0 for a zero gradient; determinism, position independence and the unaligned load path, bit
for bit; live rows of a stepped simulator into a rollout buffer, actor against masked critic; the torch module under
Adam; the stream form, the shards, other eps and slope, and the refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import test_entity_encoder_host as H
from test_entity_encoder_host import BIG, BIG_E, CASES, DTYPES, EMBED_DIMS, PARAM_ROWS, ROW, TABLES

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
    return dict(rows=torch.from_numpy(np.array(x["rows"])).cuda().to(dt), params=torch.from_numpy(np.array(x["params"])).cuda(),
                grad=torch.from_numpy(np.array(x["grad"])).cuda().to(dt))


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype.is_floating_point else t.detach().cpu().numpy()


def _bits(t):
    import torch
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _check_forward(out, x, E, dtype, tag, eps=H.EPS, slope=H.SLOPE):
    """Features within the derived bound of the f32 restatement; the chosen entity's float64 value within twice the
    feature tolerance of the float64 maximum."""
    r32 = H.forward(np.float32, x["rows"], x["params"], E, eps, slope)
    r64 = H.forward(np.float64, x["rows"], x["params"], E, eps, slope)
    got, want = _np(out["features"]).astype(np.float64), r32["features"].astype(np.float64)
    err, bound = np.abs(got - want), H.feature_bound(want, E, dtype)
    print(f"{tag}: features: largest |got - want| = {float(err.max()):.3e} (tolerances {H.feature_tolerance(E)}), {int((got != want).sum())} of {got.size} differ")
    assert np.isfinite(got).all() and (err <= bound).all(), (tag, float((err - bound).max()))
    am = _np(out["argmax"])
    assert am.dtype == np.uint8 and am.shape == (got.shape[0], 3, E)
    for g in (1, 2, 3):
        assert am[:, g - 1].max() < TABLES[g][3], (tag, "an entity that is not there")
        a64 = r64["a"][g]
        chosen = np.take_along_axis(a64, am[:, g - 1, None, :].astype(np.int64), 1)[:, 0]
        assert (a64.max(1) - chosen <= 2 * H.feature_tolerance(E)[g]).all(), (tag, TABLES[g][0])
    return am


def _check_backward(gp, x, am, case, tag, eps=H.EPS, slope=H.SLOPE):
    E = case[1]
    want = H.backward(np.float64, x["rows"], x["params"], x["grad"], am, E, eps, slope)
    got = _np(gp).astype(np.float64)
    err, bound = np.abs(got - want), H.grad_bound(case)
    print(f"{tag}: grad_params: largest |got - want| = {float(err.max()):.3e} (tolerances {H.grad_tolerance(case)}, largest gradient {float(np.abs(want).max()):.3e})")
    assert gp.dtype.is_floating_point and gp.element_size() == 4 and np.isfinite(got).all()
    assert (err <= bound).all(), (tag, float((err - bound).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", EMBED_DIMS)
def test_parity_with_the_restatement(sim, E, dtype):
    import torch
    for n in H.sizes(E):
        case = (n, E, dtype)
        x = H.inputs(*case)
        d = _dev(x, dtype)
        out = sim.encode_entities(d["rows"], d["params"], embed_dim=E, argmax=True)
        assert set(out) == {"features", "argmax"} and out["features"].dtype == getattr(torch, dtype) and out["features"].shape == (n, 4 * E)
        am = _check_forward(out, x, E, dtype, case)
        res = sim.encode_entities_backward(d["rows"], d["params"], d["grad"], out["argmax"], embed_dim=E)
        assert set(res) == {"grad_params"} and res["grad_params"].shape == (PARAM_ROWS * E,)
        _check_backward(res["grad_params"], x, am, case, case)


def test_past_the_backward_grid_cap(sim):
    from gpu_hideseek import entity_encoder as N
    case = CASES[-1]
    assert case[:2] == (BIG, BIG_E) and BIG == N.MAX_GRID_BWD * N.rows_per_block(BIG_E) + 3
    x = H.inputs(*case)
    d = _dev(x, case[2])
    out = sim.encode_entities(d["rows"], d["params"], embed_dim=BIG_E, argmax=True)
    am = _check_forward(out, x, BIG_E, case[2], case)
    _check_backward(sim.encode_entities_backward(d["rows"], d["params"], d["grad"], out["argmax"], embed_dim=BIG_E)["grad_params"], x, am, case, case)


def test_crafted_exact_ties(sim):
    import torch
    E = 64
    x = H.inputs(7, E, "float32")
    rows = np.array(x["rows"])
    _, col, K, _ = TABLES[2]
    rows[:, col + 2 * K:col + 3 * K] *= 3.0                  # box 2 stands out in many channels; box 5 is its copy
    rows[:, col + 5 * K:col + 6 * K] = rows[:, col + 2 * K:col + 3 * K]
    rows[0, 45:] = 0.0                                       # every pooled entity of row 0 masked
    out = sim.encode_entities(torch.from_numpy(rows).cuda(), torch.from_numpy(np.array(x["params"])).cuda(), embed_dim=E, argmax=True)
    am = _np(out["argmax"])
    assert not am[0].any()
    want = H.forward(np.float32, rows, x["params"], E)["argmax"]
    assert (want[:, 1] == 2).any() and not (am[:, 1] == 5).any()
    assert ((am[:, 1] == 2) == (want[:, 1] == 2)).mean() > 0.99 and (am[:, 1] == 2).any()


def test_zero_gradient_gives_plus_zero(sim):
    import torch
    for E, dtype in ((32, "float32"), (64, "bfloat16"), (128, "float16")):
        n = 3 * H.rows_per_block(E) + 2
        d = _dev(H.inputs(n, E, dtype), dtype)
        out = sim.encode_entities(d["rows"], d["params"], embed_dim=E, argmax=True)
        gp = torch.full((PARAM_ROWS * E,), -7.0, device="cuda")
        sim.encode_entities_backward(d["rows"], d["params"], torch.zeros_like(d["grad"]), out["argmax"], embed_dim=E, grad_params=gp)
        assert not _bits(gp).any().item(), (E, dtype)


def test_determinism_position_and_load_paths(sim):
    import torch
    for E, dtype in ((32, "bfloat16"), (64, "bfloat16"), (64, "float32"), (128, "float16")):
        n = 3 * H.rows_per_block(E) + 2
        d = _dev(H.inputs(n, E, dtype), dtype)
        kw = dict(embed_dim=E, argmax=True)
        first, again = sim.encode_entities(d["rows"], d["params"], **kw), sim.encode_entities(d["rows"], d["params"], **kw)
        for k in ("features", "argmax"):
            assert torch.equal(_bits(first[k]), _bits(again[k])), (E, dtype, k)
        g1 = sim.encode_entities_backward(d["rows"], d["params"], d["grad"], first["argmax"], embed_dim=E)["grad_params"]
        g2 = sim.encode_entities_backward(d["rows"], d["params"], d["grad"], first["argmax"], embed_dim=E)["grad_params"]
        assert torch.equal(_bits(g1), _bits(g2)), (E, dtype)
        # a row at another index of a batch of another size
        perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
        moved = sim.encode_entities(d["rows"][perm].contiguous(), d["params"], **kw)
        for k in ("features", "argmax"):
            assert torch.equal(_bits(moved[k]), _bits(first[k][perm])), (E, dtype, k)
        sub = sim.encode_entities(d["rows"][3:6].contiguous(), d["params"], **kw)
        assert torch.equal(_bits(sub["features"]), _bits(first["features"][3:6]))
        # rows that start off a 16-byte boundary take the by-element path: the same bits
        assert d["rows"].data_ptr() % 16 == 0
        flat = torch.zeros(n * ROW + 8, dtype=d["rows"].dtype, device="cuda")
        off = flat[1:1 + n * ROW].view(n, ROW)
        off.copy_(d["rows"])
        assert off.data_ptr() % 16 == d["rows"].element_size()
        un = sim.encode_entities(off, d["params"], **kw)
        for k in ("features", "argmax"):
            assert torch.equal(_bits(un[k]), _bits(first[k])), (E, dtype, "unaligned", k)
        gu = sim.encode_entities_backward(off, d["params"], d["grad"], un["argmax"], embed_dim=E)["grad_params"]
        assert torch.equal(_bits(gu), _bits(g1))
        # only what is requested is written
        only = sim.encode_entities(d["rows"], d["params"], embed_dim=E, features=None, argmax=True)
        assert set(only) == {"argmax"} and torch.equal(only["argmax"], first["argmax"])
        assert set(sim.encode_entities(d["rows"], d["params"], embed_dim=E)) == {"features"}


def test_live_rows_into_a_rollout_buffer():
    import torch
    from gpu_hideseek import policy_inputs as P
    worlds, agents, T, E = 6, 6, 3, 64
    s = _sim(worlds, agents, seed=3)
    s.init()
    rows = worlds * agents
    x = H.inputs(rows, E, "float32")
    params = torch.from_numpy(np.array(x["params"])).cuda()
    actor, critic = torch.empty(rows, ROW, device="cuda"), torch.empty(rows, ROW, device="cuda")
    buf = torch.full((T, 2, rows, 4 * E), -7.0, device="cuda")
    hidden = 0
    for t in range(T):
        for _ in range(4):
            s.step()
        s.pack_policy_inputs(actor=actor, critic=critic)
        for i, r in enumerate((actor, critic)):
            out = s.encode_entities(r, params, embed_dim=E, features=buf[t, i], argmax=True)
            assert out["features"].data_ptr() == buf[t, i].data_ptr()
            _check_forward(out, dict(rows=r.cpu().numpy(), params=x["params"]), E, "float32", ("live", t, i))
        assert bool((buf[t + 1:] == -7).all())
        # the actor's rows are the critic's with the hidden entities zeroed: masking on the host gives the same features
        masked = critic.clone()
        for name, getter in P.MASKS.items():
            lo, hi, (NE, K) = P.LAYOUT[name]
            m = getattr(s, getter + "_tensor")().to_torch().reshape(rows, NE, 1).float()
            hidden += int((m == 0).sum())
            masked[:, lo:hi] = (masked[:, lo:hi].view(rows, NE, K) * m).view(rows, NE * K)
        host = s.encode_entities(masked, params, embed_dim=E)["features"]
        assert torch.equal(_bits(host), _bits(buf[t, 0]))
    assert hidden > 0, "no world with a hidden entity"
    s.close()


def test_the_module_trains(sim):
    import torch
    from gpu_hideseek import entity_encoder as N
    for E in (32, 64):
        n = H.SEPARATED_N
        x = H.separated(n, E)
        enc = N.EntityEncoder(E).cuda()
        assert [tuple(p.shape) for p in enc.parameters()] == [(PARAM_ROWS * E,)] and enc.params.dtype == torch.float32
        with torch.no_grad():
            enc.params.copy_(torch.from_numpy(x["params"]))
        rows, w = torch.from_numpy(x["rows"]).cuda(), torch.from_numpy(x["grad"]).cuda()
        feats = enc(sim, rows)
        assert feats.requires_grad and feats.shape == (n, 4 * E)
        loss = (feats * w).sum() + 0.5 * (feats ** 2).mean()
        loss.backward()
        fused = enc.params.grad.clone()
        ref = torch.from_numpy(x["params"]).cuda().requires_grad_()
        fe = N.eager(rows, ref, E)
        le = (fe * w).sum() + 0.5 * (fe ** 2).mean()
        le.backward()
        r64 = H.forward(np.float64, x["rows"], x["params"], E)
        assert (np.abs(_np(feats).astype(np.float64) - r64["features"]) <= H.feature_bound(r64["features"], E, "float32")).all()
        assert (np.abs(_np(fe).astype(np.float64) - r64["features"]) <= 4 * H.feature_bound(r64["features"], E, "float32")).all()
        # both gradients against the float64 restatement with the loss's own upstream gradient: the f32-vs-float64 gap of
        # the restatement on these inputs, 4 x for the kernel and 4 x more for eager's other order
        up = x["grad"].astype(np.float64) + r64["features"] / r64["features"].size
        g64 = H.backward(np.float64, x["rows"], x["params"], up, r64["argmax"], E)
        g32 = H.backward(np.float32, x["rows"], x["params"], up.astype(np.float32), r64["argmax"], E)
        for sl in H.table_slices(E):
            gap = float(np.abs(g32.astype(np.float64) - g64)[sl].max())
            ek, ee = float(np.abs(_np(fused) - g64)[sl].max()), float(np.abs(_np(ref.grad) - g64)[sl].max())
            print(f"E = {E}: module gradient: kernel {ek:.3e}, eager {ee:.3e} (f32-vs-f64 gap {gap:.3e})")
            assert ek <= 4 * gap and ee <= 16 * gap and gap < 1e-4 * float(np.abs(g64[sl]).max())
        opt = torch.optim.Adam(enc.parameters(), lr=1e-2)
        before = enc.params.detach().clone()
        opt.step()
        assert torch.isfinite(enc.params).all().item() and (enc.params != before).float().mean().item() > 0.9


def test_the_stream_form_the_shards_and_other_constants(sim):
    import gpu_hideseek
    import torch
    E, dtype = 64, "bfloat16"
    n = 3 * H.rows_per_block(E) + 2
    x = H.inputs(n, E, dtype)
    d = _dev(x, dtype)
    blocking = sim.encode_entities(d["rows"], d["params"], embed_dim=E, argmax=True)
    gb = sim.encode_entities_backward(d["rows"], d["params"], d["grad"], blocking["argmax"], embed_dim=E)["grad_params"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = sim.encode_entities(d["rows"], d["params"], embed_dim=E, argmax=True, stream=side)
    gs = sim.encode_entities_backward(d["rows"], d["params"], d["grad"], got["argmax"], embed_dim=E, stream=side.cuda_stream)["grad_params"]
    side.synchronize()
    for k in ("features", "argmax"):
        assert torch.equal(_bits(got[k]), _bits(blocking[k])), k
    assert torch.equal(_bits(gs), _bits(gb))
    kw = dict(sim_flags=0, rand_seed=0, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0, 0], 6, **kw)
    ss.init()
    cuts = [slice(0, 5), slice(5, 9), slice(9, n)]
    parts = [d["rows"][c].contiguous() for c in cuts]
    res = ss.encode_entities(parts, d["params"], embed_dim=E, argmax=True)
    assert len(res) == 3
    for r, c in zip(res, cuts):
        for k in ("features", "argmax"):
            assert torch.equal(_bits(r[k]), _bits(blocking[k][c])), k
    back = ss.encode_entities_backward(parts, [d["params"]] * 3, [d["grad"][c].contiguous() for c in cuts], [r["argmax"] for r in res], embed_dim=E)
    for b, p, c in zip(back, parts, cuts):
        one = sim.encode_entities_backward(p, d["params"], d["grad"][c].contiguous(), blocking["argmax"][c].contiguous(), embed_dim=E)["grad_params"]
        assert torch.equal(_bits(b["grad_params"]), _bits(one))
    ss.close()
    # other constants: within the tolerances of their own restatement (the derived ones: the same arithmetic, the same inputs)
    eps, slope = 1e-3, 0.2
    out = sim.encode_entities(d["rows"], d["params"], embed_dim=E, eps=eps, slope=slope, argmax=True)
    am = _check_forward(out, x, E, dtype, "eps, slope", eps, slope)
    assert not torch.equal(_bits(out["features"]), _bits(blocking["features"]))
    gp = sim.encode_entities_backward(d["rows"], d["params"], d["grad"], out["argmax"], embed_dim=E, eps=eps, slope=slope)["grad_params"]
    _check_backward(gp, x, am, (n, E, dtype), "eps, slope", eps, slope)


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import entity_encoder as N
    INVALID = 1
    n, E = 9, 64
    x = H.inputs(n, E, "float32")
    pad = 16
    rows = torch.zeros(n * ROW + pad, device="cuda")
    rows[:n * ROW] = torch.from_numpy(np.array(x["rows"])).reshape(-1)
    params = torch.zeros(PARAM_ROWS * E + pad, device="cuda")
    params[:PARAM_ROWS * E] = torch.from_numpy(np.array(x["params"]))
    grad = torch.zeros(n * 4 * E + pad, device="cuda")
    grad[:n * 4 * E] = torch.from_numpy(np.array(x["grad"])).reshape(-1)
    rows_h = torch.zeros(n * ROW + pad, dtype=torch.bfloat16, device="cuda")
    feat = torch.full((n * 4 * E + pad,), -7.0, device="cuda")
    feat_h = torch.full((n * 4 * E + pad,), -7.0, dtype=torch.float16, device="cuda")
    am = torch.full((n * 3 * E + pad,), 77, dtype=torch.uint8, device="cuda")
    gp = torch.full((PARAM_ROWS * E + pad,), -7.0, device="cuda")
    ins = (rows, params, grad)
    saved = [t.clone() for t in ins]

    def fwd(rows=rows.data_ptr(), params=params.data_ptr(), n=n, rdt=1, E=E, fdt=1, eps=1e-6, slope=0.01, features=feat.data_ptr(), argmax=am.data_ptr()):
        return N.HsEntityEncodeRequest(rows, params, n, rdt, E, fdt, eps, slope, features, argmax)

    def bwd(rows=rows.data_ptr(), params=params.data_ptr(), grad_features=grad.data_ptr(), argmax=am.data_ptr(), n=n, rdt=1, E=E, gdt=1, eps=1e-6,
            slope=0.01, grad_params=gp.data_ptr()):
        return N.HsEntityEncodeBackwardRequest(rows, params, grad_features, argmax, n, rdt, E, gdt, eps, slope, grad_params)

    def untouched():
        torch.cuda.synchronize()
        same = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(ins, saved))
        return same and all(bool((t == -7).all()) for t in (feat, feat_h, gp)) and bool((am == 77).all())

    def call(s, r, stream=False):
        fn = "hs_entity_encode_backward" if isinstance(r, N.HsEntityEncodeBackwardRequest) else "hs_entity_encode"
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
    for fn in ("hs_entity_encode", "hs_entity_encode_backward"):
        assert getattr(s._L, fn)(s._h, None) == INVALID and "null request" in message(s)
        assert getattr(s._L, fn + "_async")(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), None) == INVALID and "null request" in message(s)
    nan, inf = float("nan"), float("inf")
    bad = {}
    for name, make in (("forward", fwd), ("backward", bwd)):
        bad.update({
            (name, "null rows"): (make(rows=None), "null rows"), (name, "null params"): (make(params=None), "null params"),
            (name, "rows dtype"): (make(rdt=2), "dtype"), (name, "E 48"): (make(E=48), "embed_dim"), (name, "E 0"): (make(E=0), "embed_dim"),
            (name, "E 256"): (make(E=256), "embed_dim"), (name, "n 0"): (make(n=0), "n must"), (name, "n -1"): (make(n=-1), "n must"),
            (name, "n x 296"): (make(n=2 ** 23), "n must"), (name, "n x 4 E"): (make(n=2 ** 22, E=128), "n must"),
            (name, "eps nan"): (make(eps=nan), "eps and slope"), (name, "eps 0"): (make(eps=0.0), "eps and slope"),
            (name, "eps < 0"): (make(eps=-1e-6), "eps and slope"), (name, "eps inf"): (make(eps=inf), "eps and slope"),
            (name, "slope nan"): (make(slope=nan), "eps and slope"), (name, "slope inf"): (make(slope=-inf), "eps and slope"),
            (name, "rows +2"): (make(rows=rows.data_ptr() + 2), "aligned"), (name, "rows bf16 +1"): (make(rows=rows_h.data_ptr() + 1, rdt=3), "aligned"),
            (name, "params +2"): (make(params=params.data_ptr() + 2), "4-byte aligned"),
        })
    bad.update({
        "no output": (fwd(features=None, argmax=None), "every output is null"), "features dtype": (fwd(fdt=0), "dtype"),
        "features +2": (fwd(features=feat.data_ptr() + 2), "aligned"), "features f16 +1": (fwd(features=feat_h.data_ptr() + 1, fdt=4), "aligned"),
        "features is rows": (fwd(features=rows.data_ptr()), "features overlaps rows"),
        "features in params": (fwd(features=params.data_ptr() + 64), "features overlaps params"),
        "argmax in rows": (fwd(argmax=rows.data_ptr() + 3), "argmax overlaps rows"),
        "argmax in features": (fwd(argmax=feat.data_ptr() + 5), "argmax overlaps features"),
        "null grad_features": (bwd(grad_features=None), "null grad_features"), "null argmax": (bwd(argmax=None), "null argmax"),
        "null grad_params": (bwd(grad_params=None), "null grad_params"), "grad dtype": (bwd(gdt=9), "dtype"),
        "grad_features +2": (bwd(grad_features=grad.data_ptr() + 2), "aligned"), "grad_params +1": (bwd(grad_params=gp.data_ptr() + 1), "4-byte aligned"),
        "grad_params is params": (bwd(grad_params=params.data_ptr()), "grad_params overlaps params"),
        "grad_params in rows": (bwd(grad_params=rows.data_ptr() + 8), "grad_params overlaps rows"),
        "grad_params in grad_features": (bwd(grad_params=grad.data_ptr() + 4), "grad_params overlaps"),
        "grad_params on argmax": (bwd(grad_params=am.data_ptr()), "grad_params overlaps"),
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
    assert not untouched() and bool((feat[n * 4 * E:] == -7).all()) and bool((am[n * 3 * E:] == 77).all())
    want = H.forward(np.float32, x["rows"], x["params"], E)
    got = feat[:n * 4 * E].cpu().numpy().reshape(n, 4 * E).astype(np.float64)
    assert (np.abs(got - want["features"]) <= H.feature_bound(want["features"], E, "float32")).all()
    assert call(s, bwd()) == 0
    torch.cuda.synchronize()
    assert bool((gp[PARAM_ROWS * E:] == -7).all()) and not bool((gp[:PARAM_ROWS * E] == -7).any())
    _check_backward(gp[:PARAM_ROWS * E], x, am[:n * 3 * E].view(n, 3, E).cpu().numpy(), (n, E, "float32"), "C ABI")
    assert call(s, fwd(features=feat_h.data_ptr(), fdt=4, argmax=None)) == 0
    assert bool((feat_h[n * 4 * E:] == -7).all()) and not bool((feat_h[:n * 4 * E] == -7).any())
    s.close()
