"""The attention core of the entity self-attention encoder on the GPU (sim.attend_entities / attend_entities_backward,
hs_entity_attend, csrc/hs_k_attend.h) against the numpy restatement of tests/test_entity_attention_host.py within the
tolerances derived there: one row, a partial round, one row past a round, ten workgroups and (forward only) past the
sweep; both widths and every dtype; the null mask; the stream form, the shards and the refusals of the C ABI; the
autograd face against eager(); AttentionEncoder fused against fused=False on packed rows of a stepped simulator; and bit
for bit: determinism, position independence, NaN and Inf in masked keys, +0 for masked keys and for a zero gradient, and
v_0 where only self is valid."""
import ctypes as C

import numpy as np
import pytest

import test_entity_attention_host as H
from test_entity_attention_host import BIG_FWD, DTYPES, EMBED_DIMS, HEADS, S, SIZES

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
    for k in ("qkv", "grad_out"):
        t[k] = t[k].to(dt)
    return t


def _np(t):
    return t.detach().float().cpu().numpy()


def _bits(t):
    import torch
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _fwd(sim, d, mask=True, **kw):
    return sim.attend_entities(d["qkv"], d["key_mask"] if mask else None, **kw)


def _bwd(sim, d, mask=True, **kw):
    return sim.attend_entities_backward(d["qkv"], d["key_mask"] if mask else None, d["grad_out"], **kw)


def _check(got, want, names, case, tag, mask=True):
    """Every output within its derived bound of the f32 restatement."""
    for k in names:
        g, w = _np(got[k]).astype(np.float64), want[k].astype(np.float64)
        err, limit = np.abs(g - w), H.bound(k, w, case, mask=mask)
        print(f"{tag}: {k}: largest |got - want| = {float(err.max()):.3e}, largest excess over the bound {float((err - limit).max()):.3e}, "
              f"{int((g != w).sum())} of {g.size} differ")
        assert g.shape == w.shape and np.isfinite(g).all() and (err <= limit).all(), (tag, k, float((err - limit).max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("embed", EMBED_DIMS)
def test_parity_with_the_restatement(sim, embed, dtype):
    import torch
    for n in SIZES:
        case = (n, embed, dtype)
        d = _dev(H.inputs(*case), dtype)
        for mask in (True, False):                                              # the key_mask, and the null-mask form
            want = H.both(case, mask)[0]
            out = _fwd(sim, d, mask)
            assert set(out) == {"out"} and out["out"].dtype == getattr(torch, dtype) and out["out"].shape == (n, S, embed)
            _check(out, want, ("out",), case, (case, mask), mask)
            res = _bwd(sim, d, mask)
            assert set(res) == {"grad_qkv"} and res["grad_qkv"].dtype == getattr(torch, dtype) and res["grad_qkv"].shape == (n, S, 3, HEADS, embed // HEADS)
            _check(res, want, ("grad_qkv",), case, (case, mask), mask)


def test_past_the_forward_sweep(sim):
    x = H.inputs(*BIG_FWD)
    _check(_fwd(sim, _dev(x, BIG_FWD[2])), H.both(BIG_FWD)[0], ("out",), BIG_FWD, BIG_FWD)


def test_mixed_dtypes(sim):
    """A narrow qkv with an f32 out, and an f32 qkv with a bf16 gradient: grad_qkv has grad_out's dtype."""
    import torch
    case = (5, 128, "bfloat16")
    x = H.inputs(*case)
    d = _dev(x, "bfloat16")
    out = _fwd(sim, d, out_dtype=torch.float32)["out"]
    want = H.both(case)[0]["out"].astype(np.float64)
    assert out.dtype == torch.float32 and float(np.abs(_np(out) - want).max()) <= H.tolerance(case)["out"]
    g = sim.attend_entities_backward(d["qkv"].float(), d["key_mask"], d["grad_out"])["grad_qkv"]
    assert g.dtype == torch.bfloat16 and torch.equal(_bits(g), _bits(_bwd(sim, d)["grad_qkv"]))          # bf16 values widen exactly


def test_determinism_and_position(sim):
    import torch
    for embed, dtype, n in ((64, "float32", 37), (128, "bfloat16", 37), (128, "float16", 37)):
        d = _dev(H.inputs(n, embed, dtype), dtype)
        first, again = _fwd(sim, d), _fwd(sim, d)
        assert torch.equal(_bits(first["out"]), _bits(again["out"])), (embed, dtype)
        g1, g2 = _bwd(sim, d), _bwd(sim, d)
        assert torch.equal(_bits(g1["grad_qkv"]), _bits(g2["grad_qkv"])), (embed, dtype)
        # a row at another index of a batch of another size: the same bits
        perm = torch.from_numpy(np.random.default_rng(3).permutation(n)).cuda()
        moved = {k: v[perm].contiguous() for k, v in d.items()}
        assert torch.equal(_bits(_fwd(sim, moved)["out"]), _bits(first["out"][perm])), (embed, dtype)
        assert torch.equal(_bits(_bwd(sim, moved)["grad_qkv"]), _bits(g1["grad_qkv"][perm])), (embed, dtype)
        sub = {k: v[4:7].contiguous() for k, v in d.items()}
        assert torch.equal(_bits(_fwd(sim, sub)["out"]), _bits(first["out"][4:7]))
        assert torch.equal(_bits(_bwd(sim, sub)["grad_qkv"]), _bits(g1["grad_qkv"][4:7]))


def test_masked_keys_special_rows_and_zero_gradients(sim):
    import torch
    for embed, dtype in ((64, "float32"), (128, "bfloat16"), (64, "float16")):
        n = 37
        x = H.inputs(n, embed, dtype)
        d = _dev(x, dtype)
        valid = torch.from_numpy(H.valid_keys(x["key_mask"], n)).cuda()
        gone = ~valid
        out, g = _fwd(sim, d)["out"], _bwd(sim, d)["grad_qkv"]
        # NaN and Inf in the masked keys' k and v: every output keeps its bits
        bad = d["qkv"].clone()
        bad[:, :, 1][gone] = float("nan")
        bad[:, :, 2][gone] = float("inf")
        db = dict(d, qkv=bad)
        assert torch.equal(_bits(_fwd(sim, db)["out"]), _bits(out)), (embed, dtype)
        gb = _bwd(sim, db)["grad_qkv"]
        assert torch.equal(_bits(gb), _bits(g)) and torch.isfinite(gb.float()).all().item(), (embed, dtype)
        # masked keys: dk and dv are +0; the valid keys' and the masked queries' gradients are not all zero
        assert not _bits(g)[:, :, 1:][gone].any().item() and bool((g[:, :, 1:][valid] != 0).any()) and bool((g[:, :, 0][gone] != 0).any())
        # only self valid (an all-zero mask row, and a row with byte 0 alone): out_i = v_0, bit for bit
        for row in (2, 3, 9, 10):
            assert int(valid[row].sum()) == 1
            v0 = d["qkv"][row, 0, 2].reshape(embed)
            assert torch.equal(_bits(out[row]), _bits(v0.expand(S, embed))), (embed, dtype, row)
        # a zero grad_out: grad_qkv all +0
        z = _bwd(sim, dict(d, grad_out=torch.zeros_like(d["grad_out"])), grad_qkv=torch.full_like(d["qkv"], -7.0))["grad_qkv"]
        assert not _bits(z).any().item(), (embed, dtype)
        # a preallocated slot of a larger buffer is written, its neighbours are not
        buf = torch.full((3, n, S, embed), -7.0, dtype=out.dtype, device="cuda")
        _fwd(sim, d, out=buf[1])
        assert torch.equal(_bits(buf[1]), _bits(out)) and bool((buf[0] == -7).all()) and bool((buf[2] == -7).all())


def test_the_stream_form_and_the_shards(sim):
    import gpu_hideseek
    import torch
    embed, dtype, n = 128, "bfloat16", 14
    d = _dev(H.inputs(n, embed, dtype), dtype)
    blocking, gb = _fwd(sim, d), _bwd(sim, d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = _fwd(sim, d, stream=side)
    gs = _bwd(sim, d, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(_bits(got["out"]), _bits(blocking["out"])) and torch.equal(_bits(gs["grad_qkv"]), _bits(gb["grad_qkv"]))
    kw = dict(sim_flags=0, rand_seed=0, min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
    ss = gpu_hideseek.ShardedSimulator([0, 0, 0], 6, **kw)
    ss.init()
    cuts = [slice(0, 5), slice(5, 9), slice(9, n)]
    part = lambda k: [d[k][c].contiguous() for c in cuts]                   # noqa: E731
    res = ss.attend_entities(part("qkv"), part("key_mask"))
    assert len(res) == 3
    for r, c in zip(res, cuts):
        assert torch.equal(_bits(r["out"]), _bits(blocking["out"][c]))
    back = ss.attend_entities_backward(part("qkv"), part("key_mask"), part("grad_out"))
    for b, c in zip(back, cuts):
        assert torch.equal(_bits(b["grad_qkv"]), _bits(gb["grad_qkv"][c]))
    full = ss.attend_entities(part("qkv"))                                  # key_mask None for every shard
    assert torch.equal(_bits(full[1]["out"]), _bits(_fwd(sim, d, False)["out"][cuts[1]]))
    ss.close()


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import entity_attention as A
    INVALID = 1
    n, embed = 9, 64
    case = (n, embed, "float32")
    x = H.inputs(37, embed, "float32")
    x = {k: v[:n] for k, v in x.items()}
    pad = 16

    def padded(a, dtype=torch.float32, fill=None):
        a = np.array(a)
        t = torch.zeros(a.size + pad, dtype=dtype, device="cuda") if fill is None else torch.full((a.size + pad,), fill, dtype=dtype, device="cuda")
        if fill is None:
            t[:a.size] = torch.from_numpy(a).reshape(-1).to(dtype)
        return t
    nq, no = n * S * 3 * embed, n * S * embed
    qkv, mask, go = padded(x["qkv"]), padded(x["key_mask"], torch.uint8), padded(x["grad_out"])
    q_h = torch.zeros(nq + pad, dtype=torch.bfloat16, device="cuda")
    out, gq = padded(np.zeros(no), fill=-7.0), padded(np.zeros(nq), fill=-7.0)
    ins, outs = (qkv, mask, go), (out, gq)
    saved = [t.clone() for t in ins]
    P = lambda t: t.data_ptr()                                              # noqa: E731
    assert all(P(t) % 16 == 0 for t in ins + outs + (q_h,))

    def fwd(qkv=P(qkv), key_mask=P(mask), n=n, embed=embed, qdt=1, odt=1, out=P(out)):
        return A.HsEntityAttendRequest(qkv, key_mask, n, embed, qdt, odt, out)

    def bwd(qkv=P(qkv), key_mask=P(mask), grad_out=P(go), n=n, embed=embed, qdt=1, gdt=1, grad_qkv=P(gq)):
        return A.HsEntityAttendBackwardRequest(qkv, key_mask, grad_out, n, embed, qdt, gdt, grad_qkv)

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip(ins, saved)) and all(bool((t == -7).all()) for t in outs)

    def call(s, r, stream=False):
        fn = "hs_entity_attend_backward" if isinstance(r, A.HsEntityAttendBackwardRequest) else "hs_entity_attend"
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
    for fn in ("hs_entity_attend", "hs_entity_attend_backward"):
        assert getattr(s._L, fn)(s._h, None) == INVALID and "null request" in message(s)
        assert getattr(s._L, fn + "_async")(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), None) == INVALID and "null request" in message(s)
    bad = {}
    for name, make in (("forward", fwd), ("backward", bwd)):
        bad.update({
            (name, "null qkv"): (make(qkv=None), "null qkv"), (name, "qkv dtype"): (make(qdt=2), "qkv dtype"),
            (name, "E 32"): (make(embed=32), "embed_dim must"), (name, "E 0"): (make(embed=0), "embed_dim must"), (name, "E 96"): (make(embed=96), "embed_dim must"),
            (name, "E 256"): (make(embed=256), "embed_dim must"), (name, "n 0"): (make(n=0), "n must"), (name, "n -1"): (make(n=-1), "n must"),
            (name, "n 2^24"): (make(n=1 << 24), "n must"),
            (name, "qkv +4"): (make(qkv=P(qkv) + 4), "qkv must be 16-byte aligned"), (name, "qkv bf16 +2"): (make(qkv=P(q_h) + 2, qdt=3), "qkv must be 16-byte aligned"),
        })
    bad.update({
        "no output": (fwd(out=None), "null out"), "out dtype": (fwd(odt=0), "out dtype"), "out dtype 5": (fwd(odt=5), "out dtype"),
        "out +8": (fwd(out=P(out) + 8), "16-byte aligned"), "out is qkv": (fwd(out=P(qkv)), "out overlaps qkv"), "out in qkv": (fwd(out=P(qkv) + 64), "out overlaps qkv"),
        "out on key_mask": (fwd(out=P(mask)), "out overlaps key_mask"),
        "null grad_out": (bwd(grad_out=None), "null grad_out"), "null grad_qkv": (bwd(grad_qkv=None), "null grad_qkv"), "grad dtype": (bwd(gdt=2), "grad dtype"),
        "grad_out +8": (bwd(grad_out=P(go) + 8), "16-byte aligned"), "grad_qkv +4": (bwd(grad_qkv=P(gq) + 4), "16-byte aligned"),
        "grad_qkv is qkv": (bwd(grad_qkv=P(qkv)), "grad_qkv overlaps qkv"), "grad_qkv in grad_out": (bwd(grad_qkv=P(go) + 16), "grad_qkv overlaps grad_out"),
        "grad_qkv on key_mask": (bwd(grad_qkv=P(mask)), "grad_qkv overlaps key_mask"),
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
    assert call(s, fwd()) == 0 and call(s, bwd()) == 0                       # the calls do write, and only their own ranges
    torch.cuda.synchronize()
    want = H.run(np.float32, x)
    tol = {k: 4.0 * v for k, v in H.gaps(want, H.run(np.float64, x)).items()}
    for t, k, size in ((out, "out", no), (gq, "grad_qkv", nq)):
        assert bool((t[size:] == -7).all()) and not bool((t[:size] == -7).any()), k
        err = np.abs(_np(t[:size]).reshape(want[k].shape).astype(np.float64) - want[k])
        assert float(err.max()) <= tol[k], (k, float(err.max()), tol[k])
    assert call(s, fwd(key_mask=None)) == 0 and call(s, bwd(key_mask=None)) == 0           # the null mask is no fault
    s.close()


def test_autograd_against_eager(sim):
    """entity_attention.attend under autograd: the kernels against eager() in float32 on the device, both within the
    derived bound of the float64 restatement."""
    import torch
    from gpu_hideseek import entity_attention as A
    for embed in EMBED_DIMS:
        case = (37, embed, "float32")
        d = _dev(H.inputs(*case))
        r64 = H.both(case)[1]
        for fused in (True, False):
            qkv = d["qkv"].clone().requires_grad_()
            out = A.attend(sim, qkv, d["key_mask"], fused)
            assert out.requires_grad and out.shape == (37, S, embed)
            (out * d["grad_out"]).sum().backward()
            for k, t in (("out", out), ("grad_qkv", qkv.grad)):
                err = np.abs(_np(t).astype(np.float64) - r64[k])
                print(f"attend, E = {embed}, fused {fused}: {k}: largest |got - float64| = {float(err.max()):.3e}")
                assert (err <= (1.0 if fused else 4.0) * H.bound(k, r64[k], case)).all(), (embed, fused, k)      # eager: another order, as on the host
    # bf16 through the face: out and the gradient in bf16
    qb = d["qkv"].bfloat16().requires_grad_()
    ob = A.attend(sim, qb, None)
    ob.float().sum().backward()
    assert ob.dtype == torch.bfloat16 and qb.grad.dtype == torch.bfloat16 and torch.isfinite(qb.grad.float()).all().item()


@pytest.fixture(scope="module")
def packed_rows():
    """37 actor rows and 37 critic rows packed from a stepped 6 x 6 simulator: the 36 of one step and one of the next."""
    import torch
    s = _sim(seed=3)
    s.init()
    for _ in range(30):
        s.step()
    a, c = torch.empty(2, 36, 296, device="cuda"), torch.empty(2, 36, 296, device="cuda")
    for t in range(2):
        s.step()
        s.pack_policy_inputs(actor=a[t], critic=c[t])
    actor, critic = (torch.cat([r[0], r[1, 17:18]]).cpu().numpy() for r in (a, c))
    s.close()
    return actor, critic


@pytest.mark.parametrize("masked", (True, False))
def test_encoder_fused_against_eager(sim, packed_rows, masked):
    """AttentionEncoder fused against fused=False in the features and every parameter's gradient, both within 4 x
    |float32 eager - float64 eager| (on the CPU, the same rows and parameters) of the float64 result: the rule of
    tests/test_gpu_policy.py."""
    import torch
    rows = packed_rows[0 if masked else 1]
    n = rows.shape[0]
    assert n == 37 == H.ENCODER["n"]
    if masked:
        gone = 1.0 - H.encoder_net(False).key_mask(torch.from_numpy(rows)).float().mean().item()
        assert 0.02 < gone < 0.98, gone                                          # some entities are invisible, some are not
    weight = np.random.default_rng([H.SEED, 8]).standard_normal((n, H.ENCODER["out"])).astype(np.float32)
    allow, f64 = H.encoder_allowance(rows, weight, masked)
    assert all(np.abs(v).max() > 0 for v in f64.values()), "every parameter has a gradient"
    fused = H.encoder_net(True, "cuda")
    f = fused(sim, torch.from_numpy(rows).cuda(), torch.float32, masked)
    assert f.shape == (n, H.ENCODER["out"]) and f.requires_grad
    (f * torch.from_numpy(weight).cuda()).sum().add(0.5 * (f ** 2).mean()).backward()
    got = {"features": f}
    got.update({k: p.grad for k, p in fused.named_parameters()})
    eager = H.encoder_eager(torch.float32, rows, weight, "cuda", masked)
    assert set(got) == set(eager) == set(f64)
    for k in f64:
        ef, ee = float(np.abs(_np(got[k]).astype(np.float64) - f64[k]).max()), float(np.abs(eager[k] - f64[k]).max())
        print(f"encoder, masked {masked}: {k}: fused {ef:.3e}, eager on the device {ee:.3e} from float64 (allowance {allow[k]:.3e}, "
              f"largest value {float(np.abs(f64[k]).max()):.3e})")
    for k in f64:
        assert float(np.abs(_np(got[k]).astype(np.float64) - f64[k]).max()) <= allow[k], ("fused", k)
        assert float(np.abs(eager[k] - f64[k]).max()) <= allow[k], ("eager on the device", k)
