"""The dynamic loss scale on the GPU (hs_ppo_loss_scaled, hs_twohot_value_scaled, hs_adam_step_scaled;
csrc/hs_k_loss_scale.h): with a power of two as the scale every entry point has the bits of its unscaled form (the loss
kernels with grad_scale = S on the host, the optimiser on the gradients without their 2^k); what float16 keeps of a
minibatch's gradient at S = 2^16 against the bound tests/test_loss_scale_host.py derives; the scaler's state against the
numpy rule over 24 calls with planted infinities and NaNs; and the refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import test_loss_scale_host as LS
import test_optim_host as A
import test_ppo_loss_host as PH
import test_value_head_host as VH
from test_gpu_optim import _dev, _same, _sim, _u
from test_gpu_ppo_loss import _bits, _call as _ppo_call, _dev as _ppo_dev
from test_gpu_value_head import _call as _twohot_call, _dev as _twohot_dev

pytestmark = pytest.mark.gpu

SCALES = (1.0, 2.0 ** -3, 2.0 ** 16)
INVALID = 1


@pytest.fixture(scope="module")
def sim():
    s = _sim()
    s.init()
    yield s
    s.close()


def _state(S, good=0.0, backoffs=0.0, growths=0.0):
    import torch
    return torch.tensor([S, good, backoffs, growths], dtype=torch.float64, device="cuda")


def _equal(a, b, tag):
    import torch
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), tag


# ---- 1. the loss kernels ----
@pytest.mark.parametrize("vmode", PH.VALUE_MODES)
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("dtype", PH.DTYPES)
def test_ppo_loss_scaled_has_the_bits_of_the_host_scale(sim, dtype, masked, vmode):
    for buckets in PH.BUCKETS:
        for n in PH.SIZES:
            d = _ppo_dev(PH.inputs(n, buckets, dtype, masked, vmode), dtype)
            one = _ppo_call(sim, d)
            for S in SCALES:
                state = _state(S, 5.0, 1.0, 2.0)
                want, got = _ppo_call(sim, d, grad_scale=S), _ppo_call(sim, d, loss_scale=state)
                assert set(got) == set(want)
                tag = (n, buckets, dtype, masked, vmode, S)
                _equal(got["grad_logits"], want["grad_logits"], tag)
                if vmode != "none":
                    _equal(got["grad_value"], want["grad_value"], tag)
                _equal(got["stats"], one["stats"], tag)
                assert state.tolist() == [S, 5.0, 1.0, 2.0], tag
                assert got["coefficients"]["grad_scale"] == 1.0


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("dtype", VH.DTYPES)
def test_twohot_value_scaled_has_the_bits_of_the_host_scale(sim, dtype, masked):
    for bins in VH.BINS:
        for n in VH.SIZES:
            d = _twohot_dev(VH.inputs(n, bins, dtype, masked), dtype)
            one = _twohot_call(sim, d)
            for S in SCALES:
                state = _state(S, 5.0, 1.0, 2.0)
                want, got = _twohot_call(sim, d, grad_scale=S), _twohot_call(sim, d, loss_scale=state)
                tag = (n, bins, dtype, masked, S)
                _equal(got["grad_logits"], want["grad_logits"], tag)
                _equal(got["value"], one["value"], tag)
                _equal(got["stats"], one["stats"], tag)
                assert state.tolist() == [S, 5.0, 1.0, 2.0], tag


# ---- 2. what float16 keeps ----
def test_float16_gradient_at_the_default_scale(sim):
    """n = 262 144 masked float16 samples at S = 2^16: the float16 gradient is the float32 gradient of the existing kernel
    times 2^16, rounded to nearest even, bit for bit; its relative L2 error is within the bound derived from the format
    and below that of the unscaled float16 call.  Expected from the CPU restatement: 2.1e-4 and 3.7 % flushed against
    6.6e-3 and 25.4 %."""
    import torch
    n, S = 262144, 2.0 ** 16
    d = _ppo_dev(PH.inputs(n, PH.BUCKETS[0], "float16", True, "none", 0, True), "float16")
    g32 = _ppo_call(sim, d, grad_dtype=torch.float32, stats=None)["grad_logits"]
    plain = _ppo_call(sim, d, stats=None)["grad_logits"]
    scaled = _ppo_call(sim, d, stats=None, loss_scale=_state(S))["grad_logits"]
    assert g32.dtype == torch.float32 and plain.dtype == scaled.dtype == torch.float16
    assert torch.isfinite(scaled).all().item()
    _equal(scaled, (g32 * S).to(torch.float16), "round to nearest even of 2^16 x the float32 gradient")
    g = g32.double()
    live = g != 0
    norm = g.pow(2).sum().sqrt().item()
    err = {k: ((x.double() / s - g).pow(2).sum().sqrt().item() / norm) for k, x, s in (("plain", plain, 1.0), ("scaled", scaled, S))}
    flushed = {k: ((x == 0) & live).sum().item() / live.sum().item() for k, x in (("plain", plain), ("scaled", scaled))}
    bound = LS.f16_bound(g32.cpu().numpy(), S)
    print(f"float16 grad_logits, n = {n}: relative L2 error {err['scaled']:.3g} at S = 2^16 (bound {bound:.3g}, {100 * flushed['scaled']:.1f} % flushed to 0) "
          f"against {err['plain']:.3g} unscaled ({100 * flushed['plain']:.1f} % flushed)")
    assert err["scaled"] <= bound and err["scaled"] < err["plain"]


# ---- 3. the optimiser ----
def _adam(sim, t, g, state, scale=None, **kw):
    return sim.adam_step(t["p"], g, t["m"], t["v"], state, loss_scale=scale, **kw)["stats"]


def _scale(state, **settings):
    """An optim.LossScale around a state tensor of the test's own."""
    from gpu_hideseek import optim
    ls = optim.LossScale("cuda", **dict(dict(init_scale=1.0, min_scale=2.0 ** -20, max_scale=2.0 ** 20), **settings))
    ls.state = state
    return ls


@pytest.mark.parametrize("n", A.SIZES + (A.POLICY_FLAT,))
def test_adam_step_scaled_has_the_bits_of_the_unscaled_step(sim, n):
    x = A.inputs(n)
    grads = [_dev(A.gradients(n, i, norm)) for i, norm in enumerate(A.ADAM_NORMS)]
    for kw in A.ADAM_CASES:
        for zero in (True, False):
            want = []
            t, state = {q: _dev(x[q]) for q in "pmv"}, _dev(A.fresh_state())
            for g in grads:
                gd = g.clone()
                st = _adam(sim, t, gd, state, zero_grad=zero, **kw)
                want.append(([t[q].clone() for q in "pmv"], state.clone(), st.clone(), gd))
            clips = [w[2][1].item() for w in want]
            assert any(c < 1 for c in clips) and any(c == 1 for c in clips), clips
            for k in (0, 7, 16):
                for again in range(2):
                    S = 2.0 ** k
                    t, state, ls = {q: _dev(x[q]) for q in "pmv"}, _dev(A.fresh_state()), _state(S)
                    scale = _scale(ls, growth_interval=2 ** 30)
                    for i, g in enumerate(grads):
                        gd = g * S
                        st = _adam(sim, t, gd, state, scale, zero_grad=zero, **kw)
                        tag = (n, kw["weight_decay"], zero, k, again, i)
                        for q, w in zip("pmv", want[i][0]):
                            _same(t[q], w, tag + (q,))
                        _same(state, want[i][1], tag + ("state",))
                        _same(st, want[i][2], tag + ("stats",))
                        _same(gd, want[i][3] * (1.0 if zero else S), tag + ("g",))
                        assert ls.tolist() == [S, i + 1.0, 0.0, 0.0], tag


# ---- 4. the scaler ----
def test_the_scaler_follows_the_rule_over_24_calls(sim):
    n = 1025
    settings = dict(growth=2.0, backoff=0.5, growth_interval=3, min_scale=2.0 ** -2, max_scale=2.0 ** 4)
    # 9 good calls: 4 -> 8 -> 16 -> 16 (the clamp, growths = 3); 7 bad ones: down to 1/4 and one more at the clamp; two
    # good ones and a bad one, which resets the run; then five good ones: one growth, two steps into the next run
    bad = {9: (0, np.inf), 10: (n - 1, np.nan), 11: (515, -np.inf), 12: (n - 1, np.inf), 13: (0, np.nan), 14: (515, np.inf), 15: (n - 1, -np.inf),
           18: (0, np.inf)}
    assert A.grid(n) == 2                                                 # element n - 1 is the short quad, workgroup 1's; 0 and 515 are workgroup 0's
    x = A.inputs(n)
    t, state, ls = {q: _dev(x[q]) for q in "pmv"}, _dev(A.fresh_state()), _state(4.0)
    scale = _scale(ls, **settings)
    ref, rstate, rls = {q: x[q] for q in "pmv"}, A.fresh_state(), LS.fresh(4.0)
    seen = []
    for i in range(24):
        g = (A.gradients(n, i, A.ADAM_NORMS[i % 5]) * np.float32(rls[0])).astype(np.float32)
        if i in bad:
            g[bad[i][0]] = bad[i][1]
        gd = _dev(g)
        before = {q: t[q].clone() for q in "pmv"}
        st = _adam(sim, t, gd, state, scale, **A.HYPER)
        out, rstate, rstats, rls = LS.scaled_step(np.float32, dict(ref, g=g), rstate, rls, settings, **A.HYPER)
        ref = {q: out[q] for q in "pmv"}
        for q in "pmv":
            _same(t[q], ref[q], (i, q))
        _same(state, rstate, (i, "adam state"))
        _same(st, rstats, (i, "stats"))
        _same(ls, rls, (i, "loss-scale state"))
        assert not _u(gd).any(), (i, "the gradients are zeroed")
        if i in bad:
            assert st[2].item() == 1 and all(np.array_equal(_u(t[q]), _u(before[q])) for q in "pmv"), i
        seen.append(rls[0])
    assert max(seen) == 16.0 and min(seen) == 0.25 and seen.count(16.0) >= 2 and seen.count(0.25) >= 2
    assert rls.tolist() == [0.5, 2.0, 8.0, 4.0] and rstate.tolist()[2:] == [16.0, 8.0]


def test_the_stream_form_updates_the_state_for_the_next_loss_call(sim):
    """On one stream, without a wait in between: a skipped step halves S, and the next scaled loss call reads the new S."""
    import torch
    n = 255
    x = A.inputs(n)
    t, state, ls = {q: _dev(x[q]) for q in "pmv"}, _dev(A.fresh_state()), _state(2.0 ** 16)
    g = np.array(A.gradients(n, 0, 20.0))
    g[7] = np.inf
    gd = _dev(g)
    d = _ppo_dev(PH.inputs(33, PH.BUCKETS[0], "float32", True, "none"), "float32")
    want = _ppo_call(sim, d, grad_scale=2.0 ** 15)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    from gpu_hideseek import optim
    scale = _scale(ls, max_scale=2.0 ** 20)
    sim.adam_step(t["p"], gd, t["m"], t["v"], state, loss_scale=scale, stream=side, **A.HYPER)
    got = _ppo_call(sim, d, loss_scale=ls, stream=side)
    side.synchronize()
    assert ls.tolist() == [2.0 ** 15, 0.0, 1.0, 0.0] and isinstance(scale, optim.LossScale)
    _equal(got["grad_logits"], want["grad_logits"], "the next loss call")


# ---- 5. the refusals of the C ABI ----
def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import optim, ppo_loss, value_head
    n = 37
    f64 = torch.float64
    d = _ppo_dev(PH.inputs(n, PH.BUCKETS[0], "float32", True, "value"), "float32")
    e = _twohot_dev(VH.inputs(n, VH.BINS[2], "float32", True), "float32")
    x = dict(A.inputs(n), g=A.gradients(n, 0, 20.0))
    arr = {q: _dev(x[q]) for q in "pgmv"}
    adam_state, adam_stats = _dev(A.fresh_state()), torch.full((4,), -7.0, dtype=f64, device="cuda")
    ls = torch.cat([_state(4.0), torch.full((4,), -7.0, dtype=f64, device="cuda")])
    outs = dict(gl=torch.full((n, 19), -7.0, device="cuda"), gv=torch.full((n,), -7.0, device="cuda"), st=torch.full((7,), -7.0, dtype=f64, device="cuda"),
                tgl=torch.full((n, 255), -7.0, device="cuda"), tv=torch.full((n,), -7.0, device="cuda"), tst=torch.full((6,), -7.0, dtype=f64, device="cuda"))
    _, ppo_req = ppo_loss.request(0, d["logits"], d["action"], d["old_log_prob"], d["advantage"], mask=d["mask"], value=d["value"], returns=d["returns"],
                                  grad_logits=outs["gl"], grad_value=outs["gv"], stats=outs["st"])
    _, two_req = value_head.request(0, e["logits"], e["returns"], mask=e["mask"], value=outs["tv"], grad_logits=outs["tgl"], stats=outs["tst"])
    _, adam_req = optim.request(0, arr["p"], arr["g"], arr["m"], arr["v"], adam_state, stats=adam_stats)
    everything = list(arr.values()) + [adam_state, adam_stats, ls] + list(outs.values())
    saved = [t.clone() for t in everything]
    P = lambda t: t.data_ptr()                                              # noqa: E731

    def untouched():
        torch.cuda.synchronize()
        return all(np.array_equal(_u(a), _u(b)) for a, b in zip(everything, saved))

    def message(s):
        return s._L.hs_last_error().decode()

    def call(s, fn, req, last, stream):
        r = None if req is None else C.byref(req)
        if stream:
            return getattr(s._L, fn + "_async")(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), r, last)
        return getattr(s._L, fn)(s._h, r, last)

    def scale(state=P(ls), growth=2.0, backoff=0.5, min_scale=1.0, max_scale=2.0 ** 24, growth_interval=2000, reserved=0):
        return optim.HsLossScale(state, growth, backoff, min_scale, max_scale, growth_interval, reserved)

    def refused(s, fn, req, last, msg, what):
        for stream in (False, True):
            assert call(s, fn, req, last, stream) == INVALID, (fn, what)
            assert msg in message(s), (fn, what, message(s))

    losses = (("hs_ppo_loss_scaled", ppo_req), ("hs_twohot_value_scaled", two_req))
    s = _sim(4, 4)
    for fn, req in losses:
        refused(s, fn, req, C.c_void_p(P(ls)), "before hs_init", "no init")
    refused(s, "hs_adam_step_scaled", adam_req, C.byref(scale()), "before hs_init", "no init")
    assert untouched()
    s.init()
    # what the unscaled entry points refuse
    for fn, req in losses:
        refused(s, fn, None, C.c_void_p(P(ls)), "null request", "null request")
    refused(s, "hs_adam_step_scaled", None, C.byref(scale()), "null request", "null request")
    r = ppo_loss.HsPpoRequest.from_buffer_copy(ppo_req)
    r.clip_coef = 0.0
    refused(s, "hs_ppo_loss_scaled", r, C.c_void_p(P(ls)), "clip_coef", "clip_coef 0")
    r = value_head.HsTwohotRequest.from_buffer_copy(two_req)
    r.bins = 1
    refused(s, "hs_twohot_value_scaled", r, C.c_void_p(P(ls)), "bins must", "bins 1")
    r = optim.HsAdamRequest.from_buffer_copy(adam_req)
    r.n = 0
    refused(s, "hs_adam_step_scaled", r, C.byref(scale()), "n must", "n 0")
    r = optim.HsAdamRequest.from_buffer_copy(adam_req)
    r.grads = r.params
    refused(s, "hs_adam_step_scaled", r, C.byref(scale()), "grads overlaps params", "grads is params")
    # the state pointer
    for fn, req in losses:
        refused(s, fn, req, None, "null loss_scale_state", "null state")
        refused(s, fn, req, C.c_void_p(P(ls) + 4), "8-byte aligned", "state + 4")
    for t, name in ((outs["gl"], "grad_logits"), (outs["gv"], "grad_value"), (outs["st"], "stats"), (d["logits"], "logits"), (d["advantage"], "advantage"),
                    (d["mask"], "mask"), (d["returns"], "returns")):
        refused(s, "hs_ppo_loss_scaled", ppo_req, C.c_void_p(P(t) + 8), f"loss_scale_state overlaps {name}", name)
    for t, name in ((outs["tgl"], "grad_logits"), (outs["tv"], "value"), (outs["tst"], "stats"), (e["logits"], "logits"), (e["returns"], "returns"), (e["mask"], "mask")):
        refused(s, "hs_twohot_value_scaled", two_req, C.c_void_p(P(t) + 8), f"loss_scale_state overlaps {name}", name)
    refused(s, "hs_adam_step_scaled", adam_req, None, "null loss scale", "null struct")
    refused(s, "hs_adam_step_scaled", adam_req, C.byref(scale(state=None)), "null loss_scale_state", "null state")
    refused(s, "hs_adam_step_scaled", adam_req, C.byref(scale(state=P(ls) + 4)), "8-byte aligned", "state + 4")
    for t, name in ((arr["p"], "params"), (arr["g"], "grads"), (arr["m"], "m"), (arr["v"], "v"), (adam_state, "state"), (adam_stats, "stats")):
        refused(s, "hs_adam_step_scaled", adam_req, C.byref(scale(state=P(t) + 8)), f"loss_scale_state overlaps {name}", name)
    # the factors and the bounds
    nan, inf = float("nan"), float("inf")
    bad = [(dict(growth=g), "growth must") for g in (0.5, 3.0, 0.0, -2.0, nan, inf, 2.0 ** 127)]
    bad += [(dict(backoff=b), "backoff must") for b in (2.0, 0.0, 0.3, -0.5, nan, inf)]
    bad += [(dict(min_scale=m), "min_scale and max_scale") for m in (0.0, -1.0, 3.0, nan, 2.0 ** 25)]
    bad += [(dict(max_scale=m), "min_scale and max_scale") for m in (0.5, 1000.0, 2.0 ** 127, inf, nan)]
    bad += [(dict(growth_interval=0), "growth_interval must"), (dict(growth_interval=-5), "growth_interval must"), (dict(reserved=1), "reserved must")]
    for kw, msg in bad:
        refused(s, "hs_adam_step_scaled", adam_req, C.byref(scale(**kw)), msg, kw)
    assert untouched()
    s.step_begin()
    for fn, req in losses:
        refused(s, fn, req, C.c_void_p(P(ls)), "open step", "open step")
    refused(s, "hs_adam_step_scaled", adam_req, C.byref(scale()), "open step", "open step")
    s.step_end()
    assert untouched()
    # the accepted calls write, and only their own ranges; the widest accepted settings pass
    for fn, req in losses:
        assert call(s, fn, req, C.c_void_p(P(ls)), False) == 0, message(s)
    assert call(s, "hs_adam_step_scaled", adam_req, C.byref(scale(growth=2.0 ** 126, backoff=2.0 ** -126, min_scale=2.0 ** -200, max_scale=2.0 ** 126, growth_interval=1)),
                True) == 0, message(s)
    torch.cuda.synchronize()
    assert all((t != -7).any().item() for t in outs.values()) and (adam_stats != -7).all().item()
    assert ls.tolist() == [2.0 ** 126, 0.0, 0.0, 1.0, -7.0, -7.0, -7.0, -7.0]         # one good step at growth_interval 1: min(4 x 2^126, max_scale)
    s.close()
