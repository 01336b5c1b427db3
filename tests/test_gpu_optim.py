"""The optimiser on the GPU (sim.adam_step, hs_adam_step, csrc/hs_k_adam.h; gpu_hideseek.optim) against the numpy
restatement of tests/test_optim_host.py, bit for bit: p, m, v, the zeroed gradients, the state and the statistics over
three consecutive steps at one element, a full and a short quad, idle lanes, two workgroups and a second grid-stride trip
with a ragged tail, with the clip active, inactive and off, with and without weight decay and with a loss scale;
determinism, position independence and guard elements; non-finite gradients; only the requested outputs; the stream
form; the refusals of the C ABI; and optim.Adam over the policy's parameters against the restatement and against
clip_grad_norm_ + torch.optim.Adam within the tolerance the host file derives."""
import copy
import ctypes as C

import numpy as np
import pytest

import test_optim_host as H
from test_optim_host import HYPER, SIZES

pytestmark = pytest.mark.gpu

GUARD = 64


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


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _u(a):
    """The bits of a float array (numpy or torch) as unsigned integers of its width."""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, tag):
    g, w = _u(got), _u(want)
    assert g.shape == w.shape and np.array_equal(g, w), (tag, int((g != w).sum()), g.size)


def _start(n):
    x = H.inputs(n)
    return {k: _dev(x[k]) for k in "pmv"}, _dev(H.fresh_state())


def _compare(t, g, state, stats, want, tag):
    res, new, st, _ = want
    for k in "pmv":
        _same(t[k], res[k], tag + (k,))
    _same(g, res["g"], tag + ("g",))
    _same(state, new, tag + ("state",))
    _same(stats, st, tag + ("stats",))


@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_restatement(sim, n):
    for config, kw in H.CONFIGS.items():
        kw = {k: v for k, v in kw.items() if k != "norm"}
        want = H.run(np.float32, n, config, steps=3)
        t, state = _start(n)
        for k, w in enumerate(want):
            g = _dev(w[3])
            out = sim.adam_step(t["p"], g, t["m"], t["v"], state, **kw)
            assert set(out) == {"stats"} and out["stats"].shape == (4,)
            _compare(t, g, state, out["stats"], w, (n, config, k))
            st = out["stats"].cpu().numpy()
            print(f"n = {n}, {config}, step {k + 1}: gnorm {st[0]:.6g}, clip {st[1]:.6g}, skipped {st[2]:.0f}, t {st[3]:.0f}")
        clips = [float(w[2][1]) for w in want]
        assert all(c < 1 for c in clips) if config.startswith("active") else all(c == 1 for c in clips), (config, clips)
        assert float(want[-1][1][2]) == 3 and float(want[-1][1][3]) == 0


def test_determinism_and_position(sim):
    import torch
    n, config = 1025, "active, decay"
    kw = {k: v for k, v in H.CONFIGS[config].items() if k != "norm"}
    want = H.run(np.float32, n, config, steps=1)[0]

    def aligned():
        t, state = _start(n)
        g = _dev(want[3])
        out = sim.adam_step(t["p"], g, t["m"], t["v"], state, **kw)
        return t, g, state, out["stats"]
    first, again = aligned(), aligned()
    _compare(*first, want, (n, config, "first"))
    _compare(*again, want, (n, config, "again"))
    # every array 16 bytes into a 256-byte line, with 64 guard elements on either side
    x = H.inputs(n)

    def placed(a, lead):
        a = np.asarray(a)
        raw = torch.full((lead + GUARD + a.size + GUARD,), -7.0, dtype=getattr(torch, str(a.dtype)), device="cuda")
        view = raw[lead + GUARD:lead + GUARD + a.size]
        view.copy_(_dev(a))
        return raw, view
    bufs = {k: placed(a, 4) for k, a in (("p", x["p"]), ("g", want[3]), ("m", x["m"]), ("v", x["v"]))}
    bufs["state"], bufs["stats"] = placed(H.fresh_state(), 2), placed(np.zeros(4), 2)
    for k, (raw, view) in bufs.items():
        assert raw.data_ptr() % 256 == 0 and view.data_ptr() % 256 == 16 and view.data_ptr() % 16 == 0, k
    v = {k: b[1] for k, b in bufs.items()}
    out = sim.adam_step(v["p"], v["g"], v["m"], v["v"], v["state"], stats=v["stats"], **kw)
    assert out["stats"].data_ptr() == v["stats"].data_ptr()
    _compare(v, v["g"], v["state"], v["stats"], want, (n, config, "16 bytes into a line"))
    for k, (raw, view) in bufs.items():
        lead = 4 if raw.dtype == torch.float32 else 2
        assert bool((raw[:lead + GUARD] == -7).all()) and bool((raw[lead + GUARD + view.numel():] == -7).all()), k


def test_non_finite_gradients(sim):
    n = 1025
    x = dict(H.inputs(n), g=H.gradients(n, 0, 20.0))
    warm, wstate, _ = H.step(np.float32, x, H.fresh_state(), **HYPER)
    cases = (("inf", np.inf, 1.0, 20.0), ("nan", np.nan, 1.0, 20.0), ("the norm overflows through grad_scale alone", None, 1e300, 1e32))
    for name, bad, scale, norm in cases:
        for zero in (True, False):
            t, state = {k: _dev(warm[k]) for k in "pmv"}, _dev(wstate)
            g = np.array(H.gradients(n, 1, norm))
            if bad is not None:
                g[77] = bad
            assert np.isfinite(H.sum_squares(g)[0]) == (bad is None)
            gd = _dev(g)
            kw = dict(HYPER, grad_scale=scale, zero_grad=zero)
            out = sim.adam_step(t["p"], gd, t["m"], t["v"], state, **kw)
            want = H.step(np.float32, dict(warm, g=g), wstate, **kw)
            _compare(t, gd, state, out["stats"], want + (g,), (name, zero))
            for k in "pmv":                                                   # said again without the restatement: nothing moved
                _same(t[k], warm[k], (name, zero, k))
            st, s = out["stats"].cpu().numpy(), state.cpu().numpy()
            assert st[2] == 1 and st[3] == 1 and not np.isfinite(st[0]) and s.tolist() == [wstate[0], wstate[1], 1.0, 1.0]
            assert (not _u(gd).any()) if zero else np.array_equal(_u(gd), _u(g))
            # the next finite step is the restatement's, from the state with one skip
            g2 = H.gradients(n, 2, 20.0)
            gd2 = _dev(g2)
            out = sim.adam_step(t["p"], gd2, t["m"], t["v"], state, **HYPER)
            nxt = H.step(np.float32, dict(warm, g=g2), want[1], **HYPER)
            _compare(t, gd2, state, out["stats"], nxt + (g2,), (name, zero, "next"))
            assert state.cpu().numpy().tolist()[2:] == [2.0, 1.0]


def test_only_what_is_requested_is_written(sim):
    n = 255
    config = "inactive, decay"
    kw = {k: v for k, v in H.CONFIGS[config].items() if k != "norm"}
    want = H.run(np.float32, n, config, steps=1)[0]
    t, state = _start(n)
    g = _dev(want[3])
    out = sim.adam_step(t["p"], g, t["m"], t["v"], state, zero_grad=False, stats=None, **kw)
    assert out == {}
    for k in "pmv":
        _same(t[k], want[0][k], k)
    _same(g, want[3], "the gradients stay")
    _same(state, want[1], "state")
    assert _u(g).any()


def test_the_stream_form(sim):
    import torch
    n, config = SIZES[-1], "active"
    kw = {k: v for k, v in H.CONFIGS[config].items() if k != "norm"}
    want = H.run(np.float32, n, config, steps=1)[0]
    t, state = _start(n)
    g = _dev(want[3])
    stats = torch.zeros(4, dtype=torch.float64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = sim.adam_step(t["p"], g, t["m"], t["v"], state, stats=stats, stream=side, **kw)
    side.synchronize()
    _compare(t, g, state, out["stats"], want, (n, config, "side stream"))
    t2, state2 = _start(n)
    g2 = _dev(want[3])
    sim.adam_step(t2["p"], g2, t2["m"], t2["v"], state2, stats=stats, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    _compare(t2, g2, state2, stats, want, (n, config, "raw handle"))


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import optim
    INVALID = 1
    n = 37
    x = dict(H.inputs(n), g=H.gradients(n, 0, 20.0))
    pad = 16
    arr = {k: torch.cat([_dev(x[k]), torch.full((pad,), -7.0, device="cuda")]) for k in "pgmv"}
    state = torch.cat([_dev(H.fresh_state()), torch.full((4,), -7.0, dtype=torch.float64, device="cuda")])
    stats = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    everything = list(arr.values()) + [state, stats]
    saved = [t.clone() for t in everything]
    P = lambda t: t.data_ptr()                                              # noqa: E731
    assert all(P(t) % 16 == 0 for t in everything)

    def req(params=P(arr["p"]), grads=P(arr["g"]), m=P(arr["m"]), v=P(arr["v"]), n=n, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
            max_grad_norm=5.0, grad_scale=1.0, zero_grad=1, state=P(state), stats=P(stats)):
        return optim.HsAdamRequest(params, grads, m, v, n, lr, beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale, zero_grad, state, stats)

    def untouched():
        torch.cuda.synchronize()
        return all(np.array_equal(_u(a), _u(b)) for a, b in zip(everything, saved))

    def call(s, r, stream=False):
        if stream:
            return s._L.hs_adam_step_async(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(r))
        return s._L.hs_adam_step(s._h, C.byref(r))

    def message(s):
        return s._L.hs_last_error().decode()

    s = _sim(4, 4)
    for stream in (False, True):
        assert call(s, req(), stream) == INVALID and "before hs_init" in message(s)
    assert untouched()
    s.init()
    assert s._L.hs_adam_step(s._h, None) == INVALID and "null request" in message(s)
    assert s._L.hs_adam_step_async(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), None) == INVALID and "null request" in message(s)
    nan, inf = float("nan"), float("inf")
    bad = {
        "null params": (req(params=None), "null params"), "null grads": (req(grads=None), "null grads"), "null m": (req(m=None), "null m"),
        "null v": (req(v=None), "null v"), "null state": (req(state=None), "null state"),
        "n 0": (req(n=0), "n must"), "n -1": (req(n=-1), "n must"), "n 2^31": (req(n=2 ** 31), "n must"), "n 2^40": (req(n=2 ** 40), "n must"),
        "params +4": (req(params=P(arr["p"]) + 4), "16-byte aligned"), "grads +8": (req(grads=P(arr["g"]) + 8), "16-byte aligned"),
        "m +4": (req(m=P(arr["m"]) + 4), "16-byte aligned"), "v +12": (req(v=P(arr["v"]) + 12), "16-byte aligned"),
        "state +4": (req(state=P(state) + 4), "8-byte aligned"), "stats +4": (req(stats=P(stats) + 4), "8-byte aligned"),
        "lr nan": (req(lr=nan), "must be finite"), "lr inf": (req(lr=inf), "must be finite"), "eps nan": (req(eps=nan), "must be finite"),
        "eps inf": (req(eps=inf), "must be finite"), "weight_decay nan": (req(weight_decay=nan), "must be finite"),
        "weight_decay inf": (req(weight_decay=inf), "must be finite"), "grad_scale nan": (req(grad_scale=nan), "must be finite"),
        "grad_scale inf": (req(grad_scale=inf), "must be finite"), "max_grad_norm nan": (req(max_grad_norm=nan), "must be finite"),
        "max_grad_norm inf": (req(max_grad_norm=inf), "must be finite"), "max_grad_norm -inf": (req(max_grad_norm=-inf), "must be finite"),
        "eps 0": (req(eps=0.0), "eps must"), "eps < 0": (req(eps=-1e-8), "eps must"), "lr < 0": (req(lr=-1e-4), "lr must"),
        "weight_decay < 0": (req(weight_decay=-0.01), "weight_decay must"), "grad_scale 0": (req(grad_scale=0.0), "grad_scale must"),
        "grad_scale < 0": (req(grad_scale=-1.0), "grad_scale must"),
        "beta1 1": (req(beta1=1.0), "beta1 and beta2"), "beta1 < 0": (req(beta1=-0.1), "beta1 and beta2"), "beta1 nan": (req(beta1=nan), "beta1 and beta2"),
        "beta2 1": (req(beta2=1.0), "beta1 and beta2"), "beta2 1.5": (req(beta2=1.5), "beta1 and beta2"), "beta2 nan": (req(beta2=nan), "beta1 and beta2"),
        "grads is params": (req(grads=P(arr["p"])), "grads overlaps params"), "m in params": (req(m=P(arr["p"]) + 16), "m overlaps params"),
        "v is m": (req(v=P(arr["m"])), "v overlaps m"), "v in grads": (req(v=P(arr["g"]) + 32), "v overlaps grads"),
        "state in v": (req(state=P(arr["v"]) + 16), "state overlaps v"), "stats in state": (req(stats=P(state) + 16), "stats overlaps state"),
        "stats in params": (req(stats=P(arr["p"])), "stats overlaps params"),
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
    # the call does write, and only its own ranges; max_grad_norm <= 0 and a null stats are accepted
    want = H.step(np.float32, x, H.fresh_state(), **HYPER)
    assert call(s, req()) == 0
    torch.cuda.synchronize()
    for k in "pgmv":
        _same(arr[k][:n], want[0][k], ("C ABI", k))
        assert bool((arr[k][n:] == -7).all()), k
    _same(state[:4], want[1], "state")
    _same(stats[:4], want[2], "stats")
    assert bool((state[4:] == -7).all()) and bool((stats[4:] == -7).all())
    assert call(s, req(max_grad_norm=-1.0, stats=None, zero_grad=0)) == 0
    torch.cuda.synchronize()
    assert bool((stats[4:] == -7).all()) and state[:4].cpu().tolist()[2:] == [2.0, 0.0]
    s.close()


# ---- the module ----
ROWS, T = 8, 4


def test_the_module_over_the_policy():
    """optim.Adam over policy.make_policy(torch.float32) on R = 8 rows, T = 4: each of five steps against the restatement
    on the gradients backward left in the flat buffer, bit for bit; against a deep copy trained by clip_grad_norm_ +
    torch.optim.Adam on the same gradients within the host file's TOL["p"] (derived for |p| <= P_MAX, asserted here: what
    differs is the order of a handful of f32 operations per step, clip_grad_norm_'s 1e-6 in the clip factor and torch's
    foreach sum of squares); the objective falls; the gradients are +0 after every step; the state round trip."""
    import torch
    from gpu_hideseek import optim, policy as P, ppo_loss, value_head
    sim = _sim(2, 4, seed=3)
    sim.init()
    actor, critic = torch.empty(T, ROWS, 296, device="cuda"), torch.empty(T, ROWS, 296, device="cuda")
    clears = torch.empty(T, ROWS, dtype=torch.int32, device="cuda")
    for t in range(T):
        sim.step()
        sim.pack_policy_inputs(actor=actor[t], critic=critic[t])
        clears[t] = sim.done_tensor().to_torch().reshape(ROWS)
    net = P.make_policy(torch.float32, generator=torch.Generator().manual_seed(41))
    with torch.no_grad():
        net.critic_head.weight.copy_(0.05 * torch.randn(net.critic_head.weight.shape, generator=torch.Generator().manual_seed(42)))
    net = net.cuda()
    twin = copy.deepcopy(net)
    lr = 3e-4                                                   # as the policy's own test of five Adam steps
    hyper = dict(HYPER, lr=lr)
    opt = optim.Adam(sim, net.named_parameters(), lr=lr, max_grad_norm=5)
    opt2 = torch.optim.Adam(twin.parameters(), lr=lr)
    lay = opt.layout()
    assert len(lay) == 24 and opt.flat.params.numel() == H.POLICY_FLAT and opt.flat.params.is_cuda and opt.flat.detached() is None
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == 24
    n = T * ROWS
    state0 = net.init_state(ROWS, "cuda")
    with torch.no_grad():
        logits, _, _ = net.sequence(sim, actor, critic, state0, clears)
    action = torch.empty(T, ROWS, 5, dtype=torch.int32, device="cuda")
    old_log_prob = torch.empty(T, ROWS, device="cuda")
    for t in range(T):
        sim.sample_actions(logits[t].contiguous(), seed=(5, 6), counter=t, action=action[t], log_prob=old_log_prob[t])
    g = torch.Generator().manual_seed(43)
    advantage, returns = torch.randn(n, generator=g).cuda(), (2.0 * torch.randn(n, generator=g)).cuda()
    losses, kept = [], None
    for k in range(5):
        logits, critic_logits, _ = net.sequence(sim, actor, critic, state0, clears)
        logits, critic_logits = logits.reshape(n, 19), critic_logits.reshape(n, 255)
        pol = sim.ppo_loss(logits.detach(), action.view(n, 5), old_log_prob.view(n), advantage)
        val = sim.value_head(critic_logits.detach(), returns, loss_coef=0.5)
        loss = ppo_loss.attach(logits, None, pol) + value_head.attach(critic_logits, val)
        loss.backward()
        assert opt.flat.detached() is None
        before = {"p": opt.flat.params, "g": opt.flat.grads, "m": opt.m, "v": opt.v}
        before = {q: a.detach().cpu().numpy().copy() for q, a in before.items()}
        sbefore = opt.adam_state.cpu().numpy().copy()
        assert before["g"].any() and float(np.abs(before["p"]).max()) <= H.P_MAX
        kept = before["g"] if kept is None else kept
        for name, p in twin.named_parameters():
            lo, hi, shape = lay[name]
            p.grad = torch.from_numpy(before["g"][lo:hi].reshape(shape).copy()).cuda()
        stats = opt.step()
        want, wstate, wstats = H.step(np.float32, before, sbefore, **hyper)
        for q, a in (("p", opt.flat.params), ("m", opt.m), ("v", opt.v)):
            _same(a, want[q], ("module", k, q))
        _same(opt.adam_state, wstate, ("module", k, "state"))
        _same(stats, wstats, ("module", k, "stats"))
        assert stats.data_ptr() == opt.stats.data_ptr() and not _u(opt.flat.grads).any()            # +0 everywhere after the step
        assert optim.stats_to_metrics(stats) == {"grad_norm": wstats[0], "clip": wstats[1], "skipped": False, "step": k + 1}
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 5.0)
        opt2.step()
        worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(net.parameters(), twin.parameters()))
        losses.append(float(loss.detach()))
        print(f"step {k + 1}: loss {losses[-1]:.6f}, gnorm {wstats[0]:.4f}, clip {wstats[1]:.4f}, largest |p - torch's p| = {worst:.3e} (bound {H.TOL['p']:.1e})")
        assert worst <= H.TOL["p"], (k, worst)
    assert all(np.isfinite(losses)) and all(b < a for a, b in zip(losses, losses[1:])), losses
    # the hyper-parameters are read from param_groups[0] on every call: lr = 0 moves nothing, but t advances
    held = opt.flat.params.clone()
    opt.param_groups[0]["lr"] = 0.0
    opt.flat.grads.copy_(torch.from_numpy(kept).cuda())
    assert optim.stats_to_metrics(opt.step())["step"] == 6 and torch.equal(opt.flat.params, held)
    opt.param_groups[0]["lr"] = lr
    # state_dict -> a fresh optimiser over a copy of the parameters -> load_state_dict: the next step has the same bits
    net3 = copy.deepcopy(net)
    opt3 = optim.Adam(sim, net3.named_parameters(), lr=lr, max_grad_norm=5)
    sd = opt.state_dict()
    assert set(sd) == {"m", "v", "state", "layout", "param_groups"} and sd["layout"] == lay and sd["m"].data_ptr() != opt.m.data_ptr()
    opt3.load_state_dict(sd)
    _same(opt3.flat.params, opt.flat.params, "the copy")
    for o in (opt, opt3):
        o.flat.grads.copy_(torch.from_numpy(kept).cuda())
    s1, s3 = opt.step().clone(), opt3.step().clone()
    for a, b in ((opt.flat.params, opt3.flat.params), (opt.m, opt3.m), (opt.v, opt3.v), (opt.adam_state, opt3.adam_state), (s1, s3)):
        _same(a, b, "round trip")
    assert float(opt.adam_state[2]) == 7
    other = optim.Adam(sim, [torch.nn.Parameter(torch.zeros(5, device="cuda"))])
    with pytest.raises(ValueError, match="layout"):
        other.load_state_dict(sd)
    # a gradient detached by hand is refused by name; zero_grad() attaches the views again
    name = list(lay)[3]
    dict(net.named_parameters())[name].grad = None
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        opt.step()
    opt.zero_grad()
    assert opt.flat.detached() is None and not _u(opt.flat.grads).any()
    opt.step()
    assert float(opt.adam_state[2]) == 8
    sim.close()
