"""The dynamic loss scale without a GPU (gpu_hideseek.optim.LossScale; hs_ppo_loss_scaled, hs_twohot_value_scaled,
hs_adam_step_scaled): the rule of include/hideseek.h restated in numpy on top of the restatements of the unscaled calls
(test_optim_host.step with grad_scale / S, test_ppo_loss_host.ppo and test_value_head_host.twohot with grad_scale * S);
the rule's properties on hand-written sequences; the power-of-two equivalences the GPU tests rely on; what float16 keeps of
a minibatch's gradient with and without the scale, and the error bound derived from the format; the refusals of
LossScale, the request builders and TrainConfig before any library call; and the header's struct and symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import test_optim_host as A
from test_optim_host import HYPER, step
from test_ppo_loss_host import BUCKETS, inputs as ppo_inputs, ppo
from test_value_head_host import BINS, inputs as twohot_inputs, twohot

STATE = 4                                                    # HS_LOSS_SCALE_STATE: S, good steps, backoffs, growths
DEFAULTS = dict(init_scale=2.0 ** 16, growth=2.0, backoff=0.5, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24)
F16_MIN_NORMAL, F16_HALF_SUBNORMAL, F16_HALF_ULP = 2.0 ** -14, 2.0 ** -25, 2.0 ** -11


# ---- the contract ----
def fresh(init_scale=DEFAULTS["init_scale"]):
    return np.array([init_scale, 0.0, 0.0, 0.0], np.float64)


def scaler(state, skipped, growth=2.0, backoff=0.5, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24, **_):
    """The loss-scale state after a step, in float64 as the header has it."""
    S, good, backoffs, growths = (np.float64(v) for v in state)
    if skipped:
        return np.array([max(S * backoff, min_scale), 0.0, backoffs + 1.0, growths], np.float64)
    good = good + 1.0
    if good >= growth_interval:
        return np.array([min(S * growth, max_scale), 0.0, backoffs, growths + 1.0], np.float64)
    return np.array([S, good, backoffs, growths], np.float64)


def scaled_step(ft, x, adam_state, scale_state, settings, zero_grad=True, **hyper):
    """hs_adam_step_scaled: hs_adam_step with e = grad_scale / S (f64) where it has grad_scale, then the rule.  Returns
    (arrays, Adam state, stats, loss-scale state)."""
    kw = dict(hyper, grad_scale=np.float64(hyper["grad_scale"]) / np.float64(scale_state[0]))
    out, new, stats = step(ft, x, adam_state, zero_grad=zero_grad, **kw)
    return out, new, stats, scaler(scale_state, stats[2] != 0, **settings)


def run_rule(init, skips, **settings):
    """The states after each of the steps `skips` (booleans) from fresh(init)."""
    s, out = fresh(init), []
    for k in skips:
        s = scaler(s, k, **settings)
        out.append(s.tolist())
    return out


# ---- the rule on hand-written sequences ----
def test_backoff_halves_down_to_min_scale_and_stays():
    got = run_rule(4.0, [True] * 6, growth_interval=3, min_scale=0.25, max_scale=16.0)
    assert [s[0] for s in got] == [2.0, 1.0, 0.5, 0.25, 0.25, 0.25]
    assert [s[2] for s in got] == [1, 2, 3, 4, 5, 6] and all(s[1] == 0 and s[3] == 0 for s in got)


def test_growth_exactly_at_the_interval_and_up_to_max_scale():
    got = run_rule(4.0, [False] * 10, growth_interval=3, min_scale=0.25, max_scale=16.0)
    assert [s[0] for s in got] == [4, 4, 8, 8, 8, 16, 16, 16, 16, 16]
    assert [s[1] for s in got] == [1, 2, 0, 1, 2, 0, 1, 2, 0, 1]
    assert [s[3] for s in got] == [0, 0, 1, 1, 1, 2, 2, 2, 3, 3]              # growths still counts at the clamp
    assert all(s[2] == 0 for s in got)
    assert run_rule(4.0, [False], growth_interval=1)[0] == [8.0, 0.0, 0.0, 1.0]


def test_a_skipped_step_resets_the_run_of_good_steps():
    got = run_rule(4.0, [False, False, True, False, False, False], growth_interval=3, min_scale=0.25, max_scale=16.0)
    assert got == [[4, 1, 0, 0], [4, 2, 0, 0], [2, 0, 1, 0], [2, 1, 1, 0], [2, 2, 1, 0], [4, 0, 1, 1]]


def test_the_defaults_are_the_published_rule():
    from gpu_hideseek import optim
    assert optim.LOSS_SCALE_DEFAULTS == DEFAULTS and optim.loss_scale_settings() == DEFAULTS
    s = fresh()
    for _ in range(1999):
        s = scaler(s, False, **DEFAULTS)
    assert s.tolist() == [2.0 ** 16, 1999, 0, 0]
    assert scaler(s, False, **DEFAULTS).tolist() == [2.0 ** 17, 0, 0, 1]
    assert scaler(s, True, **DEFAULTS).tolist() == [2.0 ** 15, 0, 1, 0]


# ---- a power of two is exact everywhere ----
@pytest.mark.parametrize("k", (0, 7, 16))
def test_scaled_gradients_give_the_bits_of_the_unscaled_step(k):
    n, S = 1025, 2.0 ** k
    for kw in A.ADAM_CASES:
        x = A.inputs(n)
        plain, scaled, state, sstate, ls = dict(x), dict(x), A.fresh_state(), A.fresh_state(), fresh(S)
        for i, norm in enumerate(A.ADAM_NORMS):
            g = A.gradients(n, i, norm)
            want, state, stats = step(np.float32, dict(plain, g=g), state, **kw)
            got, sstate, sstats, ls = scaled_step(np.float32, dict(scaled, g=(g * np.float32(S)).astype(np.float32)), sstate, ls,
                                                  dict(DEFAULTS, growth_interval=2 ** 30), **kw)
            for q in "pgmv":
                assert np.array_equal(got[q].view(np.uint32), want[q].view(np.uint32)), (k, i, q)
            assert np.array_equal(sstate, state) and np.array_equal(sstats, stats) and ls[0] == S
            plain, scaled = {q: want[q] for q in "pmv"}, {q: got[q] for q in "pmv"}
        assert ls.tolist() == [S, len(A.ADAM_NORMS), 0, 0]


def test_an_overflow_is_skipped_and_backs_off():
    n = 255
    x = dict(A.inputs(n), g=A.gradients(n, 0, 20.0))
    for bad in (np.inf, -np.inf, np.nan):
        g = np.array(x["g"])
        g[n - 1] = bad
        out, state, stats, ls = scaled_step(np.float32, dict(x, g=g), A.fresh_state(), fresh(), DEFAULTS, **HYPER)
        assert stats[2] == 1 and state.tolist() == [1, 1, 0, 1] and ls.tolist() == [2.0 ** 15, 0, 1, 0]
        assert all(np.array_equal(out[q], x[q]) for q in "pmv") and not out["g"].any()


@pytest.mark.parametrize("S", (1.0, 2.0 ** -3, 2.0 ** 16))
def test_the_scaled_losses_are_the_unscaled_ones_with_the_product(S):
    """grad_scale * S enters as one f32 product, so a power of two scales every gradient exactly (nothing here is near
    f32's subnormals) and the statistics hold no S."""
    x = ppo_inputs(1806, BUCKETS[0], "float32", True, "clipped")
    one, got = ppo(np.float32, x), ppo(np.float32, x, grad_scale=1.0 * S)
    for q in ("grad_logits", "grad_value"):
        assert np.array_equal(got[q], one[q] * np.float32(S)) and np.isfinite(got[q]).all(), q
    assert np.array_equal(got["stats"], one["stats"])
    y = twohot_inputs(1806, BINS[2], "float32", True)
    one, got = twohot(np.float32, y), twohot(np.float32, y, grad_scale=1.0 * S)
    assert np.array_equal(got["grad_logits"], one["grad_logits"] * np.float32(S)) and np.array_equal(got["stats"], one["stats"])
    assert np.array_equal(got["value"], one["value"])


# ---- what float16 keeps of the gradient ----
def f16_report(g32, S):
    """Of the nonzero entries of g32 (the f32 gradient at scale 1): the shares that are subnormal and that are flushed to
    0 as float16 at scale S, the median relative error, and the relative L2 error of float16(S g) / S."""
    g = g32[g32 != 0].astype(np.float64)
    h = (g * S).astype(np.float32).astype(np.float16)
    assert np.isfinite(h).all()
    back = h.astype(np.float64) / S
    mag = np.abs(g * S)
    return dict(subnormal=float((mag < F16_MIN_NORMAL).mean()), flushed=float((h == 0).mean()), median=float(np.median(np.abs(back - g) / np.abs(g))),
                l2=float(np.sqrt(((back - g) ** 2).sum() / (g ** 2).sum())), largest=float(mag.max()))


def f16_bound(g32, S):
    """The bound on that relative L2 error from the format alone: an entry whose scaled value is in float16's normal range
    is off by at most half an ulp, 2^-11 of its size; a subnormal one by at most half the subnormal spacing, 2^-25,
    which is 2^-25 / S at scale 1; the entries' bounds combined in L2."""
    g = np.abs(g32[g32 != 0].astype(np.float64))
    per = np.where(g * S >= F16_MIN_NORMAL, F16_HALF_ULP * g, F16_HALF_SUBNORMAL / S)
    return float(np.sqrt((per ** 2).sum() / (g ** 2).sum()))


def test_float16_keeps_the_gradient_only_with_the_scale():
    """The issue's table at n = 65 536, recomputed and printed."""
    n = 65536
    r = ppo(np.float32, ppo_inputs(n, BUCKETS[0], "float16", True, "none", 0, True))
    g = r["grad_logits"]
    rows = {S: f16_report(g, S) for S in (1.0, 2.0 ** 16)}
    for S, t in rows.items():
        print(f"n = {n}, cnt = {r['cnt']}, scale {S:g}: subnormal {100 * t['subnormal']:.2f} %, flushed to 0 {100 * t['flushed']:.1f} %, "
              f"median relative error {t['median']:.2g}, relative L2 error {t['l2']:.3g} (bound {f16_bound(g, S):.3g}), largest {t['largest']:.3g}")
    plain, scaled = rows[1.0], rows[2.0 ** 16]
    assert plain["subnormal"] > 0.99 and scaled["subnormal"] < 0.1 and scaled["largest"] < 65504
    for S, t in rows.items():
        assert t["l2"] <= f16_bound(g, S), (S, t["l2"], f16_bound(g, S))
    assert scaled["l2"] < 0.5 * plain["l2"] and scaled["flushed"] < plain["flushed"] and scaled["median"] < plain["median"]
    assert f16_bound(g, 2.0 ** 16) < f16_bound(g, 1.0)


# ---- refusals before any library call ----
def test_loss_scale_refuses_its_settings():
    from gpu_hideseek import optim
    ok = optim.LossScale("cpu")
    assert ok.state.tolist() == [2.0 ** 16, 0, 0, 0] and ok.state.dtype == torch.float64 and ok.settings() == {k: v for k, v in DEFAULTS.items() if k != "init_scale"}
    assert ok.read() == {"scale": 2.0 ** 16, "good_steps": 0, "backoffs": 0, "growths": 0}
    r = ok.request()
    assert (r.state, r.growth, r.backoff, r.min_scale, r.max_scale, r.growth_interval, r.reserved) == (ok.state.data_ptr(), 2.0, 0.5, 1.0, 2.0 ** 24, 2000, 0)
    nan, inf = float("nan"), float("inf")
    bad = [("init_scale", 3.0), ("init_scale", 0.5), ("init_scale", 2.0 ** 25), ("init_scale", nan), ("init_scale", "1"), ("growth", 0.5), ("growth", 3.0),
           ("growth", inf), ("growth", 2.0 ** 127), ("backoff", 2.0), ("backoff", 0.0), ("backoff", 0.3), ("backoff", -0.5), ("min_scale", 0.0),
           ("min_scale", -1.0), ("min_scale", 1.5), ("max_scale", 0.5), ("max_scale", 2.0 ** 127), ("max_scale", 1000.0),
           ("max_scale", True), ("growth_interval", 0), ("growth_interval", -1), ("growth_interval", 2.5), ("growth_interval", True), ("growth_interval", 2 ** 31)]
    for key, value in bad:
        with pytest.raises(ValueError, match=f"{key} must be"):
            optim.LossScale("cpu", **{key: value})
    with pytest.raises(ValueError, match="max_scale must be a power of two, at least min_scale"):
        optim.LossScale("cpu", min_scale=2.0 ** 25)
    with pytest.raises(ValueError, match="unknown loss scale settings"):
        optim.loss_scale_settings(decay=0.5)
    small = optim.LossScale("cpu", init_scale=2.0 ** -3, min_scale=2.0 ** -140, max_scale=2.0 ** 126, growth=1.0, backoff=1.0, growth_interval=1)
    assert small.state[0] == 0.125
    # the checkpoint
    d = optim.LossScale("cpu", init_scale=4.0, growth_interval=7, max_scale=16.0).state_dict()
    d["state"][1:] = torch.tensor([3.0, 2.0, 1.0], dtype=torch.float64)
    ok.load_state_dict(d)
    assert ok.state.tolist() == [4, 3, 2, 1] and ok.growth_interval == 7 and ok.max_scale == 16.0 and ok.state.data_ptr() != d["state"].data_ptr()
    for wrong in (dict(d, state=torch.zeros(3, dtype=torch.float64)), dict(d, state=torch.zeros(4)), dict(d, growth=3.0)):
        with pytest.raises(ValueError):
            ok.load_state_dict(wrong)


class _Lib:                                      # any call into the library fails the test
    def __getattr__(self, name):
        raise AssertionError(f"library function {name} called")


class _Sim:
    num_worlds, agents_per_world, gpu_id = 8, 4, 0
    _L, _h = _Lib(), None


def test_requests_refuse_a_bad_state_before_the_library_is_called():
    from gpu_hideseek import optim, ppo_loss, value_head
    n = 40
    f64 = torch.float64
    bad = ((torch.zeros(4), "dtype"), (torch.zeros(5, dtype=f64), "shape"), (torch.zeros(4, 1, dtype=f64), "shape"), (torch.zeros(8, dtype=f64)[::2], "contiguous"),
           (2.0 ** 16, "loss_scale must be"), (optim.LossScale("cpu"), "loss_scale must be"))
    ppo_args = (torch.zeros(n, 19), torch.zeros(n, 5, dtype=torch.int32), torch.zeros(n), torch.zeros(n))
    for state, what in bad:
        with pytest.raises(ValueError, match=what):
            ppo_loss.compute(_Sim(), *ppo_args, loss_scale=state)
        with pytest.raises(ValueError, match=what):
            value_head.compute(_Sim(), torch.zeros(n, 255), torch.zeros(n), loss_scale=state)
    both = torch.zeros(12, dtype=f64)
    with pytest.raises(ValueError, match="stats overlaps loss_scale"):
        ppo_loss.compute(_Sim(), *ppo_args, loss_scale=both[:4], stats=both[2:9])
    with pytest.raises(ValueError, match="stats overlaps loss_scale"):
        value_head.compute(_Sim(), torch.zeros(n, 255), torch.zeros(n), loss_scale=both[:4], stats=both[3:9])
    raw = torch.zeros(n * 19 + 8)
    with pytest.raises(ValueError, match="grad_logits overlaps loss_scale"):
        ppo_loss.compute(_Sim(), *ppo_args, loss_scale=raw.view(f64)[:4], grad_logits=raw[:n * 19].view(n, 19))
    for ok in (dict(), dict(loss_scale=torch.zeros(4, dtype=f64))):           # well-formed tensors on the wrong device
        with pytest.raises(ValueError, match="on cpu"):
            ppo_loss.compute(_Sim(), *ppo_args, **ok)
    # the optimiser takes the LossScale itself
    good = [torch.zeros(n) for _ in range(4)] + [optim.fresh_state()]
    for state, what in ((torch.zeros(4, dtype=f64), "loss_scale must be None or an optim.LossScale"), ("dynamic", "loss_scale must be None or an optim.LossScale")):
        with pytest.raises(ValueError, match=what):
            optim.compute(_Sim(), *good, loss_scale=state)
    ls = optim.LossScale("cpu")
    ls.state = good[2].view(f64)[:4]
    with pytest.raises(ValueError, match="loss_scale overlaps m"):
        optim.compute(_Sim(), *good, loss_scale=ls)
    ls.state = good[4]
    with pytest.raises(ValueError, match="loss_scale overlaps state"):
        optim.compute(_Sim(), *good, loss_scale=ls)
    with pytest.raises(ValueError, match="on cpu"):
        optim.compute(_Sim(), *good, loss_scale=optim.LossScale("cpu"))


def test_train_config_refuses_a_bad_setting():
    from gpu_hideseek import trainer
    rows = 36
    assert trainer.TrainConfig().loss_scale is None and trainer.loss_scale_settings(None) is None
    assert trainer.loss_scale_settings("dynamic") == DEFAULTS
    assert trainer.loss_scale_settings({"init_scale": 256.0, "growth_interval": 2}) == dict(DEFAULTS, init_scale=256.0, growth_interval=2)
    cfg = dict(steps_per_update=8, num_bptt_chunks=2, num_minibatches=2, num_epochs=2)
    trainer.check_config(trainer.TrainConfig(loss_scale="dynamic", **cfg), rows)
    for bad, what in (("static", "loss_scale must be"), (65536.0, "loss_scale must be"), (True, "loss_scale must be"), ({"init_scale": 3.0}, "init_scale must be"),
                      ({"scale": 4.0}, "unknown loss scale settings"), ({"growth_interval": 0}, "growth_interval must be")):
        with pytest.raises(ValueError, match=what):
            trainer.check_config(trainer.TrainConfig(loss_scale=bad, **cfg), rows)
    assert "loss_scale" not in trainer.Trainer.METRIC_NAMES


# ---- the header ----
def test_header_states_the_struct_and_the_entry_points(hideseek_lib):
    from gpu_hideseek import optim, _request
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hideseek.h")).read()
    assert re.search(r"HS_LOSS_SCALE_STATE = (\d+)", src).group(1) == str(STATE) == str(_request.LOSS_SCALE_STATE)
    body = re.search(r"typedef struct hs_loss_scale \{(.*?)\} hs_loss_scale;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.split()
        if words:
            for part in " ".join(words[1:]).split(","):
                part = part.strip()
                fields.append((part.lstrip("*").strip(), C.c_void_p if part.startswith("*") else A.CTYPES[words[0]]))
    assert fields == list(optim.HsLossScale._fields_), fields
    assert [f[0] for f in fields] == ["state", "growth", "backoff", "min_scale", "max_scale", "growth_interval", "reserved"]
    R = optim.HsLossScale
    assert C.sizeof(R) == 48 and R.growth.offset == 8 and R.backoff.offset == 16 and R.min_scale.offset == 24 and R.max_scale.offset == 32
    assert R.growth_interval.offset == 40 and R.reserved.offset == 44
    lib = C.CDLL(hideseek_lib)
    for fn, req, last in (("hs_ppo_loss_scaled", "hs_ppo_request", r"const double \*\w+"), ("hs_twohot_value_scaled", "hs_twohot_request", r"const double \*\w+"),
                          ("hs_adam_step_scaled", "hs_adam_request", r"const hs_loss_scale \*\w+")):
        assert re.search(rf"int32_t {fn}\(hs_sim \*\w*, const {req} \*\w*, {last}\);", src), fn
        assert re.search(rf"int32_t {fn}_async\(hs_sim \*\w*, void \*hip_stream, const {req} \*\w*, {last}\);", src), fn
        assert hasattr(lib, fn) and hasattr(lib, fn + "_async")
    for phrase in ("w = (grad_scale * S) / (float)cnt", "e = grad_scale / S", "gnorm = e * sqrt(sum)", "s = (float)(e * clip)",
                   "S' = max(S * backoff, min_scale)", "S' = min(S * growth, max_scale)", "good' >= growth_interval"):
        assert phrase in src, phrase
    csrc = os.path.join(root, "marl-hideandseek_amd", "csrc")
    kernel, host = (open(os.path.join(csrc, f)).read() for f in ("hs_k_loss_scale.h", "hideseek.hip"))
    assert int(re.search(r"kLossScaleState = (\d+);", kernel).group(1)) == STATE
    assert "HS_LOSS_SCALE_STATE == hs::kLossScaleState" in host and "atomic" not in kernel
    assert len(re.findall(r"__global__", kernel)) == 4 and "for (" not in kernel      # the element loops are hs_k_adam.h's, hs_k_ppo.h's and hs_k_twohot.h's
    includes = re.findall(r'#include "(hs_\w+\.h)"', host)
    # the last two kernel headers, in this order; behind them only the scalar core's probe table, which holds no kernel
    assert includes[-3:] == ["hs_k_loss_scale.h", "hs_k_adam.h", "hs_core_probe.h"]
    assert "__global__" not in open(os.path.join(csrc, "hs_core_probe.h")).read()
    entry = open(os.path.join(root, "__graft_entry__.py")).read()
    for fn in ("hs_ppo_loss_scaled", "hs_twohot_value_scaled", "hs_adam_step_scaled"):
        assert f'"{fn}"' in entry and f'"{fn}_async"' in entry
