"""The PPO loss and its gradients: a minibatch's new logits and values, stored actions, old log-probabilities, advantages
and returns turned into d loss / d logits, d loss / d value and the loss statistics by one kernel (hs_ppo_loss,
csrc/hs_k_ppo.h).

The leg after the network's forward pass of a minibatch.  include/hideseek.h states the arithmetic, IEEE f32 in a fixed
order: the clipped surrogate, the (optionally clipped) value loss and the entropy bonus with their closed-form gradients.
No autograd graph of the loss exists; a bucket masked with -inf gets a gradient of exactly 0 where autograd through
log_softmax gives NaN.

    logits, value = net(obs[mb])                                  # [n, 19], [n, 1], with grad
    out = sim.ppo_loss(logits.detach(), actions[mb], old_log_prob[mb], advantages[mb], adv_moments=gae["moments"],
                       mask=masks[mb], value=value.detach(), returns=returns[mb], old_value=old_values[mb])
    torch.autograd.backward([logits, value], [out["grad_logits"], out["grad_value"].view_as(value)])     # no extra op
    metrics = ppo_loss.stats_to_metrics(out["stats"], entropy_coef=0.01, value_loss_coef=0.5)

or, for a learner that wants a loss tensor to call backward on:

    loss = ppo_loss.attach(logits, value, out)                    # a scalar; loss.backward() hands the gradients on
"""
import ctypes as C

from .action_sampling import DEFAULT_BUCKETS, HEADS, MAX_BUCKETS, MAX_LOGITS
from .advantages import MOMENTS
from ._request import (_DTYPES, _OUTPUT, _above_zero, _dtype_arg, _finite, _loss_scale_input, _name, _outputs, _rows, _run, _shard_calls, _stride, _tensor,
                       _vector, _wanted)

STATS = 7             # HS_PPO_STATS: sum pg, sum vl, sum ent, sum kl, policy-clipped, value-clipped, count
STAT_COUNT = 6        # where the count of active samples lies in the statistics
ROWS_PER_BLOCK = 32   # kPpoRows: samples a workgroup takes at a time
MAX_GRID = 2048       # kPpoMaxGrid: workgroups of a call at the most
DEFAULT_CLIP = 0.2
DEFAULT_VALUE_LOSS_COEF = 0.5
DEFAULT_ENTROPY_COEF = 0.01


class HsPpoRequest(C.Structure):
    """hs_ppo_request (include/hideseek.h)."""
    _fields_ = [("logits", C.c_void_p), ("action", C.c_void_p), ("old_log_prob", C.c_void_p), ("advantage", C.c_void_p),
                ("adv_moments", C.c_void_p), ("mask", C.c_void_p), ("value", C.c_void_p), ("returns", C.c_void_p),
                ("old_value", C.c_void_p), ("n", C.c_int32), ("logits_dtype", C.c_int32), ("logits_stride", C.c_int32),
                ("grad_dtype", C.c_int32), ("grad_stride", C.c_int32), ("value_dtype", C.c_int32),
                ("buckets", C.c_int32 * HEADS), ("clip_coef", C.c_float), ("value_loss_coef", C.c_float),
                ("entropy_coef", C.c_float), ("grad_scale", C.c_float), ("grad_logits", C.c_void_p),
                ("grad_value", C.c_void_p), ("stats", C.c_void_p)]


def request(gpu_id, logits, action, old_log_prob, advantage, buckets=DEFAULT_BUCKETS, adv_moments=None, mask=None,
            value=None, returns=None, old_value=None, clip_coef=DEFAULT_CLIP, value_loss_coef=DEFAULT_VALUE_LOSS_COEF,
            entropy_coef=DEFAULT_ENTROPY_COEF, grad_scale=1.0, grad_logits=True, grad_value=None, stats=True,
            grad_dtype=None, loss_scale=None):
    """Validate a call over the n = logits.shape[0] samples of a minibatch on GPU `gpu_id`, allocate the outputs given as
    True (grad_logits in `grad_dtype`, by default the dtype of the logits; grad_value=None means True with a value and
    nothing without), and return ({name: tensor}, HsPpoRequest).  `loss_scale` is None or the float64 [4] state of an
    optim.LossScale on the device, which no output may overlap (compute then runs hs_ppo_loss_scaled: the gradients are
    multiplied by state[0], the statistics are not).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    buckets = tuple(int(b) for b in buckets)
    if len(buckets) != HEADS or any(b < 1 or b > MAX_BUCKETS for b in buckets):
        raise ValueError(f"buckets must be {HEADS} counts in [1, {MAX_BUCKETS}], got {buckets}")
    L = sum(buckets)
    if L > MAX_LOGITS:
        raise ValueError(f"buckets sum to {L} logits per sample, more than {MAX_LOGITS}")
    coefs = {k: _finite(k, v) for k, v in (("clip_coef", clip_coef), ("value_loss_coef", value_loss_coef), ("entropy_coef", entropy_coef),
                                           ("grad_scale", grad_scale))}
    _above_zero("clip_coef", clip_coef)
    if grad_value is None:
        grad_value = value is not None
    outputs = _wanted((("grad_logits", grad_logits), ("grad_value", grad_value), ("stats", stats)), "none of grad_logits, grad_value and stats requested")
    if "grad_value" in outputs and value is None:
        raise ValueError("grad_value needs value")
    if value is not None and returns is None:
        raise ValueError("value needs returns")
    if value is None and (returns is not None or old_value is not None):
        raise ValueError("returns and old_value need value")

    stride = _rows("logits", logits, None, L, dev, "n")
    n = int(logits.shape[0])
    _tensor("action", action, (n, HEADS), ("int32",), dev)
    _vector("old_log_prob", old_log_prob, n, dev, ("float32",))
    _vector("advantage", advantage, n, dev, ("float32",))
    if adv_moments is not None:
        _tensor("adv_moments", adv_moments, (MOMENTS,), ("float64",), dev)
    if mask is not None:
        _vector("mask", mask, n, dev, ("float32",))
    if value is not None:
        _vector("value", value, n, dev, _DTYPES)
        _vector("returns", returns, n, dev, ("float32",))
        if old_value is not None:
            _vector("old_value", old_value, n, dev, ("float32",))
    inputs = [(k, t) for k, t in (("logits", logits), ("action", action), ("old_log_prob", old_log_prob), ("advantage", advantage),
                                  ("adv_moments", adv_moments), ("mask", mask), ("value", value), ("returns", returns),
                                  ("old_value", old_value)) if t is not None] + _loss_scale_input(loss_scale, dev)
    gdt = logits.dtype if grad_dtype is None else grad_dtype
    if outputs.get("grad_logits") is True:
        _dtype_arg("grad_dtype", gdt)
    W = int(logits.shape[1])
    # grad_logits is as wide as the logits tensor, so that logits.backward() takes it: zeros where it is wider than L
    specs = {"grad_logits": ((n, W), gdt, lambda k, t: _rows(k, t, n, L, dev, n), W > L), "stats": ((STATS,), torch.float64)}
    if value is not None:
        specs["grad_value"] = (tuple(value.shape), value.dtype, lambda k, t: _vector(k, t, n, dev, (_name(value.dtype),), _OUTPUT))
    res, out = _outputs(outputs, specs, inputs, dev)
    g = outputs.get("grad_logits")
    gstride = L if g is None else max(W, L) if g is True else _stride(g, L)

    def ptr(t):
        return t.data_ptr() if t is not None else None
    req = HsPpoRequest(ptr(logits), ptr(action), ptr(old_log_prob), ptr(advantage), ptr(adv_moments), ptr(mask), ptr(value),
                       ptr(returns), ptr(old_value), n, _DTYPES[_name(logits.dtype)], stride,
                       _DTYPES[_name(res["grad_logits"].dtype)] if "grad_logits" in res else 0, gstride,
                       _DTYPES[_name(value.dtype)] if value is not None else 0, (C.c_int32 * HEADS)(*buckets),
                       coefs["clip_coef"], coefs["value_loss_coef"], coefs["entropy_coef"], coefs["grad_scale"],
                       out("grad_logits"), out("grad_value"), out("stats"))
    res["coefficients"] = {k: C.c_float(v).value for k, v in coefs.items()}       # as the kernel saw them (f32)
    return res, req


def compute(sim, logits, action, old_log_prob, advantage, stream=None, **kw):
    """HideAndSeekSimulator.ppo_loss."""
    res, req = request(sim.gpu_id, logits, action, old_log_prob, advantage, **kw)
    scale = kw.get("loss_scale")
    if scale is None:
        _run(sim, "hs_ppo_loss", req, stream)
    else:
        _run(sim, "hs_ppo_loss_scaled", req, stream, C.c_void_p(scale.data_ptr()))
    return res


_PER_SHARD = ("adv_moments", "mask", "value", "returns", "old_value", "grad_logits", "grad_value", "stats")


def compute_sharded(ssim, logits, action, old_log_prob, advantage, stream=None, **kw):
    """ShardedSimulator.ppo_loss: every shard computes its own minibatch on its own device.  Every shard divides by its
    own count of active samples: weigh the shards' gradients with grad_scale when their counts differ."""
    return _shard_calls(ssim, "hs_ppo_loss", request, stream, dict(logits=logits, action=action, old_log_prob=old_log_prob, advantage=advantage),
                        per_shard={k: kw.pop(k) for k in _PER_SHARD if k in kw}, kw=kw)


def stats_to_metrics(stats, entropy_coef=DEFAULT_ENTROPY_COEF, value_loss_coef=DEFAULT_VALUE_LOSS_COEF, grad_scale=1.0):
    """{"loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "value_clip_fraction", "count"} in
    float64 from the stats of ppo_loss, on their device and without a synchronisation: the means over the active samples,
    and loss = grad_scale * (policy_loss - entropy_coef * entropy + value_loss_coef * value_loss), the quantity the
    gradients belong to.  With no active sample everything is 0."""
    import torch
    s = stats.to(torch.float64)
    if s.shape != (STATS,):
        raise ValueError(f"stats have shape ({STATS},), got {tuple(s.shape)}")
    count = s[STAT_COUNT]
    n = torch.clamp(count, min=1.0)
    pg, vl, ent = s[0] / n, s[1] / n, s[2] / n
    return {"loss": grad_scale * (pg - entropy_coef * ent + value_loss_coef * vl), "policy_loss": pg, "value_loss": vl,
            "entropy": ent, "approx_kl": s[3] / n, "clip_fraction": s[4] / n, "value_clip_fraction": s[5] / n, "count": count}


def attach(logits, value, out):
    """The scalar float64 loss of a ppo_loss call as a tensor of the autograd graph of `logits` and `value` (None without
    a value term): computed from out["stats"] on the device without a synchronisation; its backward hands
    out["grad_logits"] x upstream and out["grad_value"] x upstream to autograd.  `out` is the result of the call that was
    given logits.detach() and value.detach(); it must hold stats and the gradients of what requires grad.
    torch.autograd.backward([logits, value], [out["grad_logits"], out["grad_value"].view_as(value)]) is the path with no
    extra op."""
    import torch
    if "stats" not in out or "grad_logits" not in out or (value is not None and "grad_value" not in out):
        raise ValueError("attach needs the stats, grad_logits and (with a value) grad_value of the ppo_loss call")
    if tuple(out["grad_logits"].shape) != tuple(logits.shape):
        raise ValueError(f"grad_logits has shape {tuple(out['grad_logits'].shape)}, logits {tuple(logits.shape)}")
    c = out["coefficients"]
    loss = stats_to_metrics(out["stats"], c["entropy_coef"], c["value_loss_coef"], c["grad_scale"])["loss"]

    class _Attach(torch.autograd.Function):
        @staticmethod
        def forward(ctx, *inputs):
            return loss.clone()

        @staticmethod
        def backward(ctx, up):
            gl = out["grad_logits"]
            grads = [(gl * up.to(gl.dtype)).to(logits.dtype)]
            if value is not None:
                gv = out["grad_value"]
                grads.append((gv * up.to(gv.dtype)).view_as(value))
            return tuple(grads)

    return _Attach.apply(*((logits,) if value is None else (logits, value)))
