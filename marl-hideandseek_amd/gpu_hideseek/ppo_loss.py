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
import math

from .action_sampling import DEFAULT_BUCKETS, HEADS, MAX_BUCKETS, MAX_LOGITS
from .advantages import MOMENTS
from ._request import _DTYPES, _disjoint, _name, _per_shard, _rows, _run, _sharded, _vector

STATS = 7             # HS_PPO_STATS: sum pg, sum vl, sum ent, sum kl, policy-clipped, value-clipped, count
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
            grad_dtype=None):
    """Validate a call over the n = logits.shape[0] samples of a minibatch on GPU `gpu_id`, allocate the outputs given as
    True (grad_logits in `grad_dtype`, by default the dtype of the logits; grad_value=None means True with a value and
    nothing without), and return ({name: tensor}, HsPpoRequest).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    buckets = tuple(int(b) for b in buckets)
    if len(buckets) != HEADS or any(b < 1 or b > MAX_BUCKETS for b in buckets):
        raise ValueError(f"buckets must be {HEADS} counts in [1, {MAX_BUCKETS}], got {buckets}")
    L = sum(buckets)
    if L > MAX_LOGITS:
        raise ValueError(f"buckets sum to {L} logits per sample, more than {MAX_LOGITS}")
    coefs = dict(clip_coef=float(clip_coef), value_loss_coef=float(value_loss_coef), entropy_coef=float(entropy_coef),
                 grad_scale=float(grad_scale))
    for k, v in coefs.items():
        if not math.isfinite(v) or not math.isfinite(C.c_float(v).value):
            raise ValueError(f"{k} must be finite, got {v}")
    if not coefs["clip_coef"] > 0.0 or not C.c_float(coefs["clip_coef"]).value > 0.0:
        raise ValueError(f"clip_coef must be above 0, got {clip_coef}")
    if grad_value is None:
        grad_value = value is not None
    outputs = {k: t for k, t in (("grad_logits", grad_logits), ("grad_value", grad_value), ("stats", stats))
               if t is not None and t is not False}
    if not outputs:
        raise ValueError("nothing to do: none of grad_logits, grad_value and stats requested")
    if "grad_value" in outputs and value is None:
        raise ValueError("grad_value needs value")
    if value is not None and returns is None:
        raise ValueError("value needs returns")
    if value is None and (returns is not None or old_value is not None):
        raise ValueError("returns and old_value need value")

    stride = _rows("logits", logits, None, L, dev, "n")
    n = int(logits.shape[0])
    _vector("action", action, n, dev, ("int32",), (HEADS,))
    _vector("old_log_prob", old_log_prob, n, dev, ("float32",))
    _vector("advantage", advantage, n, dev, ("float32",))
    if adv_moments is not None:
        _vector("adv_moments", adv_moments, MOMENTS, dev, ("float64",))
        if tuple(adv_moments.shape) != (MOMENTS,):
            raise ValueError(f"adv_moments must have shape ({MOMENTS},): its shape is {tuple(adv_moments.shape)}")
    if mask is not None:
        _vector("mask", mask, n, dev, ("float32",))
    if value is not None:
        _vector("value", value, n, dev, tuple(_DTYPES))
        _vector("returns", returns, n, dev, ("float32",))
        if old_value is not None:
            _vector("old_value", old_value, n, dev, ("float32",))
    inputs = [(k, t) for k, t in (("logits", logits), ("action", action), ("old_log_prob", old_log_prob), ("advantage", advantage),
                                  ("adv_moments", adv_moments), ("mask", mask), ("value", value), ("returns", returns),
                                  ("old_value", old_value)) if t is not None]
    given = {k: t for k, t in outputs.items() if t is not True}
    gstride = L
    if "grad_logits" in given:
        gstride = _rows("grad_logits", given["grad_logits"], n, L, dev, n)
    elif "grad_logits" in outputs:
        gdt = logits.dtype if grad_dtype is None else grad_dtype
        if _name(gdt) not in _DTYPES:
            raise ValueError(f"grad_dtype must be one of {', '.join(_DTYPES)}, got {gdt}")
    if "grad_value" in given:
        _vector("grad_value", given["grad_value"], n, dev, (_name(value.dtype),))
    if "stats" in given:
        _vector("stats", given["stats"], STATS, dev, ("float64",))
        if tuple(given["stats"].shape) != (STATS,):
            raise ValueError(f"stats must have shape ({STATS},): its shape is {tuple(given['stats'].shape)}")
    _disjoint(list(given.items()), inputs, dev)

    res = dict(given)
    if outputs.get("grad_logits") is True:        # as wide as the logits tensor, so that logits.backward() takes it
        W = int(logits.shape[1])
        res["grad_logits"] = (torch.zeros if W > L else torch.empty)((n, W), dtype=gdt, device=dev)
        gstride = max(W, L)
    if outputs.get("grad_value") is True:
        res["grad_value"] = torch.empty(tuple(value.shape), dtype=value.dtype, device=dev)
    if outputs.get("stats") is True:
        res["stats"] = torch.empty(STATS, dtype=torch.float64, device=dev)
    res = {k: res[k] for k in outputs}

    def ptr(t):
        return t.data_ptr() if t is not None else None
    req = HsPpoRequest(ptr(logits), ptr(action), ptr(old_log_prob), ptr(advantage), ptr(adv_moments), ptr(mask), ptr(value),
                       ptr(returns), ptr(old_value), n, _DTYPES[_name(logits.dtype)], stride,
                       _DTYPES[_name(res["grad_logits"].dtype)] if "grad_logits" in res else 0, gstride,
                       _DTYPES[_name(value.dtype)] if value is not None else 0, (C.c_int32 * HEADS)(*buckets),
                       coefs["clip_coef"], coefs["value_loss_coef"], coefs["entropy_coef"], coefs["grad_scale"],
                       ptr(res.get("grad_logits")), ptr(res.get("grad_value")), ptr(res.get("stats")))
    res["coefficients"] = {k: C.c_float(v).value for k, v in coefs.items()}       # as the kernel saw them (f32)
    return res, req


def compute(sim, logits, action, old_log_prob, advantage, stream=None, **kw):
    """HideAndSeekSimulator.ppo_loss."""
    res, req = request(sim.gpu_id, logits, action, old_log_prob, advantage, **kw)
    _run(sim, "hs_ppo_loss", req, stream)
    return res


_PER_SHARD = ("adv_moments", "mask", "value", "returns", "old_value", "grad_logits", "grad_value", "stats")


def compute_sharded(ssim, logits, action, old_log_prob, advantage, stream=None, **kw):
    """ShardedSimulator.ppo_loss: every shard computes its own minibatch on its own device.  `logits`, `action`,
    `old_log_prob` and `advantage` have one tensor per shard; adv_moments, mask, value, returns, old_value, each output
    and `stream` are True / None for all shards or a list with one entry per shard; returns the list of the shards'
    results.  With stream=None every shard's call is enqueued on a side stream of its device, ordered after that device's
    current stream, before any is waited for.  Every shard divides by its own count of active samples: weigh the shards'
    gradients with grad_scale when their counts differ."""
    import torch
    n = len(ssim.shards)
    for name, arg in (("logits", logits), ("action", action), ("old_log_prob", old_log_prob), ("advantage", advantage)):
        if isinstance(arg, torch.Tensor) or len(arg) != n:
            raise ValueError(f"{name}: one tensor per shard ({n}) expected")
    per = {k: _per_shard(ssim, k, kw.pop(k)) for k in _PER_SHARD if k in kw}
    return _sharded(ssim, "hs_ppo_loss", lambda i, s: request(s.gpu_id, logits[i], action[i], old_log_prob[i], advantage[i],
                                                              **{k: v[i] for k, v in per.items()}, **kw), stream)


def stats_to_metrics(stats, entropy_coef=DEFAULT_ENTROPY_COEF, value_loss_coef=DEFAULT_VALUE_LOSS_COEF, grad_scale=1.0):
    """{"loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "value_clip_fraction", "count"} in
    float64 from the stats of ppo_loss, on their device and without a synchronisation: the means over the active samples,
    and loss = grad_scale * (policy_loss - entropy_coef * entropy + value_loss_coef * value_loss), the quantity the
    gradients belong to.  With no active sample everything is 0."""
    import torch
    s = stats.to(torch.float64)
    if s.shape != (STATS,):
        raise ValueError(f"stats have shape ({STATS},), got {tuple(s.shape)}")
    count = s[6]
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
