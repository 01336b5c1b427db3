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
from .policy_inputs import _DTYPES, _per_shard, stream_handle

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


def _name(dtype):
    return str(dtype).replace("torch.", "")


def _rows(name, t, n, L, dev, what):
    """Check a [n, W >= L] tensor that is contiguous in its last dimension (logits, grad_logits)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    what = f"{name} must be a {' / '.join(_DTYPES)} tensor of shape ({what}, W >= {L}), contiguous in its last dimension, on {dev}"
    if t.dim() != 2 or t.shape[0] < 1 or (n is not None and t.shape[0] != n) or t.shape[1] < L:
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if _name(t.dtype) not in _DTYPES:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    stride = max(int(t.stride(0)), L) if t.shape[0] > 1 else max(int(t.shape[1]), L)
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < L) or t.shape[0] * stride >= 2 ** 31:
        raise ValueError(f"{what}: its stride is {tuple(t.stride())} (n * stride must stay below 2^31)")
    return stride


def _vector(name, t, n, dev, dtypes, tail=()):
    """Check a contiguous per-sample tensor [n] + tail (or [n, 1] when tail is empty)."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    shape = (n,) + tail
    what = f"{name} must be a contiguous {' / '.join(dtypes)} tensor of shape {shape} on {dev}"
    if tuple(t.shape) != shape and not (not tail and tuple(t.shape) == (n, 1)):
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if _name(t.dtype) not in dtypes:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: it is not contiguous")


def _overlap(a, b):
    """Whether the storage ranges of two tensors intersect."""
    def span(t):
        last = sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
        return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


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
    for k, t in given.items():
        for k2, t2 in inputs:
            if _overlap(t, t2):
                raise ValueError(f"{k} overlaps {k2}")
    names = list(given)
    for i, k in enumerate(names):
        for k2 in names[:i]:
            if _overlap(given[k], given[k2]):
                raise ValueError(f"{k} overlaps {k2}")
    # shapes, dtypes and strides first, so that every one of them is reported whatever device the tensors are on
    for k, t in inputs + list(given.items()):
        if t.device != dev:
            raise ValueError(f"{k} must be on {dev}: it is on {t.device}")

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
    from ._native import check
    res, req = request(sim.gpu_id, logits, action, old_log_prob, advantage, **kw)
    if stream is None:
        check(sim._L.hs_ppo_loss(sim._h, C.byref(req)))
    else:
        check(sim._L.hs_ppo_loss_async(sim._h, C.c_void_p(stream_handle(stream)), C.byref(req)))
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
    from ._native import check
    n = len(ssim.shards)
    for name, arg in (("logits", logits), ("action", action), ("old_log_prob", old_log_prob), ("advantage", advantage)):
        if isinstance(arg, torch.Tensor) or len(arg) != n:
            raise ValueError(f"{name}: one tensor per shard ({n}) expected")
    per = {k: _per_shard(ssim, k, kw.pop(k)) for k in _PER_SHARD if k in kw}
    streams = _per_shard(ssim, "stream", stream)
    reqs = [request(s.gpu_id, lg, a, lp, adv, **{k: v[i] for k, v in per.items()}, **kw)
            for i, (s, lg, a, lp, adv) in enumerate(zip(ssim.shards, logits, action, old_log_prob, advantage))]
    waits = []
    for s, (res, req), st in zip(ssim.shards, reqs, streams):
        if st is None:
            st = torch.cuda.Stream(device=s.gpu_id)
            st.wait_stream(torch.cuda.current_stream(s.gpu_id))
            waits.append(st)
        check(s._L.hs_ppo_loss_async(s._h, C.c_void_p(stream_handle(st)), C.byref(req)))
    for st in waits:
        st.synchronize()
    return [res for res, _ in reqs]


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
