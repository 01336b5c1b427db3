"""The two-hot symlog critic head: a critic's logits over bins in symlog space turned into the decoded value and, with
returns, into the gradient of the cross-entropy against the two-hot target and the value statistics by one kernel
(hs_twohot_value, csrc/hs_k_twohot.h).

The value leg of a learner whose critic is the reference's DreamerV3Critic (scripts/jax_policy.py:369; Hafner et al.
2023).  include/hideseek.h states the arithmetic, IEEE f32 in a fixed order.  In the rollout the call decodes:

    values[t] = ...                                               # a [T, rows] buffer
    sim.value_head(critic_logits, value=values[t])                # symexp(softmax(logits) . bins) into the slot
    gae = sim.compute_advantages(rewards, dones, values, bootstrap)

and in the update it stands next to ppo_loss without its value term:

    logits, critic_logits = net(obs[mb])                          # [n, 19], [n, 255], with grad
    pol = sim.ppo_loss(logits.detach(), actions[mb], old_log_prob[mb], advantages[mb], mask=masks[mb])
    val = sim.value_head(critic_logits.detach(), returns[mb], mask=masks[mb], loss_coef=0.5)
    torch.autograd.backward([logits, critic_logits], [pol["grad_logits"], val["grad_logits"]])
    metrics = value_head.stats_to_metrics(val["stats"])

Both calls divide by the same count of active samples, so their gradients add to those of the total loss.  bins(),
symlog(), symexp() and twohot() are the eager composition in plain torch, for readers and for tools/twohot_bench.py.
"""
import ctypes as C

from ._request import _DTYPES, _OUTPUT, _dtype_arg, _finite, _loss_scale_input, _name, _outputs, _rows, _run, _shard_calls, _stride, _vector, _wanted

STATS = 6             # HS_TWOHOT_STATS: sum ce, sum (v - R)^2, sum v, sum R, sum R^2, count
MAX_BINS = 256        # HS_TWOHOT_MAX_BINS
ROWS_PER_BLOCK = 32   # kTwRows: samples a workgroup takes at a time
MAX_GRID = 2048       # kTwMaxGrid: workgroups of a call at the most
DEFAULT_BINS, DEFAULT_LO, DEFAULT_HI = 255, -20.0, 20.0


class HsTwohotRequest(C.Structure):
    """hs_twohot_request (include/hideseek.h)."""
    _fields_ = [("logits", C.c_void_p), ("returns", C.c_void_p), ("mask", C.c_void_p), ("n", C.c_int32),
                ("logits_dtype", C.c_int32), ("logits_stride", C.c_int32), ("bins", C.c_int32), ("lo", C.c_float),
                ("hi", C.c_float), ("loss_coef", C.c_float), ("grad_scale", C.c_float), ("value_dtype", C.c_int32),
                ("grad_dtype", C.c_int32), ("grad_stride", C.c_int32), ("reserved", C.c_int32), ("value", C.c_void_p),
                ("grad_logits", C.c_void_p), ("stats", C.c_void_p)]


# ---- the eager composition ----
def bins(B=DEFAULT_BINS, lo=DEFAULT_LO, hi=DEFAULT_HI, device=None):
    """[B] float32: b_i = lo + i * step with step = (hi - lo) / (B - 1), as the header has them."""
    import torch
    step = (torch.tensor(hi, dtype=torch.float32) - torch.tensor(lo, dtype=torch.float32)) / float(B - 1)
    return (torch.tensor(lo, dtype=torch.float32) + torch.arange(B, dtype=torch.float32) * step).to(device)


def symlog(x):
    import torch
    return torch.sign(x) * torch.log1p(torch.abs(x))


def symexp(x):
    import torch
    return torch.sign(x) * torch.expm1(torch.abs(x))


def twohot(returns, B=DEFAULT_BINS, lo=DEFAULT_LO, hi=DEFAULT_HI):
    """[n, B]: the two-hot target of symlog(returns) over the bins, in the dtype of `returns`: weight 1 - f on bin k and
    f on bin k + 1, where clamp(symlog(R), lo, hi) lies the fraction f of a step above bin k."""
    import torch
    step = (hi - lo) / (B - 1)
    u = (torch.clamp(symlog(returns), lo, hi) - lo) / step
    k = torch.clamp(torch.floor(u), 0, B - 2)
    f = torch.clamp(u - k, 0, 1)
    k = k.long()
    t = torch.zeros(returns.shape + (B,), dtype=returns.dtype, device=returns.device)
    t.scatter_(-1, k.unsqueeze(-1), (1 - f).unsqueeze(-1))
    t.scatter_(-1, (k + 1).unsqueeze(-1), f.unsqueeze(-1))
    return t


def decode(logits, B=DEFAULT_BINS, lo=DEFAULT_LO, hi=DEFAULT_HI):
    """Eager value: symexp(softmax(logits) . bins), in float32."""
    import torch
    lg = logits.float()
    return symexp(torch.softmax(lg, dim=-1) @ bins(B, lo, hi, device=lg.device))


def eager_loss(logits, returns, mask=None, B=DEFAULT_BINS, lo=DEFAULT_LO, hi=DEFAULT_HI):
    """Eager loss: the masked mean of -(twohot(returns) * log_softmax(logits)).sum(-1), in float32."""
    import torch
    ce = -(twohot(returns.float(), B, lo, hi) * torch.log_softmax(logits.float(), dim=-1)).sum(-1)
    return ce.mean() if mask is None else (ce * mask).sum() / mask.sum()


# ---- the fused call ----
def request(gpu_id, logits, returns=None, bins=DEFAULT_BINS, lo=DEFAULT_LO, hi=DEFAULT_HI, mask=None, value=True,
            grad_logits=None, stats=None, loss_coef=1.0, grad_scale=1.0, grad_dtype=None, value_dtype=None, loss_scale=None):
    """Validate a call over the n = logits.shape[0] samples on GPU `gpu_id`, allocate the outputs given as True (value in
    `value_dtype` and grad_logits in `grad_dtype`, by default the dtype of the logits; grad_logits=None and stats=None
    mean True exactly when returns are given), and return ({name: tensor}, HsTwohotRequest).  `loss_scale` is None or
    the float64 [4] state of an optim.LossScale on the device, which no output may overlap (compute then runs
    hs_twohot_value_scaled: grad_logits is multiplied by state[0], value and stats are not).  Raises ValueError before
    the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    if isinstance(bins, bool) or not isinstance(bins, int) or bins < 2 or bins > MAX_BINS:
        raise ValueError(f"bins must be an integer in [2, {MAX_BINS}], got {bins}")
    B = bins
    coefs = {k: _finite(k, v) for k, v in (("lo", lo), ("hi", hi), ("loss_coef", loss_coef), ("grad_scale", grad_scale))}
    if not C.c_float(coefs["lo"]).value < C.c_float(coefs["hi"]).value:
        raise ValueError(f"lo must be below hi, got lo {lo}, hi {hi}")
    if grad_logits is None:
        grad_logits = returns is not None
    if stats is None:
        stats = returns is not None
    outputs = _wanted((("value", value), ("grad_logits", grad_logits), ("stats", stats)), "none of value, grad_logits and stats requested")
    if returns is None and ("grad_logits" in outputs or "stats" in outputs):
        raise ValueError("grad_logits and stats need returns")

    stride = _rows("logits", logits, None, B, dev, "n")
    n = int(logits.shape[0])
    if returns is not None:
        _vector("returns", returns, n, dev, ("float32",))
    if mask is not None:
        _vector("mask", mask, n, dev, ("float32",))
    inputs = [(k, t) for k, t in (("logits", logits), ("returns", returns), ("mask", mask)) if t is not None] + _loss_scale_input(loss_scale, dev)
    _dtype_arg("value_dtype", value_dtype)
    _dtype_arg("grad_dtype", grad_dtype)
    W = int(logits.shape[1])
    # grad_logits is as wide as the logits tensor, so that logits.backward() takes it: zeros where it is wider than B
    specs = {"value": ((n,), logits.dtype if value_dtype is None else value_dtype, lambda k, t: _vector(k, t, n, dev, _DTYPES, _OUTPUT)),
             "grad_logits": ((n, W), logits.dtype if grad_dtype is None else grad_dtype, lambda k, t: _rows(k, t, n, B, dev, n), W > B),
             "stats": ((STATS,), torch.float64)}
    res, out = _outputs(outputs, specs, inputs, dev)
    g = outputs.get("grad_logits")
    gstride = B if g is None else max(W, B) if g is True else _stride(g, B)

    def ptr(t):
        return t.data_ptr() if t is not None else None
    req = HsTwohotRequest(ptr(logits), ptr(returns), ptr(mask), n, _DTYPES[_name(logits.dtype)], stride, B, coefs["lo"], coefs["hi"],
                          coefs["loss_coef"], coefs["grad_scale"], _DTYPES[_name(res["value"].dtype)] if "value" in res else 0,
                          _DTYPES[_name(res["grad_logits"].dtype)] if "grad_logits" in res else 0, gstride, 0,
                          out("value"), out("grad_logits"), out("stats"))
    res["coefficients"] = {k: C.c_float(v).value for k, v in coefs.items()}       # as the kernel saw them (f32)
    return res, req


def compute(sim, logits, returns=None, stream=None, **kw):
    """HideAndSeekSimulator.value_head."""
    res, req = request(sim.gpu_id, logits, returns, **kw)
    scale = kw.get("loss_scale")
    if scale is None:
        _run(sim, "hs_twohot_value", req, stream)
    else:
        _run(sim, "hs_twohot_value_scaled", req, stream, C.c_void_p(scale.data_ptr()))
    return res


_PER_SHARD = ("mask", "value", "grad_logits", "stats")


def compute_sharded(ssim, logits, returns=None, stream=None, **kw):
    """ShardedSimulator.value_head: every shard computes its own samples on its own device.  Every shard divides by its
    own count of active samples."""
    return _shard_calls(ssim, "hs_twohot_value", request, stream, dict(logits=logits),
                        per_shard=dict({k: kw.pop(k) for k in _PER_SHARD if k in kw}, returns=returns), kw=kw)


def stats_to_metrics(stats):
    """{"value_loss", "mse", "explained_variance", "mean_value", "count"} in float64 from the stats of value_head, on
    their device and without a synchronisation: value_loss the mean cross-entropy, mse the mean of (v - R)^2,
    explained_variance = 1 - mse / var(R) (0 where var(R) is 0), mean_value the mean decoded value.  With no active sample
    everything is 0."""
    import torch
    s = stats.to(torch.float64)
    if s.shape != (STATS,):
        raise ValueError(f"stats have shape ({STATS},), got {tuple(s.shape)}")
    count = s[5]
    n = torch.clamp(count, min=1.0)
    mse, mean_r = s[1] / n, s[3] / n
    var = torch.clamp(s[4] / n - mean_r * mean_r, min=0.0)
    ev = torch.where(var > 0, 1.0 - mse / torch.where(var > 0, var, torch.ones_like(var)), torch.zeros_like(var))
    return {"value_loss": s[0] / n, "mse": mse, "explained_variance": ev, "mean_value": s[2] / n, "count": count}


def attach(logits, out):
    """The scalar float64 value loss of a value_head call — grad_scale * loss_coef * mean cross-entropy, the quantity the
    gradient belongs to — as a tensor of the autograd graph of `logits`: computed from out["stats"] on the device without
    a synchronisation; its backward hands out["grad_logits"] x upstream to autograd.  `out` is the result of the call that
    was given logits.detach().  torch.autograd.backward([logits], [out["grad_logits"]]) is the path with no extra op."""
    import torch
    if "stats" not in out or "grad_logits" not in out:
        raise ValueError("attach needs the stats and grad_logits of the value_head call")
    if tuple(out["grad_logits"].shape) != tuple(logits.shape):
        raise ValueError(f"grad_logits has shape {tuple(out['grad_logits'].shape)}, logits {tuple(logits.shape)}")
    c = out["coefficients"]
    loss = c["grad_scale"] * c["loss_coef"] * stats_to_metrics(out["stats"])["value_loss"]

    class _Attach(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return loss.clone()

        @staticmethod
        def backward(ctx, up):
            gl = out["grad_logits"]
            return (gl * up.to(gl.dtype)).to(logits.dtype)

    return _Attach.apply(logits)
