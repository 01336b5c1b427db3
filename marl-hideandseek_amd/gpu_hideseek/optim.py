"""The optimiser of the update loop: the clip by the global gradient norm and the Adam step of the reference's learner
(scripts/jax_train.py: lr = 1e-4, max_grad_norm = 5) over one flat float32 buffer, in two kernels (hs_adam_step,
csrc/hs_k_adam.h).  include/hideseek.h states the arithmetic: the norm in float64 in a fixed order, the update in IEEE
float32 in a fixed order, so the same inputs give the same bits on every call.  madrona_learn's optimiser is not part of
the reference's tree: the rule is optax's clip_by_global_norm followed by Adam (AdamW with weight_decay > 0), the
project's statement of it.

    net = policy.make_policy(torch.bfloat16).cuda()
    opt = optim.Adam(sim, net.named_parameters(), lr=1e-4, max_grad_norm=5)     # or net.parameters(): names "0", "1", ..
    for minibatch in ...:
        loss(net(...)).backward()            # autograd accumulates straight into the flat gradient buffer
        stats = opt.step()                   # clip + Adam + zero the gradients: two launches, no host synchronisation
    optim.stats_to_metrics(stats)            # {"grad_norm": .., "clip": .., "skipped": .., "step": ..}  (this one waits)

Adam() moves the parameters into one buffer (flatten): every parameter's .data becomes a view of it and every .grad a
view of a gradient buffer of the same layout, each parameter starting at a multiple of PAD = 64 elements (256 bytes) with
zeros in between, which the update leaves at zero and which add nothing to the norm.  Autograd accumulates into a defined
.grad in place, so backward fills the flat buffer without a copy; step() zeroes it again, so there is no zero_grad() in
the loop.

Where this differs from torch.optim.Adam: a parameter that took no part in the graph has a ZERO gradient here and is still
moved by its momentum (and its moments decay), where torch skips a parameter whose .grad is None; a step whose gradient
norm is not finite is skipped as a whole (nothing but the skip count changes; the gradients are still zeroed); the clip
is optax's (g * max_norm / norm when norm > max_norm), not clip_grad_norm_'s max_norm / (norm + 1e-6).

The dynamic loss scale of float16 training (LossScale; hs_adam_step_scaled, csrc/hs_k_loss_scale.h): a scale S on the
device that the two loss kernels multiply their gradients by (ppo_loss and value_head take LossScale.state as
loss_scale=) and that Adam(..., loss_scale=LossScale(device)) divides out again; a step whose norm overflows is skipped
and halves S, growth_interval good steps in a row double it.  Nothing of it reads the device from the host.  The rule is
torch.cuda.amp.GradScaler's and flax's DynamicScale's, the project's statement of it.

Several devices (reduce_gradients; hs_reduce_gradients, csrc/hs_k_reduce.h): data-parallel training keeps one replica of
the parameters and one Adam per shard, and before every step each replica replaces its gradient with the mean over all
shards' active samples, the shards' flat gradient buffers weighted by their counts, in one kernel and in a fixed order.
Every replica reduces copies of the same buffers and so steps with the same bits: nothing is broadcast.  host_reduce is
the numpy restatement of that arithmetic; trainer.ShardedTrainer is the loop built on it.

Not part of this module: parameters SPREAD over several devices (every replica holds all of them), one process per device,
RCCL, overlapping the reduction with the backward pass, a reduce-scatter form for many shards, a bfloat16 / float16 shadow
copy of the weights (the modules cast their weights inside the autograd graph), and a loss scale per parameter group.
"""
import ctypes as C
import math

from ._request import LOSS_SCALE_STATE, _OUTPUT, _above_zero, _disjoint, _finite, _loss_scale_input, _overlap, _run, _tensor

ALIGN = 16                # bytes: params, grads, m and v
PAD = 64                  # elements: every parameter of a flat buffer starts at a multiple of it
MAX_GRID = 256            # HS_ADAM_MAX_GRID: workgroups, and partial sums, of the norm kernel at the most
THREADS = 256             # lanes of a workgroup
VEC = 4                   # floats of a quad: one 16-byte access
STATE = 4                 # HS_ADAM_STATE: beta1^t, beta2^t, t, skipped steps
STATS = 4                 # HS_ADAM_STATS: gnorm, clip, skipped, t after the call
DEFAULTS = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=5.0, grad_scale=1.0)


class HsAdamRequest(C.Structure):
    """hs_adam_request (include/hideseek.h)."""
    _fields_ = [("params", C.c_void_p), ("grads", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64), ("lr", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float), ("max_grad_norm", C.c_double),
                ("grad_scale", C.c_double), ("zero_grad", C.c_int32), ("state", C.c_void_p), ("stats", C.c_void_p)]


class HsLossScale(C.Structure):
    """hs_loss_scale (include/hideseek.h)."""
    _fields_ = [("state", C.c_void_p), ("growth", C.c_double), ("backoff", C.c_double), ("min_scale", C.c_double), ("max_scale", C.c_double),
                ("growth_interval", C.c_int32), ("reserved", C.c_int32)]


REDUCE_MAX_SHARDS = 16    # HS_REDUCE_MAX_SHARDS


class HsGradReduceRequest(C.Structure):
    """hs_grad_reduce_request (include/hideseek.h)."""
    _fields_ = [("src", C.c_void_p * REDUCE_MAX_SHARDS), ("count", C.c_void_p), ("dst", C.c_void_p), ("n", C.c_int64), ("shards", C.c_int32),
                ("total", C.c_void_p)]


def _power_of_two(name, x, lo, hi, bounds):
    """x as a float: 2^k exactly and in [lo, hi]; `bounds` is how the message names the range."""
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(float(x)) or not lo <= float(x) <= hi or math.frexp(float(x))[0] != 0.5:
        raise ValueError(f"{name} must be a power of two, {bounds}, got {x!r}")
    return float(x)


LOSS_SCALE_DEFAULTS = dict(init_scale=2.0 ** 16, growth=2.0, backoff=0.5, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24)
LOSS_SCALE_TOP = 2.0 ** 126           # the largest factor and bound hs_loss_scale takes


def loss_scale_settings(**kw):
    """LossScale's keywords, the missing ones from LOSS_SCALE_DEFAULTS, as checked floats (growth_interval an int):
    powers of two in their ranges.  Raises ValueError; nothing of the device is touched."""
    unknown = sorted(set(kw) - set(LOSS_SCALE_DEFAULTS))
    if unknown:
        raise ValueError(f"unknown loss scale settings {unknown}: expected some of {sorted(LOSS_SCALE_DEFAULTS)}")
    s = dict(LOSS_SCALE_DEFAULTS, **kw)
    tiny, top = 5e-324, LOSS_SCALE_TOP
    out = {"growth": _power_of_two("growth", s["growth"], 1.0, top, "at least 1 and at most 2^126"),
           "backoff": _power_of_two("backoff", s["backoff"], tiny, 1.0, "above 0 and at most 1"),
           "min_scale": _power_of_two("min_scale", s["min_scale"], tiny, top, "above 0 and at most 2^126")}
    out["max_scale"] = _power_of_two("max_scale", s["max_scale"], out["min_scale"], top, "at least min_scale and at most 2^126")
    out["init_scale"] = _power_of_two("init_scale", s["init_scale"], out["min_scale"], out["max_scale"], "in [min_scale, max_scale]")
    n = s["growth_interval"]
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n < 2 ** 31:
        raise ValueError(f"growth_interval must be an integer in [1, 2^31), got {n!r}")
    out["growth_interval"] = n
    return out


class LossScale:
    """The dynamic loss scale: `state`, float64 [4] on `device` = [S, good steps since S last changed, backoffs so far,
    growths so far], starting at [init_scale, 0, 0, 0], and the rule's settings.  A step of an Adam that was given this
    object multiplies S by `backoff` (not below min_scale) when the gradient norm is not finite, and by `growth` (not
    above max_scale) after `growth_interval` good steps in a row; all of them powers of two, so that scaling is exact.
    The bounds are settings, not measurements.  Only read() copies to the host."""

    def __init__(self, device, init_scale=2.0 ** 16, growth=2.0, backoff=0.5, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24):
        s = loss_scale_settings(init_scale=init_scale, growth=growth, backoff=backoff, growth_interval=growth_interval, min_scale=min_scale,
                                max_scale=max_scale)
        init = s.pop("init_scale")
        for k, v in s.items():
            setattr(self, k, v)
        import torch
        self.state = torch.tensor([init, 0.0, 0.0, 0.0], dtype=torch.float64, device=device)

    def request(self):
        """The HsLossScale of a call."""
        return HsLossScale(self.state.data_ptr(), self.growth, self.backoff, self.min_scale, self.max_scale, self.growth_interval, 0)

    def settings(self):
        return {k: getattr(self, k) for k in ("growth", "backoff", "growth_interval", "min_scale", "max_scale")}

    def state_dict(self):
        """{"state": a clone of the state, and the settings}."""
        return dict(self.settings(), state=self.state.clone())

    def load_state_dict(self, state_dict):
        """Load what state_dict() returned: the state and the settings."""
        t = state_dict["state"]
        if tuple(t.shape) != (LOSS_SCALE_STATE,) or t.dtype != self.state.dtype:
            raise ValueError(f"the loss scale's state has shape {tuple(t.shape)} and dtype {t.dtype}: expected ({LOSS_SCALE_STATE},), {self.state.dtype}")
        s = loss_scale_settings(init_scale=state_dict["min_scale"], **{k: state_dict[k] for k in self.settings()})
        for k in self.settings():
            setattr(self, k, s[k])
        self.state.copy_(t)

    def read(self):
        """{"scale", "good_steps", "backoffs", "growths"} as Python numbers (this copies to the host and so waits)."""
        s, good, backoffs, growths = self.state.detach().cpu().tolist()
        return {"scale": s, "good_steps": int(good), "backoffs": int(backoffs), "growths": int(growths)}


def _scaler(loss_scale):
    if loss_scale is not None and not isinstance(loss_scale, LossScale):
        raise ValueError(f"loss_scale must be None or an optim.LossScale, got {loss_scale!r}")
    return loss_scale


def fresh_state(device=None):
    """A state before the first step: float64 [beta1^0, beta2^0, t, skipped steps] = [1, 1, 0, 0]."""
    import torch
    return torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64, device=device)


# ---- the fused call ----
def _f32(name, x):
    """x as the float32 the request carries; finite before and after the rounding."""
    if isinstance(x, bool) or not isinstance(x, (int, float)):
        raise ValueError(f"{name} must be a number, got {x!r}")
    return C.c_float(_finite(name, x)).value


def _f64(name, x):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(float(x)):
        raise ValueError(f"{name} must be finite, got {x!r}")
    return float(x)


def _hyper(lr, betas, eps, weight_decay, max_grad_norm, grad_scale):
    lr, eps, wd = _f32("lr", lr), _f32("eps", eps), _f32("weight_decay", weight_decay)
    gs, mgn = _f64("grad_scale", grad_scale), _f64("max_grad_norm", 0.0 if max_grad_norm is None else max_grad_norm)
    _above_zero("eps", eps)
    if lr < 0.0:
        raise ValueError(f"lr must be at least 0, got {lr}")
    if wd < 0.0:
        raise ValueError(f"weight_decay must be at least 0, got {wd}")
    if not gs > 0.0:
        raise ValueError(f"grad_scale must be above 0, got {gs}")
    try:
        b1, b2 = betas
        b1, b2 = float(b1), float(b2)
    except (TypeError, ValueError):
        raise ValueError(f"betas must be a pair of numbers, got {betas!r}") from None
    b1, b2 = (C.c_float(b).value if math.isfinite(b) else b for b in (b1, b2))
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"betas must be in [0, 1) as float32, got {betas!r}")
    return lr, b1, b2, eps, wd, mgn, gs


def request(gpu_id, params, grads, m, v, state, lr=DEFAULTS["lr"], betas=DEFAULTS["betas"], eps=DEFAULTS["eps"],
            weight_decay=DEFAULTS["weight_decay"], max_grad_norm=DEFAULTS["max_grad_norm"], grad_scale=DEFAULTS["grad_scale"], zero_grad=True,
            stats=True, loss_scale=None):
    """Validate one optimiser step on GPU `gpu_id` over the flat float32 tensors params, grads, m and v [n] (contiguous,
    16-byte aligned, no two overlapping) and the float64 state [4] (fresh_state()), allocate stats [4] float64 when given
    as True (None: no statistics), and return ({"stats": tensor} or {}, HsAdamRequest).  max_grad_norm <= 0 or None
    switches the clip off.  `loss_scale` is None or a LossScale, whose state may overlap none of the others (compute then
    runs hs_adam_step_scaled).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    hyper = _hyper(lr, betas, eps, weight_decay, max_grad_norm, grad_scale)
    _scaler(loss_scale)
    if not isinstance(params, torch.Tensor):
        raise ValueError("params must be a torch tensor")
    if params.dim() != 1 or not 1 <= params.shape[0] < 2 ** 31:
        raise ValueError(f"params must be a contiguous float32 tensor of shape (n,), 1 <= n < 2^31, on {dev}: its shape is {tuple(params.shape)}")
    n = int(params.shape[0])
    arrays = [("params", params), ("grads", grads), ("m", m), ("v", v)]
    for name, t in arrays:
        _tensor(name, t, (n,), ("float32",), dev, align=ALIGN)
    _tensor("state", state, (STATE,), ("float64",), dev)
    arrays.append(("state", state))
    if stats is not None and stats is not False:
        if stats is not True:
            _tensor("stats", stats, (STATS,), ("float64",), dev, _OUTPUT)
            arrays.append(("stats", stats))
    else:
        stats = None
    arrays += _loss_scale_input(None if loss_scale is None else loss_scale.state, dev)
    _disjoint(arrays, [], dev)
    if stats is True:
        stats = torch.empty(STATS, dtype=torch.float64, device=dev)
    req = HsAdamRequest(params.data_ptr(), grads.data_ptr(), m.data_ptr(), v.data_ptr(), n, *hyper, 1 if zero_grad else 0, state.data_ptr(),
                        None if stats is None else stats.data_ptr())
    return ({} if stats is None else {"stats": stats}), req


def compute(sim, params, grads, m, v, state, stream=None, **kw):
    """HideAndSeekSimulator.adam_step."""
    res, req = request(sim.gpu_id, params, grads, m, v, state, **kw)
    _step(sim, req, kw.get("loss_scale"), stream)
    return res


def _step(sim, req, loss_scale, stream):
    if loss_scale is None:
        _run(sim, "hs_adam_step", req, stream)
    else:
        _run(sim, "hs_adam_step_scaled", req, stream, C.byref(loss_scale.request()))


def stats_to_metrics(stats):
    """The statistics of a step as Python numbers (this copies to the host and so waits for the step)."""
    gnorm, clip, skipped, step = stats.detach().cpu().tolist()
    return {"grad_norm": gnorm, "clip": clip, "skipped": bool(skipped), "step": int(step)}


# ---- the reduction of gradients between shards ----
def host_reduce(srcs, counts):
    """hs_reduce_gradients in numpy, operation by operation as include/hideseek.h states it: (dst float32 [n], C).  The
    counts, their sum C (in index order, over the counts that are not 0) and the quotients are float64; a weight is the
    quotient rounded to float32 once; every product and every sum is float32, the first product taken as it is and the
    others added in index order.  A shard whose count is 0 is left out, whatever it holds; with every count 0 the result
    is +0."""
    import numpy as np
    srcs = [np.asarray(x, np.float32).reshape(-1) for x in srcs]
    counts = np.asarray(counts, np.float64).reshape(-1)
    if not 1 <= len(srcs) <= REDUCE_MAX_SHARDS or counts.shape[0] != len(srcs) or any(x.shape != srcs[0].shape for x in srcs):
        raise ValueError(f"1 to {REDUCE_MAX_SHARDS} arrays of one length and one count for each expected")
    live = [g for g in range(len(srcs)) if counts[g] != 0.0]
    total = np.float64(0.0)
    acc = np.zeros(srcs[0].shape[0], np.float32)
    with np.errstate(all="ignore"):
        for g in live:
            total = total + counts[g]
        for k, g in enumerate(live):
            prod = np.float32(counts[g] / total) * srcs[g]
            acc = prod if k == 0 else acc + prod
    assert acc.dtype == np.float32
    return acc, float(total)


def reduce_request(gpu_id, srcs, counts, out=None, total=None):
    """Validate one reduction on GPU `gpu_id`: `srcs`, a list of 1 to REDUCE_MAX_SHARDS float32 tensors [n] (contiguous,
    16-byte aligned), `counts` float64 [len(srcs)], `out` None or True (allocated) or a float32 tensor [n] that is one of
    the sources (the same address) or overlaps none, `total` None, True or a float64 tensor [1] that overlaps nothing else.
    Returns ({"out": tensor[, "total": tensor]}, HsGradReduceRequest).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    if isinstance(srcs, torch.Tensor) or not isinstance(srcs, (list, tuple)) or not 1 <= len(srcs) <= REDUCE_MAX_SHARDS:
        raise ValueError(f"srcs must be a list of 1 to {REDUCE_MAX_SHARDS} torch tensors, one per shard")
    G = len(srcs)
    if not isinstance(srcs[0], torch.Tensor):
        raise ValueError("srcs[0] must be a torch tensor")
    if srcs[0].dim() != 1 or not 1 <= srcs[0].shape[0] < 2 ** 31:
        raise ValueError(f"srcs[0] must be a contiguous float32 tensor of shape (n,), 1 <= n < 2^31, on {dev}: its shape is {tuple(srcs[0].shape)}")
    n = int(srcs[0].shape[0])
    inputs = [(f"srcs[{g}]", t) for g, t in enumerate(srcs)]
    for name, t in inputs:
        _tensor(name, t, (n,), ("float32",), dev, align=ALIGN)
    _tensor("counts", counts, (G,), ("float64",), dev)
    inputs.append(("counts", counts))
    given = []
    if out is not None and out is not True:
        _tensor("out", out, (n,), ("float32",), dev, _OUTPUT, align=ALIGN)
        given.append(("out", out))
    if total is not None and total is not False and total is not True:
        _tensor("total", total, (1,), ("float64",), dev, _OUTPUT)
        given.append(("total", total))
    for k, (name, t) in enumerate(given):                    # out may be one source itself; total overlaps nothing
        same = [other for other, x in inputs[:G] if name == "out" and x.data_ptr() == t.data_ptr()]
        if len(same) > 1:
            raise ValueError(f"out is more than one of the sources: {', '.join(same)}")
        for other, x in inputs + given[:k]:
            if other not in same and _overlap(t, x):
                raise ValueError(f"{name} overlaps {other}" + (" without being it" if other.startswith("srcs") and name == "out" else ""))
    _disjoint([], inputs + given, dev)                       # the device, last
    res = {"out": torch.empty(n, dtype=torch.float32, device=dev) if out is None or out is True else out}
    if total is not None and total is not False:
        res["total"] = torch.empty(1, dtype=torch.float64, device=dev) if total is True else total
    req = HsGradReduceRequest()
    for g, t in enumerate(srcs):
        req.src[g] = t.data_ptr()
    req.count, req.dst, req.n, req.shards = counts.data_ptr(), res["out"].data_ptr(), n, G
    req.total = res["total"].data_ptr() if "total" in res else None
    return res, req


def reduce_gradients(sim, srcs, counts, out=None, total=None, stream=None):
    """HideAndSeekSimulator.reduce_gradients."""
    res, req = reduce_request(sim.gpu_id, srcs, counts, out, total)
    _run(sim, "hs_reduce_gradients", req, stream)
    return res


# ---- the flat buffer ----
def _named(parameters):
    """[(name, parameter)] of an iterable of parameters ("0", "1", ...) or of (name, parameter) pairs."""
    import torch
    out = []
    for i, item in enumerate(parameters):
        name, p = item if isinstance(item, tuple) else (str(i), item)
        if not isinstance(name, str) or not isinstance(p, torch.Tensor):
            raise ValueError(f"parameters must be tensors or (name, tensor) pairs, got {item!r}")
        out.append((name, p))
    if not out:
        raise ValueError("no parameters")
    if len({name for name, _ in out}) != len(out) or len({id(p) for _, p in out}) != len(out):
        raise ValueError("a parameter or a name is given twice")
    return out


class Flat:
    """What flatten() made: `params` and `grads`, the two flat float32 buffers, and `entries`, [(name, parameter, first,
    one past the last, shape)] in the order given."""

    def __init__(self, params, grads, entries):
        self.params, self.grads, self.entries = params, grads, entries

    def layout(self):
        """{name: (first, one past the last, shape)}: the element range of every parameter in either buffer."""
        return {name: (lo, hi, shape) for name, _, lo, hi, shape in self.entries}

    def view(self, buf, name):
        lo, hi, shape = self.layout()[name]
        return buf[lo:hi].view(shape)

    def attach(self):
        """Point every parameter's .data and .grad at its views again (after a zero_grad(set_to_none=True) by hand)."""
        for _, p, lo, hi, shape in self.entries:
            p.data = self.params[lo:hi].view(shape)
            p.grad = self.grads[lo:hi].view(shape)

    def detached(self):
        """The name of the first parameter whose .data or .grad no longer starts where its view does, or None."""
        size, p0, g0 = self.params.element_size(), self.params.data_ptr(), self.grads.data_ptr()
        for name, p, lo, _, _ in self.entries:
            g = p.grad
            if g is None or g.data_ptr() != g0 + lo * size or p.data_ptr() != p0 + lo * size:
                return name
        return None


def flatten(parameters, device=None):
    """Copy the parameters (tensors or (name, tensor) pairs, float32) into one float32 buffer on `device` (by default the
    first parameter's), in the order given, each starting at a multiple of PAD elements, zeros in between and up to the
    padded length; re-point every parameter's .data at its view; make a gradient buffer of the same layout (a .grad
    that exists is copied in) and set every .grad to its view.  Returns a Flat."""
    import torch
    named = _named(parameters)
    for name, p in named:
        if p.dtype != torch.float32:
            raise ValueError(f"parameter {name} must be float32: its dtype is {p.dtype}")
    device = named[0][1].device if device is None else torch.device(device)
    spans, at = [], 0
    for name, p in named:
        spans.append((at, at + p.numel()))
        at = -(-(at + p.numel()) // PAD) * PAD
    if not 1 <= at < 2 ** 31:
        raise ValueError(f"the flat buffer would have {at} elements: 1 <= n < 2^31")
    flat, grads = torch.zeros(at, dtype=torch.float32, device=device), torch.zeros(at, dtype=torch.float32, device=device)
    entries = []
    with torch.no_grad():
        for (name, p), (lo, hi) in zip(named, spans):
            shape = tuple(p.shape)
            flat[lo:hi].view(shape).copy_(p.detach())
            if p.grad is not None:
                grads[lo:hi].view(shape).copy_(p.grad.detach())
            entries.append((name, p, lo, hi, shape))
    out = Flat(flat, grads, entries)
    out.attach()
    return out


# ---- the optimiser ----
def _optimizer_base():
    import torch
    return torch.optim.Optimizer


class Adam(_optimizer_base()):
    """A torch optimiser with one parameter group over flatten()'s buffers on `sim`'s device.  step() makes one
    hs_adam_step call (sim.adam_step's entry point) with zero_grad=True, reading lr, betas, eps, weight_decay, max_grad_norm and grad_scale from
    param_groups[0] on every call (LR schedulers and PBT's exploration of lr change them there), and returns the device
    tensor of the statistics without synchronising: the optimiser's own tensor, overwritten by the next step (clone it to
    keep it; stats_to_metrics reads it).  With loss_scale, a LossScale on the same device, step() makes the
    hs_adam_step_scaled call instead: the gradients are divided by the scale, a step that overflowed is skipped and the
    scale adjusted, all on the device.  The module docstring says where this differs from torch.optim.Adam."""

    def __init__(self, sim, parameters, lr=DEFAULTS["lr"], betas=DEFAULTS["betas"], eps=DEFAULTS["eps"], weight_decay=DEFAULTS["weight_decay"],
                 max_grad_norm=DEFAULTS["max_grad_norm"], grad_scale=DEFAULTS["grad_scale"], loss_scale=None):
        import torch
        named = _named(parameters)
        _hyper(lr, betas, eps, weight_decay, max_grad_norm, grad_scale)
        self.sim, self.loss_scale = sim, _scaler(loss_scale)
        device = torch.device("cuda", sim.gpu_id)
        self.flat = flatten(named, device)
        self.m, self.v = torch.zeros_like(self.flat.params), torch.zeros_like(self.flat.params)
        self.adam_state = fresh_state(device)
        self.stats = torch.zeros(STATS, dtype=torch.float64, device=device)
        request(sim.gpu_id, self.flat.params, self.flat.grads, self.m, self.v, self.adam_state, stats=self.stats,
                loss_scale=self.loss_scale)                                                                               # the buffers, checked once
        super().__init__([p for _, p in named], dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                                     max_grad_norm=max_grad_norm, grad_scale=grad_scale))

    def layout(self):
        return self.flat.layout()

    def step(self, stream=None):
        """Clip, update and zero the gradients: blocking with stream=None, else enqueued on the torch.cuda.Stream (or raw
        handle) without synchronising.  Raises ValueError, naming the parameter, if a .grad (or .data) is no longer the
        optimiser's view."""
        if callable(stream):
            raise ValueError("closures are not supported: step(stream=None)")
        lost = self.flat.detached()
        if lost is not None:
            raise ValueError(f"parameter {lost}: its .grad or .data is no longer the optimiser's view of the flat buffer "
                             "(zero_grad(set_to_none=True)?): call this optimiser's zero_grad() to attach the views again")
        g = self.param_groups[0]
        hyper = _hyper(g["lr"], g["betas"], g["eps"], g["weight_decay"], g["max_grad_norm"], g["grad_scale"])
        # the buffers are the optimiser's own and passed request() when it was built: only the hyper-parameters are new
        req = HsAdamRequest(self.flat.params.data_ptr(), self.flat.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.flat.params.numel(),
                            *hyper, 1, self.adam_state.data_ptr(), self.stats.data_ptr())
        _step(self.sim, req, self.loss_scale, stream)
        return self.stats

    def zero_grad(self, set_to_none=False):
        """Attach the views again and zero the flat gradient buffer (set_to_none is ignored: the gradients stay the
        views).  step() zeroes the gradients itself; this is only needed after they were detached by hand."""
        self.flat.attach()
        self.flat.grads.zero_()

    def state_dict(self):
        """{"m", "v": the flat moments, "state": the 4-element state, "layout": {name: (first, last, shape)},
        "param_groups": the hyper-parameters}: clones.  With a loss scale also "loss_scale": its state_dict()."""
        hyper = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
        out = {"m": self.m.clone(), "v": self.v.clone(), "state": self.adam_state.clone(),
               "layout": {k: (lo, hi, tuple(shape)) for k, (lo, hi, shape) in self.layout().items()}, "param_groups": hyper}
        if self.loss_scale is not None:
            out["loss_scale"] = self.loss_scale.state_dict()
        return out

    def load_state_dict(self, state_dict):
        """Load what state_dict() returned.  Raises ValueError if its layout is not this optimiser's, or if only one of
        the two has a loss scale."""
        if ("loss_scale" in state_dict) != (self.loss_scale is not None):
            raise ValueError("the state %s a loss scale and this optimiser %s" % (("has", "has none") if "loss_scale" in state_dict else ("has no", "has one")))
        theirs = {k: (int(lo), int(hi), tuple(shape)) for k, (lo, hi, shape) in state_dict["layout"].items()}
        if theirs != self.layout() or list(theirs) != list(self.layout()):
            raise ValueError("the state's layout differs from this optimiser's: other parameters, shapes or order")
        for k, t in (("m", self.m), ("v", self.v), ("state", self.adam_state)):
            if tuple(state_dict[k].shape) != tuple(t.shape) or state_dict[k].dtype != t.dtype:
                raise ValueError(f"the state's {k} has shape {tuple(state_dict[k].shape)} and dtype {state_dict[k].dtype}: expected {tuple(t.shape)}, {t.dtype}")
        for k, t in (("m", self.m), ("v", self.v), ("state", self.adam_state)):
            t.copy_(state_dict[k])
        if self.loss_scale is not None:
            self.loss_scale.load_state_dict(state_dict["loss_scale"])
        for g, saved in zip(self.param_groups, state_dict.get("param_groups", [])):
            g.update({k: v for k, v in saved.items() if k != "params"})

    stats_to_metrics = staticmethod(stats_to_metrics)
