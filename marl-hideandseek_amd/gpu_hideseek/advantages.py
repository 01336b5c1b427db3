"""Advantages and value targets: the rewards, dones and critic values of a rollout turned into GAE advantages and
returns by one kernel (hs_compute_gae, csrc/hs_k_gae.h).

The leg after the last step of a rollout, as the reference trains (scripts/jax_train.py:45,152-153: gamma 0.998,
gae_lambda 0.95, 40 steps per update).  include/hideseek.h states the arithmetic, IEEE f32 in a fixed order: the result
is the same bit for bit on every call, and for every way of dealing the worlds to shards.

    rewards[t].copy_(sim.reward_tensor().to_torch()[:, 0])        # after every step of the rollout, likewise dones, masks
    ...
    out = sim.compute_advantages(rewards, dones, values, bootstrap, mask=masks, moments=True)
    mean, std = advantages.moments_to_mean_std(out["moments"])["advantages"]
    adv = (out["advantages"] - mean) / (std + 1e-8)
"""
import ctypes as C
import math

from ._request import _DTYPES, _name, _per_shard, _run, _sharded

MAX_STEPS = 4096      # HS_GAE_MAX_STEPS
MOMENTS = 5           # HS_GAE_MOMENTS: sum adv, sum adv^2, sum ret, sum ret^2, count of active (t, row) pairs
DEFAULT_GAMMA = 0.998         # scripts/jax_train.py:152
DEFAULT_LAMBDA = 0.95         # scripts/jax_train.py:153


class HsGaeRequest(C.Structure):
    """hs_gae_request (include/hideseek.h)."""
    _fields_ = [("reward", C.c_void_p), ("done", C.c_void_p), ("value", C.c_void_p), ("bootstrap", C.c_void_p),
                ("mask", C.c_void_p), ("value_dtype", C.c_int32), ("steps", C.c_int32), ("gamma", C.c_float),
                ("lambda", C.c_float), ("advantage", C.c_void_p), ("returns", C.c_void_p), ("moments", C.c_void_p)]


def moments_to_mean_std(moments):
    """{"count": n, "advantages": (mean, std), "returns": (mean, std)} in float64 from the moments of
    compute_advantages: the statistics (biased standard deviation) of the active (t, row) pairs, for the advantage
    normaliser and the value normaliser.  With no active pair, mean and std are 0."""
    import torch
    m = moments.to(torch.float64)
    if m.shape != (MOMENTS,):
        raise ValueError(f"moments have shape ({MOMENTS},), got {tuple(m.shape)}")
    count = m[4]
    n = torch.clamp(count, min=1.0)

    def mean_std(s1, s2):
        mean = s1 / n
        return mean, torch.sqrt(torch.clamp(s2 / n - mean * mean, min=0.0))
    return {"count": count, "advantages": mean_std(m[0], m[1]), "returns": mean_std(m[2], m[3])}


def _steps_of(t, rows, worlds, agents):
    """T of a [T, rows] / [T, rows, 1] / [T, worlds, agents] tensor, or None."""
    shape = tuple(t.shape)
    if len(shape) >= 2 and shape[1:] in ((rows,), (rows, 1), (worlds, agents)):
        return shape[0]
    return None


def _input(name, t, steps, rows, worlds, agents, dev, dtypes):
    """Check the layout of [T, rows]-shaped input `name` (steps None: take T from it) and return T."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    what = (f"{name} must be a contiguous {' / '.join(dtypes)} tensor of shape ({'T' if steps is None else steps}, {rows}) "
            f"or ({'T' if steps is None else steps}, {worlds}, {agents}) on {dev}")
    T = _steps_of(t, rows, worlds, agents)
    if T is None or (steps is not None and T != steps):
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if _name(t.dtype) not in dtypes:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: it is not contiguous")
    return T


def _output(name, t, like, steps, rows, worlds, agents, dev):
    """The tensor output `name` is written to: `t` itself when it is a tensor (checked), a new one when it is True."""
    import torch
    if name == "moments":
        shape, dt = (MOMENTS,), "float64"
    else:
        shape, dt = tuple(like.shape), "float32"
    if t is True:
        return torch.empty(shape, dtype=getattr(torch, dt), device=dev)
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be True, None or a torch tensor")
    what = f"{name} must be a contiguous {dt} tensor of shape {shape} on {dev}"
    if tuple(t.shape) != shape and (name == "moments" or _steps_of(t, rows, worlds, agents) != steps):
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if _name(t.dtype) != dt:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: it is not contiguous")
    return t


def request(num_worlds, agents, gpu_id, rewards, dones, values, bootstrap, gamma=DEFAULT_GAMMA, gae_lambda=DEFAULT_LAMBDA,
            mask=None, advantages=True, returns=True, moments=None):
    """Validate a call over num_worlds x agents agent rows on GPU `gpu_id`, allocate the outputs given as True, and
    return ({name: tensor}, HsGaeRequest).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    rows = num_worlds * agents
    gamma, gae_lambda = float(gamma), float(gae_lambda)
    if not (math.isfinite(gamma) and 0.0 <= gamma <= 1.0):
        raise ValueError(f"gamma must be finite and in [0, 1], got {gamma}")
    if not (math.isfinite(gae_lambda) and 0.0 <= gae_lambda <= 1.0):
        raise ValueError(f"gae_lambda must be finite and in [0, 1], got {gae_lambda}")
    outputs = {k: t for k, t in (("advantages", advantages), ("returns", returns), ("moments", moments))
               if t is not None and t is not False}
    if not outputs:
        raise ValueError("nothing to do: none of advantages, returns and moments requested")

    steps = _input("rewards", rewards, None, rows, num_worlds, agents, dev, ("float32",))
    if steps < 1 or steps > MAX_STEPS:
        raise ValueError(f"rewards must have T in [1, {MAX_STEPS}] steps, got T = {steps}")
    _input("dones", dones, steps, rows, num_worlds, agents, dev, ("int32",))
    _input("values", values, steps, rows, num_worlds, agents, dev, tuple(_DTYPES))
    if mask is not None:
        _input("mask", mask, steps, rows, num_worlds, agents, dev, ("float32",))
    if not isinstance(bootstrap, torch.Tensor):
        raise ValueError("bootstrap must be a torch tensor")
    what = f"bootstrap must be a contiguous {_name(values.dtype)} tensor (the dtype of values) of shape ({rows},) or ({num_worlds}, {agents}) on {dev}"
    if tuple(bootstrap.shape) not in ((rows,), (rows, 1), (num_worlds, agents)):
        raise ValueError(f"{what}: its shape is {tuple(bootstrap.shape)}")
    if bootstrap.dtype != values.dtype:
        raise ValueError(f"{what}: its dtype is {bootstrap.dtype}")
    if not bootstrap.is_contiguous():
        raise ValueError(f"{what}: it is not contiguous")
    given = {k: _output(k, t, rewards, steps, rows, num_worlds, agents, dev) for k, t in outputs.items() if t is not True}
    # shapes, dtypes and strides first, so that every one of them is reported whatever device the tensors are on
    for k, t in (("rewards", rewards), ("dones", dones), ("values", values), ("bootstrap", bootstrap), ("mask", mask), *given.items()):
        if t is not None and t.device != dev:
            raise ValueError(f"{k} must be on {dev}: it is on {t.device}")
    res = {k: given[k] if k in given else _output(k, True, rewards, steps, rows, num_worlds, agents, dev) for k in outputs}

    def ptr(k):
        return res[k].data_ptr() if k in res else None
    req = HsGaeRequest(rewards.data_ptr(), dones.data_ptr(), values.data_ptr(), bootstrap.data_ptr(),
                       mask.data_ptr() if mask is not None else None, _DTYPES[_name(values.dtype)], steps, gamma,
                       gae_lambda, ptr("advantages"), ptr("returns"), ptr("moments"))
    return res, req


def compute(sim, rewards, dones, values, bootstrap, stream=None, **kw):
    """HideAndSeekSimulator.compute_advantages."""
    res, req = request(sim.num_worlds, sim.agents_per_world, sim.gpu_id, rewards, dones, values, bootstrap, **kw)
    _run(sim, "hs_compute_gae", req, stream)
    return res


def compute_sharded(ssim, rewards, dones, values, bootstrap, stream=None, mask=None, advantages=True, returns=True,
                    moments=None, **kw):
    """ShardedSimulator.compute_advantages: every shard computes its own rows on its own device.  `rewards`, `dones`,
    `values` and `bootstrap` have one tensor per shard; `mask`, each output and `stream` are True / None for all shards
    or a list with one entry per shard; returns the list of the shards' results.  With stream=None every shard's call is
    enqueued on a side stream of its device, ordered after that device's current stream, before any is waited for."""
    import torch
    n = len(ssim.shards)
    for name, arg in (("rewards", rewards), ("dones", dones), ("values", values), ("bootstrap", bootstrap)):
        if isinstance(arg, torch.Tensor) or len(arg) != n:
            raise ValueError(f"{name}: one tensor per shard ({n}) expected")
    opt = {k: _per_shard(ssim, k, v) for k, v in (("mask", mask), ("advantages", advantages), ("returns", returns), ("moments", moments))}
    return _sharded(ssim, "hs_compute_gae",
                    lambda i, s: request(s.num_worlds, s.agents_per_world, s.gpu_id, rewards[i], dones[i], values[i], bootstrap[i],
                                         **{k: v[i] for k, v in opt.items()}, **kw), stream)
