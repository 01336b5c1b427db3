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

from ._request import _DTYPES, _OUTPUT, _disjoint, _name, _run, _shard_calls, _tensor, _wanted

MAX_STEPS = 4096      # HS_GAE_MAX_STEPS
MOMENTS = 5           # HS_GAE_MOMENTS: sum adv, sum adv^2, sum ret, sum ret^2, count of active (t, row) pairs
DEFAULT_GAMMA = 0.998         # scripts/jax_train.py:152
DEFAULT_LAMBDA = 0.95         # scripts/jax_train.py:153


class HsGaeRequest(C.Structure):
    """hs_gae_request (include/hideseek.h)."""
    _fields_ = [("reward", C.c_void_p), ("done", C.c_void_p), ("value", C.c_void_p), ("bootstrap", C.c_void_p),
                ("mask", C.c_void_p), ("value_dtype", C.c_int32), ("steps", C.c_int32), ("gamma", C.c_float),
                ("lambda", C.c_float), ("advantage", C.c_void_p), ("returns", C.c_void_p), ("moments", C.c_void_p)]


class HsGaeGroupedRequest(C.Structure):
    """hs_gae_grouped_request (include/hideseek.h)."""
    _fields_ = [("gae", HsGaeRequest), ("groups", C.c_int32), ("reserved", C.c_int32)]


MAX_GROUPS = 16       # HS_LEAGUE_MAX_POLICIES


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


def request(num_worlds, agents, gpu_id, rewards, dones, values, bootstrap, gamma=DEFAULT_GAMMA, gae_lambda=DEFAULT_LAMBDA,
            mask=None, advantages=True, returns=True, moments=None, groups=None):
    """Validate a call over num_worlds x agents agent rows on GPU `gpu_id`, allocate the outputs given as True, and
    return ({name: tensor}, HsGaeRequest).  With `groups` = G (an integer in [1, MAX_GROUPS] that divides the rows) the
    rows are G groups of rows / G consecutive rows, `moments` is [G, 5], one vector per group, and the request is an
    HsGaeGroupedRequest (hs_compute_gae_grouped).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    rows = num_worlds * agents
    if groups is not None:
        if isinstance(groups, bool) or not isinstance(groups, int) or not 1 <= groups <= MAX_GROUPS:
            raise ValueError(f"groups must be None or an integer in [1, {MAX_GROUPS}], got {groups!r}")
        if rows % groups:
            raise ValueError(f"the number of agent rows ({rows}) must be a multiple of groups ({groups})")
    mshape = (MOMENTS,) if groups is None else (groups, MOMENTS)
    gamma, gae_lambda = float(gamma), float(gae_lambda)
    if not (math.isfinite(gamma) and 0.0 <= gamma <= 1.0):
        raise ValueError(f"gamma must be finite and in [0, 1], got {gamma}")
    if not (math.isfinite(gae_lambda) and 0.0 <= gae_lambda <= 1.0):
        raise ValueError(f"gae_lambda must be finite and in [0, 1], got {gae_lambda}")
    outputs = _wanted((("advantages", advantages), ("returns", returns), ("moments", moments)), "none of advantages, returns and moments requested")

    def per_step(T):      # the shapes of a [T, rows] tensor
        return [(T, rows), (T, rows, 1), (T, num_worlds, agents)]
    empty = isinstance(rewards, torch.Tensor) and rewards.dim() > 1 and rewards.shape[0] == 0      # T = 0 is told as a count of steps below
    _tensor("rewards", rewards, per_step(0 if empty else "T"), ("float32",), dev)
    steps = int(rewards.shape[0])
    if steps < 1 or steps > MAX_STEPS:
        raise ValueError(f"rewards must have T in [1, {MAX_STEPS}] steps, got T = {steps}")
    _tensor("dones", dones, per_step(steps), ("int32",), dev)
    _tensor("values", values, per_step(steps), _DTYPES, dev)
    if mask is not None:
        _tensor("mask", mask, per_step(steps), ("float32",), dev)
    _tensor("bootstrap", bootstrap, [(rows,), (rows, 1), (num_worlds, agents)], (_name(values.dtype),), dev)      # the dtype of values
    given = {k: t for k, t in outputs.items() if t is not True}
    for k, t in given.items():
        if k == "moments":
            _tensor(k, t, mshape, ("float64",), dev, _OUTPUT)
        else:
            _tensor(k, t, per_step(steps), ("float32",), dev, _OUTPUT)
    # overlaps are left to the library, which refuses them: only the devices are looked at here, and last
    _disjoint([], [(k, t) for k, t in (("rewards", rewards), ("dones", dones), ("values", values), ("bootstrap", bootstrap), ("mask", mask),
                                       *given.items()) if t is not None], dev)
    res = {k: given[k] if k in given else torch.empty(mshape if k == "moments" else tuple(rewards.shape),
                                                      dtype=torch.float64 if k == "moments" else torch.float32, device=dev) for k in outputs}

    def ptr(k):
        return res[k].data_ptr() if k in res else None
    req = HsGaeRequest(rewards.data_ptr(), dones.data_ptr(), values.data_ptr(), bootstrap.data_ptr(),
                       mask.data_ptr() if mask is not None else None, _DTYPES[_name(values.dtype)], steps, gamma,
                       gae_lambda, ptr("advantages"), ptr("returns"), ptr("moments"))
    if groups is not None:
        req = HsGaeGroupedRequest(req, groups, 0)
    return res, req


def compute(sim, rewards, dones, values, bootstrap, stream=None, **kw):
    """HideAndSeekSimulator.compute_advantages."""
    res, req = request(sim.num_worlds, sim.agents_per_world, sim.gpu_id, rewards, dones, values, bootstrap, **kw)
    _run(sim, "hs_compute_gae_grouped" if isinstance(req, HsGaeGroupedRequest) else "hs_compute_gae", req, stream)
    return res


def compute_sharded(ssim, rewards, dones, values, bootstrap, stream=None, mask=None, advantages=True, returns=True,
                    moments=None, **kw):
    """ShardedSimulator.compute_advantages: every shard computes its own rows on its own device."""
    return _shard_calls(ssim, "hs_compute_gae", request, stream, dict(rewards=rewards, dones=dones, values=values, bootstrap=bootstrap),
                        per_shard=dict(mask=mask, advantages=advantages, returns=returns, moments=moments), kw=kw,
                        lead=lambda s: (s.num_worlds, s.agents_per_world, s.gpu_id))
