"""Action sampling: the actor's logits of every agent row turned into the [rows, 5] int32 action the next step reads,
with the log-probability and entropy a PPO learner stores, by one kernel (hs_sample_actions, csrc/hs_k_sample.h).

The leg after the network, for a multi-discrete actor head as the reference's learner has it
(scripts/jax_train.py:146-148, actions_num_buckets = [5, 5, 5, 2, 2]).  include/hideseek.h states the arithmetic and how
the uniform of a (row, head) is keyed by (seed, counter, global agent row): a draw does not depend on how the worlds are
dealt to shards.

    out = sim.sample_actions(logits, seed=(run_seed, 0), counter=t, log_prob=rollout_lp[t], entropy=True)
    sim.step()                                  # the actions are already in action_tensor()
    ...
    new = sim.sample_actions(new_logits, mode="evaluate", action=rollout_actions[t], log_prob=True, entropy=True)
"""
import ctypes as C

from ._request import _DTYPES, _name, _run, _shard_calls

HEADS = 5             # HS_SAMPLE_HEADS
MAX_BUCKETS = 16      # HS_SAMPLE_MAX_BUCKETS
MAX_LOGITS = 64       # HS_SAMPLE_MAX_LOGITS
MODES = {"draw": 0, "greedy": 1, "evaluate": 2}       # HS_SAMPLE_DRAW / _GREEDY / _EVALUATE
ZERO_INACTIVE = 1     # HS_SAMPLE_ZERO_INACTIVE
DEFAULT_BUCKETS = (5, 5, 5, 2, 2)

# output -> (trailing shape, dtype name)
_OUTPUTS = {"action": ((HEADS,), "int32"), "log_prob": ((), "float32"), "entropy": ((), "float32"),
            "head_log_prob": ((HEADS,), "float32")}


class HsSampleRequest(C.Structure):
    """hs_sample_request (include/hideseek.h)."""
    _fields_ = [("logits", C.c_void_p), ("logits_dtype", C.c_int32), ("logits_stride", C.c_int32),
                ("buckets", C.c_int32 * HEADS), ("mode", C.c_int32), ("flags", C.c_uint32), ("seed", C.c_uint32 * 2),
                ("counter", C.c_uint32), ("action", C.c_void_p), ("log_prob", C.c_void_p), ("entropy", C.c_void_p),
                ("head_log_prob", C.c_void_p)]


def _output(name, t, rows, dev):
    """The tensor output `name` is written to: `t` itself when it is a tensor (checked), a new one when it is True."""
    import torch
    tail, dt = _OUTPUTS[name]
    shape = (rows,) + tail
    if t is True:
        return torch.empty(shape, dtype=getattr(torch, dt), device=dev)
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be True, None or a torch tensor")
    what = f"{name} must be a contiguous {dt} tensor of shape {shape} on {dev}"
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if _name(t.dtype) != dt:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: it is not contiguous")
    if t.device != dev:
        raise ValueError(f"{what}: it is on {t.device}")
    return t


def request(rows, gpu_id, logits, buckets=DEFAULT_BUCKETS, mode="draw", seed=(0, 0), counter=0, action=None,
            log_prob=None, entropy=None, head_log_prob=None, zero_inactive=False):
    """Validate a sampling call over `rows` agent rows on GPU `gpu_id`, allocate the outputs given as True, and return
    ({name: tensor}, HsSampleRequest).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    buckets = tuple(int(b) for b in buckets)
    if len(buckets) != HEADS or any(b < 1 or b > MAX_BUCKETS for b in buckets):
        raise ValueError(f"buckets must be {HEADS} counts in [1, {MAX_BUCKETS}], got {buckets}")
    L = sum(buckets)
    if L > MAX_LOGITS:
        raise ValueError(f"buckets sum to {L} logits per row, more than {MAX_LOGITS}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {', '.join(MODES)}, got {mode!r}")
    if len(seed) != 2:
        raise ValueError("seed must be a pair of 32-bit integers")
    outputs = {k: t for k, t in (("action", action), ("log_prob", log_prob), ("entropy", entropy),
                                 ("head_log_prob", head_log_prob)) if t is not None and t is not False}
    if mode == "evaluate":
        if action is True:
            raise ValueError("mode 'evaluate' reads the actions: action must be a tensor or None (action_tensor())")
        if not any(k != "action" for k in outputs):
            raise ValueError("nothing to do: mode 'evaluate' with no output requested")

    if not isinstance(logits, torch.Tensor):
        raise ValueError("logits must be a torch tensor")
    what = f"logits must be a {' / '.join(_DTYPES)} tensor of shape ({rows}, W >= {L}), contiguous in its last dimension, on {dev}"
    if logits.dim() != 2 or logits.shape[0] != rows or logits.shape[1] < L:
        raise ValueError(f"{what}: its shape is {tuple(logits.shape)}")
    if _name(logits.dtype) not in _DTYPES:
        raise ValueError(f"{what}: its dtype is {logits.dtype}")
    if logits.stride(1) != 1 or (rows > 1 and logits.stride(0) < L) or logits.stride(0) >= 2 ** 31:
        raise ValueError(f"{what}: its stride is {tuple(logits.stride())}")
    if logits.device != dev:
        raise ValueError(f"{what}: it is on {logits.device}")
    res = {k: _output(k, t, rows, dev) for k, t in outputs.items()}

    def ptr(k):
        return res[k].data_ptr() if k in res else None
    req = HsSampleRequest(logits.data_ptr(), _DTYPES[_name(logits.dtype)], max(int(logits.stride(0)), L),
                          (C.c_int32 * HEADS)(*buckets), MODES[mode], ZERO_INACTIVE if zero_inactive else 0,
                          (C.c_uint32 * 2)(int(seed[0]) & 0xFFFFFFFF, int(seed[1]) & 0xFFFFFFFF),
                          int(counter) & 0xFFFFFFFF, ptr("action"), ptr("log_prob"), ptr("entropy"), ptr("head_log_prob"))
    return res, req


def _result(sim, res):
    """{name: tensor} of a call; with action=None the simulator's own action tensor stands for `action`."""
    if "action" not in res:
        res = dict(res, action=sim.action_tensor().to_torch())
    return res


def sample(sim, logits, stream=None, **kw):
    """HideAndSeekSimulator.sample_actions."""
    res, req = request(sim.num_worlds * sim.agents_per_world, sim.gpu_id, logits, **kw)
    _run(sim, "hs_sample_actions", req, stream)
    return _result(sim, res)


def sample_sharded(ssim, logits, stream=None, action=None, log_prob=None, entropy=None, head_log_prob=None, **kw):
    """ShardedSimulator.sample_actions: every shard samples its own rows on its own device from its own logits tensor."""
    res = _shard_calls(ssim, "hs_sample_actions", request, stream, dict(logits=logits),
                       per_shard=dict(action=action, log_prob=log_prob, entropy=entropy, head_log_prob=head_log_prob), kw=kw,
                       lead=lambda s: (s.num_worlds * s.agents_per_world, s.gpu_id))
    return [_result(s, r) for s, r in zip(ssim.shards, res)]
