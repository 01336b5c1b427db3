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

For a league or a population the routed form does the same from logits in SLOT order (row_of_slot of league_step): the
actions go to the rows, where the next step reads them, and what a learner stores stays in slot order, in one launch
(hs_sample_actions_routed, csrc/hs_k_sample_routed.h), bit for bit what sample_actions gives every row.

    sim.sample_actions_routed(logits_by_slot, row_of_slot, seed=(run_seed, 0), counter=t, action=buf.action[t], log_prob=buf.log_prob[t])
"""
import ctypes as C

from ._request import _DTYPES, _disjoint, _name, _rows, _run, _shard_calls, _tensor

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


class HsSampleRoutedRequest(C.Structure):
    """hs_sample_routed_request (include/hideseek.h)."""
    _fields_ = [("logits", C.c_void_p), ("logits_dtype", C.c_int32), ("logits_stride", C.c_int32),
                ("buckets", C.c_int32 * HEADS), ("mode", C.c_int32), ("flags", C.c_uint32), ("seed", C.c_uint32 * 2),
                ("counter", C.c_uint32), ("row_of_slot", C.c_void_p), ("action_rows", C.c_void_p), ("action", C.c_void_p),
                ("log_prob", C.c_void_p), ("entropy", C.c_void_p), ("head_log_prob", C.c_void_p), ("bad", C.c_void_p)]


ROUTED_MODES = ("draw", "greedy")


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


def request_routed(rows, gpu_id, logits, row_of_slot, buckets=DEFAULT_BUCKETS, mode="draw", seed=(0, 0), counter=0, action_rows=None, action=None,
                   log_prob=None, entropy=None, head_log_prob=None, bad=None, flags=0):
    """Validate a routed sampling call over `rows` agent rows on GPU `gpu_id`: `logits` [rows, W >= sum(buckets)] indexed by
    slot, `row_of_slot` int32 [rows] (or [rows, 1]); mode "draw" or "greedy"; `action_rows` None (the simulator's action
    tensor) or an int32 [rows, 5] tensor indexed by row; `action`, `log_prob`, `entropy`, `head_log_prob`, indexed by slot,
    each None, True or a tensor; `bad` None, True or int32 [1]; `flags` must be 0.  Returns ({name: tensor},
    HsSampleRoutedRequest).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    buckets = tuple(int(b) for b in buckets)
    if len(buckets) != HEADS or any(b < 1 or b > MAX_BUCKETS for b in buckets):
        raise ValueError(f"buckets must be {HEADS} counts in [1, {MAX_BUCKETS}], got {buckets}")
    L = sum(buckets)
    if L > MAX_LOGITS:
        raise ValueError(f"buckets sum to {L} logits per row, more than {MAX_LOGITS}")
    if mode not in ROUTED_MODES:
        raise ValueError(f"mode must be one of {', '.join(ROUTED_MODES)} (the update scores stored actions with ppo_loss), got {mode!r}")
    if isinstance(flags, bool) or flags != 0:
        raise ValueError(f"flags must be 0, got {flags!r}")
    if len(seed) != 2:
        raise ValueError("seed must be a pair of 32-bit integers")
    stride = _rows("logits", logits, rows, L, dev, str(rows))
    _tensor("row_of_slot", row_of_slot, [(rows,), (rows, 1)], ("int32",), dev)
    outputs = {k: t for k, t in (("action", action), ("log_prob", log_prob), ("entropy", entropy), ("head_log_prob", head_log_prob))
               if t is not None and t is not False}
    if action_rows is not None:
        _tensor("action_rows", action_rows, (rows, HEADS), ("int32",), dev, "None or a torch tensor")
        if not outputs:
            raise ValueError("nothing to do: action_rows given and no slot-order output requested (sample_actions on the gathered logits does that)")
    if bad is not None and bad is not True:
        _tensor("bad", bad, (1,), ("int32",), dev, "None, True or a torch tensor")
    for k, t in outputs.items():
        if t is not True:
            tail, dt = _OUTPUTS[k]
            _tensor(k, t, (rows,) + tail, (dt,), dev, "True, None or a torch tensor")
    given = [(k, t) for k, t in (("action_rows", action_rows), *outputs.items(), ("bad", bad)) if t is not None and t is not True]
    _disjoint(given, [("logits", logits), ("row_of_slot", row_of_slot)], dev)
    res = {k: _output(k, t, rows, dev) for k, t in outputs.items()}
    if action_rows is not None:
        res["action_rows"] = action_rows
    if bad is not None:
        res["bad"] = torch.empty(1, dtype=torch.int32, device=dev) if bad is True else bad

    def ptr(k):
        return res[k].data_ptr() if k in res else None
    req = HsSampleRoutedRequest(logits.data_ptr(), _DTYPES[_name(logits.dtype)], stride, (C.c_int32 * HEADS)(*buckets), MODES[mode], 0,
                                (C.c_uint32 * 2)(int(seed[0]) & 0xFFFFFFFF, int(seed[1]) & 0xFFFFFFFF), int(counter) & 0xFFFFFFFF,
                                row_of_slot.data_ptr(), ptr("action_rows"), ptr("action"), ptr("log_prob"), ptr("entropy"), ptr("head_log_prob"), ptr("bad"))
    return res, req


def sample_routed(sim, logits, row_of_slot, stream=None, **kw):
    """HideAndSeekSimulator.sample_actions_routed."""
    res, req = request_routed(sim.num_worlds * sim.agents_per_world, sim.gpu_id, logits, row_of_slot, **kw)
    _run(sim, "hs_sample_actions_routed", req, stream)
    if "action_rows" not in res:
        res = dict(res, action_rows=sim.action_tensor().to_torch())
    return res


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
