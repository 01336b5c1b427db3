"""Policy inputs: the observation exports of every agent packed into one row of 296 features, in the learner's dtype
and in the learner's own storage, by one kernel (hs_pack_policy_inputs, csrc/hs_k_pack.h).

What the reference's policy does to the observation tensors before its network sees them
(scripts/jax_policy.py:84-98, 262-280, 372-390): prep_counter / 96, self_type and the masks cast to the compute type,
`prep_counter, self_data, self_type, lidar` concatenated into the "self" row, the entity tables multiplied by their
visibility masks for the actor (the critic sees them unmasked), and per-feature statistics for the observation
normaliser.

    sim.step()
    out = sim.pack_policy_inputs(actor=rollout_actor[t], critic=rollout_critic[t], moments=True)
    tables = policy_inputs.views(rollout_actor[t])       # {"self": [R,45], "agents": [R,5,14], "boxes": ..., "ramps": ...}
    count, mean, var = policy_inputs.moments_to_mean_var(out["moments"])
"""
import ctypes as C

ROW = 296            # HS_PACK_ROW
MOMENTS = 593        # HS_PACK_MOMENTS: sum m x [296], sum m x x [296], sum m

# name -> (first column, one past the last, shape of a row's slice); columns of the packed row in order
LAYOUT = {
    "prep_counter": (0, 1, (1,)),
    "self_data": (1, 14, (13,)),
    "self_type": (14, 15, (1,)),
    "lidar": (15, 45, (30,)),
    "agent_data": (45, 115, (5, 14)),
    "box_data": (115, 268, (9, 17)),
    "ramp_data": (268, 296, (2, 14)),
}
# the visibility mask the actor's variant multiplies each entity table by (export getter names)
MASKS = {"agent_data": "visible_agents_mask", "box_data": "visible_boxes_mask", "ramp_data": "visible_ramps_mask"}
# the policy's four tables as column ranges of the row (extract_self_obs, then agents / boxes / ramps)
TABLES = {"self": (0, 45, (45,)), "agents": LAYOUT["agent_data"], "boxes": LAYOUT["box_data"], "ramps": LAYOUT["ramp_data"]}

_DTYPES = {"float32": 1, "bfloat16": 3, "float16": 4}      # HS_DTYPE_F32 / _BF16 / _F16


class HsPackRequest(C.Structure):
    """hs_pack_request (include/hideseek.h)."""
    _fields_ = [("actor", C.c_void_p), ("actor_dtype", C.c_int32), ("critic", C.c_void_p), ("critic_dtype", C.c_int32),
                ("moments", C.c_void_p)]


def views(packed):
    """The policy's tables as zero-copy views of packed rows [..., 296]: {"self": [..., 45], "agents": [..., 5, 14],
    "boxes": [..., 9, 17], "ramps": [..., 2, 14]}."""
    if packed.shape[-1] != ROW:
        raise ValueError(f"packed rows have {ROW} columns, got shape {tuple(packed.shape)}")
    return {name: packed[..., lo:hi].unflatten(-1, shape) for name, (lo, hi, shape) in TABLES.items()}


def moments_to_mean_var(moments):
    """(count, mean [296], biased variance [296]) in float64 from the moments of pack_policy_inputs: the statistics of
    the active agent rows.  With no active row, mean and variance are 0."""
    import torch
    m = moments.to(torch.float64)
    if m.shape != (MOMENTS,):
        raise ValueError(f"moments have shape ({MOMENTS},), got {tuple(m.shape)}")
    count = m[2 * ROW]
    n = torch.clamp(count, min=1.0)
    mean = m[:ROW] / n
    var = torch.clamp(m[ROW:2 * ROW] / n - mean * mean, min=0.0)
    return count, mean, var


def _output(name, t, rows, dev, dtype):
    """The tensor output `name` is written to: `t` itself when it is a tensor (checked), a new one when it is True."""
    import torch
    shape = (MOMENTS,) if name == "moments" else (rows, ROW)
    allowed = ("float64",) if name == "moments" else tuple(_DTYPES)
    if t is True:
        dt = torch.float64 if name == "moments" else (torch.float32 if dtype is None else dtype)
        if str(dt).replace("torch.", "") not in allowed:
            raise ValueError(f"dtype must be one of {', '.join(allowed)}, got {dt}")
        return torch.empty(shape, dtype=dt, device=dev)
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be True, None or a torch tensor")
    what = f"{name} must be a contiguous, 16-byte aligned {' / '.join(allowed)} tensor of shape {shape} on {dev}"
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if str(t.dtype).replace("torch.", "") not in allowed:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: it is not contiguous")
    if t.device != dev:
        raise ValueError(f"{what}: it is on {t.device}")
    if t.data_ptr() % 16:
        raise ValueError(f"{what}: it starts {t.data_ptr() % 16} bytes past a 16-byte boundary")
    return t


def request(rows, gpu_id, actor=None, critic=None, moments=None, dtype=None):
    """Validate the outputs of a pack of `rows` agent rows on GPU `gpu_id`, allocate the ones given as True, and return
    ({name: tensor}, HsPackRequest).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    res = {k: _output(k, t, rows, dev, dtype) for k, t in (("actor", actor), ("critic", critic), ("moments", moments))
           if t is not None and t is not False}
    if not res:
        raise ValueError("no output requested")

    def code(k):
        return _DTYPES[str(res[k].dtype).replace("torch.", "")] if k in res else 0

    def ptr(k):
        return res[k].data_ptr() if k in res else None
    return res, HsPackRequest(ptr("actor"), code("actor"), ptr("critic"), code("critic"), ptr("moments"))


def stream_handle(stream):
    """The raw hipStream_t of a torch.cuda.Stream (or the integer itself)."""
    return int(getattr(stream, "cuda_stream", stream))


def pack(sim, actor=None, critic=None, moments=None, dtype=None, stream=None):
    """HideAndSeekSimulator.pack_policy_inputs."""
    from ._native import check
    res, req = request(sim.num_worlds * sim.agents_per_world, sim.gpu_id, actor, critic, moments, dtype)
    if stream is None:
        check(sim._L.hs_pack_policy_inputs(sim._h, C.byref(req)))
    else:
        check(sim._L.hs_pack_policy_inputs_async(sim._h, C.c_void_p(stream_handle(stream)), C.byref(req)))
    return res


def _per_shard(ssim, name, arg):
    n = len(ssim.shards)
    if arg is None or arg is True or arg is False:
        return [arg] * n
    if len(arg) != n:
        raise ValueError(f"{name}: one entry per shard ({n}) expected")
    return list(arg)


def pack_sharded(ssim, actor=None, critic=None, moments=None, dtype=None, stream=None):
    """ShardedSimulator.pack_policy_inputs: every shard packs its own rows on its own device.  Each of `actor`,
    `critic`, `moments` (and `stream`) is True / None for all shards or a list with one entry per shard; returns the list
    of the shards' results.  With stream=None every shard's pack is enqueued on a side stream of its device, ordered
    after that device's current stream, before any is waited for."""
    import torch
    from ._native import check
    args = [_per_shard(ssim, k, v) for k, v in (("actor", actor), ("critic", critic), ("moments", moments))]
    streams = _per_shard(ssim, "stream", stream)
    reqs = [request(s.num_worlds * s.agents_per_world, s.gpu_id, a, c, m, dtype) for s, a, c, m in zip(ssim.shards, *args)]
    waits = []
    for s, (res, req), st in zip(ssim.shards, reqs, streams):
        if st is None:
            st = torch.cuda.Stream(device=s.gpu_id)
            st.wait_stream(torch.cuda.current_stream(s.gpu_id))
            waits.append(st)
        check(s._L.hs_pack_policy_inputs_async(s._h, C.c_void_p(stream_handle(st)), C.byref(req)))
    for st in waits:
        st.synchronize()
    return [res for res, _ in reqs]
