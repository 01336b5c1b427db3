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

The normaliser the reference wraps around its policy (jax_policy.py:372-390, an exponential moving average with decay
0.99999 over every column but prep_counter and self_type) lives on the device as an ObsNormaliser: the pack normalises
with its table and collects the moments of the raw rows in the same launch, and update() folds them in with one kernel
(hs_obs_norm_update), with no host synchronisation in between.

    norm = policy_inputs.ObsNormaliser(gpu_id)
    out = sim.pack_policy_inputs(actor=rollout_actor[t], critic=rollout_critic[t], moments=mom[t], normaliser=norm)
    norm.update(sim, mom)                                # [T, 593], after the rollout

For a league or a population (gpu_hideseek.league, gpu_hideseek.population) pack_routed does the same in one launch for
N policies that share the simulator: every row goes to its slot (row_of_slot of hs_league_step), is normalised with the
table of the policy that owns the slot (the rows of one [N, 592] buffer: ObsNormaliser(..., table=tables[p])), and the
moments are collected per policy (hs_pack_policy_inputs_routed, csrc/hs_k_pack_routed.h).

    sim.pack_policy_inputs_routed(row_of_slot, N, actor=buf_actor[t], critic=buf_critic[t], moments=mom[:, t],
                                  moments_stride=T * 593, tables=tables)          # mom [N, T, 593]
"""
import ctypes as C

from ._request import _DTYPES, _overlap, _per_shard, _run, _sharded, _tensor, stream_handle      # noqa: F401 (stream_handle: part of this module's face)

ROW = 296            # HS_PACK_ROW
MOMENTS = 593        # HS_PACK_MOMENTS: sum m x [296], sum m x x [296], sum m
NORM_STATE = 593     # HS_NORM_STATE: m1 [296], m2 [296], N
NORM_TABLE = 592     # HS_NORM_TABLE: mu [296], inv [296]
NORM_MAX_MOMENTS = 4096      # HS_NORM_MAX_MOMENTS
NORM_SKIP = ("prep_counter", "self_type")      # the columns an ObsNormaliser leaves alone (HS_NORM_SKIP_*)

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

class HsPackRequest(C.Structure):
    """hs_pack_request (include/hideseek.h)."""
    _fields_ = [("actor", C.c_void_p), ("actor_dtype", C.c_int32), ("critic", C.c_void_p), ("critic_dtype", C.c_int32),
                ("moments", C.c_void_p)]


class HsPackRoutedRequest(C.Structure):
    """hs_pack_routed_request (include/hideseek.h)."""
    _fields_ = [("actor", C.c_void_p), ("actor_dtype", C.c_int32), ("critic", C.c_void_p), ("critic_dtype", C.c_int32),
                ("row_of_slot", C.c_void_p), ("num_policies", C.c_int32), ("tables", C.c_void_p), ("moments", C.c_void_p),
                ("moments_stride", C.c_int64), ("bad", C.c_void_p)]


MAX_POLICIES = 16    # HS_LEAGUE_MAX_POLICIES


class HsObsNormRequest(C.Structure):
    """hs_obs_norm_request (include/hideseek.h)."""
    _fields_ = [("moments", C.c_void_p), ("num_moments", C.c_int32), ("decay", C.c_double), ("eps", C.c_double),
                ("state", C.c_void_p), ("table", C.c_void_p)]


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
    align = 8 if name == "moments" else 16       # a row mom[t] of a [T, 593] float64 buffer is 8-byte aligned
    what = f"{name} must be a contiguous, {align}-byte aligned {' / '.join(allowed)} tensor of shape {shape} on {dev}"
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if str(t.dtype).replace("torch.", "") not in allowed:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: it is not contiguous")
    if t.device != dev:
        raise ValueError(f"{what}: it is on {t.device}")
    if t.data_ptr() % align:
        raise ValueError(f"{what}: it starts {t.data_ptr() % align} bytes past a {align}-byte boundary")
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


def norm_table(normaliser, gpu_id):
    """The f32 [592] table tensor of `normaliser` (an ObsNormaliser or the tensor itself), checked for GPU `gpu_id`."""
    import torch
    dev = torch.device("cuda", gpu_id)
    t = normaliser.table if isinstance(normaliser, ObsNormaliser) else normaliser
    if not isinstance(t, torch.Tensor):
        raise ValueError("normaliser must be None, an ObsNormaliser or a torch tensor")
    what = f"normaliser must be (or own) a contiguous, 16-byte aligned float32 table of shape ({NORM_TABLE},) on {dev}"
    if tuple(t.shape) != (NORM_TABLE,):
        raise ValueError(f"{what}: its shape is {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: its dtype is {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: it is not contiguous")
    if t.device != dev:
        raise ValueError(f"{what}: it is on {t.device}")
    if t.data_ptr() % 16:
        raise ValueError(f"{what}: it starts {t.data_ptr() % 16} bytes past a 16-byte boundary")
    return t


def _launch(sim, req, table, stream):
    """The pack entry point that fits (table, stream)."""
    if table is None:
        _run(sim, "hs_pack_policy_inputs", req, stream)
    else:
        _run(sim, "hs_pack_policy_inputs_normalized", req, stream, C.c_void_p(table.data_ptr()))


def pack(sim, actor=None, critic=None, moments=None, dtype=None, stream=None, normaliser=None):
    """HideAndSeekSimulator.pack_policy_inputs."""
    res, req = request(sim.num_worlds * sim.agents_per_world, sim.gpu_id, actor, critic, moments, dtype)
    table = None if normaliser is None else norm_table(normaliser, sim.gpu_id)
    _launch(sim, req, table, stream)
    return res


def pack_sharded(ssim, actor=None, critic=None, moments=None, dtype=None, stream=None, normaliser=None):
    """ShardedSimulator.pack_policy_inputs: every shard packs its own rows on its own device.  Each of `actor`,
    `critic`, `moments` (and `stream`) is True / None for all shards or a list with one entry per shard; returns the list
    of the shards' results.  With stream=None every shard's pack is enqueued on a side stream of its device, ordered
    after that device's current stream, before any is waited for.  `normaliser` is None, a list with one ObsNormaliser
    or table tensor per shard (each on its shard's device), or one of either for every shard, which then all have to be
    on its device: a table is read by the kernel and is not copied between devices here.  With the shards on several
    devices, keep one ObsNormaliser, update it with the shards' moments stacked on its device, and hand each other device
    a copy of its table."""
    a, c, m = (_per_shard(ssim, k, v) for k, v in (("actor", actor), ("critic", critic), ("moments", moments)))
    norms = normaliser if isinstance(normaliser, (list, tuple)) else [normaliser] * len(ssim.shards)
    if len(norms) != len(ssim.shards):
        raise ValueError(f"normaliser: one entry per shard ({len(ssim.shards)}) expected")

    def make(i, s):        # the "request" of a shard is its (request, table)
        res, req = request(s.num_worlds * s.agents_per_world, s.gpu_id, a[i], c[i], m[i], dtype)
        return res, (req, None if norms[i] is None else norm_table(norms[i], s.gpu_id))
    return _sharded(ssim, lambda s, rt, st: _launch(s, *rt, st), make, stream)


def request_routed(rows, gpu_id, row_of_slot, num_policies, actor=None, critic=None, moments=None, moments_stride=None, tables=None, bad=None,
                   dtype=None):
    """Validate a routed pack of `rows` agent rows on GPU `gpu_id` for `num_policies` policies: `row_of_slot` int32 [rows]
    (or [rows, 1]); `actor` / `critic` as request() takes them, indexed by slot; `moments` None, True (a new [N, 593]) or a
    float64 tensor whose first dimension is the policy, [N, 593] or a view such as mom[:, t] of [N, T, 593]: policy p's
    vector is read at p * moments_stride doubles (by default the tensor's own stride(0)); `tables` None or a contiguous,
    16-byte aligned float32 [N, 592]; `bad` None or int32 [1].  Returns ({name: tensor}, HsPackRoutedRequest).  Raises
    ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    N = num_policies
    if isinstance(N, bool) or not isinstance(N, int) or not 1 <= N <= MAX_POLICIES:
        raise ValueError(f"num_policies must be an integer in [1, {MAX_POLICIES}], got {N!r}")
    if rows < 1 or rows % N:
        raise ValueError(f"the number of agent rows ({rows}) must be a multiple of num_policies ({N})")
    _tensor("row_of_slot", row_of_slot, [(rows,), (rows, 1)], ("int32",), dev)
    if tables is not None:
        _tensor("tables", tables, (N, NORM_TABLE), ("float32",), dev, "None or a torch tensor", align=16)
    if bad is not None:
        _tensor("bad", bad, (1,), ("int32",), dev, "None or a torch tensor")
    res = {k: _output(k, t, rows, dev, dtype) for k, t in (("actor", actor), ("critic", critic)) if t is not None and t is not False}
    stride = 0
    if moments is True:
        res["moments"] = torch.empty(N, MOMENTS, dtype=torch.float64, device=dev)
    elif moments is not None and moments is not False:
        what = f"moments must be True, None or a float64 tensor of shape ({N}, {MOMENTS}) on {dev} whose rows are contiguous and 8-byte aligned"
        if not isinstance(moments, torch.Tensor):
            raise ValueError(what)
        if tuple(moments.shape) != (N, MOMENTS):
            raise ValueError(f"{what}: its shape is {tuple(moments.shape)}")
        if moments.dtype != torch.float64:
            raise ValueError(f"{what}: its dtype is {moments.dtype}")
        if moments.stride(1) != 1:
            raise ValueError(f"{what}: its stride is {tuple(moments.stride())}")
        if moments.device != dev:
            raise ValueError(f"{what}: it is on {moments.device}")
        if moments.data_ptr() % 8:
            raise ValueError(f"{what}: it starts {moments.data_ptr() % 8} bytes past an 8-byte boundary")
        res["moments"] = moments
    if "moments" in res:
        own = int(res["moments"].stride(0)) if N > 1 else MOMENTS
        stride = own if moments_stride is None else moments_stride
        if isinstance(stride, bool) or not isinstance(stride, int) or stride < MOMENTS:
            raise ValueError(f"moments_stride must be an integer of at least {MOMENTS} doubles, got {stride!r}")
        if N > 1 and stride != own:
            raise ValueError(f"moments_stride is {stride}, the moments tensor has {own} doubles between its policies")
    if not res:
        raise ValueError("no output requested")
    for k, t in (("row_of_slot", row_of_slot), ("tables", tables), ("bad", bad)):
        if t is not None and t.device != dev:
            raise ValueError(f"{k} must be on {dev}: it is on {t.device}")
    if bad is not None:
        res["bad"] = bad
    inputs = [("row_of_slot", row_of_slot)] + ([("tables", tables)] if tables is not None else [])
    outs = [(k, res[k]) for k in ("actor", "critic", "moments", "bad") if k in res]
    for i, (k, t) in enumerate(outs):
        for k2, t2 in inputs + outs[:i]:
            if _overlap(t, t2):
                raise ValueError(f"{k} overlaps {k2}")

    def code(k):
        return _DTYPES[str(res[k].dtype).replace("torch.", "")] if k in res else 0

    def ptr(k):
        return res[k].data_ptr() if k in res else None
    return res, HsPackRoutedRequest(ptr("actor"), code("actor"), ptr("critic"), code("critic"), row_of_slot.data_ptr(), N,
                                    None if tables is None else tables.data_ptr(), ptr("moments"), stride, ptr("bad"))


def pack_routed(sim, row_of_slot, num_policies, actor=None, critic=None, moments=None, moments_stride=None, tables=None, bad=None, dtype=None,
                stream=None):
    """HideAndSeekSimulator.pack_policy_inputs_routed."""
    res, req = request_routed(sim.num_worlds * sim.agents_per_world, sim.gpu_id, row_of_slot, num_policies, actor, critic, moments, moments_stride,
                              tables, bad, dtype)
    _run(sim, "hs_pack_policy_inputs_routed", req, stream)
    return res


def table_of_state(state, eps):
    """The table [592] float32 (numpy) of a state [593] float64 (numpy), by the formula of hs_obs_norm_update."""
    import numpy as np
    m1, m2, N = state[:ROW], state[ROW:2 * ROW], state[2 * ROW]
    mu, inv = np.zeros(ROW, np.float32), np.ones(ROW, np.float32)
    if N > 0:
        mean = m1 / N
        v = m2 / N - mean * mean
        v = np.where(v < 0, 0.0, v)
        mu, inv = mean.astype(np.float32), (1.0 / np.sqrt(v + eps)).astype(np.float32)
        for name in NORM_SKIP:
            mu[LAYOUT[name][0]], inv[LAYOUT[name][0]] = 0.0, 1.0
    return np.concatenate([mu, inv])


def _decay_eps(decay, eps):
    import math
    decay, eps = float(decay), float(eps)
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"decay must be in [0, 1), got {decay}")
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError(f"eps must be finite and above 0, got {eps}")
    return decay, eps


class ObsNormaliser:
    """The observation normaliser of the reference's policy (jax_policy.py:372-390) on GPU `gpu_id`: an exponential
    moving average of the first and second moments of every column of the packed row, bias-corrected, kept in `state`
    (float64 [593]: m1, m2, N) and turned into `table` (float32 [592]: mean, 1 / sqrt(var + eps); 0 and 1 for
    prep_counter and self_type) by update().  Hand it to pack_policy_inputs(normaliser=...).  The arithmetic is stated
    with hs_obs_norm_request in include/hideseek.h.  `table`, if given, is the float32 [592] tensor (contiguous, 16-byte
    aligned, on the GPU) the table is kept in, instead of one allocated here: the tables of N normalisers are then the
    rows of one [N, 592] buffer, which is what pack_routed reads."""

    def __init__(self, gpu_id, decay=0.99999, eps=1e-5, table=None):
        import torch
        self.gpu_id = int(gpu_id)
        self.decay, self.eps = _decay_eps(decay, eps)
        dev = torch.device("cuda", self.gpu_id)
        self.table = torch.empty(NORM_TABLE, dtype=torch.float32, device=dev) if table is None else norm_table(table, self.gpu_id)
        self.state = torch.zeros(NORM_STATE, dtype=torch.float64, device=dev)
        self.reset()

    def reset(self):
        """A fresh normaliser: the state all zeros, the table the identity."""
        self.state.zero_()
        self.table[:ROW] = 0.0
        self.table[ROW:] = 1.0

    def update(self, sim, moments, stream=None):
        """Fold the moments of one batch into the state and rewrite the table, in one kernel (hs_obs_norm_update).
        `moments` is what pack_policy_inputs(moments=...) wrote: float64 [593], or [K, 593] for K shards or K steps of
        a rollout (one batch), contiguous, on this normaliser's GPU, which is also `sim`'s.  stream=None blocks; a
        torch.cuda.Stream or raw handle enqueues there without synchronising."""
        import torch
        dev = self.state.device
        what = f"moments must be a contiguous float64 tensor of shape ({MOMENTS},) or (K, {MOMENTS}), K <= {NORM_MAX_MOMENTS}, on {dev}"
        if not isinstance(moments, torch.Tensor):
            raise ValueError(f"{what}: got {type(moments).__name__}")
        shape = tuple(moments.shape)
        if not (shape == (MOMENTS,) or (len(shape) == 2 and shape[1] == MOMENTS and 1 <= shape[0] <= NORM_MAX_MOMENTS)):
            raise ValueError(f"{what}: its shape is {shape}")
        if moments.dtype != torch.float64:
            raise ValueError(f"{what}: its dtype is {moments.dtype}")
        if not moments.is_contiguous():
            raise ValueError(f"{what}: it is not contiguous")
        if moments.device != dev:
            raise ValueError(f"{what}: it is on {moments.device}")
        if sim.gpu_id != self.gpu_id:
            raise ValueError(f"the simulator is on GPU {sim.gpu_id}, the normaliser on GPU {self.gpu_id}")
        req = HsObsNormRequest(moments.data_ptr(), moments.numel() // MOMENTS, self.decay, self.eps, self.state.data_ptr(),
                               self.table.data_ptr())
        _run(sim, "hs_obs_norm_update", req, stream)

    def mean_var(self):
        """(mean [296], biased variance [296], N) in float64 on the device, from the state, without synchronising: the
        bias-corrected statistics of every column (the skipped ones included).  A fresh normaliser gives zeros."""
        import torch
        m1, m2, N = self.state[:ROW], self.state[ROW:2 * ROW], self.state[2 * ROW]
        n = torch.where(N > 0, N, torch.ones_like(N))
        mean = m1 / n
        return mean, torch.clamp(m2 / n - mean * mean, min=0.0), N

    def state_dict(self):
        return {"state": self.state.detach().cpu().clone(), "decay": self.decay, "eps": self.eps}

    def load_state_dict(self, d):
        """Restore a state_dict(): the state, decay and eps; the table is computed again on the host by the formula of
        hs_obs_norm_update."""
        import torch
        state = torch.as_tensor(d["state"])
        if tuple(state.shape) != (NORM_STATE,) or state.dtype != torch.float64:
            raise ValueError(f"state must be a float64 tensor of shape ({NORM_STATE},), got {state.dtype} {tuple(state.shape)}")
        self.decay, self.eps = _decay_eps(d["decay"], d["eps"])
        self.state.copy_(state)
        self.table.copy_(torch.from_numpy(table_of_state(state.cpu().numpy(), self.eps)))
