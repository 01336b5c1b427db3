"""The rollout buffer of the update loop and the gather that cuts a shuffled minibatch of sequences out of it in one
launch (hs_gather_sequences, csrc/hs_k_gather.h; include/hideseek.h states the contract).

The reference trains on back-propagation-through-time chunks (scripts/jax_train.py: steps_per_update = 40,
num_bptt_chunks = 8): a rollout of T steps over n agent rows is K chunks of L = T / K consecutive steps, K n sequences in
all, and sequence id s = k n + r is chunk k of row r.  A minibatch is m ids, an int32 tensor that stays on the device.

    buf = rollout.Rollout(sim, steps=40, chunks=8, dtype=torch.bfloat16)
    ...                                              # the trainer fills the slots (gpu_hideseek.trainer)
    perm = torch.randperm(buf.sequences, device="cuda", dtype=torch.int32)
    mb = buf.minibatch(perm[:buf.sequences // 2])    # one launch; mb = buf.minibatch(perm[...], out=mb) allocates nothing
    mb["actor"]      [L, m, 296]        mb["clear"] [L, m]        mb["actor_h"] [m, H]   the state at the chunk's start

The time alignment, stated once.  Slot t holds
    actor[t], critic[t]     the observation o_t, packed (and normalised)
    clear[t]                the done export of the sim.step() that produced o_t
    action[t], log_prob[t], value[t]     the action drawn from the policy's output on o_t, its log-probability, and the
                            critic's decoded value of o_t (hs_gae_request: "V(observation the action of step t was chosen
                            from)")
    reward[t], done[t]      the reward and done exports of the sim.step() that consumed action[t] (hs_gae_request: "the
                            done export of step t; nonzero = the episode ended with step t")
    mask[t]                 the self_mask export with o_t
so clear[t + 1] = done[t], and clear[0] is the done of the last step of the previous rollout.  actor_h / actor_c /
critic_h / critic_c [k] are the LSTM states as the forward of slot k L received them: where a chunk's sequence starts.

Where an episode starts.  A step runs, in the reference's order (src/sim.cpp: outputRewardsDonesSystem, resetSystem,
collectObservationsSystem), the rewards and dones, then the reset, then the observations: the observation exported
together with done != 0 is already the FIRST one of the next episode (prep_counter = 96).  So the state that goes INTO
the forward of slot t is zero where clear[t] != 0.  done is written for the agents active in the episode that ends: a row
that joins with the new episode exports done = 0 with its first observation, and a row that leaves keeps a stale done = 1
(and a stale reward) while it is out.  Hence the rule, state_zero_into(): the state into slot t is zero where
clear[t] != 0, where mask[t] == 0 or where mask[t - 1] == 0, so a row that is out carries zero and a row that joins
starts from zero.  The trainer applies it to the carried state after every sim.step(); the update gives it to the
recurrent core, whose `clear` zeroes the state carried OUT of a step, as the clear of the step BEFORE: chunk_clears().
Resets the host requests in mid-episode set no done and are not covered.

minibatch_eager() is the same result by torch indexing, for readers, the tests and tools/gather_bench.py.
"""
import ctypes as C

from ._request import _disjoint, _run, _tensor

MAX_FIELDS = 16            # HS_GATHER_MAX_FIELDS
MAX_ROW_BYTES = 1 << 20    # HS_GATHER_MAX_ROW_BYTES
VEC = 16                   # bytes: a field with row_bytes % VEC == 0 and both bases VEC-aligned moves as 16-byte pieces
ROW = 296                  # policy_inputs.ROW
MOMENTS = 593              # policy_inputs.MOMENTS
HEADS = 5                  # action_sampling.HEADS


class HsGatherField(C.Structure):
    """hs_gather_field (include/hideseek.h)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("row_bytes", C.c_int32), ("per_chunk", C.c_int32)]


class HsGatherRequest(C.Structure):
    """hs_gather_request (include/hideseek.h)."""
    _fields_ = [("index", C.c_void_p), ("m", C.c_int32), ("chunks", C.c_int32), ("chunk_steps", C.c_int32), ("rows", C.c_int32),
                ("num_fields", C.c_int32), ("reserved", C.c_int32), ("bad", C.c_void_p), ("fields", HsGatherField * MAX_FIELDS)]


def sequence_rows(ids, chunks, chunk_steps, rows):
    """What the id formula says, as Python integers: for every id s = k * rows + r of `ids`, (k, r) and the L source
    steps k * L .. k * L + L - 1 of a per-step field."""
    out = []
    for s in ids:
        s = int(s)
        if not 0 <= s < chunks * rows:
            raise ValueError(f"sequence id {s} is outside [0, {chunks * rows})")
        k, r = divmod(s, rows)
        out.append((k, r, list(range(k * chunk_steps, (k + 1) * chunk_steps))))
    return out


def epoch_parts(perm, num_minibatches):
    """The minibatches of an epoch: `perm` (a permutation of the sequence ids) cut into num_minibatches equal,
    contiguous parts (views).  Raises ValueError if it does not divide."""
    total = int(perm.shape[0])
    if isinstance(num_minibatches, bool) or not isinstance(num_minibatches, int) or num_minibatches < 1:
        raise ValueError(f"num_minibatches must be a positive integer, got {num_minibatches!r}")
    if total % num_minibatches:
        raise ValueError(f"the {total} sequences (chunks * rows) do not divide into {num_minibatches} minibatches")
    m = total // num_minibatches
    return [perm[i * m:(i + 1) * m] for i in range(num_minibatches)]


# ---- where an episode starts ----
def state_zero_into(clear, mask, mask_before):
    """The rows (bool, of the arguments' shape) whose LSTM state is zero as it goes INTO the forward of a slot: `clear` is
    the done export that came with the slot's observation, `mask` its self_mask export and `mask_before` the self_mask of
    the slot before (the module docstring states why).  The one statement of the rule: collect() and the update use it."""
    return (clear != 0) | (mask == 0) | (mask_before == 0)


def zero_where(zero, *tensors):
    """Zero, in place, the rows of every [n, ...] tensor of `tensors` (carried LSTM states) where `zero` [n] (bool) is set."""
    zero = zero.unsqueeze(1)
    for x in tensors:
        x.masked_fill_(zero, 0)


def chunk_clears(clear, mask):
    """The `clear` [L, m] int32 that the recurrent core takes over a chunk of L slots whose per-slot fields are `clear`
    and `mask` [L, m]: the core zeroes the state carried OUT of a step, so step t < L - 1 takes state_zero_into() of slot
    t + 1, and the last step none, because what it carries out is not used.  The state into the chunk's first slot is the
    stored one, which collect() has put through the rule already."""
    import torch
    out = torch.zeros(clear.shape, dtype=torch.int32, device=clear.device)
    if clear.shape[0] > 1:
        out[:-1] = state_zero_into(clear[1:], mask[1:], mask[:-1])
    return out


# ---- the fused call ----
def _positive(name, v):
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"{name} must be a positive integer, got {v!r}")
    return v


def _tail_bytes(t):
    b = t.element_size()
    for d in t.shape[2:]:
        b *= int(d)
    return b


def request(gpu_id, index, fields, chunks, chunk_steps, rows, bad=None):
    """Validate a gather of the m = index.shape[0] sequences `index` (int32 [m], contiguous) on GPU `gpu_id` out of a
    rollout of `chunks` x `chunk_steps` steps over `rows` rows.  `fields` is a list of up to MAX_FIELDS (src, dst,
    per_chunk): a per-step src is contiguous [chunks * chunk_steps, rows, ...] and its dst [chunk_steps, m, ...], a
    per-chunk src [chunks, rows, ...] and its dst [m, ...], of the src's dtype and trailing shape; dst None allocates it.
    A row (the trailing shape) is a multiple of 4 bytes and every base 4-byte aligned.  `bad` is None, True or an int32
    [1] tensor for the count of ids out of range.  Returns ({"fields": [dst, ...], "bad": tensor (when asked for)},
    HsGatherRequest).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    K, L, n = _positive("chunks", chunks), _positive("chunk_steps", chunk_steps), _positive("rows", rows)
    if K * n >= 2 ** 31:
        raise ValueError(f"chunks * rows = {K * n} must stay below 2^31")
    _tensor("index", index, ("m >= 1",), ("int32",), dev)
    m = int(index.shape[0])
    fields = list(fields)
    if not 1 <= len(fields) <= MAX_FIELDS:
        raise ValueError(f"between 1 and {MAX_FIELDS} fields per call, got {len(fields)}")
    if (len(fields) + 1) * m >= 2 ** 31:
        raise ValueError(f"(fields + 1) * m = {(len(fields) + 1) * m} must stay below 2^31")
    inputs, outputs, made, table = [("index", index)], [], [], []
    for i, item in enumerate(fields):
        try:
            src, dst, per_chunk = item
        except (TypeError, ValueError):
            raise ValueError(f"field {i} must be (src, dst or None, per_chunk), got {item!r}") from None
        per_chunk = bool(per_chunk)
        lead = K if per_chunk else K * L
        if not isinstance(src, torch.Tensor):
            raise ValueError(f"field {i}: src must be a torch tensor")
        what = f"field {i}: src must be a contiguous tensor of shape ({lead}, {n}, ...) on {dev}"
        if src.dim() < 2 or tuple(src.shape[:2]) != (lead, n):
            raise ValueError(f"{what}: its shape is {tuple(src.shape)}")
        if not src.is_contiguous():
            raise ValueError(f"{what}: it is not contiguous")
        row_bytes = _tail_bytes(src)
        if row_bytes < 4 or row_bytes % 4 or row_bytes > MAX_ROW_BYTES:
            raise ValueError(f"field {i}: a row must be a multiple of 4 bytes in [4, {MAX_ROW_BYTES}], src has {row_bytes} ({src.dtype} x {tuple(src.shape[2:])})")
        if src.data_ptr() % 4:
            raise ValueError(f"field {i}: src must be 4-byte aligned: its address is {src.data_ptr():#x}")
        shape = ((m,) if per_chunk else (L, m)) + tuple(src.shape[2:])
        if dst is None:
            made.append(i)
        else:
            if not isinstance(dst, torch.Tensor):
                raise ValueError(f"field {i}: dst must be None or a torch tensor")
            what = f"field {i}: dst must be a contiguous {src.dtype} tensor of shape {shape} on {dev}"
            if tuple(dst.shape) != shape:
                raise ValueError(f"{what}: its shape is {tuple(dst.shape)}")
            if dst.dtype != src.dtype:
                raise ValueError(f"{what}: its dtype is {dst.dtype}")
            if not dst.is_contiguous():
                raise ValueError(f"{what}: it is not contiguous")
            if dst.data_ptr() % 4:
                raise ValueError(f"field {i}: dst must be 4-byte aligned: its address is {dst.data_ptr():#x}")
            outputs.append((f"field {i}: dst", dst))
        inputs.append((f"field {i}: src", src))
        table.append([src, dst, row_bytes, per_chunk, shape])
    if bad is not None and bad is not False and bad is not True:
        _tensor("bad", bad, (1,), ("int32",), dev, "None, True or a torch tensor")
        outputs.append(("bad", bad))
    _disjoint(outputs, inputs, dev)
    for i in made:
        src, _, _, _, shape = table[i]
        table[i][1] = torch.empty(shape, dtype=src.dtype, device=dev)
    res = {"fields": [f[1] for f in table]}
    if bad is True:
        bad = torch.empty(1, dtype=torch.int32, device=dev)
    if bad is not None and bad is not False:
        res["bad"] = bad
    req = HsGatherRequest(index.data_ptr(), m, K, L, n, len(table), 0, res["bad"].data_ptr() if "bad" in res else None)
    for i, (src, dst, row_bytes, per_chunk, _) in enumerate(table):
        req.fields[i] = HsGatherField(src.data_ptr(), dst.data_ptr(), row_bytes, 1 if per_chunk else 0)
    return res, req


def compute(sim, index, fields, chunks, chunk_steps, rows, bad=None, stream=None):
    """HideAndSeekSimulator.gather_sequences."""
    res, req = request(sim.gpu_id, index, fields, chunks, chunk_steps, rows, bad)
    _run(sim, "hs_gather_sequences", req, stream)
    return res


def gather_eager(index, src, chunks, chunk_steps, rows, per_chunk=False):
    """One field by torch indexing: dst [L, m, ...] (or [m, ...]) of src, for valid ids."""
    import torch
    idx = index.long()
    k, r = torch.div(idx, rows, rounding_mode="floor"), idx % rows
    if per_chunk:
        return src[k, r]
    t = torch.arange(chunk_steps, device=index.device).unsqueeze(1)
    return src[k.unsqueeze(0) * chunk_steps + t, r.unsqueeze(0)]


# ---- the buffer ----
PER_STEP = ("actor", "critic", "action", "log_prob", "value", "advantage", "returns", "mask", "clear")      # what a minibatch takes per step
PER_CHUNK = ("actor_h", "actor_c", "critic_h", "critic_c")                                                  # and per chunk


class Rollout:
    """The buffers of one rollout of `steps` = T steps in `chunks` = K chunks over the n agent rows of `sim`, allocated
    once on its device: actor, critic [T, n, 296] in `dtype`; action [T, n, 5] int32; log_prob, value, reward, advantage,
    returns, mask [T, n] float32; done, clear [T, n] int32; moments [T, 593] float64 (pack_policy_inputs's); and the LSTM
    states at the chunks' starts, actor_h, critic_h [K, n, hidden] in `dtype` and actor_c, critic_c [K, n, hidden]
    float32.  The module docstring states what slot t holds.  T % K == 0 is required."""

    def __init__(self, sim, steps, chunks, dtype=None, hidden=256, rows=None, device=None):
        import torch
        T, K = _positive("steps", steps), _positive("chunks", chunks)
        if T % K:
            raise ValueError(f"steps ({T}) must be a multiple of chunks ({K}): a chunk is steps / chunks consecutive steps")
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"dtype must be float32, bfloat16 or float16, got {dtype}")
        H = _positive("hidden", hidden)
        n = _positive("rows", sim.num_worlds * sim.agents_per_world if rows is None else rows)
        if K * n >= 2 ** 31:
            raise ValueError(f"chunks * rows = {K * n} must stay below 2^31")
        dev = torch.device("cuda", sim.gpu_id) if device is None else torch.device(device)
        self.sim, self.steps, self.chunks, self.chunk_steps, self.rows, self.hidden, self.dtype, self.device = sim, T, K, T // K, n, H, dtype, dev
        self.sequences = K * n
        f32, i32 = torch.float32, torch.int32
        self.actor, self.critic = (torch.zeros(T, n, ROW, dtype=dtype, device=dev) for _ in range(2))
        self.action = torch.zeros(T, n, HEADS, dtype=i32, device=dev)
        self.log_prob, self.value, self.reward, self.advantage, self.returns, self.mask = (torch.zeros(T, n, dtype=f32, device=dev) for _ in range(6))
        self.done, self.clear = (torch.zeros(T, n, dtype=i32, device=dev) for _ in range(2))
        self.moments = torch.zeros(T, MOMENTS, dtype=torch.float64, device=dev)
        self.actor_h, self.critic_h = (torch.zeros(K, n, H, dtype=dtype, device=dev) for _ in range(2))
        self.actor_c, self.critic_c = (torch.zeros(K, n, H, dtype=f32, device=dev) for _ in range(2))

    def snapshot_state(self, k, state, cols=slice(None)):
        """The carried LSTM states `state` = ((h, c) of the actor, (h, c) of the critic), as the forward of chunk k's first
        slot receives them, into actor_h, actor_c, critic_h and critic_c [k] (with `cols`, into that block of columns)."""
        for dst, src in zip((self.actor_h, self.actor_c, self.critic_h, self.critic_c), (t for s in state for t in s)):
            dst[k, cols].copy_(src)

    def tensors(self):
        """{name: tensor} of every buffer."""
        names = PER_STEP + PER_CHUNK + ("reward", "done", "moments")
        return {k: getattr(self, k) for k in names}

    def fields(self, out=None):
        """The field table of a minibatch: [(src, dst or None, per_chunk)] in the order PER_STEP + PER_CHUNK, the
        destinations taken from `out` (what minibatch() returned before)."""
        get = (lambda k: None) if out is None else (lambda k: out[k])
        return [(getattr(self, k), get(k), False) for k in PER_STEP] + [(getattr(self, k), get(k), True) for k in PER_CHUNK]

    def minibatch(self, index, out=None, stream=None):
        """The sequences `index` (int32 [m] on the device) of every field in one launch: {name: tensor}, [L, m, ...] for
        PER_STEP and [m, hidden] for PER_CHUNK.  With `out` (a result of an earlier call with the same m) the same
        tensors are written again and nothing is allocated."""
        if out is not None and set(out) != set(PER_STEP + PER_CHUNK):
            raise ValueError("out must be what minibatch() returned")
        res = compute(self.sim, index, self.fields(out), self.chunks, self.chunk_steps, self.rows, stream=stream)
        return dict(zip(PER_STEP + PER_CHUNK, res["fields"]))

    def minibatch_eager(self, index):
        """minibatch() by torch indexing (new tensors)."""
        return {k: gather_eager(index, getattr(self, k), self.chunks, self.chunk_steps, self.rows, k in PER_CHUNK) for k in PER_STEP + PER_CHUNK}
