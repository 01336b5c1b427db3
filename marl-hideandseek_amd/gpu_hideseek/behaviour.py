"""Behaviour statistics: what the agents do with the level, kept on the device by one kernel after every step
(hs_behaviour_stats, csrc/hs_k_behaviour.h).  Forts, ramp use and ramp defence do not show in the return; they show in
how far the boxes and ramps are moved in the preparation phase and in the main phase, in how many of them each side has
locked when the seekers are released and at the end, and in how much each side travels and grabs.

include/hideseek.h states the arithmetic and which observation belongs to which episode (rollout.py documents the trap
for the recurrent state): what is exported together with done is the first observation of the NEXT episode, a row that
left keeps a stale done, a row that joins exports done = 0.  A reset the host requests in mid-episode sets no done and
is not covered.

    bh = behaviour.BehaviourStats(sim)
    bh.arm(from_start=True)                       # right after sim.init(); bh.arm() anywhere else
    for _ in range(steps):
        ...                                       # write the actions
        sim.step()
        bh.step()                                 # the enqueued launches only, no read of the device
    print(bh.read())                              # one copy to the host; the table starts again from zero

The table is 27 float64 sums (stats_to_metrics turns them into means): world episodes, those that reached the main
phase, calls that found a world without an active row; for the boxes and then the ramps the nine sums of KIND_NAMES;
for the seekers and then the hiders travel, grabs and agent steps.  A call adds to it, without atomics and in a fixed
order: the same steps give the same bits.  eager_step is the same update written with torch operations, for readers,
tools/behaviour_bench.py and the tests.
"""
import ctypes as C
import math

from ._request import _disjoint, _run, _shard_calls, _tensor, on_current_stream

STATS = 27                # HS_BEHAVIOUR_STATS
KIND_STATS, SIDE_STATS = 9, 3                     # HS_BEHAVIOUR_KIND_STATS / _SIDE_STATS
UNARMED, PREP, MAIN, WAITING = 0, 1, 2, 3         # HS_BEHAVIOUR_UNARMED / _PREP / _MAIN / _WAITING: a world's phase
WORLD_EPISODES, REACHED_MAIN, BAD, BOXES, RAMPS, SEEKERS, HIDERS = 0, 1, 2, 3, 12, 21, 24
KIND_NAMES = ("max_prep", "max_main", "moved_prep", "moved_main", "hider_locked_prep", "seeker_locked_prep", "hider_locked_end",
              "seeker_locked_end", "objects")     # HS_BEHAVIOUR_KIND_*, in the table's order
SIDE_NAMES = ("travel", "grab", "agent_steps")    # HS_BEHAVIOUR_SIDE_*
SEEKER, HIDER = 0, 1      # self_type, and the order of the sides in the table and in n_side, travel, grab, agent_steps
OBJECTS, BODIES, MAX_BOXES, MAX_RAMPS, MAX_AGENTS = 11, 17, 9, 2, 6
# An object counts as moved above this displacement.  A setting, not a measurement: the level's boxes are 8 x 1.5 and
# 2 x 2 and its ramps are wider still, so 0.5 is a third of the thinnest object.  Contact jitter and an agent brushing
# past stay far below it; any push or carry that changes what an object blocks is above it.
DEFAULT_MOVE_EPS = 0.5
WORLD_STATE = (("phase", "int32", ()), ("n_obj", "int32", (2,)), ("n_side", "int32", (2,)), ("start_pos", "float32", (OBJECTS, 2)),
               ("prep_pos", "float32", (OBJECTS, 2)), ("last_pos", "float32", (BODIES, 2)), ("prep_locks", "int32", (OBJECTS,)),
               ("last_locks", "int32", (OBJECTS,)), ("travel", "float32", (2,)), ("grab", "int32", (2,)), ("agent_steps", "int32", (2,)))
ROW_STATE = (("was_active", "int32"),)
STATE_KEYS = tuple(k for k, _, _ in WORLD_STATE) + tuple(k for k, _ in ROW_STATE)
ROW_INPUTS = (("prep_counter", "int32"), ("done", "int32"), ("self_type", "int32"), ("self_mask", "float32"))


class HsBehaviourRequest(C.Structure):
    """hs_behaviour_request (include/hideseek.h), 176 bytes."""
    _fields_ = [("positions", C.c_void_p), ("locks", C.c_void_p), ("counts", C.c_void_p), ("prep_counter", C.c_void_p), ("done", C.c_void_p),
                ("self_type", C.c_void_p), ("self_mask", C.c_void_p), ("grabbing", C.c_void_p), ("grab_stride", C.c_int32), ("move_eps", C.c_float),
                ("phase", C.c_void_p), ("n_obj", C.c_void_p), ("n_side", C.c_void_p), ("start_pos", C.c_void_p), ("prep_pos", C.c_void_p),
                ("last_pos", C.c_void_p), ("prep_locks", C.c_void_p), ("last_locks", C.c_void_p), ("travel", C.c_void_p), ("grab", C.c_void_p),
                ("agent_steps", C.c_void_p), ("was_active", C.c_void_p), ("table", C.c_void_p)]


def new_state(num_worlds, agents, device):
    """A tracker's state, {name: tensor}, all zero: no world armed (its next observation starts an episode), no row
    active in the previous call."""
    import torch
    st = {k: torch.zeros((num_worlds,) + shape, dtype=getattr(torch, d), device=device) for k, d, shape in WORLD_STATE}
    st.update({k: torch.zeros(num_worlds * agents, dtype=getattr(torch, d), device=device) for k, d in ROW_STATE})
    return st


def _move_eps(move_eps):
    v = float(move_eps)
    if not (math.isfinite(v) and math.isfinite(C.c_float(v).value) and v >= 0.0):
        raise ValueError(f"move_eps must be finite and at least 0, got {move_eps}")
    return v


def stats_to_metrics(table):
    """The table (a [27] tensor, or 27 numbers) as Python numbers in float64: world_episodes, reached_main, bad;
    {"boxes": {...}, "ramps": {...}} with the per-episode means max_move_prep, max_move_main, moved_prep, moved_main,
    hider_locked_prep, seeker_locked_prep, hider_locked_end, seeker_locked_end and objects, and each count but the last
    also as a `_fraction` of the objects present; {"seekers": {...}, "hiders": {...}} with agent_steps, travel_per_step
    and grab_rate.  Everything is 0.0 where its count is 0."""
    t = [float(x) for x in (table.tolist() if hasattr(table, "tolist") else table)]
    if len(t) != STATS:
        raise ValueError(f"table has {STATS} values, got {len(t)}")
    n = t[WORLD_EPISODES]
    out = {}
    for name, o in (("boxes", BOXES), ("ramps", RAMPS)):
        s = dict(zip(KIND_NAMES, t[o:o + KIND_STATS]))
        kind = {"max_move_prep": s["max_prep"] / n if n > 0 else 0.0, "max_move_main": s["max_main"] / n if n > 0 else 0.0}
        for k in KIND_NAMES[2:]:
            kind[k] = s[k] / n if n > 0 else 0.0
        for k in KIND_NAMES[2:8]:
            kind[k + "_fraction"] = s[k] / s["objects"] if s["objects"] > 0 else 0.0
        out[name] = kind
    for name, o in (("seekers", SEEKERS), ("hiders", HIDERS)):
        travel, grab, steps = t[o:o + SIDE_STATS]
        out[name] = dict(agent_steps=steps, travel_per_step=travel / steps if steps > 0 else 0.0, grab_rate=grab / steps if steps > 0 else 0.0)
    out["world_episodes"], out["reached_main"], out["bad"] = n, t[REACHED_MAIN], t[BAD]
    return out


def request(num_worlds, agents, gpu_id, state, table, move_eps=DEFAULT_MOVE_EPS, positions=None, locks=None, counts=None, prep_counter=None,
            done=None, self_type=None, self_mask=None, grabbing=None):
    """Validate a call over num_worlds worlds of `agents` agent rows on GPU `gpu_id`: `state` as new_state() makes it,
    `table` [27] float64, and the inputs given explicitly: positions [num_worlds, 17, 2] float32, locks [num_worlds, 11]
    and counts [num_worlds, 4] int32, prep_counter, done, self_type int32 and self_mask float32 ([rows], [rows, 1] or
    [num_worlds, agents]); grabbing a float32 [rows] with any positive stride, such as self_data[:, 12]; None means the
    simulator's own.  Returns ({"table": table, "state": state}, HsBehaviourRequest).  Raises ValueError before the
    library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    rows = num_worlds * agents
    move_eps = _move_eps(move_eps)
    if not isinstance(state, dict) or set(state) != set(STATE_KEYS):
        raise ValueError("state must be a dict of " + ", ".join(STATE_KEYS) + " (behaviour.new_state)")
    per_row = [(rows,), (rows, 1), (num_worlds, agents)]
    given = dict(prep_counter=prep_counter, done=done, self_type=self_type, self_mask=self_mask)
    inputs = []
    for k, t, shape, d in (("positions", positions, (num_worlds, BODIES, 2), "float32"), ("locks", locks, (num_worlds, OBJECTS), "int32"),
                           ("counts", counts, (num_worlds, 4), "int32")):
        if t is not None:
            _tensor(k, t, shape, (d,), dev, "None or a torch tensor")
            inputs.append((k, t))
    for k, d in ROW_INPUTS:
        if given[k] is not None:
            _tensor(k, given[k], per_row, (d,), dev, "None or a torch tensor")
            inputs.append((k, given[k]))
    grab_stride = 0
    if grabbing is not None:
        what = f"grabbing must be None or a float32 tensor of shape ({rows},) with a stride of at least 1 on {dev}"
        if not isinstance(grabbing, torch.Tensor):
            raise ValueError(what)
        if tuple(grabbing.shape) != (rows,):
            raise ValueError(f"{what}: its shape is {tuple(grabbing.shape)}")
        if grabbing.dtype != torch.float32:
            raise ValueError(f"{what}: its dtype is {grabbing.dtype}")
        grab_stride = int(grabbing.stride(0)) if rows > 1 else 1
        if grab_stride < 1 or rows * grab_stride >= 2 ** 31:
            raise ValueError(f"{what}: its stride is {grab_stride} (rows * stride must stay below 2^31)")
        inputs.append(("grabbing", grabbing))
    outputs = []
    for k, d, shape in WORLD_STATE:
        _tensor(k, state[k], [(num_worlds,) + shape] + ([(num_worlds, 1)] if not shape else []), (d,), dev)
        outputs.append((k, state[k]))
    for k, d in ROW_STATE:
        _tensor(k, state[k], per_row, (d,), dev)
        outputs.append((k, state[k]))
    _tensor("table", table, (STATS,), ("float64",), dev)
    outputs.append(("table", table))
    _disjoint(outputs, inputs, dev)

    def ptr(t):
        return None if t is None else t.data_ptr()
    req = HsBehaviourRequest(ptr(positions), ptr(locks), ptr(counts), ptr(prep_counter), ptr(done), ptr(self_type), ptr(self_mask), ptr(grabbing),
                             grab_stride, move_eps, *(state[k].data_ptr() for k in STATE_KEYS), table.data_ptr())
    return {"table": table, "state": state}, req


def compute(sim, state, table, stream=None, **kw):
    """HideAndSeekSimulator.behaviour_stats."""
    res, req = request(sim.num_worlds, sim.agents_per_world, sim.gpu_id, state, table, **kw)
    _run(sim, "hs_behaviour_stats", req, stream)
    return res


def compute_sharded(ssim, state, table, stream=None, move_eps=DEFAULT_MOVE_EPS, **inputs):
    """ShardedSimulator.behaviour_stats: every shard tracks its own worlds on its own device."""
    return _shard_calls(ssim, "hs_behaviour_stats", request, stream, dict(state=state, table=table), per_shard=inputs, kw=dict(move_eps=move_eps),
                        lead=lambda s: (s.num_worlds, s.agents_per_world, s.gpu_id))


def eager_step(state, table, agents, positions, locks, counts, prep_counter, done, self_type, self_mask, grabbing, move_eps=DEFAULT_MOVE_EPS):
    """The contract of hs_behaviour_stats as torch operations on tensors of any one device: `state` (new_state) is
    updated in place, `table` is added to.  Every f32 operation of the contract is one torch operation, so for finite
    positions the state comes out with the kernel's bits up to the rounding of torch.sqrt (its vectorised CPU form is
    within one ulp, not correctly rounded); the table's sums are torch's, in another order of addition."""
    import torch
    A = agents
    W = state["phase"].shape[0]
    dev = state["phase"].device
    f32 = torch.float32

    def dist(a, b):
        dx, dy = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]
        return torch.sqrt(dx * dx + dy * dy)
    positions = positions.reshape(W, BODIES, 2)
    locks, counts = locks.reshape(W, OBJECTS), counts.reshape(W, 4)
    act, was, dn = self_mask.reshape(W, A) != 0, state["was_active"].reshape(W, A) != 0, done.reshape(W, A) != 0
    hider, grabs = self_type.reshape(W, A) != 0, grabbing.reshape(W, A) != 0
    ended, restarted, has = (dn & was).any(1), (act & ~was & ~dn).any(1), act.any(1)
    p = prep_counter.reshape(W, A).gather(1, act.to(torch.int32).argmax(1, keepdim=True))[:, 0]
    phase = state["phase"].reshape(W).clone()
    armed, main = (phase == PREP) | (phase == MAIN), phase == MAIN
    # step 2
    book = ended & armed
    start_pos, prep_pos, last_pos = state["start_pos"], state["prep_pos"], state["last_pos"]
    last_obj = last_pos[:, :OBJECTS]
    zero = torch.zeros((), dtype=f32, device=dev)
    move_prep = torch.where(main[:, None], dist(prep_pos, start_pos), dist(last_obj, start_pos))
    move_main = torch.where(main[:, None], dist(last_obj, prep_pos), zero)
    lock_prep = torch.where(main[:, None], state["prep_locks"], state["last_locks"])
    idx = torch.arange(OBJECTS, device=dev)
    n_obj = state["n_obj"]
    present = torch.where(idx < MAX_BOXES, idx < n_obj[:, :1], idx - MAX_BOXES < n_obj[:, 1:]) & book[:, None]
    add = torch.zeros(STATS, dtype=torch.float64, device=dev)
    add[WORLD_EPISODES], add[REACHED_MAIN], add[BAD] = book.sum(), (book & main).sum(), (~has).sum()
    eps = torch.tensor(move_eps, dtype=f32, device=dev)
    for (lo, hi), o in (((0, MAX_BOXES), BOXES), ((MAX_BOXES, OBJECTS), RAMPS)):
        pr = present[:, lo:hi]
        add[o + 0] = torch.where(pr, move_prep[:, lo:hi], zero).amax(1).double().sum()
        add[o + 1] = torch.where(pr, move_main[:, lo:hi], zero).amax(1).double().sum()
        add[o + 2], add[o + 3] = (pr & (move_prep[:, lo:hi] > eps)).sum(), (pr & (move_main[:, lo:hi] > eps)).sum()
        add[o + 4], add[o + 5] = (pr & (lock_prep[:, lo:hi] == 1)).sum(), (pr & (lock_prep[:, lo:hi] == 2)).sum()
        add[o + 6], add[o + 7] = (pr & (state["last_locks"][:, lo:hi] == 1)).sum(), (pr & (state["last_locks"][:, lo:hi] == 2)).sum()
        add[o + 8] = pr.sum()
    for side, o in ((SEEKER, SEEKERS), (HIDER, HIDERS)):
        add[o + 0] = torch.where(book, state["travel"][:, side], zero).double().sum()
        add[o + 1], add[o + 2] = (state["grab"][:, side] * book).sum(), (state["agent_steps"][:, side] * book).sum()
    # steps 3 and 4
    start = has & (ended | (phase == UNARMED) | ((phase != WAITING) & restarted))
    cont = has & ~start & armed
    release = cont & (phase == PREP) & (p == 0)
    nb, nr, nh = counts[:, 0].clamp(0, MAX_BOXES), counts[:, 1].clamp(0, MAX_RAMPS), counts[:, 2].clamp(0, MAX_AGENTS)
    ns = torch.minimum(counts[:, 3].clamp(min=0), MAX_AGENTS - nh)
    lh, ls = state["n_side"][:, HIDER], state["n_side"][:, SEEKER]
    d_agent = dist(positions[:, OBJECTS:], last_pos[:, OBJECTS:])
    travel_s, travel_h = state["travel"][:, SEEKER], state["travel"][:, HIDER]
    for i in range(MAX_AGENTS):
        travel_h = torch.where(cont & (i < lh), travel_h + d_agent[:, i], travel_h)
        travel_s = torch.where(cont & (i >= lh) & (i - lh < ls), travel_s + d_agent[:, i], travel_s)
    steps = torch.stack([(act & ~hider).sum(1), (act & hider).sum(1)], 1).to(torch.int32)
    grab = torch.stack([(act & ~hider & grabs).sum(1), (act & hider & grabs).sum(1)], 1).to(torch.int32)
    s1, s2, s3 = start[:, None], start[:, None, None], (start | cont)[:, None, None]
    new = dict(
        n_obj=torch.where(s1, torch.stack([nb, nr], 1), n_obj), n_side=torch.where(s1, torch.stack([ns, nh], 1), state["n_side"]),
        start_pos=torch.where(s2, positions[:, :OBJECTS], start_pos),
        prep_pos=torch.where((start | release)[:, None, None], positions[:, :OBJECTS], prep_pos),
        last_pos=torch.where(s3, positions, last_pos),
        prep_locks=torch.where((start | release)[:, None], locks, state["prep_locks"]),
        last_locks=torch.where((start | cont)[:, None], locks, state["last_locks"]),
        travel=torch.where(s1, zero, torch.stack([travel_s, travel_h], 1)),
        grab=torch.where(s1, grab, torch.where(cont[:, None], state["grab"] + grab, state["grab"])),
        agent_steps=torch.where(s1, steps, torch.where(cont[:, None], state["agent_steps"] + steps, state["agent_steps"])),
        phase=torch.where(start, torch.where(p > 0, PREP, MAIN), torch.where(release, MAIN, phase)),
        was_active=act.reshape(-1))
    for k, v in new.items():
        state[k].copy_(v.reshape(state[k].shape))
    table += add


class BehaviourStats:
    """The tracker of one simulator: it owns the state and the table.  arm() once, step() after every sim.step(), read()
    whenever the numbers are wanted."""

    def __init__(self, sim, move_eps=DEFAULT_MOVE_EPS):
        import torch
        self.sim, self.move_eps = sim, _move_eps(move_eps)
        self.device = torch.device("cuda", sim.gpu_id)
        self.state = new_state(sim.num_worlds, sim.agents_per_world, self.device)
        self.table = torch.zeros(STATS, dtype=torch.float64, device=self.device)
        self.steps = 0                    # step() calls since the tracker was made
        # the tensors above stay where they are: the request is checked and built once
        self._req = request(sim.num_worlds, sim.agents_per_world, sim.gpu_id, self.state, self.table, self.move_eps)[1]
        self.arm()

    def arm(self, from_start=False):
        """Every world waits for its next episode start (a done), so that no episode is booked of which a part was not
        seen.  With from_start=True, right after sim.init(): the episodes start now, so the positions, locks and counts
        are latched from the simulator as it stands.  The table is left as it is."""
        for t in self.state.values():
            t.zero_()
        if from_start:                    # an unarmed world starts at once: the kernel's own latch
            with on_current_stream():
                _run(self.sim, "hs_behaviour_stats", self._req, None)
        else:
            self.state["phase"].fill_(WAITING)
        return self

    def step(self):
        """After a sim.step(): the kernel and its fold on torch's current stream, nothing read back."""
        with on_current_stream():
            _run(self.sim, "hs_behaviour_stats", self._req, None)
        self.steps += 1

    def read(self, reset=True):
        """stats_to_metrics of the table, by one copy to the host (which waits for the device); with `reset` the table
        starts again from zero.  The worlds' running episodes are not touched."""
        host = self.table.cpu()
        if reset:
            self.table.zero_()
        return stats_to_metrics(host)
