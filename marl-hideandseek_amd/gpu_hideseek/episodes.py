"""Episode statistics: the return and length of every finished episode per side, and who won, kept on the device by one
kernel after every step (hs_episode_stats, csrc/hs_k_episode.h).

include/hideseek.h states the arithmetic and the three traps it handles (rollout.py documents them for the recurrent
state): the observation exported together with done, and with it self_type and self_mask, belongs to the NEXT episode; a
row that left keeps a stale done and reward; a row that joins exports done = 0.  A reset the host requests in
mid-episode sets no done and is not covered.

    ep = episodes.EpisodeStats(sim, gamma=0.998)
    ep.arm(from_start=True)                       # right after sim.init(); ep.arm() anywhere else
    for _ in range(steps):
        ...                                       # write the actions
        sim.step()
        ep.step()                                 # one launch, no read of the device
    print(ep.read())                              # one copy to the host; the table starts again from zero

The table is 14 float64 sums (stats_to_metrics turns them into means): for the seekers, then for the hiders, episodes,
sum of returns, of their squares, of the discounted returns and of the lengths; then hider wins, seeker wins, draws and
world episodes.  A call adds to it, without atomics and in a fixed order: the same steps give the same bits.
"""
import ctypes as C
import math

from ._request import _disjoint, _run, _shard_calls, _tensor, on_current_stream

STATS = 14                # HS_EPISODE_STATS
SIDE_STATS = 5            # HS_EPISODE_SIDE_STATS: episodes, sum ret, sum ret^2, sum disc, sum len
OUT, TRACKED, WAITING = 0, 1, 2                   # HS_EPISODE_OUT / _TRACKED / _WAITING: a row's phase
SEEKER, HIDER = 0, 1      # self_type, and the order of the sides in the table
HIDER_WINS, SEEKER_WINS, DRAWS, WORLD_EPISODES = 10, 11, 12, 13
DEFAULT_GAMMA = 0.998     # scripts/jax_train.py:152
ROW_STATE = (("ret", "float32"), ("disc", "float32"), ("gpow", "float32"), ("len", "int32"), ("type", "int32"), ("phase", "int32"))
WORLD_STATE = (("world_hider_team", "int32"), ("world_phase", "int32"))
ROW_INPUTS = (("reward", "float32"), ("done", "int32"), ("self_type", "int32"), ("self_mask", "float32"))


class HsEpisodeRequest(C.Structure):
    """hs_episode_request (include/hideseek.h)."""
    _fields_ = [("reward", C.c_void_p), ("done", C.c_void_p), ("self_type", C.c_void_p), ("self_mask", C.c_void_p),
                ("episode_result", C.c_void_p), ("hider_team", C.c_void_p), ("gamma", C.c_float), ("reserved", C.c_int32),
                ("ret", C.c_void_p), ("disc", C.c_void_p), ("gpow", C.c_void_p), ("len", C.c_void_p), ("type", C.c_void_p),
                ("phase", C.c_void_p), ("world_hider_team", C.c_void_p), ("world_phase", C.c_void_p), ("table", C.c_void_p)]


def new_state(num_worlds, agents, device):
    """A tracker's state, {name: tensor}: every row out with zero sums (gpow 1), no world's team order latched."""
    import torch
    rows = num_worlds * agents
    st = {k: torch.zeros(rows, dtype=getattr(torch, d), device=device) for k, d in ROW_STATE}
    st.update({k: torch.zeros(num_worlds, dtype=getattr(torch, d), device=device) for k, d in WORLD_STATE})
    st["gpow"].fill_(1.0)
    return st


def stats_to_metrics(table):
    """The table (a [14] tensor, or 14 numbers) as Python numbers in float64: {"seekers": {...}, "hiders": {...}} with
    episodes, return_mean, return_std (biased), discounted_return_mean and length_mean of the side's finished episodes,
    and world_episodes, hider_win_rate, seeker_win_rate, draw_rate.  Everything is 0.0 where the count is 0."""
    t = [float(x) for x in (table.tolist() if hasattr(table, "tolist") else table)]
    if len(t) != STATS:
        raise ValueError(f"table has {STATS} values, got {len(t)}")
    out = {}
    for name, o in (("seekers", SEEKER * SIDE_STATS), ("hiders", HIDER * SIDE_STATS)):
        n, s1, s2, sd, sl = t[o:o + SIDE_STATS]
        if n > 0:
            mean = s1 / n
            side = dict(episodes=n, return_mean=mean, return_std=math.sqrt(max(s2 / n - mean * mean, 0.0)), discounted_return_mean=sd / n, length_mean=sl / n)
        else:
            side = dict(episodes=0.0, return_mean=0.0, return_std=0.0, discounted_return_mean=0.0, length_mean=0.0)
        out[name] = side
    w = t[WORLD_EPISODES]
    out["world_episodes"] = w
    for name, i in (("hider_win_rate", HIDER_WINS), ("seeker_win_rate", SEEKER_WINS), ("draw_rate", DRAWS)):
        out[name] = t[i] / w if w > 0 else 0.0
    return out


def request(num_worlds, agents, gpu_id, state, table, gamma=DEFAULT_GAMMA, reward=None, done=None, self_type=None, self_mask=None,
            episode_result=None, hider_team=None):
    """Validate a call over num_worlds x agents agent rows on GPU `gpu_id`: `state` as new_state() makes it, `table`
    [14] float64, and the inputs given explicitly ([rows], [rows, 1] or [num_worlds, agents]; episode_result
    [num_worlds, 2]; hider_team [num_worlds] or [num_worlds, 1]); None means the simulator's own.  Returns
    ({"table": table, "state": state}, HsEpisodeRequest).  Raises ValueError before the library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    rows = num_worlds * agents
    gamma = float(gamma)
    if not (math.isfinite(gamma) and 0.0 <= gamma <= 1.0):
        raise ValueError(f"gamma must be finite and in [0, 1], got {gamma}")
    if not isinstance(state, dict) or set(state) != {k for k, _ in ROW_STATE + WORLD_STATE}:
        raise ValueError("state must be a dict of " + ", ".join(k for k, _ in ROW_STATE + WORLD_STATE) + " (episodes.new_state)")
    per_row, per_world = [(rows,), (rows, 1), (num_worlds, agents)], [(num_worlds,), (num_worlds, 1)]
    given = dict(reward=reward, done=done, self_type=self_type, self_mask=self_mask)
    inputs = []
    for k, d in ROW_INPUTS:
        if given[k] is not None:
            _tensor(k, given[k], per_row, (d,), dev, "None or a torch tensor")
            inputs.append((k, given[k]))
    if episode_result is not None:
        _tensor("episode_result", episode_result, (num_worlds, 2), ("float32",), dev, "None or a torch tensor")
        inputs.append(("episode_result", episode_result))
    if hider_team is not None:
        _tensor("hider_team", hider_team, per_world, ("int32",), dev, "None or a torch tensor")
        inputs.append(("hider_team", hider_team))
    outputs = []
    for k, d in ROW_STATE:
        _tensor(k, state[k], per_row, (d,), dev)
        outputs.append((k, state[k]))
    for k, d in WORLD_STATE:
        _tensor(k, state[k], per_world, (d,), dev)
        outputs.append((k, state[k]))
    _tensor("table", table, (STATS,), ("float64",), dev)
    outputs.append(("table", table))
    _disjoint(outputs, inputs, dev)

    def ptr(t):
        return None if t is None else t.data_ptr()
    req = HsEpisodeRequest(ptr(reward), ptr(done), ptr(self_type), ptr(self_mask), ptr(episode_result), ptr(hider_team), gamma, 0,
                           *(state[k].data_ptr() for k, _ in ROW_STATE + WORLD_STATE), table.data_ptr())
    return {"table": table, "state": state}, req


def compute(sim, state, table, stream=None, **kw):
    """HideAndSeekSimulator.episode_stats."""
    res, req = request(sim.num_worlds, sim.agents_per_world, sim.gpu_id, state, table, **kw)
    _run(sim, "hs_episode_stats", req, stream)
    return res


def compute_sharded(ssim, state, table, stream=None, gamma=DEFAULT_GAMMA, **inputs):
    """ShardedSimulator.episode_stats: every shard tracks its own worlds on its own device."""
    return _shard_calls(ssim, "hs_episode_stats", request, stream, dict(state=state, table=table), per_shard=inputs, kw=dict(gamma=gamma),
                        lead=lambda s: (s.num_worlds, s.agents_per_world, s.gpu_id))


def step_trackers(*hooks):
    """After a driver's sim.step(): step() of every tracker, in order.  A hook is None, a tracker or a list of trackers."""
    for hook in hooks:
        for tracker in ([] if hook is None else hook if isinstance(hook, (list, tuple)) else [hook]):
            tracker.step()


class EpisodeStats:
    """The tracker of one simulator: it owns the state and the table.  arm() once, step() after every sim.step(), read()
    whenever the numbers are wanted."""

    def __init__(self, sim, gamma=DEFAULT_GAMMA):
        import torch
        gamma = float(gamma)
        if not (math.isfinite(gamma) and 0.0 <= gamma <= 1.0):
            raise ValueError(f"gamma must be finite and in [0, 1], got {gamma}")
        self.sim, self.gamma = sim, gamma
        self.device = torch.device("cuda", sim.gpu_id)
        self.state = new_state(sim.num_worlds, sim.agents_per_world, self.device)
        self.table = torch.zeros(STATS, dtype=torch.float64, device=self.device)
        self.steps = 0                    # step() calls since the tracker was made or loaded
        # the tensors above stay where they are (load_state_dict copies into them): the request is checked and built once
        self._req = request(sim.num_worlds, sim.agents_per_world, sim.gpu_id, self.state, self.table, gamma)[1]
        self.arm()

    def arm(self, from_start=False):
        """Every row waits for its next episode start (a done), so that no episode is counted of which a part was not
        seen.  With from_start=True, right after sim.init(): the episodes start now, so the rows' type and mask and the
        worlds' team order are latched from the simulator as it stands.  The sums of the rows start from zero either
        way; the table is left as it is."""
        st = self.state
        for k in ("ret", "disc", "len", "type", "world_hider_team", "world_phase"):
            st[k].zero_()
        st["gpow"].fill_(1.0)
        st["phase"].fill_(OUT if from_start else WAITING)
        if from_start:                    # a row that is out restarts at once: the kernel's own latch, and no reward is used
            with on_current_stream():
                _run(self.sim, "hs_episode_stats", self._req, None)
        return self

    def step(self):
        """After a sim.step(): one launch on torch's current stream, nothing read back."""
        with on_current_stream():
            _run(self.sim, "hs_episode_stats", self._req, None)
        self.steps += 1

    def read(self, reset=True):
        """stats_to_metrics of the table, by one copy to the host (which waits for the device); with `reset` the table
        starts again from zero.  The rows' running episodes are not touched."""
        host = self.table.cpu()
        if reset:
            self.table.zero_()
        return stats_to_metrics(host)

    def state_dict(self):
        return {"state": {k: t.clone() for k, t in self.state.items()}, "table": self.table.clone(), "gamma": self.gamma, "steps": self.steps}

    def load_state_dict(self, d):
        if set(d["state"]) != set(self.state):
            raise ValueError("not an EpisodeStats state")
        for k, t in self.state.items():
            if tuple(d["state"][k].shape) != tuple(t.shape):
                raise ValueError(f"{k} has shape {tuple(d['state'][k].shape)}, this simulator needs {tuple(t.shape)}")
        for k, t in self.state.items():
            t.copy_(d["state"][k])
        self.table.copy_(d["table"])
        self.gamma, self.steps = float(d["gamma"]), int(d["steps"])
        self._req.gamma = self.gamma
