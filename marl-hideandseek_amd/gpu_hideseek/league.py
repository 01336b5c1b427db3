"""Competitive evaluation: several policies play each other on one simulator and are rated (the function of the
reference's eval_competitive with num_policies > 1 and of its print_elos).  One call after every step, hs_league_step
(csrc/hs_k_league.h), routes every agent row to a policy, books the games that ended with the step in a P x P table and
moves the Elo ratings; include/hideseek.h states the schedule, the routing, the outcomes and the rating arithmetic.
madrona_learn's matchmaking is not in the reference's tree: the contract is the project's own.

    lg = league.League(sim, [(net_a, norm_a), (net_b, norm_b)], team_size=3, mode="draw")     # sim right after sim.init()
    lg.run(2400)
    out = lg.read()                                   # {"counts": [P][P][4], "games": n, "elo": [...], "bad": 0}
    league.print_elos(out["elo"])

The schedule is fixed: world w plays pair q = w mod P^2, policy q // P the hiders and policy q % P the seekers, so every
policy owns exactly R / P of the R agent rows at every step whatever RandomFlipTeams does, the P forwards have fixed
shapes, and nothing is read back from the device to size them.  counts[i][j] = (hider wins, seeker wins, draws, played
without an outcome) of hiders i against seekers j.  Ratings are batched by step: the games that end with one step are all
rated against the ratings before it.

Table is that state on the device with the step that moves it; League holds one, and so does population.Population.
host_step is the contract in plain numpy (int64 counts, float64 ratings, the same pair order): the tests' reference, and
it needs no GPU.  Single device: there is no ShardedSimulator form, because the ratings would have to cross the shards.
Training several policies at once on this schedule (several train states, live ratings, hyper-parameter exploration) is
gpu_hideseek.population.

A schedule can also be a TABLE (hs_league_set_schedule, hs_league_step_scheduled): `pairs`, a list of G (hider_policy,
seeker_policy) over N policies; world w plays pairs[w mod G] and g = w // G is its group.  check_schedule states what makes
a table valid; the rule that matters is that it is REGULAR, every policy holding the same number c = 2 G / N of sides per
group, because that is exactly what gives every policy R / N rows at every step: the routing stays a permutation with
equal blocks, and the routed pack, the routed sampler and the grouped advantages run on it unchanged.
all_pairs_schedule(P) is the fixed schedule as a table; past_play_schedule(T, Q) is the population's pool of past
policies (the reference's --pbt-past-policies with past_play_portion = 1): learners 0 .. T-1 play the frozen policies
T .. T+Q-1 on both sides, never past against past.  The League evaluator itself plays the fixed schedule only.
"""
import ctypes as C
import math

from . import policy_inputs, replay, rollout
from ._request import _disjoint, _run, _tensor, on_current_stream
from .episodes import step_trackers

MAX_POLICIES = 16         # HS_LEAGUE_MAX_POLICIES
MAX_GROUP = 256           # HS_LEAGUE_MAX_GROUP
FILLS = ("cross", "self")
OUTCOMES = 4              # HS_LEAGUE_OUTCOMES
HIDERS_WIN, SEEKERS_WIN, DRAW, NO_OUTCOME = 0, 1, 2, 3
DEFAULT_K_FACTOR = 32.0
INITIAL_ELO = 1500.0
MODES = ("draw", "greedy")
WORLD_STATE = (("world_hider_team", "int32"), ("world_phase", "int32"))
ROW_INPUTS = (("done", "int32"), ("self_type", "int32"), ("self_mask", "float32"))
ROUTING = ("policy_assignments", "slot", "row_of_slot", "clear_slot")


class HsLeagueRequest(C.Structure):
    """hs_league_request (include/hideseek.h)."""
    _fields_ = [("done", C.c_void_p), ("self_type", C.c_void_p), ("self_mask", C.c_void_p), ("episode_result", C.c_void_p),
                ("hider_team", C.c_void_p), ("num_policies", C.c_int32), ("team_size", C.c_int32), ("k_factor", C.c_double),
                ("policy_assignments", C.c_void_p), ("slot", C.c_void_p), ("row_of_slot", C.c_void_p), ("clear_slot", C.c_void_p),
                ("world_hider_team", C.c_void_p), ("world_phase", C.c_void_p), ("bad", C.c_void_p), ("counts", C.c_void_p), ("elo", C.c_void_p)]


def _league_shape(num_worlds, agents, num_policies, team_size, group=None):
    for name, v in (("num_policies", num_policies), ("team_size", team_size)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if not 1 <= num_policies <= MAX_POLICIES:
        raise ValueError(f"num_policies must be in [1, {MAX_POLICIES}], got {num_policies}")
    if team_size < 1 or agents != 2 * team_size:
        raise ValueError(f"team_size must be at least 1 and the simulator's agents per world 2 * team_size: team_size {team_size}, {agents} agents")
    if group is None:
        if num_worlds < 1 or num_worlds % (num_policies * num_policies):
            raise ValueError(f"num_worlds must be a multiple of num_policies^2 = {num_policies * num_policies}, got {num_worlds}")
    else:
        if isinstance(group, bool) or not isinstance(group, int) or not 1 <= group <= MAX_GROUP:
            raise ValueError(f"group must be an integer in [1, {MAX_GROUP}], got {group!r}")
        if num_worlds < 1 or num_worlds % group:
            raise ValueError(f"num_worlds must be a multiple of the schedule's group = {group}, got {num_worlds}")
    if num_worlds * agents >= 2 ** 31:
        raise ValueError("num_worlds * agents must stay below 2^31")


def _k_factor(k_factor):
    k = float(k_factor)
    if not (math.isfinite(k) and k > 0.0):
        raise ValueError(f"k_factor must be finite and above 0, got {k_factor}")
    return k


def schedule(num_worlds, num_policies):
    """(hider_policy[w], seeker_policy[w]) as lists: world w plays pair q = w mod P^2, q // P against q % P."""
    P = int(num_policies)
    if not 1 <= P <= MAX_POLICIES or num_worlds < 1 or num_worlds % (P * P):
        raise ValueError(f"num_worlds must be a multiple of num_policies^2 with num_policies in [1, {MAX_POLICIES}]: {num_worlds} worlds, {num_policies} policies")
    return [(w % (P * P)) // P for w in range(num_worlds)], [(w % (P * P)) % P for w in range(num_worlds)]


def check_schedule(pairs, num_policies):
    """The table `pairs` over `num_policies` policies as a list of (int, int), or ValueError naming the first rule it breaks,
    in this order: 1 <= N <= 16; 1 <= G <= 256; every entry in [0, N); regular, every policy holding the same number
    c = 2 G / N of sides per group (a pair (i, i) gives i two)."""
    N = num_policies
    if isinstance(N, bool) or not isinstance(N, int) or not 1 <= N <= MAX_POLICIES:
        raise ValueError(f"num_policies must be an integer in [1, {MAX_POLICIES}], got {N!r}")
    try:
        table = [(int(i), int(j)) for i, j in pairs]
    except (TypeError, ValueError):
        raise ValueError("pairs must be a list of (hider_policy, seeker_policy)") from None
    G = len(table)
    if not 1 <= G <= MAX_GROUP:
        raise ValueError(f"the group, len(pairs), must be in [1, {MAX_GROUP}], got {G}")
    for q, (i, j) in enumerate(table):
        if not (0 <= i < N and 0 <= j < N):
            raise ValueError(f"pairs[{q}] = ({i}, {j}) is out of range: every entry must be in [0, {N})")
    sides = [0] * N
    for i, j in table:
        sides[i] += 1
        sides[j] += 1
    if any(n * N != 2 * G for n in sides):
        raise ValueError(f"the schedule is not regular: every policy must hold 2 G / N = {2 * G}/{N} sides per group, they hold {sides}")
    return table


def all_pairs_schedule(num_policies):
    """The fixed schedule as a table: pair q is (q // P, q % P)."""
    P = int(num_policies)
    return [(q // P, q % P) for q in range(P * P)]


def past_play_schedule(num_train, num_past, fill="cross"):
    """The table of T = num_train learners (policies 0 .. T-1) and a pool of Q = num_past frozen ones (T .. T+Q-1), with
    1 <= Q <= T and T + Q <= 16: for t in 0..T-1, for u in 0..Q-1: (t, T+u) then (T+u, t); then, for r in 1..T-Q, for t in
    0..T-1: (t, (t+r) % T) with fill "cross", (t, t) with fill "self".  G = T (T + Q), every policy holds 2 T sides, and
    no pair is past against past.  Q > T is refused: the pool would hold fewer sides than the learners, and only games
    between past policies, which nobody learns from, could fill the gap."""
    T, Q = num_train, num_past
    for name, v in (("num_train", T), ("num_past", Q)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if fill not in FILLS:
        raise ValueError(f"fill must be one of {FILLS}, got {fill!r}")
    if not 1 <= Q <= T:
        raise ValueError(f"num_past must be in [1, num_train]: num_train {T}, num_past {Q}")
    if T + Q > MAX_POLICIES:
        raise ValueError(f"num_train + num_past must be at most {MAX_POLICIES}, got {T} + {Q}")
    pairs = [x for t in range(T) for u in range(Q) for x in ((t, T + u), (T + u, t))]
    pairs += [(t, (t + r) % T if fill == "cross" else t) for r in range(1, T - Q + 1) for t in range(T)]
    return pairs


def _held(pairs, num_policies):
    """held[q][p]: the sides policy p holds in the pairs before q."""
    held, row = [], [0] * num_policies
    for i, j in pairs:
        held.append(list(row))
        row[i] += 1
        row[j] += 1
    return held


def new_state(num_worlds, device):
    """The per-world state, {name: tensor}: no world's team order latched."""
    import torch
    return {k: torch.zeros(num_worlds, dtype=getattr(torch, d), device=device) for k, d in WORLD_STATE}


def print_elos(elos, file=None):
    """The ratings four to a line, each as f"{idx:>3}: {elo:>8.2f}": the layout of the reference's table."""
    vals = [float(e) for e in (elos.tolist() if hasattr(elos, "tolist") else elos)]
    for lo in range(0, len(vals), 4):
        print("".join(f"{idx:>3}: {elo:>8.2f}       " for idx, elo in enumerate(vals[lo:lo + 4], lo)), file=file)


def host_step(state, counts, elo, num_policies, team_size, done, self_type, self_mask, episode_result, hider_team, k_factor=DEFAULT_K_FACTOR, pairs=None):
    """The contract of hs_league_step in plain numpy, one world at a time.  `state` {"world_hider_team", "world_phase"}
    (int32 [worlds]), `counts` (int64 [P, P, 4]) and `elo` (float64 [P]) are updated in place; done, self_type, self_mask
    are [R], episode_result [worlds, 2], hider_team [worlds].  Returns {"policy_assignments", "slot", "row_of_slot",
    "clear_slot": int32 [R], "bad": int}.  With `pairs` (a table that passes check_schedule for num_policies) it is the
    contract of hs_league_step_scheduled: world w plays pairs[w mod G], and only the pair and the slot are found otherwise."""
    import numpy as np
    P, k = int(num_policies), int(team_size)
    A = 2 * k
    done, self_type, self_mask = (np.asarray(x).reshape(-1) for x in (done, self_type, self_mask))
    worlds = done.shape[0] // A
    R = worlds * A
    episode_result, hider_team = np.asarray(episode_result).reshape(worlds, 2), np.asarray(hider_team).reshape(worlds)
    policy, slot = np.zeros(R, np.int32), np.zeros(R, np.int32)
    delta = np.zeros((P, P, OUTCOMES), np.int64)
    bad = 0
    if pairs is None:
        G, c = P * P, 2 * P
        held = [[sum((qq // P == p) + (qq % P == p) for qq in range(q)) for p in range(P)] for q in range(P * P)]
    else:
        G, c = len(pairs), 2 * len(pairs) // P
        held = _held(pairs, P)
    for w in range(worlds):
        rows = slice(w * A, (w + 1) * A)
        hider = self_type[rows] != 0
        if int(hider.sum()) != k or bool((self_mask[rows] == 0).any()):
            bad += 1
            hider = np.arange(A) < k
        g, q = divmod(w, G)
        i, j = divmod(q, P) if pairs is None else pairs[q]
        for r in range(A):
            p = i if hider[r] else j
            sides = held[q][p]                  # the sides p holds in the worlds of the group before q
            rank = sum(1 for b in range(r) if (i if hider[b] else j) == p)
            policy[w * A + r] = p
            slot[w * A + r] = p * (R // P) + g * c * k + k * sides + rank
        ended = done[w * A] != 0
        if ended and state["world_phase"][w] == 1:
            h = int(state["world_hider_team"][w])
            o = NO_OUTCOME
            if h in (0, 1):
                x = float(episode_result[w, h])
                o = HIDERS_WIN if x == 1.0 else SEEKERS_WIN if x == 0.0 else DRAW if x == 0.5 else NO_OUTCOME
            delta[i, j, o] += 1
        if ended or state["world_phase"][w] == 0:
            state["world_hider_team"][w] = hider_team[w]
            state["world_phase"][w] = 1
    row_of_slot, clear_slot = np.zeros(R, np.int32), np.zeros(R, np.int32)
    row_of_slot[slot] = np.arange(R, dtype=np.int32)
    clear_slot[slot] = done
    counts += delta
    before = np.array(elo, np.float64)
    kf = np.float64(k_factor)
    for i in range(P):
        for j in range(P):
            n = int(delta[i, j, 0] + delta[i, j, 1] + delta[i, j, 2])
            if i == j or n == 0:
                continue
            S = np.float64(delta[i, j, 0]) + np.float64(0.5) * np.float64(delta[i, j, 2])
            E = np.float64(1.0) / (np.float64(1.0) + np.float64(10.0) ** ((before[j] - before[i]) / np.float64(400.0)))
            d = kf * (S - np.float64(n) * E)
            elo[i] = elo[i] + d
            elo[j] = elo[j] - d
    return dict(policy_assignments=policy, slot=slot, row_of_slot=row_of_slot, clear_slot=clear_slot, bad=bad)


def request(num_worlds, agents, gpu_id, num_policies, team_size, state, counts, elo, k_factor=DEFAULT_K_FACTOR, policy_assignments=None, slot=None,
            row_of_slot=None, clear_slot=None, bad=None, done=None, self_type=None, self_mask=None, episode_result=None, hider_team=None, group=None):
    """Validate a call over num_worlds x agents agent rows on GPU `gpu_id` for a league of `num_policies` with teams of
    `team_size`: `state` as new_state() makes it, `counts` [P, P, 4] int64, `elo` [P] float64; the routing outputs
    policy_assignments, slot, row_of_slot, clear_slot (int32 [rows], [rows, 1] or [num_worlds, agents]) and bad (int32 [1])
    are each None or a tensor (policy_assignments None: the simulator's own export is written); the inputs given
    explicitly as in episodes.request, None meaning the simulator's own.  Returns ({"counts", "elo", "state" and the
    outputs given}, HsLeagueRequest).  With `group` (the G of a schedule table) the request is one for
    hs_league_step_scheduled: num_worlds must be a multiple of group, not of num_policies^2.  Raises ValueError before the
    library is involved."""
    import torch
    dev = torch.device("cuda", gpu_id)
    _league_shape(num_worlds, agents, num_policies, team_size, group)
    k_factor = _k_factor(k_factor)
    P, rows = num_policies, num_worlds * agents
    if not isinstance(state, dict) or set(state) != {k for k, _ in WORLD_STATE}:
        raise ValueError("state must be a dict of " + ", ".join(k for k, _ in WORLD_STATE) + " (league.new_state)")
    per_row, per_world = [(rows,), (rows, 1), (num_worlds, agents)], [(num_worlds,), (num_worlds, 1)]
    given = dict(done=done, self_type=self_type, self_mask=self_mask)
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
    routing = dict(policy_assignments=policy_assignments, slot=slot, row_of_slot=row_of_slot, clear_slot=clear_slot)
    for k in ROUTING:
        if routing[k] is not None:
            _tensor(k, routing[k], per_row, ("int32",), dev, "None or a torch tensor")
            outputs.append((k, routing[k]))
    for k, d in WORLD_STATE:
        _tensor(k, state[k], per_world, (d,), dev)
        outputs.append((k, state[k]))
    if bad is not None:
        _tensor("bad", bad, (1,), ("int32",), dev, "None or a torch tensor")
        outputs.append(("bad", bad))
    _tensor("counts", counts, (P, P, OUTCOMES), ("int64",), dev, align=8)
    _tensor("elo", elo, (P,), ("float64",), dev, align=8)
    outputs += [("counts", counts), ("elo", elo)]
    _disjoint(outputs, inputs, dev)

    def ptr(t):
        return None if t is None else t.data_ptr()
    req = HsLeagueRequest(ptr(done), ptr(self_type), ptr(self_mask), ptr(episode_result), ptr(hider_team), P, team_size, k_factor,
                          *(ptr(routing[k]) for k in ROUTING), *(state[k].data_ptr() for k, _ in WORLD_STATE), ptr(bad), counts.data_ptr(), elo.data_ptr())
    res = {"counts": counts, "elo": elo, "state": state}
    res.update({k: t for k, t in routing.items() if t is not None})
    if bad is not None:
        res["bad"] = bad
    return res, req


def compute(sim, num_policies, team_size, state, counts, elo, stream=None, **kw):
    """HideAndSeekSimulator.league_step."""
    res, req = request(sim.num_worlds, sim.agents_per_world, sim.gpu_id, num_policies, team_size, state, counts, elo, **kw)
    _run(sim, "hs_league_step", req, stream)
    return res


def set_schedule(sim, pairs, num_policies):
    """HideAndSeekSimulator.set_league_schedule."""
    from ._native import check
    if pairs is None:
        check(sim._L.hs_league_set_schedule(sim._h, None, 0, 0))
        sim._league_schedule = None
        return None
    table = check_schedule(pairs, num_policies)
    flat = (C.c_int32 * (2 * len(table)))(*(x for pair in table for x in pair))
    check(sim._L.hs_league_set_schedule(sim._h, flat, len(table), num_policies))
    sim._league_schedule = (len(table), num_policies)
    return table


def compute_scheduled(sim, num_policies, team_size, state, counts, elo, stream=None, **kw):
    """HideAndSeekSimulator.league_step_scheduled."""
    sched = getattr(sim, "_league_schedule", None)
    if sched is None:
        raise ValueError("no schedule is set: call set_league_schedule(pairs, num_policies) first")
    if num_policies != sched[1]:
        raise ValueError(f"num_policies must equal the schedule's {sched[1]}, got {num_policies!r}")
    res, req = request(sim.num_worlds, sim.agents_per_world, sim.gpu_id, num_policies, team_size, state, counts, elo, group=sched[0], **kw)
    _run(sim, "hs_league_step_scheduled", req, stream)
    return res


def table_views(table, num_policies):
    """The three views of a packed league table `table` (int64 [P P 4 + P + 1], on any device) for P = num_policies:
    (counts [P, P, 4] int64, elo [P] float64, bad_total [1] int64).  They alias `table`."""
    import torch
    P, n = num_policies, num_policies * num_policies * OUTCOMES
    return table[:n].view(P, P, OUTCOMES), table[n:n + P].view(torch.float64), table[n + P:]


class Table:
    """The league's state on the device for `num_policies` policies on `sim`: the routing of the last step (TENSORS[:4]),
    the per-world state `world`, and counts | elo | bad_total (the malformed worlds of all steps) packed in `_table`, so
    that read() is one copy.  The tensors are never replaced: the request is checked and built once.  With `schedule`
    (a table of pairs) it is set on the simulator and step() is hs_league_step_scheduled.  Raises ValueError for the
    shape, then for k_factor, before anything touches the device."""
    TENSORS = ("slot", "row_of_slot", "clear_slot", "bad", "world", "_table", "counts", "elo", "bad_total")

    def __init__(self, sim, num_policies, team_size, k_factor=DEFAULT_K_FACTOR, schedule=None):
        import torch
        P, group = num_policies, None if schedule is None else len(schedule)
        _league_shape(sim.num_worlds, sim.agents_per_world, P, team_size, group)
        self.k_factor = _k_factor(k_factor)
        self.sim, self.num_policies = sim, P
        dev = torch.device("cuda", sim.gpu_id)
        i32 = dict(dtype=torch.int32, device=dev)
        self.slot, self.row_of_slot, self.clear_slot = (torch.zeros(sim.num_worlds * sim.agents_per_world, **i32) for _ in range(3))
        self.bad = torch.zeros(1, **i32)
        self.world = new_state(sim.num_worlds, dev)
        self._table = torch.zeros(P * P * OUTCOMES + P + 1, dtype=torch.int64, device=dev)
        self.counts, self.elo, self.bad_total = table_views(self._table, P)
        self.elo.fill_(INITIAL_ELO)
        if schedule is not None:
            sim.set_league_schedule(schedule, P)
        self._fn = "hs_league_step" if schedule is None else "hs_league_step_scheduled"
        self._req = request(sim.num_worlds, sim.agents_per_world, sim.gpu_id, P, team_size, self.world, self.counts, self.elo, self.k_factor,
                            slot=self.slot, row_of_slot=self.row_of_slot, clear_slot=self.clear_slot, bad=self.bad, group=group)[1]

    def bind(self, owner):
        """Set every tensor of TENSORS as an attribute of `owner` under its name here.  Returns self."""
        for k in self.TENSORS:
            setattr(owner, k, getattr(self, k))
        return self

    def step(self):
        """The entry point on the simulator's exports as they stand, on torch's current stream, then bad_total += bad."""
        with on_current_stream():
            _run(self.sim, self._fn, self._req, None)
        self.bad_total.add_(self.bad)

    def read(self):
        """{"counts": [P][P][4] lists (hider wins, seeker wins, draws, played without an outcome, of hiders i against
        seekers j), "games": their sum, "elo": [P], "bad": the malformed worlds seen} by one copy to the host (which waits
        for the device).  Nothing is reset."""
        counts, elo, bad_total = table_views(self._table.cpu(), self.num_policies)
        return {"counts": counts.tolist(), "games": int(counts.sum()), "elo": elo.tolist(), "bad": int(bad_total[0])}

    def state_dict(self):
        """{"world": clones of the per-world state, "table": a clone of the packed buffer}."""
        return {"world": {k: t.clone() for k, t in self.world.items()}, "table": self._table.clone()}

    def load_state_dict(self, d):
        """Copy what state_dict() returned into the tensors held here."""
        self._table.copy_(d["table"])
        for k, t in self.world.items():
            t.copy_(d["world"][k])


class League:
    """`policies`, a list of (net, normaliser or None) with net a policy.ActorCritic on the simulator's device, playing
    each other on `sim` under the fixed schedule: the multi-policy sibling of evaluate.Evaluator.  The simulator has
    team_size hiders and team_size seekers in every world and a number of worlds that is a multiple of len(policies)^2,
    and comes right from sim.init().  mode "draw" samples the actions with the uniforms keyed by (seed, step, global agent
    row), as the Evaluator's are; "greedy" takes every head's first maximum.  Nothing in a run changes a policy or a
    normaliser.  Single device: there is no ShardedSimulator form, because the ratings would have to cross the shards.
    `episodes` and `behaviour`, None by default: an episodes.EpisodeStats and a behaviour.BehaviourStats of the same
    simulator whose step() run() calls after every step."""

    def __init__(self, sim, policies, team_size, mode="draw", seed=0, k_factor=DEFAULT_K_FACTOR):
        import torch
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        policies = [tuple(p) for p in policies]
        if not policies or any(len(p) != 2 for p in policies):
            raise ValueError("policies must be a list of (net, normaliser or None)")
        P = len(policies)
        self.league_table = Table(sim, P, team_size, k_factor).bind(self)      # refuses the shape, then k_factor, before the nets are looked at
        self.k_factor = self.league_table.k_factor
        nets = [net for net, _ in policies]
        if any(net.buckets != nets[0].buckets for net in nets):
            raise ValueError("every policy must have the same action heads")
        self.sim, self.policies, self.team_size, self.mode, self.seed = sim, policies, int(team_size), mode, int(seed)
        self.num_policies = P
        self.rows = R = sim.num_worlds * sim.agents_per_world
        self.block = m = R // P                   # the rows of a policy, and the length of its block of slots
        self.device = dev = torch.device("cuda", sim.gpu_id)
        self.logit_width = L = sum(nets[0].buckets)
        # With one compute dtype (always, from tools/league.py) one routed pack writes every policy's block of slots under
        # that policy's table (hs_pack_policy_inputs_routed): `tables` holds a copy of each normaliser's table, the identity
        # for a policy without one, refreshed by arm() and at the start of run().  With several dtypes every policy packs
        # all rows with its own normaliser and gathers its block: one pair of buffers per compute dtype.
        self.routed = len({net.dtype for net in nets}) == 1
        self.packed = {net.dtype: torch.zeros(R, rollout.ROW, dtype=net.dtype, device=dev) for net in nets}
        self.gathered = {} if self.routed else {net.dtype: torch.zeros(1, m, rollout.ROW, dtype=net.dtype, device=dev) for net in nets}
        self.tables = torch.zeros(P, policy_inputs.NORM_TABLE, dtype=torch.float32, device=dev)
        self.logits_by_slot = torch.zeros(1, R, L, dtype=torch.float32, device=dev)
        self._acted_slot = torch.zeros(R, dtype=torch.int32, device=dev)      # `slot` as the last act() had it: the routing its logits belong to
        self.state = [net.actor.init_state(m, dev, net.dtype) for net in nets]
        self.counter = 0
        self.episodes = None
        self.behaviour = None
        self.arm()

    def refresh_tables(self):
        """Copy every normaliser's table as it stands into `tables` (the identity for a policy without normaliser): what
        the routed pack of act() reads.  arm() and run() call it; a caller that updates a normaliser between two act()
        calls of its own calls it too."""
        for p, (_, normaliser) in enumerate(self.policies):
            if normaliser is None:
                self.tables[p, :policy_inputs.ROW] = 0.0
                self.tables[p, policy_inputs.ROW:] = 1.0
            else:
                self.tables[p].copy_(policy_inputs.norm_table(normaliser, self.sim.gpu_id))

    def arm(self):
        """Right after sim.init(): no world's team order is latched, every carried LSTM state is zero, and the rows are
        routed from the simulator as it stands (which latches the team orders; no game is booked).  counts and elo are
        left as they are."""
        self.refresh_tables()
        for t in self.world.values():
            t.zero_()
        for s in self.state:
            for x in s:
                x.zero_()
        self.league_table.step()
        return self

    def act(self):
        """The observation in the simulator's exports -> the action tensor: every policy's forward over its own block of
        slots, its carried state advanced."""
        import torch
        sim, R, m = self.sim, self.rows, self.block
        with on_current_stream(), torch.no_grad():
            if self.routed:
                by_slot = self.packed[self.policies[0][0].dtype]
                sim.pack_policy_inputs_routed(self.row_of_slot, self.num_policies, actor=by_slot, tables=self.tables)
            for p, (net, normaliser) in enumerate(self.policies):
                block = slice(p * m, (p + 1) * m)
                if self.routed:
                    mine = by_slot[block]
                else:
                    packed, gathered = self.packed[net.dtype], self.gathered[net.dtype]
                    sim.pack_policy_inputs(actor=packed, normaliser=normaliser)
                    sim.gather_sequences(self.row_of_slot[block], [(packed.view(1, R, -1), gathered, False)], chunks=1, chunk_steps=1, rows=R)
                    mine = gathered[0]
                rollout.zero_where(self.clear_slot[block] != 0, *self.state[p])
                logits, self.state[p] = net.actor_logits(sim, mine, self.state[p], None)
                self.logits_by_slot[0, block] = logits.float()
            # slot-order logits -> row-order actions in one launch, with the bits sample_actions gives the gathered logits
            sim.sample_actions_routed(self.logits_by_slot[0], self.row_of_slot, buckets=self.policies[0][0].buckets, mode=self.mode, seed=(self.seed, 0),
                                      counter=self.counter)
            self._acted_slot.copy_(self.slot)
        self.counter += 1

    @property
    def logits(self):
        """The logits of the last act() in ROW order, [1, R, L] float32: gathered from logits_by_slot on request (act()
        itself samples from the slot order)."""
        return self.logits_by_slot[:, self._acted_slot.long()]

    def run(self, num_steps, record_log=None, on_step=None):
        """num_steps times: act(), sim.step(), the league's step, the attached episode tracker's; with `record_log` (a
        binary file open for writing) replay.record_step after every step; on_step(i, self), if given, after that.
        Returns read()."""
        self.refresh_tables()
        for i in range(int(num_steps)):
            self.act()
            self.sim.step()
            self.league_table.step()
            step_trackers(self.episodes, self.behaviour)
            if record_log is not None:
                replay.record_step(self.sim, record_log)
            if on_step is not None:
                on_step(i, self)
        return self.read()

    def read(self):
        """Table.read(): {"counts", "games", "elo", "bad"} by one copy to the host."""
        return self.league_table.read()


def hider_win_rates(counts):
    """[P][P]: the share of the games with an outcome that hiders i won against seekers j (0.0 where there were none)."""
    out = []
    for row in counts:
        out.append([(c[HIDERS_WIN] / (c[HIDERS_WIN] + c[SEEKERS_WIN] + c[DRAW])) if (c[HIDERS_WIN] + c[SEEKERS_WIN] + c[DRAW]) else 0.0 for c in row])
    return out
