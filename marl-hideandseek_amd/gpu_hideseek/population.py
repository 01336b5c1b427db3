"""Population training: P policies learn at once on one simulator under the league's fixed schedule (the function of the
reference's scripts/jax_train.py --pbt-ensemble-size N): the two sides improve against each other, not against a copy of
themselves.  Composition only, as gpu_hideseek.trainer is: the league's routing (hs_league_step, a league.Table), the routed
pack, the routed sampler, grouped advantages, and per policy a trainer.Learner's update.  Single device, like Trainer and League.

    sim.init()
    pop = population.Population(sim, population.PopulationConfig(num_policies=4, team_size=3, pbt_interval=10))
    for _ in range(updates):
        out = pop.update_iter()             # {"policies": [metrics per policy], "elo": [...], "games": n, "bad": n, "update": i, "fps": ...}

Everything is in SLOT order.  With R agent rows and m = R / P, policy p owns slots [p m, (p + 1) m) at every step,
whatever RandomFlipTeams does (league.py states the schedule), so the rollout is one shared rollout.Rollout of R rows whose
columns are slots, a policy's part of every [T, R, ...] buffer is the column block p, its forward is one call of fixed
shape on a block of one [R, 296] buffer, and its sequence ids are k R + p m + r' for a permutation of K m.

collect() follows Trainer.collect()'s time alignment (rollout.py states it).  Per slot t: sim.step() -> the attached
episode tracker's step() -> slot t - 1 is CLOSED: the reward and done exports are gathered into reward[t - 1] and
done[t - 1] with the routing of BEFORE this step (one gather_sequences call with two fields), because the reward of an
episode's last step belongs to the slot the row held when it acted, and the step that ends an episode may flip the teams
-> hs_league_step: the new routing, the games that ended, the ratings -> clear[t] = clear_slot -> the carried LSTM states
zeroed where clear_slot != 0 (the teams are full, so mask is 1 everywhere; a malformed world is counted in "bad") -> the
routed pack into actor[t], critic[t] and moments[:, t] -> at a chunk's first slot the snapshots of the carried states -> P
forwards on blocks -> one value_head decode over R rows -> one sample_actions_routed into the action export (row order),
action[t] and log_prob[t] (slot order).  A world's rows hold the same set of slots before and after a flip and done is the
same for every row of a world, so clear[t + 1] == done[t] holds slot for slot.
The league step runs EXACTLY ONCE per sim.step(): after the closing step of a rollout it is run there, and the next
collect() reuses that routing and clear_slot as Trainer reuses the exports, otherwise the games of that step would be
booked twice.  After the rollout: the bootstrap (a critic-only routed pack without moments, P critic forwards on the
carried critic states, which stay as they are, one decode), one compute_advantages(groups=P) whose moments [P, 5] are per
policy, and P normaliser updates from moments[p].

update() runs, per policy in turn, the learner's epochs (Learner.run_epochs: the gather with rows = R, net.sequence,
ppo_loss with adv_moments[p] and the policy's entropy_coef, value_head, backward, Adam with the policy's lr), then reads
every policy's metrics, the ratings and the counts in ONE copy to the host.

Exploit / explore.  madrona_learn's PBT is not in the reference's tree: this contract is the project's own.  With
pbt_interval = N > 0, after every N-th update and on the ratings just read, plan_exploit ranks the policies by rating
(highest first, ties to the lower index); the lowest n = max(1, floor(P * exploit_fraction)) are replaced, each by a source
drawn uniformly from the top n (exploit_fraction <= 0.5, so dst == src never occurs; with P < 2 nothing happens).  Applying
(dst, src): dst takes src's flat parameters, Adam's m, v and state, the normaliser's state and table row, and src's
rating; dst's lr and entropy_coef each become src's times a scale drawn from explore_scales, clamped to the base value
times explore_range (the reference's ParamExplore bounds, 0.1 .. 10).  The carried LSTM states stay.  One
numpy.random.Generator(cfg.seed) draws everything, on the host; nothing beyond the metrics read waits for the device.

The pool of past policies (the reference's --pbt-past-policies Q, which it runs with past_play_portion = 1).  With
num_past_policies = Q > 0 and T = num_policies there are N = T + Q policies on the simulator: the learners 0 .. T-1 and
the pool T .. T+Q-1, frozen snapshots of earlier learners, under league.past_play_schedule(T, Q, past_fill), which the
population sets on the simulator (set_league_schedule) and plays with hs_league_step_scheduled: every learner meets
every pool member on both sides, with Q < T the learners' spare sides go to each other ("cross") or to themselves
("self"), and no world is past against past.  The schedule is regular, so every one of the N policies owns m = R / N
slots and everything above holds with N for P: one routed pack over N tables, T full forwards and Q actor-only ones into
blocks of the one logits buffer, one decode, one routed sampler, compute_advantages(groups=N).  A pool member is a net of
which only the actor and its head run, a normaliser table row and a carried actor LSTM state of m rows; it has no
optimiser, no permutation generator and no update, and at construction it is a copy of learner u % T.  The pool's
columns of the shared rollout are written (what the pack, the sampler and the decode write for all R slots) but never
read by an update.  Ratings: all N move by the league's Elo rule.
Snapshots.  madrona_learn is not in the reference's tree either, so this contract is the project's own.  With
snapshot_interval = S > 0, after every S-th update, on the ratings just read and BEFORE that update's exploit step,
plan_snapshot(elo[:T], taken, Q) gives (dst, src): dst = T + taken % Q, the pool as a ring, and src the highest-rated
learner, ties to the lower index.  Applying it copies src's flat parameters, normaliser state and table row, and rating
to dst, device to device, nothing waits; dst's carried LSTM state stays, as in apply_exploit.  Exploit / explore ranks
and replaces learners only.  With snapshot_interval = 0 the pool stays what it was at construction (or at the last
load_state_dict).  Q > T is refused (league.past_play_schedule says why).

state_dict() is {"members": [...], "league", "hyper", "update_index", "counter"}; a member has Trainer.state_dict()'s
keys (Learner.state_dict()), so evaluate.load_policy(state["members"][i]) reads it; "league" is league.Table.state_dict().  With a pool it has in addition "past", one dict per pool
member ("params", "optimizer" with the source's layout alone, "normaliser", "state", "taken": the update its snapshot was
taken at), which evaluate.load_policy(state, past=i) reads, and "taken", the number of snapshots so far; the league table
is over N.  After load_state_dict() the next collect() steps the simulator before its slot 0, as the Trainer's does.
"""
import copy
import dataclasses
import math

from . import advantages, league, optim, policy, policy_inputs, rollout, trainer
from ._request import on_current_stream
from .episodes import step_trackers
from .policy_inputs import ObsNormaliser


@dataclasses.dataclass
class PopulationConfig(trainer.TrainConfig):
    """TrainConfig's knobs (lr and entropy_coef are the base values every policy starts from) and the population's."""
    num_policies: int = 2
    team_size: int = 3
    k_factor: float = league.DEFAULT_K_FACTOR
    pbt_interval: int = 0                 # exploit / explore after every N-th update; 0: never
    exploit_fraction: float = 0.25
    explore_scales: tuple = (0.8, 1.25)
    explore_range: tuple = (0.1, 10.0)
    num_past_policies: int = 0            # Q: the pool of frozen past policies; 0: none, the learners play each other's current selves
    snapshot_interval: int = 0            # a snapshot into the pool after every N-th update; 0: never
    past_fill: str = "cross"              # with Q < T, the learners' spare sides: "cross" or "self" (league.past_play_schedule)


def check_population_config(cfg, num_worlds, agents):
    """Raise ValueError for a config that does not fit the simulator: the league's shape rules (with a pool, those of
    its schedule: worlds a multiple of T (T + Q)), trainer.check_config with rows = m (a policy's slots), and the exploit /
    explore and snapshot knobs.  Returns the pool's schedule, or None without a pool."""
    for name in ("num_past_policies", "snapshot_interval"):
        v = getattr(cfg, name)
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{name} must be an integer of at least 0, got {v!r}")
    pairs = None
    if cfg.num_past_policies:
        league._league_shape(1, agents, cfg.num_policies, cfg.team_size, 1)          # the policies and the teams, before the table
        pairs = league.past_play_schedule(cfg.num_policies, cfg.num_past_policies, cfg.past_fill)
        league._league_shape(num_worlds, agents, cfg.num_policies + cfg.num_past_policies, cfg.team_size, len(pairs))
    else:
        if cfg.snapshot_interval:
            raise ValueError("snapshot_interval needs a pool: num_past_policies is 0")
        if cfg.past_fill not in league.FILLS:
            raise ValueError(f"past_fill must be one of {league.FILLS}, got {cfg.past_fill!r}")
        league._league_shape(num_worlds, agents, cfg.num_policies, cfg.team_size)
    league._k_factor(cfg.k_factor)
    trainer.check_config(cfg, num_worlds * agents // (cfg.num_policies + cfg.num_past_policies))
    if isinstance(cfg.pbt_interval, bool) or not isinstance(cfg.pbt_interval, int) or cfg.pbt_interval < 0:
        raise ValueError(f"pbt_interval must be an integer of at least 0, got {cfg.pbt_interval!r}")
    _fraction(cfg.exploit_fraction)
    scales = tuple(cfg.explore_scales)
    if not scales or any(not (math.isfinite(float(s)) and float(s) > 0.0) for s in scales):
        raise ValueError(f"explore_scales must be a non-empty tuple of finite factors above 0, got {cfg.explore_scales!r}")
    _range(cfg.explore_range)
    return pairs


def _fraction(fraction):
    f = float(fraction)
    if not 0.0 < f <= 0.5:
        raise ValueError(f"exploit_fraction must be in (0, 0.5], got {fraction!r}")
    return f


def _range(explore_range):
    try:
        lo, hi = (float(x) for x in explore_range)
    except (TypeError, ValueError):
        raise ValueError(f"explore_range must be a pair (low, high), got {explore_range!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= 1.0 <= hi):
        raise ValueError(f"explore_range must be finite with 0 < low <= 1 <= high, got {explore_range!r}")
    return lo, hi


def plan_exploit(elo, fraction, rng):
    """[(dst, src)] for ratings `elo` (a list of P numbers): the module docstring states the rule.  A pure host function;
    `rng` is a numpy.random.Generator and draws one integer per pair."""
    f = _fraction(fraction)
    vals = [float(e) for e in elo]
    P = len(vals)
    if P < 2:
        return []
    order = sorted(range(P), key=lambda i: (-vals[i], i))
    n = max(1, int(math.floor(P * f)))
    return [(dst, order[int(rng.integers(n))]) for dst in order[P - n:]]


def plan_snapshot(elo_train, taken, num_past):
    """(dst, src) of the next snapshot: `elo_train` the learners' ratings (T numbers), `taken` the snapshots so far,
    `num_past` = Q.  dst = T + taken % Q, so the pool fills as a ring; src is the highest-rated learner, ties to the
    lower index.  A pure host function."""
    vals = [float(e) for e in elo_train]
    if not vals or isinstance(taken, bool) or not isinstance(taken, int) or taken < 0 or isinstance(num_past, bool) or not isinstance(num_past, int) or num_past < 1:
        raise ValueError(f"plan_snapshot needs at least one rating, taken >= 0 and num_past >= 1: got {len(vals)} ratings, taken {taken!r}, num_past {num_past!r}")
    return len(vals) + taken % num_past, min(range(len(vals)), key=lambda i: (-vals[i], i))


def explore(value, base, scales, explore_range, rng):
    """`value` times a scale drawn from `scales` by `rng`, clamped to [base * low, base * high]."""
    lo, hi = _range(explore_range)
    scale = float(scales[int(rng.integers(len(scales)))])
    return min(max(float(value) * scale, float(base) * lo), float(base) * hi)


class _Member(trainer.Learner):
    """One policy of a population: a trainer.Learner (policy `index` seeded cfg.seed + index, its own copy of the config,
    whose lr and entropy_coef change under exploration) on the SHARED rollout, of which it owns the column block
    [first, first + rows); its adv_moments and clear are views of the population's, its normaliser's table is `table`."""

    def __init__(self, pop, index, net, table):
        m = pop.block
        self.index, self.first, self.total_rows = index, index * m, pop.rows
        super().__init__(pop.sim, dataclasses.replace(pop.cfg), net, pop.cfg.seed + index, m, pop.device, pop.dtype, pop.rollout,
                         pop.adv_moments[index], pop.clear[index * m:(index + 1) * m], table=table, fused=pop.fused)

    lr = property(lambda self: self.opt.param_groups[0]["lr"])
    entropy_coef = property(lambda self: self.cfg.entropy_coef)

    def set_hyper(self, lr, entropy_coef):
        self.opt.param_groups[0]["lr"] = float(lr)
        self.cfg.entropy_coef = float(entropy_coef)

    def permutation(self):
        """A permutation of the policy's K m sequences, mapped on the device to the ids k R + first + r' of the shared rollout."""
        import torch
        m, R = self.rows, self.total_rows
        perm = torch.randperm(self.rollout.chunks * m, generator=self.generator, device=self.device, dtype=torch.int32)
        if m == R:
            return perm
        return torch.div(perm, m, rounding_mode="floor") * R + (self.first + perm % m)


class _Past:
    """One frozen member of the pool: a copy of a learner's net (its parameters views of one flat buffer laid out as the
    learner's, so a snapshot is one copy) of which only the actor and its head run, a normaliser that is never updated
    (its table is a row of the population's tables), and the carried actor LSTM state of its block of slots."""

    def __init__(self, pop, index, source):
        self.index, self.taken = index, 0
        self.net = copy.deepcopy(source.net)
        self.flat = optim.flatten(self.net.named_parameters(), pop.device)
        self.normaliser = ObsNormaliser(pop.sim.gpu_id, table=pop.tables[index]) if source.normaliser is not None else None
        self.state = self.net.actor.init_state(pop.block, pop.device, pop.dtype)
        self.take(source, 0)

    def take(self, source, update_index):
        """Become `source` (a learner) as it stands: device-to-device copies, nothing waits."""
        import torch
        with torch.no_grad():
            self.flat.params.copy_(source.opt.flat.params)
            if self.normaliser is not None:
                self.normaliser.state.copy_(source.normaliser.state)
                self.normaliser.table.copy_(source.normaliser.table)
        self.taken = int(update_index)

    def state_dict(self):
        return {"params": self.flat.params.clone(), "optimizer": {"layout": {k: (lo, hi, tuple(shape)) for k, (lo, hi, shape) in self.flat.layout().items()}},
                "normaliser": None if self.normaliser is None else self.normaliser.state_dict(), "state": [t.clone() for t in self.state], "taken": self.taken}

    def load_state_dict(self, d):
        import torch
        if tuple(d["params"].shape) != tuple(self.flat.params.shape):
            raise ValueError(f"a pool member's parameters have shape {tuple(d['params'].shape)}: expected {tuple(self.flat.params.shape)}")
        if (d["normaliser"] is None) != (self.normaliser is None):
            raise ValueError("the state and this population differ in normalise_obs")
        with torch.no_grad():
            self.flat.params.copy_(d["params"])
            for mine, theirs in zip(self.state, d["state"]):
                mine.copy_(theirs)
        if self.normaliser is not None:
            self.normaliser.load_state_dict(d["normaliser"])
        self.taken = int(d["taken"])


class Population:
    """cfg.num_policies policies (policy.make_policy, policy p seeded cfg.seed + p, unless `nets` gives them), each with its
    optim.Adam, ObsNormaliser and permutation generator, on one simulator right after sim.init(): equal fixed teams of
    cfg.team_size and a number of worlds that is a multiple of num_policies^2; with cfg.num_past_policies = Q > 0, a pool of
    Q frozen policies as well (`past`), the schedule league.past_play_schedule set on the simulator, and a number of worlds
    that is a multiple of num_policies (num_policies + Q).  The module docstring states the loop.
    `phases` (a trainer.PhaseTimer), `episodes` (an episodes.EpisodeStats) and `behaviour` (a behaviour.BehaviourStats)
    work as on Trainer."""

    def __init__(self, sim, cfg=None, nets=None, fused=True):
        import numpy as np
        import torch
        self.sim, self.cfg, self.fused = sim, PopulationConfig() if cfg is None else cfg, bool(fused)
        cfg = self.cfg
        self.schedule = check_population_config(cfg, sim.num_worlds, sim.agents_per_world)
        self.num_policies = cfg.num_policies             # T: the learners
        self.num_past = Q = cfg.num_past_policies
        self.num_all = P = cfg.num_policies + Q           # N: every policy on the simulator, the learners first
        self.rows = R = sim.num_worlds * sim.agents_per_world
        self.block = m = R // P
        if nets is not None and len(nets) != cfg.num_policies:
            raise ValueError(f"nets must be None or {cfg.num_policies} policies, got {len(nets)}")
        self.dtype = torch.float32 if cfg.dtype is None else cfg.dtype
        self.device = dev = torch.device("cuda", sim.gpu_id)
        T = cfg.steps_per_update
        # with a pool, under its schedule, which it sets; here as slot, row_of_slot, clear_slot, bad, world, _table, counts, elo, bad_total
        self.league_table = league.Table(sim, P, cfg.team_size, cfg.k_factor, self.schedule).bind(self)
        self.tables = torch.zeros(P, policy_inputs.NORM_TABLE, dtype=torch.float32, device=dev)
        self.tables[:, policy_inputs.ROW:] = 1.0
        self.clear = torch.zeros(R, dtype=torch.int32, device=dev)       # clear_slot of a rollout's closing step: clear[0] of the next
        self.adv_moments = torch.zeros(P, advantages.MOMENTS, dtype=torch.float64, device=dev)
        nets = [None] * cfg.num_policies if nets is None else list(nets)
        if nets[0] is None:                               # the rollout needs the hidden width before the members need the rollout
            nets[0] = policy.make_policy(self.dtype, generator=torch.Generator().manual_seed(cfg.seed))
        hidden = nets[0].actor.core.hidden
        self.rollout = rollout.Rollout(sim, T, cfg.num_bptt_chunks, self.dtype, hidden=hidden)
        self.rollout.mask.fill_(1.0)                      # the teams are full
        self.members = [_Member(self, p, nets[p], self.tables[p]) for p in range(cfg.num_policies)]
        self.past = [_Past(self, cfg.num_policies + u, self.members[u % cfg.num_policies]) for u in range(Q)]
        self.taken = 0                                    # the snapshots so far
        if any(mb.net.buckets != self.members[0].net.buckets or mb.net.actor.core.hidden != hidden for mb in self.members):
            raise ValueError("every policy must have the same action heads and hidden width")
        self.buckets = self.members[0].net.buckets
        self.moments = torch.zeros(P, T, rollout.MOMENTS, dtype=torch.float64, device=dev)
        self.logits = torch.zeros(R, sum(self.buckets), dtype=self.dtype, device=dev)
        self.critic_logits = torch.zeros(R, self.members[0].net.bins, dtype=self.dtype, device=dev)
        self.boot_rows = torch.zeros(R, rollout.ROW, dtype=self.dtype, device=dev)
        self.bootstrap = torch.zeros(R, dtype=torch.float32, device=dev)
        self.rng = np.random.Generator(np.random.PCG64(cfg.seed))
        self.update_index, self.counter = 0, 0
        self.stepped = False
        self.phases, self.episodes, self.behaviour = None, None, None
        self.league_step()                                # routes the rows as they stand and latches the team orders; books no game

    # ---- what the policies hold ----
    nets = property(lambda self: [mb.net for mb in self.members])
    lr = property(lambda self: [mb.lr for mb in self.members])
    entropy_coef = property(lambda self: [mb.entropy_coef for mb in self.members])

    _phase = trainer.Learner._phase

    def _export(self, name):
        return getattr(self.sim, name + "_tensor")().to_torch()

    def league_step(self):
        """league.Table.step() on the simulator's exports as they stand: once after every sim.step()."""
        self.league_table.step()

    # ---- the rollout ----
    def _close_slot(self, t):
        """The reward and done exports of the step just taken into slot t, under the routing that slot t acted with."""
        R, buf = self.rows, self.rollout
        self.sim.gather_sequences(self.row_of_slot, [(self._export("reward").view(1, R, 1), buf.reward[t].view(1, R, 1), False),
                                                     (self._export("done").view(1, R, 1), buf.done[t].view(1, R, 1), False)],
                                  chunks=1, chunk_steps=1, rows=R)

    def _zero_carried(self, clear):
        zero, m = clear != 0, self.block
        for p, mb in enumerate(self.members):
            rollout.zero_where(zero[p * m:(p + 1) * m], *(t for s in mb.state for t in s))
        for pm in self.past:
            rollout.zero_where(zero[pm.index * m:(pm.index + 1) * m], *pm.state)

    def _after_step(self, t):
        """What follows every sim.step(): the trackers, the close of slot `t` (None: there is none), the league step."""
        step_trackers(self.episodes, self.behaviour)
        if t is not None:
            self._close_slot(t)
        self.league_step()

    def collect(self):
        """Fill the shared rollout with steps_per_update slots in slot order, the bootstrap values, the advantages and
        returns with their moments per policy, and fold every learner's moments into its normaliser.  The pool's columns
        of the rollout are written (rows, actions, log-probabilities, decoded values of stale critic logits, advantages)
        but never read by an update; its normalisers are not updated."""
        import torch
        sim, buf, cfg, P, m = self.sim, self.rollout, self.cfg, self.num_all, self.block
        T, L = buf.steps, buf.chunk_steps
        tables = self.tables if cfg.normalise_obs else None
        with on_current_stream(), torch.no_grad():
            for t in range(T):
                if t > 0 or not self.stepped:
                    with self._phase("sim"):
                        sim.step()
                    self._after_step(t - 1 if t > 0 else None)
                    buf.clear[t].copy_(self.clear_slot)
                    with self._phase("rollout_forward"):
                        self._zero_carried(self.clear_slot)
                else:                                    # the closing step of the last collect() led here, routed and zeroed
                    buf.clear[0].copy_(self.clear)
                self.stepped = False
                with self._phase("pack"):
                    sim.pack_policy_inputs_routed(self.row_of_slot, P, actor=buf.actor[t], critic=buf.critic[t], moments=self.moments[:, t], tables=tables)
                if t % L == 0:
                    for p, mb in enumerate(self.members):
                        buf.snapshot_state(t // L, mb.state, slice(p * m, (p + 1) * m))
                with self._phase("rollout_forward"):
                    for p, mb in enumerate(self.members):
                        cols = slice(p * m, (p + 1) * m)
                        self.logits[cols], self.critic_logits[cols], mb.state = mb.net(sim, buf.actor[t, cols], buf.critic[t, cols], mb.state, None)
                    for pm in self.past:                  # frozen: the actor and its head alone, as League.act runs them
                        cols = slice(pm.index * m, (pm.index + 1) * m)
                        self.logits[cols], pm.state = pm.net.actor_logits(sim, buf.actor[t, cols], pm.state, None)
                    sim.value_head(self.critic_logits, value=buf.value[t])
                    sim.sample_actions_routed(self.logits, self.row_of_slot, buckets=self.buckets, seed=(cfg.seed, 0), counter=self.counter,
                                              action=buf.action[t], log_prob=buf.log_prob[t])
                self.counter += 1
            with self._phase("sim"):
                sim.step()
            self._after_step(T - 1)
            self.stepped = True
            self.clear.copy_(self.clear_slot)
            with self._phase("rollout_forward"):
                self._zero_carried(self.clear_slot)
            with self._phase("gae"):                     # the bootstrap's critic-only forwards included
                self.bootstrap_value()
                sim.compute_advantages(buf.reward, buf.done, buf.value, self.bootstrap, gamma=cfg.gamma, gae_lambda=cfg.gae_lambda, mask=buf.mask,
                                       advantages=buf.advantage, returns=buf.returns, moments=self.adv_moments, groups=P)
                for p, mb in enumerate(self.members):
                    if mb.normaliser is not None:
                        mb.normaliser.update(sim, self.moments[p])

    def bootstrap_value(self):
        """The critics' values of the observation in the simulator's exports into self.bootstrap (slot order): a critic-only
        routed pack, every learner's critic forward on its carried critic state, which stays as it is, one decode (the
        pool has no critic that runs: its slots decode the logits buffer as it stands)."""
        import torch
        sim, m = self.sim, self.block
        with on_current_stream(), torch.no_grad():
            sim.pack_policy_inputs_routed(self.row_of_slot, self.num_all, critic=self.boot_rows, tables=self.tables if self.cfg.normalise_obs else None)
            for p, mb in enumerate(self.members):
                cols = slice(p * m, (p + 1) * m)
                self.critic_logits[cols], _ = mb.net.critic_logits(sim, self.boot_rows[cols], mb.state[1], None)
            sim.value_head(self.critic_logits, value=self.bootstrap)
        return self.bootstrap

    # ---- the update ----
    def update(self):
        """Every learner's epochs over its part of the rollout, in turn, then the metrics (the one read of the device), then,
        every snapshot_interval-th update, a snapshot into the pool, and then, every pbt_interval-th update, exploit /
        explore among the learners, both on the ratings just read.  With a pool the result has "past": the update each
        pool slot's snapshot was taken at."""
        for mb in self.members:
            mb.phases = self.phases
            mb.run_epochs()
        self.update_index += 1
        out = self.metrics()
        T, n = self.num_policies, self.cfg.snapshot_interval
        if n and self.update_index % n == 0:
            out["snapshot"] = self.snapshot(out["elo"][:T])
        if self.past:
            out["past"] = [pm.taken for pm in self.past]
        n = self.cfg.pbt_interval
        if n and self.update_index % n == 0:
            out["exploit"] = self.exploit(out["elo"][:T])
        return out

    def metrics(self):
        """{"policies": [a Trainer.metrics()-shaped dict per learner, with its "lr" and "entropy_coef"], "elo": [N] (the
        learners first, then the pool), "games", "bad", "update"}: one stacked copy to the host, which waits for the device."""
        import torch
        P, N = self.num_policies, self.num_all
        rows = torch.stack([torch.stack(mb.metric_tensors()) for mb in self.members]).reshape(-1)
        host = torch.cat([rows, self.elo, self.counts.sum().to(torch.float64).reshape(1), self.bad_total.to(torch.float64)]).cpu().tolist()
        per = len(rows) // P
        policies = []
        for p, mb in enumerate(self.members):
            d = mb.metrics_from(host[p * per:(p + 1) * per])
            d["lr"], d["entropy_coef"] = mb.lr, mb.entropy_coef
            policies.append(d)
        return {"policies": policies, "elo": host[P * per:P * per + N], "games": int(host[-2]), "bad": int(host[-1]), "update": self.update_index}

    update_iter = trainer.Trainer.update_iter             # collect() then update(): the metrics, with "fps"; the same text serves both

    # ---- the pool ----
    def snapshot(self, elo_train):
        """plan_snapshot on the learners' ratings `elo_train` (host numbers), applied.  Returns (dst, src)."""
        if not self.past:
            raise ValueError("this population has no pool: num_past_policies is 0")
        dst, src = plan_snapshot(elo_train, self.taken, self.num_past)
        self.past[dst - self.num_policies].take(self.members[src], self.update_index)
        self.elo[dst] = self.elo[src]
        self.taken += 1
        return dst, src

    # ---- exploit / explore ----
    def exploit(self, elo):
        """plan_exploit on the learners' ratings `elo` (host numbers), applied pair by pair.  Returns the pairs."""
        cfg = self.cfg
        pairs = plan_exploit(elo, cfg.exploit_fraction, self.rng)
        for dst, src in pairs:
            self.apply_exploit(dst, src)
        return pairs

    def apply_exploit(self, dst, src):
        """Policy `dst` takes policy `src`'s parameters, optimiser state (its loss scale included), normaliser and rating, and explored lr and
        entropy_coef.  Device-to-device copies: nothing waits."""
        import torch
        cfg, a, b = self.cfg, self.members[dst], self.members[src]
        if dst == src:
            raise ValueError("dst and src must differ")
        with torch.no_grad():
            a.opt.flat.params.copy_(b.opt.flat.params)
            a.opt.m.copy_(b.opt.m)
            a.opt.v.copy_(b.opt.v)
            a.opt.adam_state.copy_(b.opt.adam_state)
            if a.opt.loss_scale is not None:
                a.opt.loss_scale.state.copy_(b.opt.loss_scale.state)
            if a.normaliser is not None:
                a.normaliser.state.copy_(b.normaliser.state)
                a.normaliser.table.copy_(b.normaliser.table)
            self.elo[dst] = self.elo[src]
        a.set_hyper(explore(b.lr, cfg.lr, cfg.explore_scales, cfg.explore_range, self.rng),
                    explore(b.entropy_coef, cfg.entropy_coef, cfg.explore_scales, cfg.explore_range, self.rng))

    # ---- checkpoints ----
    def state_dict(self):
        """{"members": [Trainer.state_dict()'s keys per policy], "league": the world state, counts, ratings and malformed
        worlds, "hyper": {"lr", "entropy_coef"} per policy and the exploration generator, "update_index", "counter"}; with
        a pool also "past" (a dict per pool member) and "taken"."""
        for mb in self.members:
            mb.update_index, mb.counter = self.update_index, self.counter
        d = {"members": [mb.state_dict() for mb in self.members],
             "league": self.league_table.state_dict(),
             "hyper": {"lr": self.lr, "entropy_coef": self.entropy_coef, "rng": self.rng.bit_generator.state},
             "update_index": self.update_index, "counter": self.counter}
        if self.past:
            d["past"], d["taken"] = [pm.state_dict() for pm in self.past], self.taken
        return d

    def load_state_dict(self, d):
        """Load what state_dict() returned into a population of the same policies, config and simulator shape."""
        if len(d["members"]) != self.num_policies:
            raise ValueError(f"the state has {len(d['members'])} members: expected {self.num_policies}")
        if len(d.get("past", ())) != self.num_past:
            raise ValueError(f"the state has a pool of {len(d.get('past', ()))} past policies: expected {self.num_past}")
        if tuple(d["league"]["table"].shape) != tuple(self._table.shape):
            raise ValueError("the state's league table does not fit this population")
        for mb, md in zip(self.members, d["members"]):
            mb.load_state_dict(md)
        for mb, lr, ec in zip(self.members, d["hyper"]["lr"], d["hyper"]["entropy_coef"]):
            mb.set_hyper(lr, ec)
        for pm, pd in zip(self.past, d.get("past", ())):
            pm.load_state_dict(pd)
        self.taken = int(d.get("taken", 0))
        self.league_table.load_state_dict(d["league"])
        self.rng.bit_generator.state = d["hyper"]["rng"]
        self.update_index, self.counter = int(d["update_index"]), int(d["counter"])
        self.stepped = False
