"""The update loop: the learner's pieces called in sequence, as the reference's user gets it from scripts/jax_train.py
(`Update: N / FPS: ...`).  That loop lives in madrona_learn, which is not part of the reference's tree: the knobs and their
defaults are jax_train.py's, the order of the calls below is the project's.

    sim.init()
    tr = trainer.Trainer(sim, trainer.TrainConfig(dtype=torch.bfloat16))
    for _ in range(updates):
        metrics = tr.update_iter()          # collect() then update(); one read of the device at its end

Composition only: every kernel is another module's (policy_inputs, policy, action_sampling, value_head, advantages,
rollout, ppo_loss, optim).  Learner is what an update needs (a population.Population's members are Learners); Trainer, a
Learner that fills its own rollout, is the single-device loop; ShardedTrainer (at the end of this module) is the same loop
over the shards of a ShardedSimulator, one Trainer per shard, their gradients reduced by optim.reduce_gradients.

collect() fills the rollout (rollout.py states what slot t holds).  Per slot: sim.step() -> the done and self_mask exports
into clear[t] and mask[t] -> the carried LSTM states zeroed in the rows whose episode starts with this observation or which
are out (rollout.state_zero_into: the step resets before it observes, so the observation that comes with done is the next
episode's first; a row that joins comes with done = 0) -> pack_policy_inputs into the slot (normalised, the raw moments
into moments[t]) -> at a chunk's first slot a snapshot of the carried states, as the forward receives them -> the policy's
forward under no_grad, with no clear -> value_head's decode into value[t] -> sample_actions (seed = cfg.seed, a counter
that grows by one per slot over the whole run) into the simulator's action tensor, action[t] and log_prob[t]; the next
step's reward and done exports go into the slot it closes.
The bootstrap.  After slot T - 1 the simulator is stepped once more, which closes slot T - 1 and leaves the observation
o_T in the exports; the carried states are zeroed by the same rule.  Its value comes from a CRITIC-ONLY forward (the
critic's rows packed without moments, the policy's critic_logits on the carried critic state) whose new state is
dropped: the carried state is not advanced, the actor is not run.  The next collect() does not step before its slot 0: it packs the same exports with the normaliser as
updated since, and runs the full forward with the policy as updated since, so log_prob[0] and value[0] belong to the
policy that update() starts from, and every observation adds its moments once.  Then compute_advantages (moments=True)
over the buffers, then ObsNormaliser.update with the T moments.  With trainer.episodes set to an episodes.EpisodeStats
(None by default), collect() calls its step() after every sim.step() it makes, the closing one included, so every step
reaches the tracker once across rollouts; metrics() and state_dict() do not know about it.  trainer.behaviour, a
behaviour.BehaviourStats, works the same way.

update() runs num_epochs epochs: a fresh torch.randperm(K n) on the device from a seeded generator, cut into
num_minibatches equal parts; per part Rollout.minibatch (one launch), sequence_logits (net.sequence from the gathered
chunk-start states under rollout.chunk_clears of the gathered clears and masks), ppo_loss (adv_moments, mask) and
value_head (returns, mask, loss_coef = value_loss_coef) on the L m flattened samples, torch.autograd.backward with their two gradients (both are gradients of means over the same count
of active samples, so they add into the gradient of policy_loss - entropy_coef * entropy + value_loss_coef * value_loss),
and opt.step().  Every call is enqueued on torch's current stream (_request.on_current_stream); the statistics add up in
device tensors and are read once, at the end.

fused=False runs the policy's eager pieces (set_fused(False)) and takes the minibatch by torch indexing
(Rollout.minibatch_eager); the loss, GAE, sampling, pack and Adam kernels stay.

state_dict() holds the flat parameters, Adam's m, v and state, the normaliser, the carried LSTM state and clear, the
update index, the sampling counter and the permutation generator; not the simulator (save_checkpoints is for that).  After
load_state_dict() the next collect() steps the simulator before its slot 0, takes clear[0] from that step and zeroes the
loaded states by it (the rows that were out when the state was saved carry zero already).
"""
import dataclasses
import time

from . import advantages, optim, policy, ppo_loss, rollout, value_head
from ._request import on_current_stream
from .episodes import step_trackers
from .policy_inputs import ObsNormaliser


@dataclasses.dataclass
class TrainConfig:
    """The reference's knobs with scripts/jax_train.py's defaults.  dtype None is float32."""
    steps_per_update: int = 40
    num_bptt_chunks: int = 8
    num_minibatches: int = 2
    num_epochs: int = 4
    lr: float = 1e-4
    gamma: float = 0.998
    gae_lambda: float = 0.95
    clip_coef: float = 0.2
    value_loss_coef: float = 1.0
    entropy_coef: float = 0.01
    max_grad_norm: float = 5.0
    dtype: object = None
    seed: int = 5
    normalise_obs: bool = True
    loss_scale: object = None             # None, "dynamic" (optim.LossScale's defaults) or a dict of LossScale's keywords


def loss_scale_settings(setting):
    """None for TrainConfig.loss_scale None, else optim.LossScale's checked keywords.  Raises ValueError."""
    if setting is None:
        return None
    if isinstance(setting, str) and setting == "dynamic":
        return optim.loss_scale_settings()
    if isinstance(setting, dict):
        return optim.loss_scale_settings(**setting)
    raise ValueError(f"loss_scale must be None, \"dynamic\" or a dict of optim.LossScale's keywords, got {setting!r}")


def check_config(cfg, rows):
    """Raise ValueError for a config that does not fit `rows` agent rows: T % K, K n % num_minibatches, counts below 1;
    or for a loss_scale that optim.LossScale would refuse."""
    loss_scale_settings(cfg.loss_scale)
    for k in ("steps_per_update", "num_bptt_chunks", "num_minibatches", "num_epochs"):
        v = getattr(cfg, k)
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{k} must be a positive integer, got {v!r}")
    if cfg.steps_per_update % cfg.num_bptt_chunks:
        raise ValueError(f"steps_per_update ({cfg.steps_per_update}) must be a multiple of num_bptt_chunks ({cfg.num_bptt_chunks})")
    if (cfg.num_bptt_chunks * rows) % cfg.num_minibatches:
        raise ValueError(f"the {cfg.num_bptt_chunks * rows} sequences (num_bptt_chunks * rows) do not divide into {cfg.num_minibatches} minibatches")


PPO_STATS, VALUE_STATS, ADAM_STATS = ppo_loss.STATS, value_head.STATS, optim.STATS
PHASES = ("sim", "pack", "rollout_forward", "gae", "gather", "update_forward_backward", "adam")


class _Span:
    def __init__(self, events):
        self.events = events

    def __enter__(self):
        import torch
        self.a = torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        import torch
        b = torch.cuda.Event(enable_timing=True)
        b.record()
        self.events.append((self.a, b))
        return False


class _NoSpan:
    def __enter__(self):
        pass

    def __exit__(self, *exc):
        return False


class PhaseTimer:
    """Device events around the phases of collect() and update() (`names`, by default PHASES), for tools/train.py
    --phases: set trainer.phases = PhaseTimer(); totals() waits for the device and returns {phase: ms} since the last
    totals()."""

    def __init__(self, names=PHASES):
        self.names = tuple(names)
        self.events = {k: [] for k in self.names}

    def __call__(self, name):
        return _Span(self.events[name])

    def totals(self):
        import torch
        torch.cuda.synchronize()
        out = {k: sum(a.elapsed_time(b) for a, b in ev) for k, ev in self.events.items()}
        self.events = {k: [] for k in self.names}
        return out


def make_loss_scale(cfg, device):
    """The optim.LossScale of cfg.loss_scale on `device`, or None."""
    s = loss_scale_settings(cfg.loss_scale)
    return None if s is None else optim.LossScale(device, **s)


class Learner:
    """What an update needs, and what a Trainer and a member of a population.Population share: the policy (`net`, or with
    None policy.make_policy seeded with `seed`), optim.Adam, an ObsNormaliser (on `table`, a row of the caller's tables, if given),
    the carried LSTM state of `rows` agent rows, the permutation generator (seeded with `seed`), the statistics and the
    two counters.  `buf` (the Rollout it reads), `adv_moments` and `clear` are the caller's, kept as given: of a
    population they are shared, or views into shared tensors."""

    def __init__(self, sim, cfg, net, seed, rows, device, dtype, buf, adv_moments, clear, table=None, fused=True):
        import torch
        self.sim, self.cfg, self.fused = sim, cfg, bool(fused)
        self.rows, self.device, self.dtype = rows, device, dtype
        if net is None:
            net = policy.make_policy(dtype, generator=torch.Generator().manual_seed(seed))
        self.net = net.to(device).set_fused(self.fused)
        self.opt = optim.Adam(sim, self.net.named_parameters(), lr=cfg.lr, max_grad_norm=cfg.max_grad_norm, loss_scale=make_loss_scale(cfg, device))
        self.normaliser = ObsNormaliser(sim.gpu_id, table=table) if cfg.normalise_obs else None
        self.rollout, self.adv_moments, self.clear = buf, adv_moments, clear
        self.state = self.net.init_state(rows, device, dtype)
        self.generator = torch.Generator(device=device).manual_seed(seed)
        self.update_index, self.counter = 0, 0
        self._mb = None
        self.phases = None                # a PhaseTimer, or None: no events
        self.ppo_stats = torch.zeros(cfg.num_epochs, PPO_STATS, dtype=torch.float64, device=device)
        self.value_stats = torch.zeros(cfg.num_epochs, VALUE_STATS, dtype=torch.float64, device=device)
        self.adam_stats = torch.zeros(3, dtype=torch.float64, device=device)      # sum of norms, skipped steps, t
        self._ppo_out = torch.zeros(PPO_STATS, dtype=torch.float64, device=device)
        self._value_out = torch.zeros(VALUE_STATS, dtype=torch.float64, device=device)

    def _phase(self, name):
        return _NoSpan() if self.phases is None else self.phases(name)

    # ---- the update ----
    def minibatch(self, index):
        """The sequences `index` of the rollout: one launch into tensors that are kept (fused), or torch indexing."""
        if not self.fused:
            return self.rollout.minibatch_eager(index)
        if self._mb is not None and self._mb["clear"].shape[1] != index.shape[0]:
            self._mb = None
        self._mb = self.rollout.minibatch(index, out=self._mb)
        return self._mb

    def sequence_logits(self, mb):
        """The policy over the sequences of a minibatch (what minibatch() or Rollout.minibatch_eager() returned), as the
        update recomputes them: from the gathered chunk-start states, every step's state zeroed where the next slot's
        episode starts (rollout.chunk_clears), so that no memory and no gradient crosses an episode's end.  Returns
        (logits [L, m, sum(buckets)], critic_logits [L, m, bins]), part of the autograd graph."""
        state0 = ((mb["actor_h"], mb["actor_c"]), (mb["critic_h"], mb["critic_c"]))
        logits, critic_logits, _ = self.net.sequence(self.sim, mb["actor"], mb["critic"], state0, rollout.chunk_clears(mb["clear"], mb["mask"]))
        return logits, critic_logits

    def forward_backward(self, index, epoch=0):
        """One minibatch up to the optimiser's step: the gather, the forward, the two loss kernels and the backward, which
        adds into the flat gradient buffer.  The statistics of the two losses are added to row `epoch` of ppo_stats /
        value_stats.  Returns the results of the ppo_loss and the value_head call."""
        import torch
        sim, net, cfg = self.sim, self.net, self.cfg
        with on_current_stream(), self._phase("gather"):
            mb = self.minibatch(index)
        with on_current_stream(), self._phase("update_forward_backward"):
            S = mb["clear"].numel()
            logits, critic_logits = self.sequence_logits(mb)
            logits, critic_logits = logits.reshape(S, -1), critic_logits.reshape(S, -1)
            mask = mb["mask"].reshape(S)
            scale = None if self.opt.loss_scale is None else self.opt.loss_scale.state     # the gradients carry the scale that opt.step() divides out
            pol = sim.ppo_loss(logits.detach(), mb["action"].reshape(S, -1), mb["log_prob"].reshape(S), mb["advantage"].reshape(S), buckets=net.buckets,
                               adv_moments=self.adv_moments, mask=mask, clip_coef=cfg.clip_coef, entropy_coef=cfg.entropy_coef, stats=self._ppo_out,
                               loss_scale=scale)
            val = sim.value_head(critic_logits.detach(), mb["returns"].reshape(S), bins=net.bins, mask=mask, value=None, loss_coef=cfg.value_loss_coef,
                                 stats=self._value_out, loss_scale=scale)
            torch.autograd.backward([logits, critic_logits], [pol["grad_logits"], val["grad_logits"]])
            self.ppo_stats[epoch] += self._ppo_out
            self.value_stats[epoch] += self._value_out
        return pol, val

    def permutation(self):
        """The sequence ids of one epoch in a fresh order, int32 on the device, from the seeded generator."""
        import torch
        return torch.randperm(self.rollout.sequences, generator=self.generator, device=self.device, dtype=torch.int32)

    def run_epochs(self):
        """num_epochs epochs of num_minibatches minibatches over the rollout: an update without the read of the metrics
        (gpu_hideseek.population runs several policies' epochs before its one read)."""
        cfg = self.cfg
        self.ppo_stats.zero_()
        self.value_stats.zero_()
        self.adam_stats.zero_()
        with on_current_stream():
            for epoch in range(cfg.num_epochs):
                perm = self.permutation()
                for part in rollout.epoch_parts(perm, cfg.num_minibatches):
                    self.forward_backward(part, epoch)
                    with self._phase("adam"):
                        stats = self.opt.step()
                    self.adam_stats[:2] += stats[::2]            # the norm and whether the step was skipped
                    self.adam_stats[2] = stats[3]
        self.update_index += 1

    METRIC_NAMES = ("policy_loss", "entropy", "approx_kl", "clip_fraction", "value_loss", "explained_variance", "mean_value", "advantage_mean",
                    "advantage_std", "returns_mean", "returns_std", "grad_norm", "skipped", "adam_step")

    def metric_tensors(self):
        """The statistics of the last update as float64 scalars on the device, without synchronising: METRIC_NAMES, then
        the value loss of every epoch, then with a loss scale its value after the update."""
        import torch
        cfg = self.cfg
        steps = cfg.num_epochs * cfg.num_minibatches
        adv = advantages.moments_to_mean_std(self.adv_moments)
        pol = ppo_loss.stats_to_metrics(self.ppo_stats.sum(0), cfg.entropy_coef, cfg.value_loss_coef)
        val = value_head.stats_to_metrics(self.value_stats.sum(0))
        per_epoch = [value_head.stats_to_metrics(self.value_stats[e])["value_loss"] for e in range(cfg.num_epochs)]
        vals = [pol["policy_loss"], pol["entropy"], pol["approx_kl"], pol["clip_fraction"], val["value_loss"], val["explained_variance"], val["mean_value"],
                adv["advantages"][0], adv["advantages"][1], adv["returns"][0], adv["returns"][1], self.adam_stats[0] / steps, self.adam_stats[1], self.adam_stats[2]]
        scale = [] if self.opt.loss_scale is None else [self.opt.loss_scale.state[0]]
        return [v.to(torch.float64) for v in vals + per_epoch + scale]

    def metrics_from(self, host):
        """The metrics dict from the values of metric_tensors() as Python numbers."""
        cfg, names = self.cfg, self.METRIC_NAMES
        out = dict(zip(names, host))
        out["skipped"], out["adam_step"] = int(out["skipped"]), int(out["adam_step"])
        out["value_loss_epochs"] = host[len(names):len(names) + cfg.num_epochs]
        if self.opt.loss_scale is not None:
            out["loss_scale"] = host[len(names) + cfg.num_epochs]
        out["loss"] = out["policy_loss"] - cfg.entropy_coef * out["entropy"] + cfg.value_loss_coef * out["value_loss"]
        out["update"] = self.update_index
        return out

    def metrics(self):
        """The statistics of the last update as Python numbers: one copy to the host, which waits for the device."""
        import torch
        return self.metrics_from(torch.stack(self.metric_tensors()).cpu().tolist())

    # ---- checkpoints ----
    def state_dict(self):
        """Clones of the flat parameter buffer, the optimiser's and the normaliser's state, the carried LSTM state and
        clear, the permutation generator, and the two counters."""
        return {"params": self.opt.flat.params.clone(), "optimizer": self.opt.state_dict(),
                "normaliser": None if self.normaliser is None else self.normaliser.state_dict(),
                "state": [[t.clone() for t in s] for s in self.state], "clear": self.clear.clone(), "generator": self.generator.get_state().clone(),
                "update_index": self.update_index, "counter": self.counter}

    def load_state_dict(self, d):
        """Load what state_dict() returned into a learner of the same policy, config and row count."""
        import torch
        if tuple(d["params"].shape) != tuple(self.opt.flat.params.shape):
            raise ValueError(f"the state's parameters have shape {tuple(d['params'].shape)}: expected {tuple(self.opt.flat.params.shape)}")
        if (d["normaliser"] is None) != (self.normaliser is None):
            raise ValueError("the state and this trainer differ in normalise_obs")
        for mine, theirs in zip([t for s in self.state for t in s] + [self.clear], [t for s in d["state"] for t in s] + [d["clear"]]):
            if tuple(mine.shape) != tuple(theirs.shape) or mine.dtype != theirs.dtype:
                raise ValueError(f"a carried tensor has shape {tuple(theirs.shape)} and dtype {theirs.dtype}: expected {tuple(mine.shape)}, {mine.dtype}")
        self.opt.load_state_dict(d["optimizer"])
        with torch.no_grad():
            self.opt.flat.params.copy_(d["params"])
            for mine, theirs in zip([t for s in self.state for t in s] + [self.clear], [t for s in d["state"] for t in s] + [d["clear"]]):
                mine.copy_(theirs)
        if self.normaliser is not None:
            self.normaliser.load_state_dict(d["normaliser"])
        self.generator.set_state(d["generator"].cpu())      # a state loaded with map_location is on the device
        self.update_index, self.counter = int(d["update_index"]), int(d["counter"])


class Trainer(Learner):
    """A Learner (the policy seeded with cfg.seed, unless `net` is given) with the Rollout it fills, the bootstrap value
    and the sampling of one simulator (after sim.init()): collect(), update() and update_iter()."""

    def __init__(self, sim, cfg=None, net=None, fused=True):
        import torch
        cfg = TrainConfig() if cfg is None else cfg
        n = sim.num_worlds * sim.agents_per_world
        check_config(cfg, n)
        dtype = torch.float32 if cfg.dtype is None else cfg.dtype
        dev = torch.device("cuda", sim.gpu_id)
        if net is None:                   # the rollout needs the hidden width
            net = policy.make_policy(dtype, generator=torch.Generator().manual_seed(cfg.seed))
        buf = rollout.Rollout(sim, cfg.steps_per_update, cfg.num_bptt_chunks, dtype, hidden=net.actor.core.hidden)
        super().__init__(sim, cfg, net, cfg.seed, n, dev, dtype, buf, torch.zeros(advantages.MOMENTS, dtype=torch.float64, device=dev),
                         torch.zeros(n, dtype=torch.int32, device=dev), fused=fused)
        self.bootstrap = torch.zeros(n, dtype=torch.float32, device=dev)
        self.boot_rows = torch.zeros(n, rollout.ROW, dtype=dtype, device=dev)
        self.stepped = False              # the simulator has been stepped past the last slot: its exports are the next o_0
        self.episodes = None              # an episodes.EpisodeStats, or None: collect() calls its step() after every sim.step()
        self.behaviour = None             # a behaviour.BehaviourStats, or None: likewise

    # ---- the rollout ----
    def _export(self, name):
        return getattr(self.sim, name + "_tensor")().to_torch().reshape(self.rows, -1)

    def _close_slot(self, t):
        """The reward and done exports of the step just taken belong to slot t, whose action it consumed."""
        self.rollout.reward[t].copy_(self._export("reward")[:, 0])
        self.rollout.done[t].copy_(self._export("done")[:, 0])

    def _zero_carried(self, clear, mask, mask_before):
        """After a sim.step(): zero the carried LSTM state in the rows that rollout.state_zero_into() names, given the done
        and self_mask exports of that step and the self_mask of the slot before."""
        rollout.zero_where(rollout.state_zero_into(clear, mask, mask_before), *self.state[0], *self.state[1])

    # collect() in the pieces a slot is made of (ShardedTrainer runs them slot by slot over its members).  All of them are
    # called under on_current_stream() and torch.no_grad().
    def _after_step(self, t):
        """After the sim.step() that leads to slot t: close slot t - 1, take clear[t] and mask[t], zero the carried states."""
        buf = self.rollout
        if t > 0:
            self._close_slot(t - 1)
        buf.clear[t].copy_(self._export("done")[:, 0])
        buf.mask[t].copy_(self._export("self_mask")[:, 0])
        with self._phase("rollout_forward"):
            self._zero_carried(buf.clear[t], buf.mask[t], buf.mask[t - 1] if t > 0 else buf.mask[t])

    def _resume_slot(self):
        """Slot 0 without a step: the closing step of the last collect() led here, and zeroed."""
        buf = self.rollout
        buf.clear[0].copy_(self.clear)
        buf.mask[0].copy_(self._export("self_mask")[:, 0])

    def _slot(self, t):
        """Slot t from the exports: pack, at a chunk's first slot the snapshot of the carried states, forward, value, actions."""
        sim, buf, net, cfg = self.sim, self.rollout, self.net, self.cfg
        L = buf.chunk_steps
        self.stepped = False
        with self._phase("pack"):
            sim.pack_policy_inputs(actor=buf.actor[t], critic=buf.critic[t], moments=buf.moments[t], normaliser=self.normaliser)
        if t % L == 0:
            buf.snapshot_state(t // L, self.state)
        with self._phase("rollout_forward"):
            logits, critic_logits, self.state = net(sim, buf.actor[t], buf.critic[t], self.state, None)
            sim.value_head(critic_logits, value=buf.value[t])
            out = sim.sample_actions(logits, buckets=net.buckets, seed=(cfg.seed, 0), counter=self.counter, log_prob=buf.log_prob[t])
            buf.action[t].copy_(out["action"].reshape(self.rows, -1))
        self.counter += 1

    def _after_closing_step(self):
        """After the sim.step() past the last slot: close slot T - 1, keep its done as the next clear[0], zero the carried states."""
        buf = self.rollout
        T = buf.steps
        self.stepped = True
        self._close_slot(T - 1)
        self.clear.copy_(buf.done[T - 1])
        with self._phase("rollout_forward"):
            self._zero_carried(self.clear, self._export("self_mask")[:, 0], buf.mask[T - 1])

    def _gae(self):
        """The bootstrap value, then advantages, returns and their moments over the rollout."""
        buf, cfg = self.rollout, self.cfg
        self.bootstrap_value()
        self.sim.compute_advantages(buf.reward, buf.done, buf.value, self.bootstrap, gamma=cfg.gamma, gae_lambda=cfg.gae_lambda, mask=buf.mask,
                                    advantages=buf.advantage, returns=buf.returns, moments=self.adv_moments)

    def _fold_moments(self, moments):
        """One batch of slot moments [K, 593] into the normaliser."""
        if self.normaliser is not None:
            self.normaliser.update(self.sim, moments)

    def collect(self):
        """Fill the rollout with steps_per_update slots, the bootstrap value, the advantages and returns, and fold the
        slots' moments into the normaliser."""
        import torch
        sim, buf = self.sim, self.rollout
        with on_current_stream(), torch.no_grad():
            for t in range(buf.steps):
                if t > 0 or not self.stepped:
                    with self._phase("sim"):
                        sim.step()
                    step_trackers(self.episodes, self.behaviour)
                    self._after_step(t)
                else:
                    self._resume_slot()
                self._slot(t)
            with self._phase("sim"):
                sim.step()
            step_trackers(self.episodes, self.behaviour)
            self._after_closing_step()
            with self._phase("gae"):                     # the bootstrap's critic-only forward included
                self._gae()
                self._fold_moments(buf.moments)

    def bootstrap_value(self):
        """The critic's value of the observation in the simulator's exports into self.bootstrap, by a critic-only forward
        on the carried critic state, which stays as it is."""
        import torch
        with on_current_stream(), torch.no_grad():
            self.sim.pack_policy_inputs(critic=self.boot_rows, normaliser=self.normaliser)
            critic_logits, _ = self.net.critic_logits(self.sim, self.boot_rows, self.state[1], None)
            self.sim.value_head(critic_logits, value=self.bootstrap)
        return self.bootstrap

    # ---- the update ----
    def update(self):
        """run_epochs() over the rollout collect() filled, then the metrics (the one read of the device)."""
        self.run_epochs()
        return self.metrics()

    def update_iter(self):
        """collect() then update(): the metrics, with "fps" = rows * steps_per_update / the wall time of both."""
        import torch
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        self.collect()
        out = self.update()                      # ends with the read of the metrics: the device is idle
        out["fps"] = self.rows * self.cfg.steps_per_update / (time.perf_counter() - t0)
        return out

    def load_state_dict(self, d):
        """Learner.load_state_dict(); the next collect() then steps the simulator before its slot 0."""
        super().load_state_dict(d)
        self.stepped = False


# ---- the same loop over the shards of a ShardedSimulator ----
SHARDED_PHASES = PHASES + ("reduce",)     # the staging copies between the devices and the reduction, per minibatch


class ShardedTrainer:
    """Data-parallel training over a ShardedSimulator (after ssim.init()): one Trainer ("member") per shard, on the shard's
    device, in this process and on one host thread, as ShardedSimulator itself.  Every member is built from the same seed
    (or from a deep copy of `net`), so the flat parameter buffers start bit-equal, and they stay so: every member learns on
    its own shard's rollout but steps with the same gradient, the mean over ALL shards' active samples, which every member
    computes for itself from copies of the same buffers in a fixed order (optim.reduce_gradients, hs_reduce_gradients).
    Nothing is broadcast and there is no collective library.

    collect() goes slot by slot over all shards: ssim.step() (every shard starts before any is waited for), the trackers,
    then each member's own work for the slot (Trainer's per-slot methods) on its device.  After every member's GAE the
    members' adv_moments, raw sums, are copied to every device and added in shard order, so hs_ppo_loss normalises the
    advantages with the mean and std over all shards; every member's normaliser is updated with the [G T, 593] stack of
    all shards' slot moments, shard-major, one batch.
    run_epochs(): per epoch every member draws its own permutation (member g's generator is seeded cfg.seed + g); per
    minibatch part every member runs forward_backward on its own part; then every copy is enqueued before any reduction
    (for every device d and shard g != d, member g's gradient buffer into row g of d's staging buffer [G, n] and its
    count of active samples, _ppo_out[ppo_loss.STAT_COUNT], into d's count vector; torch orders a copy between devices on both devices'
    current streams, and no host wait is added); then every member reduces in place into its own gradient buffer, its own
    row read where it lies; then every member's own opt.step().  Both losses divide by a shard's count c_g, so
    sum (c_g / C) grad_g is the gradient of the mean over all C active samples.  The loss scale is the same S on every
    replica, because every replica sees the same norm.
    metrics(): the shards' ppo_stats and value_stats (raw sums) added on shard 0's device, the Adam statistics shard 0's,
    one read; Trainer's keys plus "shards" and "count" (C of the last minibatch).  `episodes` and `behaviour` take a
    tracker with a step() method, or a list of them (one episodes.EpisodeStats per shard, say): collect() calls step()
    after every ssim.step().  `phases`: a PhaseTimer(SHARDED_PHASES) when every shard is on one device.
    The shards may hold different numbers of worlds; a config that does not fit one of them raises, naming the shard.
    Not here: Population and League over shards, one process per GPU, RCCL, overlapping the reduction with the backward
    pass, a reduce-scatter form for many shards."""

    def __init__(self, ssim, cfg=None, net=None, fused=True):
        import copy
        import torch
        self.ssim, self.cfg, self.fused = ssim, TrainConfig() if cfg is None else cfg, bool(fused)
        cfg = self.cfg
        if not 1 <= len(ssim.shards) <= optim.REDUCE_MAX_SHARDS:
            raise ValueError(f"{len(ssim.shards)} shards: 1 to {optim.REDUCE_MAX_SHARDS} expected")
        self.ranges = [tuple(r) for r in ssim.ranges]
        self.members = []
        for g, s in enumerate(ssim.shards):
            try:
                m = Trainer(s, cfg, net=None if net is None else copy.deepcopy(net), fused=fused)
            except ValueError as e:
                raise ValueError(f"shard {g} ({s.num_worlds} worlds on GPU {s.gpu_id}): {e}") from None
            m.generator.manual_seed(cfg.seed + g)
            self.members.append(m)
        G, first = len(self.members), self.members[0]
        self.shards, self.device, self.dtype = G, first.device, first.dtype
        self.rows = sum(m.rows for m in self.members)
        n = first.opt.flat.params.numel()
        for g, m in enumerate(self.members):
            if m.opt.layout() != first.opt.layout() or not torch.equal(m.opt.flat.params.to(self.device), first.opt.flat.params):
                raise ValueError(f"shard {g}'s parameters differ from shard 0's")
        # per device: the other shards' gradients (row d itself is not used: the member's own buffer is read where it lies),
        # the counts, and C
        self.stage = [torch.zeros(G, n, dtype=torch.float32, device=m.device) for m in self.members]
        self.counts = [torch.zeros(G, dtype=torch.float64, device=m.device) for m in self.members]
        self.totals = [torch.zeros(1, dtype=torch.float64, device=m.device) for m in self.members]
        self.stepped = False
        self.episodes, self.behaviour = None, None
        self._phases = None

    # ---- what the members share ----
    @property
    def update_index(self):
        return self.members[0].update_index

    @property
    def phases(self):
        return self._phases

    @phases.setter
    def phases(self, timer):
        if timer is not None and len({m.device for m in self.members}) != 1:
            raise ValueError("phases: the events of one PhaseTimer are for one device, and the shards are on several")
        self._phases = timer
        for m in self.members:
            m.phases = timer

    _phase = Learner._phase

    def _each(self):
        """(g, member) with the member's device as torch's current one."""
        import torch
        for g, m in enumerate(self.members):
            with torch.cuda.device(m.device):
                yield g, m

    def _step(self):
        with self._phase("sim"):
            self.ssim.step()
        step_trackers(self.episodes, self.behaviour)

    # ---- the rollout ----
    def collect(self):
        """Fill every member's rollout, slot by slot over all shards; then the global advantage moments and the
        normalisers' update with all shards' slot moments."""
        import torch
        T = self.members[0].rollout.steps
        with on_current_stream(), torch.no_grad():
            for t in range(T):
                if t > 0 or not self.stepped:
                    self._step()
                    for _, m in self._each():
                        m._after_step(t)
                else:
                    for _, m in self._each():
                        m._resume_slot()
                for _, m in self._each():
                    m._slot(t)
            self._step()
            self.stepped = True
            for _, m in self._each():
                m._after_closing_step()
            with self._phase("gae"):
                for _, m in self._each():
                    m._gae()
                self._share_moments()

    def _share_moments(self):
        """Every member's adv_moments becomes the sum of all shards', added in shard order; every member's normaliser is
        updated with all shards' slot moments, shard-major."""
        import torch
        own = [m.adv_moments.clone() for m in self.members]
        slots = [m.rollout.moments for m in self.members]
        for _, m in self._each():
            m.adv_moments.copy_(own[0])                              # between devices where they differ
            for x in own[1:]:
                m.adv_moments.add_(x.to(m.device))
            m._fold_moments(torch.cat([x.to(m.device) for x in slots]))

    # ---- the update ----
    def exchange_gradients(self):
        """Enqueue every copy between the devices: for device d and shard g != d, member g's gradients into row g of d's
        staging buffer; every shard's count of active samples (its last ppo_loss call's) into d's count vector."""
        for d, md in enumerate(self.members):
            for g, mg in enumerate(self.members):
                if g != d:
                    self.stage[d][g].copy_(mg.opt.flat.grads)
                self.counts[d][g:g + 1].copy_(mg._ppo_out[ppo_loss.STAT_COUNT:ppo_loss.STAT_COUNT + 1])

    def reduce_gradients(self):
        """Every member's gradient buffer becomes the mean over all shards' active samples (after exchange_gradients())."""
        with on_current_stream():
            for d, m in self._each():
                srcs = [m.opt.flat.grads if g == d else self.stage[d][g] for g in range(self.shards)]
                m.sim.reduce_gradients(srcs, self.counts[d], out=m.opt.flat.grads, total=self.totals[d])

    def run_epochs(self):
        """num_epochs epochs of num_minibatches minibatches over the members' rollouts: update() without the read."""
        cfg = self.cfg
        for m in self.members:
            m.ppo_stats.zero_()
            m.value_stats.zero_()
            m.adam_stats.zero_()
        with on_current_stream():
            for epoch in range(cfg.num_epochs):
                parts = [rollout.epoch_parts(m.permutation(), cfg.num_minibatches) for _, m in self._each()]
                for i in range(cfg.num_minibatches):
                    for g, m in self._each():
                        m.forward_backward(parts[g][i], epoch)
                    with self._phase("reduce"):
                        self.exchange_gradients()
                        self.reduce_gradients()
                    for _, m in self._each():
                        with m._phase("adam"):
                            stats = m.opt.step()
                        m.adam_stats[:2] += stats[::2]
                        m.adam_stats[2] = stats[3]
        for m in self.members:
            m.update_index += 1

    update = Trainer.update

    def metrics(self):
        """The statistics of the last update() over all shards as Python numbers: Trainer's keys, "shards" and "count".
        One copy to the host, from shard 0's device."""
        import torch
        first = self.members[0]
        keep = first.ppo_stats.clone(), first.value_stats.clone()
        for m in self.members[1:]:                                   # raw sums: they add
            first.ppo_stats += m.ppo_stats.to(self.device)
            first.value_stats += m.value_stats.to(self.device)
        with torch.cuda.device(self.device):
            host = torch.stack(first.metric_tensors() + [self.totals[0][0]]).cpu().tolist()
        first.ppo_stats.copy_(keep[0])
        first.value_stats.copy_(keep[1])
        out = first.metrics_from(host[:-1])
        out["shards"], out["count"] = self.shards, host[-1]
        return out

    def update_iter(self):
        """collect() then update(): the metrics, with "fps" = all shards' rows * steps_per_update / the wall time."""
        import torch
        for m in self.members:
            torch.cuda.synchronize(m.device)
        t0 = time.perf_counter()
        self.collect()
        out = self.update()
        for m in self.members[1:]:                                   # the read waited for shard 0's device alone
            torch.cuda.synchronize(m.device)
        out["fps"] = self.rows * self.cfg.steps_per_update / (time.perf_counter() - t0)
        return out

    # ---- checkpoints ----
    def state_dict(self):
        """Shard 0's state_dict() (parameters, optimiser, normaliser, generator, counters: the replicas agree on them),
        with every shard's carried LSTM state, clear and permutation generator, and the shard ranges."""
        d = self.members[0].state_dict()
        d["state"] = [[[t.clone() for t in s] for s in m.state] for m in self.members]
        d["clear"] = [m.clear.clone() for m in self.members]
        d["generators"] = [m.generator.get_state().clone() for m in self.members]
        d["ranges"] = [list(r) for r in self.ranges]
        return d

    def load_state_dict(self, d):
        """Load what state_dict() returned into a ShardedTrainer of the same policy, config and shard layout.  Raises
        ValueError if the ranges differ."""
        theirs = [tuple(int(x) for x in r) for r in d.get("ranges", [])]
        if theirs != self.ranges:
            raise ValueError(f"the state's shards hold the worlds {theirs}: this trainer's hold {self.ranges}")
        for g, m in enumerate(self.members):
            m.load_state_dict(dict(d, state=d["state"][g], clear=d["clear"][g], generator=d["generators"][g]))
        self.stepped = False
