"""The update loop: the learner's pieces called in sequence, as the reference's user gets it from scripts/jax_train.py
(`Update: N / FPS: ...`).  That loop lives in madrona_learn, which is not part of the reference's tree: the knobs and their
defaults are jax_train.py's, the order of the calls below is the project's.

    sim.init()
    tr = trainer.Trainer(sim, trainer.TrainConfig(dtype=torch.bfloat16))
    for _ in range(updates):
        metrics = tr.update_iter()          # collect() then update(); one read of the device at its end

Composition only: every kernel is another module's (policy_inputs, policy, action_sampling, value_head, advantages,
rollout, ppo_loss, optim).  Single device: there is no ShardedSimulator form (optim states the same limit).

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
critic's rows packed without moments, the critic backbone and head on the carried critic state) whose new state is
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
    """Device events around the phases of collect() and update() (PHASES), for tools/train.py --phases: set
    trainer.phases = PhaseTimer(); totals() waits for the device and returns {phase: ms} since the last totals()."""

    def __init__(self):
        self.events = {k: [] for k in PHASES}

    def __call__(self, name):
        return _Span(self.events[name])

    def totals(self):
        import torch
        torch.cuda.synchronize()
        out = {k: sum(a.elapsed_time(b) for a, b in ev) for k, ev in self.events.items()}
        self.events = {k: [] for k in PHASES}
        return out


def make_loss_scale(cfg, device):
    """The optim.LossScale of cfg.loss_scale on `device`, or None."""
    s = loss_scale_settings(cfg.loss_scale)
    return None if s is None else optim.LossScale(device, **s)


class Trainer:
    """The policy (policy.make_policy, seeded with cfg.seed, unless `net` is given), optim.Adam over its parameters, an
    ObsNormaliser, the Rollout, the carried LSTM state and the sampling counter of one simulator (after sim.init())."""

    def __init__(self, sim, cfg=None, net=None, fused=True):
        import torch
        self.sim, self.cfg, self.fused = sim, TrainConfig() if cfg is None else cfg, bool(fused)
        cfg = self.cfg
        self.rows = n = sim.num_worlds * sim.agents_per_world
        check_config(cfg, n)
        self.dtype = torch.float32 if cfg.dtype is None else cfg.dtype
        self.device = dev = torch.device("cuda", sim.gpu_id)
        if net is None:
            net = policy.make_policy(self.dtype, generator=torch.Generator().manual_seed(cfg.seed))
        self.net = net.to(dev).set_fused(self.fused)
        self.opt = optim.Adam(sim, self.net.named_parameters(), lr=cfg.lr, max_grad_norm=cfg.max_grad_norm, loss_scale=make_loss_scale(cfg, dev))
        self.normaliser = ObsNormaliser(sim.gpu_id) if cfg.normalise_obs else None
        self.rollout = rollout.Rollout(sim, cfg.steps_per_update, cfg.num_bptt_chunks, self.dtype, hidden=self.net.actor.core.hidden)
        self.state = self.net.init_state(n, dev, self.dtype)
        self.clear = torch.zeros(n, dtype=torch.int32, device=dev)
        self.bootstrap = torch.zeros(n, dtype=torch.float32, device=dev)
        self.adv_moments = torch.zeros(advantages.MOMENTS, dtype=torch.float64, device=dev)
        self.boot_rows = torch.zeros(n, rollout.ROW, dtype=self.dtype, device=dev)
        self.generator = torch.Generator(device=dev).manual_seed(cfg.seed)
        self.update_index, self.counter = 0, 0
        self.stepped = False              # the simulator has been stepped past the last slot: its exports are the next o_0
        self._mb = None
        self.phases = None                # a PhaseTimer, or None: no events
        self.episodes = None              # an episodes.EpisodeStats, or None: collect() calls its step() after every sim.step()
        self.behaviour = None             # a behaviour.BehaviourStats, or None: likewise
        E = cfg.num_epochs
        self.ppo_stats = torch.zeros(E, PPO_STATS, dtype=torch.float64, device=dev)
        self.value_stats = torch.zeros(E, VALUE_STATS, dtype=torch.float64, device=dev)
        self.adam_stats = torch.zeros(3, dtype=torch.float64, device=dev)         # sum of norms, skipped steps, t
        self._ppo_out = torch.zeros(PPO_STATS, dtype=torch.float64, device=dev)
        self._value_out = torch.zeros(VALUE_STATS, dtype=torch.float64, device=dev)

    def _phase(self, name):
        return _NoSpan() if self.phases is None else self.phases(name)

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
        zero = rollout.state_zero_into(clear, mask, mask_before).unsqueeze(1)
        for x in (t for s in self.state for t in s):
            x.masked_fill_(zero, 0)

    def collect(self):
        """Fill the rollout with steps_per_update slots, the bootstrap value, the advantages and returns, and fold the
        slots' moments into the normaliser."""
        import torch
        sim, buf, net, cfg = self.sim, self.rollout, self.net, self.cfg
        T, L = buf.steps, buf.chunk_steps
        with on_current_stream(), torch.no_grad():
            for t in range(T):
                if t > 0 or not self.stepped:
                    with self._phase("sim"):
                        sim.step()
                    if self.episodes is not None:
                        self.episodes.step()
                    if self.behaviour is not None:
                        self.behaviour.step()
                    if t > 0:
                        self._close_slot(t - 1)
                    buf.clear[t].copy_(self._export("done")[:, 0])
                    buf.mask[t].copy_(self._export("self_mask")[:, 0])
                    with self._phase("rollout_forward"):
                        self._zero_carried(buf.clear[t], buf.mask[t], buf.mask[t - 1] if t > 0 else buf.mask[t])
                else:                                    # the closing step of the last collect() led here, and zeroed
                    buf.clear[0].copy_(self.clear)
                    buf.mask[0].copy_(self._export("self_mask")[:, 0])
                self.stepped = False
                with self._phase("pack"):
                    sim.pack_policy_inputs(actor=buf.actor[t], critic=buf.critic[t], moments=buf.moments[t], normaliser=self.normaliser)
                if t % L == 0:
                    k = t // L
                    for dst, src in ((buf.actor_h, self.state[0][0]), (buf.actor_c, self.state[0][1]), (buf.critic_h, self.state[1][0]), (buf.critic_c, self.state[1][1])):
                        dst[k].copy_(src)
                with self._phase("rollout_forward"):
                    logits, critic_logits, self.state = net(sim, buf.actor[t], buf.critic[t], self.state, None)
                    sim.value_head(critic_logits, value=buf.value[t])
                    out = sim.sample_actions(logits, buckets=net.buckets, seed=(cfg.seed, 0), counter=self.counter, log_prob=buf.log_prob[t])
                    buf.action[t].copy_(out["action"].reshape(self.rows, -1))
                self.counter += 1
            with self._phase("sim"):
                sim.step()
            if self.episodes is not None:
                self.episodes.step()
            if self.behaviour is not None:
                self.behaviour.step()
            self.stepped = True
            self._close_slot(T - 1)
            self.clear.copy_(buf.done[T - 1])
            with self._phase("rollout_forward"):
                self._zero_carried(self.clear, self._export("self_mask")[:, 0], buf.mask[T - 1])
            with self._phase("gae"):                     # the bootstrap's critic-only forward included
                self.bootstrap_value()
                sim.compute_advantages(buf.reward, buf.done, buf.value, self.bootstrap, gamma=cfg.gamma, gae_lambda=cfg.gae_lambda, mask=buf.mask,
                                       advantages=buf.advantage, returns=buf.returns, moments=self.adv_moments)
                if self.normaliser is not None:
                    self.normaliser.update(sim, buf.moments)

    def bootstrap_value(self):
        """The critic's value of the observation in the simulator's exports into self.bootstrap, by a critic-only forward
        on the carried critic state, which stays as it is."""
        import torch
        net = self.net
        with on_current_stream(), torch.no_grad():
            self.sim.pack_policy_inputs(critic=self.boot_rows, normaliser=self.normaliser)
            y, _ = net.critic(self.sim, self.boot_rows, self.state[1], None)
            critic_logits = torch.nn.functional.linear(y, net.critic_head.weight.to(y.dtype), net.critic_head.bias.to(y.dtype))
            self.sim.value_head(critic_logits, value=self.bootstrap)
        return self.bootstrap

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
        """num_epochs epochs of num_minibatches minibatches over the rollout collect() filled: update() without the read
        of the metrics (gpu_hideseek.population runs several policies' epochs before its one read)."""
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

    def update(self):
        """run_epochs(), then the metrics (the one read of the device)."""
        self.run_epochs()
        return self.metrics()

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
        """The statistics of the last update() as Python numbers: one copy to the host, which waits for the device."""
        import torch
        return self.metrics_from(torch.stack(self.metric_tensors()).cpu().tolist())

    def update_iter(self):
        """collect() then update(): the metrics, with "fps" = rows * steps_per_update / the wall time of both."""
        import torch
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        self.collect()
        out = self.update()                      # ends with the read of the metrics: the device is idle
        out["fps"] = self.rows * self.cfg.steps_per_update / (time.perf_counter() - t0)
        return out

    # ---- checkpoints ----
    def state_dict(self):
        """Clones of the flat parameter buffer, the optimiser's and the normaliser's state, the carried LSTM state and
        clear, the permutation generator, and the two counters."""
        return {"params": self.opt.flat.params.clone(), "optimizer": self.opt.state_dict(),
                "normaliser": None if self.normaliser is None else self.normaliser.state_dict(),
                "state": [[t.clone() for t in s] for s in self.state], "clear": self.clear.clone(), "generator": self.generator.get_state().clone(),
                "update_index": self.update_index, "counter": self.counter}

    def load_state_dict(self, d):
        """Load what state_dict() returned into a trainer of the same policy, config and row count."""
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
        self.stepped = False
