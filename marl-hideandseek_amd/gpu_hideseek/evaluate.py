"""Run a policy on the simulator without learning: the function of the reference's scripts/jax_infer.py
(madrona_learn.eval_policies with one policy), with the episode statistics of gpu_hideseek.episodes as its result and,
optionally, a replay log per step that replay.py, spectate.py and tools/render_replay.py read.

    ev = evaluate.Evaluator(sim, net, normaliser, mode="greedy")        # sim right after sim.init()
    with open("run.log", "wb") as f:
        stats = ev.run(250, record_log=f)                               # {"seekers": {...}, "hiders": {...}, "hider_win_rate": ...}

Composition only, of the pieces the trainer's collect() is made of: per step rollout.state_zero_into on the carried LSTM
state, pack_policy_inputs, the policy's forward under no_grad, sample_actions into the simulator's action tensor,
sim.step(), EpisodeStats.step().  The normaliser is frozen: no moments are collected and update() is never called, so a
run leaves the policy and the normaliser as it found them.

One policy plays both sides here.  Several policies playing each other, with their Elo ratings (the reference's
eval_competitive with num_policies > 1), is gpu_hideseek.league and tools/league.py.  Training several policies at once is
gpu_hideseek.population.
"""
from . import episodes, replay, rollout
from ._request import on_current_stream

MODES = ("draw", "greedy")


def members(d):
    """The trainer state_dicts in a checkpoint: the members of a population's (population.Population.state_dict), or the
    one of a trainer's."""
    return list(d["members"]) if "members" in d else [d]


def load_policy(path_or_dict, dtype=None, device=None, member=None, encoder=None, past=None):
    """(net, normaliser or None) from a trainer state_dict (a file torch.save wrote, or the dict): a policy.make_policy
    of `dtype` whose parameters are the state's flat "params" buffer, laid out as the state's optimiser says, and an
    ObsNormaliser with the state's moments where the trainer had one.  Of a population's checkpoint, `member` i, or
    `past` i: member i of its pool of past policies.
    `encoder` is one of policy.ENCODERS, or None for the kind whose flat parameter length is the state's."""
    import torch
    from . import optim, policy
    from .policy_inputs import ObsNormaliser
    device = torch.device("cuda", 0) if device is None else torch.device(device)
    d = torch.load(path_or_dict, map_location=device, weights_only=False) if not isinstance(path_or_dict, dict) else path_or_dict
    if past is not None:
        pool = d.get("past", ()) if "members" in d else ()
        if member is not None or isinstance(past, bool) or not isinstance(past, int) or not 0 <= past < len(pool):
            raise ValueError(f"a checkpoint with a pool of {len(pool)} past policies: past must be in [0, {len(pool)}) and member None, got past {past!r}, member {member!r}")
        d = pool[past]
    elif "members" in d:
        if member is None or not 0 <= member < len(d["members"]):
            raise ValueError(f"a population checkpoint of {len(d['members'])} members: member must be in [0, {len(d['members'])}), got {member!r}")
        d = d["members"][member]
    elif member not in (None, 0):
        raise ValueError(f"a trainer checkpoint has one policy: member must be None or 0, got {member!r}")
    if encoder is not None and encoder not in policy.ENCODERS:
        raise ValueError(f"encoder must be None or one of {policy.ENCODERS}, got {encoder!r}")
    theirs = {k: (int(lo), int(hi), tuple(shape)) for k, (lo, hi, shape) in d["optimizer"]["layout"].items()}
    net = flat = None
    for kind in policy.ENCODERS if encoder is None else (encoder,):
        cand = policy.make_policy(dtype, encoder=kind)
        length = 0                                                 # the padded flat length, as optim.flatten lays it out
        for p in cand.parameters():
            length = -(-(length + p.numel()) // optim.PAD) * optim.PAD
        if tuple(d["params"].shape) == (length,):
            net = cand.to(device)
            flat = optim.flatten(net.named_parameters(), device)
            break
    if net is None or theirs != flat.layout():
        raise ValueError("the state's parameters are not laid out as policy.make_policy's" + ("" if encoder is None else f" with encoder {encoder!r}"))
    with torch.no_grad():
        flat.params.copy_(d["params"])
    net._flat = flat                      # the parameters are views of this buffer
    normaliser = None
    if d.get("normaliser") is not None:
        normaliser = ObsNormaliser(device.index or 0)
        normaliser.load_state_dict(d["normaliser"])
    return net, normaliser


class Evaluator:
    """`net` (a policy.ActorCritic on the simulator's device) playing every agent row of `sim`.  mode "draw" samples the
    actions with the uniforms keyed by (seed, step, global agent row), "greedy" takes every head's first maximum.
    `from_start`: the simulator comes right from sim.init(), so its running episodes count (EpisodeStats.arm); otherwise
    every row is counted from its next episode start."""

    def __init__(self, sim, net, normaliser=None, mode="draw", seed=0, gamma=episodes.DEFAULT_GAMMA, from_start=True):
        import torch
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        self.sim, self.net, self.normaliser, self.mode, self.seed = sim, net, normaliser, mode, int(seed)
        self.rows = n = sim.num_worlds * sim.agents_per_world
        self.device = dev = torch.device("cuda", sim.gpu_id)
        self.dtype = net.dtype
        self.state = net.init_state(n, dev, self.dtype)
        self.actor, self.critic = (torch.zeros(n, rollout.ROW, dtype=self.dtype, device=dev) for _ in range(2))
        self.clear = torch.zeros(n, dtype=torch.int32, device=dev)
        self.mask_before = None
        self.counter = 0
        self.episodes = episodes.EpisodeStats(sim, gamma=gamma).arm(from_start=from_start)
        self.behaviour = None             # a behaviour.BehaviourStats, or None: run() calls its step() after every sim.step()

    def _export(self, name):
        return getattr(self.sim, name + "_tensor")().to_torch().reshape(self.rows, -1)

    def act(self):
        """The observation in the simulator's exports -> the action tensor, the carried state advanced."""
        import torch
        sim, net = self.sim, self.net
        with on_current_stream(), torch.no_grad():
            mask = self._export("self_mask")[:, 0]
            rollout.zero_where(rollout.state_zero_into(self.clear, mask, mask if self.mask_before is None else self.mask_before), *self.state[0], *self.state[1])
            self.mask_before = mask.clone()
            sim.pack_policy_inputs(actor=self.actor, critic=self.critic, normaliser=self.normaliser)
            logits, _, self.state = net(sim, self.actor, self.critic, self.state, None)
            sim.sample_actions(logits, buckets=net.buckets, mode=self.mode, seed=(self.seed, 0), counter=self.counter)
        self.counter += 1

    def run(self, num_steps, record_log=None, on_step=None):
        """num_steps times: act(), sim.step(), the episode tracker's step; with `record_log` (a binary file open for
        writing) replay.record_step after every step; on_step(i, self), if given, after that.  Returns
        EpisodeStats.read(): what finished during the run."""
        for i in range(int(num_steps)):
            self.act()
            self.sim.step()
            episodes.step_trackers(self.episodes, self.behaviour)
            self.clear.copy_(self._export("done")[:, 0])
            if record_log is not None:
                replay.record_step(self.sim, record_log)
            if on_step is not None:
                on_step(i, self)
        return self.episodes.read()
