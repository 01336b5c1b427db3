"""ShardedSimulator — one front-end over the GPUs of a node (BASELINE.json north_star: "the batch
shards across the 8 GPUs of one node by world index with no RCCL on the step path (only a host-side concat of
observation tensors)").

The reference is single-GPU (`Manager::Config::gpuID`, src/mgr.hpp:18), so this has no counterpart there; it keeps
the HideAndSeekSimulator call shape (src/bindings.cpp:32-96).  Shard g owns the contiguous global worlds
[start_g, start_g + n_g) on its own device with its own HIP stream and is created with `world_offset = start_g`,
so every world draws from the RNG stream of its GLOBAL index (src/sim.cpp:107-113) and the sharded run equals the
monolithic one world for world.  `step()` starts every shard (hs_step_begin) before it waits for any
(hs_step_end): the devices run concurrently from one host thread, and there is no collective.

Tensors: `sim.action_tensor()` etc. return a ShardedTensor — `.shards` are the per-device zero-copy views,
`.gather()` concatenates them into ONE pinned host tensor (rows in global world order), `.scatter(t)` writes a
host tensor of that shape back to the devices (actions, resets).
"""
from . import _tensor_getters, madrona


def shard_ranges(num_worlds, num_shards):
    """Contiguous world ranges [(start, count)] — the first `num_worlds % num_shards` shards take one world more."""
    if num_shards <= 0 or num_worlds < num_shards:
        raise ValueError("need at least one world per shard")
    base, extra = divmod(int(num_worlds), int(num_shards))
    out, start = [], 0
    for g in range(num_shards):
        n = base + (1 if g < extra else 0)
        out.append((start, n))
        start += n
    return out


def locate(ranges, world):
    """Global world index -> (shard, local world index)."""
    for g, (start, n) in enumerate(ranges):
        if start <= world < start + n:
            return g, world - start
    raise ValueError("world index out of range")


class ShardedTensor:
    def __init__(self, shards, rows_per_world, ranges):
        self.shards = shards                  # madrona.Tensor per shard, in world order
        self.rows_per_world = rows_per_world
        self.ranges = ranges
        self._host = None

    @property
    def shape(self):
        return (sum(t.shape[0] for t in self.shards),) + tuple(self.shards[0].shape[1:])

    def per_device(self):
        """The zero-copy device views (torch), one per shard."""
        return [t.to_torch() for t in self.shards]

    def row_range(self, shard):
        start, n = self.ranges[shard]
        return start * self.rows_per_world, (start + n) * self.rows_per_world

    def gather(self, out=None):
        """Host-side concat: device -> pinned host copies of every shard, rows in global world order."""
        import torch
        if out is None:
            if self._host is None:
                first = self.shards[0].to_torch()
                self._host = torch.empty(self.shape, dtype=first.dtype, pin_memory=True)
            out = self._host
        devs = self.per_device()
        for g, d in enumerate(devs):
            lo, hi = self.row_range(g)
            out[lo:hi].copy_(d, non_blocking=True)
        for d in devs:
            torch.cuda.synchronize(d.device)
        return out

    def scatter(self, host):
        """Write a host tensor of the gathered shape to the shards (actions / resets)."""
        import torch
        devs = self.per_device()
        for g, d in enumerate(devs):
            lo, hi = self.row_range(g)
            d.copy_(host[lo:hi], non_blocking=True)
        for d in devs:
            torch.cuda.synchronize(d.device)

    def to_torch(self):
        """A single handle aliases nothing across devices: one shard -> its zero-copy view, otherwise the gather."""
        return self.shards[0].to_torch() if len(self.shards) == 1 else self.gather()


@_tensor_getters
class ShardedSimulator:
    def __init__(self, gpu_ids, num_worlds, **kw):
        from . import HideAndSeekSimulator
        kw.pop("gpu_id", None)
        kw.pop("world_offset", None)
        kw.setdefault("exec_mode", madrona.ExecMode.CUDA)
        self.gpu_ids = list(gpu_ids)
        self.num_worlds = int(num_worlds)
        self.ranges = shard_ranges(self.num_worlds, len(self.gpu_ids))
        self.shards = [HideAndSeekSimulator(gpu_id=g, num_worlds=n, world_offset=start, **kw)
                       for g, (start, n) in zip(self.gpu_ids, self.ranges)]
        self.agents_per_world = self.shards[0].agents_per_world

    def init(self):
        for s in self.shards:
            s.init()

    def step(self):
        started = []
        try:
            for s in self.shards:          # every device starts its step ...
                s.step_begin()
                started.append(s)
        finally:
            err = None
            for s in started:              # ... before the host waits for any of them
                try:
                    s.step_end()
                except Exception as e:     # noqa: BLE001 - finish the other shards, then report the first failure
                    err = err or e
            if err is not None:
                raise err

    def _tensor(self, name):
        ts = [getattr(s, name + "_tensor")() for s in self.shards]
        n0 = self.ranges[0][1]
        return ShardedTensor(ts, ts[0].shape[0] // n0, self.ranges)

    def trigger_reset(self, world_idx, level_idx):
        g, local = locate(self.ranges, int(world_idx))
        self.shards[g].trigger_reset(local, level_idx)

    def set_action(self, agent_idx, x, y, r, g, l):
        A = self.agents_per_world
        shard, local = locate(self.ranges, int(agent_idx) // A)
        self.shards[shard].set_action(local * A + int(agent_idx) % A, x, y, r, g, l)

    def spectate(self, cameras, width, height, *, depth=True, rgb=True, hit=False, out=None, exact=False):
        """HideAndSeekSimulator.spectate with GLOBAL world ids: each camera is rendered by the shard that owns its world;
        the images come back in the caller's camera order, on the first shard's device (or in `out`)."""
        from . import spectate
        return spectate.render_sharded(self, cameras, width, height, depth, rgb, hit, out, exact)

    def pack_policy_inputs(self, actor=None, critic=None, moments=None, *, dtype=None, stream=None, normaliser=None):
        """HideAndSeekSimulator.pack_policy_inputs per shard: a list of the shards' results, each on its own device.
        Every argument is True / None for all shards or a list with one entry per shard; every shard's pack is enqueued
        before any is waited for.  `normaliser`: a list with one ObsNormaliser or table per shard, each on its shard's
        device, or one for all shards when they share its device (policy_inputs.pack_sharded)."""
        from . import policy_inputs
        return policy_inputs.pack_sharded(self, actor, critic, moments, dtype, stream, normaliser)

    def sample_actions(self, logits, *, buckets=(5, 5, 5, 2, 2), mode="draw", seed=(0, 0), counter=0, action=None,
                       log_prob=None, entropy=None, head_log_prob=None, zero_inactive=False, stream=None):
        """HideAndSeekSimulator.sample_actions per shard: `logits` has one tensor per shard, on the shard's device; a
        list of the shards' results.  Every output (and `stream`) is True / None for all shards or a list with one entry
        per shard.  The draws are keyed by the global agent row, so they do not depend on the number of shards."""
        from . import action_sampling
        return action_sampling.sample_sharded(self, logits, stream, action, log_prob, entropy, head_log_prob,
                                              buckets=buckets, mode=mode, seed=seed, counter=counter,
                                              zero_inactive=zero_inactive)

    def compute_advantages(self, rewards, dones, values, bootstrap, *, gamma=0.998, gae_lambda=0.95, mask=None,
                           advantages=True, returns=True, moments=None, stream=None):
        """HideAndSeekSimulator.compute_advantages per shard: `rewards`, `dones`, `values` and `bootstrap` have one
        tensor per shard, on the shard's device; a list of the shards' results.  `mask`, every output and `stream` are
        True / None for all shards or a list with one entry per shard.  A row's results depend on that row alone, so
        they do not depend on the number of shards."""
        from . import advantages as _advantages
        return _advantages.compute_sharded(self, rewards, dones, values, bootstrap, stream, mask, advantages, returns,
                                           moments, gamma=gamma, gae_lambda=gae_lambda)

    def episode_stats(self, state, table, *, gamma=0.998, reward=None, done=None, self_type=None, self_mask=None, episode_result=None,
                      hider_team=None, stream=None):
        """HideAndSeekSimulator.episode_stats per shard: `state` and `table` have one entry per shard, on the shard's
        device; every explicit input and `stream` is None for all shards or a list with one entry per shard.  A list of
        the shards' results.  A world's episodes depend on that world alone: the shards' tables add up to the counts and
        sums of the unsharded run (the sums in another order of addition)."""
        from . import episodes as _episodes
        return _episodes.compute_sharded(self, state, table, stream, gamma=gamma, reward=reward, done=done, self_type=self_type,
                                         self_mask=self_mask, episode_result=episode_result, hider_team=hider_team)

    def behaviour_stats(self, state, table, *, move_eps=0.5, positions=None, locks=None, counts=None, prep_counter=None, done=None, self_type=None,
                        self_mask=None, grabbing=None, stream=None):
        """HideAndSeekSimulator.behaviour_stats per shard: `state` and `table` have one entry per shard, on the shard's
        device; every explicit input and `stream` is None for all shards or a list with one entry per shard.  A list of
        the shards' results.  A world's statistics depend on that world alone: the shards' tables add up to the counts
        and sums of the unsharded run (the sums in another order of addition)."""
        from . import behaviour as _behaviour
        return _behaviour.compute_sharded(self, state, table, stream, move_eps=move_eps, positions=positions, locks=locks, counts=counts,
                                          prep_counter=prep_counter, done=done, self_type=self_type, self_mask=self_mask, grabbing=grabbing)

    def ppo_loss(self, logits, action, old_log_prob, advantage, *, buckets=(5, 5, 5, 2, 2), adv_moments=None, mask=None, value=None,
                 returns=None, old_value=None, clip_coef=0.2, value_loss_coef=0.5, entropy_coef=0.01, grad_scale=1.0,
                 grad_logits=True, grad_value=None, stats=True, grad_dtype=None, stream=None):
        """HideAndSeekSimulator.ppo_loss per shard: `logits`, `action`, `old_log_prob` and `advantage` have one tensor
        per shard, on the shard's device; a list of the shards' results.  Every other tensor argument, every output and
        `stream` are True / None for all shards or a list with one entry per shard.  A sample's gradients depend on that
        sample and on its shard's count of active samples (ppo_loss.compute_sharded)."""
        from . import ppo_loss as _ppo_loss
        return _ppo_loss.compute_sharded(self, logits, action, old_log_prob, advantage, stream, buckets=buckets, adv_moments=adv_moments,
                                 mask=mask, value=value, returns=returns, old_value=old_value, clip_coef=clip_coef,
                                 value_loss_coef=value_loss_coef, entropy_coef=entropy_coef, grad_scale=grad_scale,
                                 grad_logits=grad_logits, grad_value=grad_value, stats=stats, grad_dtype=grad_dtype)

    def value_head(self, logits, returns=None, *, bins=255, lo=-20.0, hi=20.0, mask=None, value=True, grad_logits=None, stats=None,
                   loss_coef=1.0, grad_scale=1.0, grad_dtype=None, value_dtype=None, stream=None):
        """HideAndSeekSimulator.value_head per shard: `logits` has one tensor per shard, on the shard's device; a list of
        the shards' results.  `returns`, `mask`, every output and `stream` are True / None for all shards or a list with
        one entry per shard (value_head.compute_sharded)."""
        from . import value_head as _value_head
        return _value_head.compute_sharded(self, logits, returns, stream, bins=bins, lo=lo, hi=hi, mask=mask, value=value,
                                           grad_logits=grad_logits, stats=stats, loss_coef=loss_coef, grad_scale=grad_scale,
                                           grad_dtype=grad_dtype, value_dtype=value_dtype)

    def encode_entities(self, rows, params, *, embed_dim=64, eps=1e-6, slope=0.01, features=True, argmax=None, dtype=None, stream=None):
        """HideAndSeekSimulator.encode_entities per shard: `rows` has one tensor per shard, on the shard's device; `params`
        is one tensor for all shards or a list; a list of the shards' results (entity_encoder.compute_sharded)."""
        from . import entity_encoder as _enc
        return _enc.compute_sharded(self, rows, params, stream, features=features, argmax=argmax, embed_dim=embed_dim, eps=eps, slope=slope, dtype=dtype)

    def encode_entities_backward(self, rows, params, grad_features, argmax, *, embed_dim=64, eps=1e-6, slope=0.01, grad_params=True, stream=None):
        """HideAndSeekSimulator.encode_entities_backward per shard: every shard's grad_params is the sum over its own rows
        (entity_encoder.compute_backward_sharded)."""
        from . import entity_encoder as _enc
        return _enc.compute_backward_sharded(self, rows, params, grad_features, argmax, stream, grad_params=grad_params, embed_dim=embed_dim,
                                             eps=eps, slope=slope)

    def hash_encode(self, rows, params, *, eps=1e-6, features=True, bin=None, dtype=None, stream=None):
        """HideAndSeekSimulator.hash_encode per shard: `rows` has one tensor per shard, on the shard's device; `params` is
        one tensor for all shards or a list; a list of the shards' results (hash_encoder.compute_sharded)."""
        from . import hash_encoder as _hash
        return _hash.compute_sharded(self, rows, params, stream, features=features, bin=bin, eps=eps, dtype=dtype)

    def hash_encode_backward(self, bin, grad_features, params, *, eps=1e-6, grad_params=True, stream=None):
        """HideAndSeekSimulator.hash_encode_backward per shard: every shard's grad_params is the sum over its own rows
        (hash_encoder.compute_backward_sharded)."""
        from . import hash_encoder as _hash
        return _hash.compute_backward_sharded(self, bin, grad_features, params, stream, grad_params=grad_params, eps=eps)

    def lstm_cell(self, gates, c_prev, cell_params, *, clear=None, hidden=None, eps=1e-6, y=True, h_next=True, c_next=True, y_dtype=None, stream=None):
        """HideAndSeekSimulator.lstm_cell per shard: `gates`, `c_prev` (and `clear`) have one tensor per shard, on the
        shard's device; `cell_params` is one tensor for all shards or a list; a list of the shards' results
        (recurrent.compute_sharded)."""
        from . import recurrent as _rec
        return _rec.compute_sharded(self, gates, c_prev, cell_params, stream, clear=clear, y=y, h_next=h_next, c_next=c_next, hidden=hidden, eps=eps,
                                    y_dtype=y_dtype)

    def lstm_cell_backward(self, gates, c_prev, cell_params, grad_y, *, clear=None, grad_h_next=None, grad_c_next=None, hidden=None, eps=1e-6,
                           grad_gates=True, grad_c_prev=True, grad_cell_params=True, stream=None):
        """HideAndSeekSimulator.lstm_cell_backward per shard: every shard's grad_cell_params is the sum over its own rows
        (recurrent.compute_backward_sharded)."""
        from . import recurrent as _rec
        return _rec.compute_backward_sharded(self, gates, c_prev, cell_params, grad_y, stream, clear=clear, grad_h_next=grad_h_next,
                                             grad_c_next=grad_c_next, grad_gates=grad_gates, grad_c_prev=grad_c_prev,
                                             grad_cell_params=grad_cell_params, hidden=hidden, eps=eps)

    def dense_norm_act(self, z, params, *, channels=None, eps=1e-6, slope=0.01, y=True, y_dtype=None, stream=None):
        """HideAndSeekSimulator.dense_norm_act per shard: `z` has one tensor per shard, on the shard's device; `params` is
        one tensor for all shards or a list; a list of the shards' results (mlp.compute_sharded)."""
        from . import mlp as _mlp
        return _mlp.compute_sharded(self, z, params, stream, y=y, channels=channels, eps=eps, slope=slope, y_dtype=y_dtype)

    def dense_norm_act_backward(self, z, params, grad_y, *, channels=None, eps=1e-6, slope=0.01, grad_z=True, grad_params=True, stream=None):
        """HideAndSeekSimulator.dense_norm_act_backward per shard: every shard's grad_params is the sum over its own rows
        (mlp.compute_backward_sharded)."""
        from . import mlp as _mlp
        return _mlp.compute_backward_sharded(self, z, params, grad_y, stream, grad_z=grad_z, grad_params=grad_params, channels=channels,
                                             eps=eps, slope=slope)

    def attend_entities(self, qkv, key_mask=None, *, out=True, out_dtype=None, stream=None):
        """HideAndSeekSimulator.attend_entities per shard: `qkv` has one tensor per shard, on the shard's device; `key_mask`
        is None for all shards or a list; a list of the shards' results (entity_attention.compute_sharded)."""
        from . import entity_attention as _att
        return _att.compute_sharded(self, qkv, key_mask, stream, out=out, out_dtype=out_dtype)

    def attend_entities_backward(self, qkv, key_mask, grad_out, *, grad_qkv=True, stream=None):
        """HideAndSeekSimulator.attend_entities_backward per shard (entity_attention.compute_backward_sharded)."""
        from . import entity_attention as _att
        return _att.compute_backward_sharded(self, qkv, key_mask, grad_out, stream, grad_qkv=grad_qkv)

    def device_status(self):
        out = {}
        for s in self.shards:
            for k, v in s.device_status().items():
                out[k] = (out.get(k, 0) + v) if not isinstance(v, bool) else (out.get(k, True) and v)
        return out

    def close(self):
        for s in self.shards:
            s.close()
