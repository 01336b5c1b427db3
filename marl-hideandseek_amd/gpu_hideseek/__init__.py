"""gpu_hideseek — Python face of the MI355X-native batch hide-and-seek simulator.

Mirrors the reference's nanobind module (src/bindings.cpp:20-121): ``HideAndSeekSimulator`` with
the same keyword constructor, ``init`` / ``step``, the 21 tensor getters, ``SimFlags`` and
``madrona.ExecMode`` so that scripts/benchmark.py runs unchanged.  Everything is forwarded through
the C ABI of ``libhideseek.so`` (include/hideseek.h) with ctypes; tensors are zero-copy views of
the simulator's HBM buffers exported through DLPack (``Tensor.to_torch`` / ``Tensor.to_jax``).

There is no CPU execution path: if the HIP library or a GPU is missing the constructor raises.
"""
import atexit
import ctypes as C
import enum
import weakref

from . import _native
from . import madrona
from ._native import HsConfig as _HsConfig, HsTensorDesc as _HsTensorDesc, check as _check, load as _load
from .madrona import Tensor

__all__ = ["HideAndSeekSimulator", "ShardedSimulator", "SimFlags", "madrona", "Tensor", "library_path",
           "train_interface"]


def library_path():
    return _native.LIB_PATH


class SimFlags(enum.IntFlag):
    """src/sim_flags.hpp:7-13 (nb::is_arithmetic enum, bindings.cpp:23-29)."""
    Default = 0
    UseFixedWorld = 1 << 0
    IgnoreEpisodeLength = 1 << 1
    RandomFlipTeams = 1 << 2
    ZeroAgentVelocity = 1 << 3
    # build-side extension (include/hideseek.h): skip the observation nodes
    ExtSkipObservations = 1 << 16
    # build-side extension: render the agent views (depth / rgb) in every init / step when enable_batch_renderer is set
    ExtRender = 1 << 17


# ExportID (src/sim.hpp:45-68) + renderer outputs
_EXPORTS = dict(reset=0, prep_counter=1, action=2, self_data=3, self_type=4, self_mask=5, agent_data=6,
                box_data=7, ramp_data=8, visible_agents_mask=9, visible_boxes_mask=10, visible_ramps_mask=11,
                lidar=12, seed=13, reward=14, done=15, global_positions=16, policy_assignments=17,
                episode_result=18, ckpt_ctrl=19, ckpt=20, depth=21, rgb=22)


_EXPORT_NAMES = {v: k for k, v in _EXPORTS.items()}
# getter -> export: the 21 getters of bindings.cpp:76-96 and Manager::episodeResultTensor / policyAssignmentsTensor
# (mgr.cpp:1312-1331; JAX interface only) are <export>_tensor()
_GETTERS = {name: name for name in _EXPORTS}
# scripts/cpu_benchmark.py:77 calls a getter the reference binding lacks
_GETTERS["agent_mask"] = "self_mask"


def _tensor_getters(cls):
    """Class decorator: a <getter>_tensor() method for every entry of _GETTERS, returning cls._tensor(<export>)."""
    def make(getter, export):
        def method(self):
            return self._tensor(export)
        method.__name__ = getter + "_tensor"
        method.__qualname__ = f"{cls.__name__}.{getter}_tensor"
        method.__doc__ = f"The `{export}` tensor of the simulator (export id {_EXPORTS[export]}, include/hideseek.h)."
        return method
    for getter, export in _GETTERS.items():
        setattr(cls, getter + "_tensor", make(getter, export))
    return cls
_ROLES = {0: "actions", 1: "resets", 2: "sim_ctrl", 3: "pbt_inputs", 4: "observations", 5: "rewards", 6: "dones",
          7: "pbt_outputs", 8: "checkpoint_data"}


def train_interface():
    """Manager::trainInterface (src/mgr.cpp:1338-1375) as the library reports it (hs_train_interface): a list of
    (name, role, getter) in the reference's order, e.g. ("self_lidar", "observations", "lidar_tensor").  The getter
    is None for the empty simCtrl tensor (mgr.cpp:1333-1336)."""
    L = _load()
    tab = C.POINTER(_native.HsIfaceEntry)()
    n = L.hs_train_interface(C.byref(tab))
    out = []
    for i in range(n):
        e = tab[i]
        getter = None if e.export_id < 0 else _EXPORT_NAMES[e.export_id] + "_tensor"
        out.append((e.name.decode(), _ROLES[e.role], getter))
    return out


_live_sims = weakref.WeakSet()
_xla_registered = False          # sim.jax() registers the four XLA custom-call targets once per process


@atexit.register
def _close_all():
    # destroy simulators while the HIP runtime is still loaded (its own teardown runs after Py_Finalize)
    for s in list(_live_sims):
        s.close()


@_tensor_getters
class HideAndSeekSimulator:
    """gpu_hideseek.HideAndSeekSimulator (src/bindings.cpp:31-118)."""

    def __init__(self, exec_mode, gpu_id, num_worlds, sim_flags, rand_seed, min_hiders, max_hiders,
                 min_seekers, max_seekers, num_pbt_policies, enable_batch_renderer=False,
                 batch_render_width=64, batch_render_height=64, world_offset=0):
        L = _load()
        cfg = _HsConfig(int(exec_mode), int(gpu_id), int(num_worlds), int(sim_flags) & 0xFFFFFFFF,
                        int(rand_seed) & 0xFFFFFFFF, int(min_hiders), int(max_hiders), int(min_seekers),
                        int(max_seekers), int(num_pbt_policies), int(bool(enable_batch_renderer)),
                        int(batch_render_width), int(batch_render_height), int(world_offset))
        self._h = C.c_void_p()
        _check(L.hs_create(C.byref(cfg), C.byref(self._h)))
        self._L = L
        self.num_worlds = int(num_worlds)
        self.world_offset = int(world_offset)
        self.gpu_id = int(gpu_id)
        self.agents_per_world = L.hs_agents_per_world(self._h)
        self._tensors = {}
        _live_sims.add(self)

    def close(self):
        """Manager::~Manager (mgr.cpp:848-859).  Tensor views — and torch / jax arrays made from them — must not be
        used afterwards: they are non-owning (madrona.Tensor)."""
        h = getattr(self, "_h", None)
        if h:
            self._tensors = {}
            self._L.hs_destroy(h)
            self._h = None

    def __del__(self):
        self.close()

    def init(self):
        _check(self._L.hs_init(self._h))

    def step(self):
        _check(self._L.hs_step(self._h))

    def render(self):
        """Render every agent's view of the current state into depth_tensor() / rgb_tensor() (hs_render;
        Manager::step's batchRender(), src/mgr.cpp:894-901).  Per step instead: SimFlags.ExtRender."""
        _check(self._L.hs_render(self._h))

    def spectate(self, cameras, width, height, *, depth=True, rgb=True, hit=False, out=None, exact=False):
        """Render spectator cameras (gpu_hideseek.spectate: Camera, look_at, top_down, agent_camera) of this handle's
        worlds at width x height (hs_render_cameras): {"depth": [V,H,W] f32, "rgb": [V,H,W,4] u8, "hit": [V,H,W] i32}
        for the requested outputs, as new tensors or in the preallocated ones of `out`.  `exact` turns the kernel's
        culls off (same output).  Writes no simulator state."""
        from . import spectate
        return spectate.render(self, cameras, width, height, depth, rgb, hit, out, exact)

    def pack_policy_inputs(self, actor=None, critic=None, moments=None, *, dtype=None, stream=None, normaliser=None):
        """Pack the observation exports into policy-input rows [num_worlds * agents_per_world, 296] in one kernel
        (gpu_hideseek.policy_inputs: LAYOUT, views, moments_to_mean_var; hs_pack_policy_inputs).  `actor` (entity tables
        times their visibility masks) and `critic` (unmasked) are each True (a new tensor of `dtype`: float32, bfloat16
        or float16), a preallocated tensor (its dtype is taken; a slot buf[t] of a [T, R, 296] rollout buffer will do) or
        None; `moments` likewise, [593] float64.  stream=None blocks; a torch.cuda.Stream or raw handle enqueues there
        without synchronising (the caller orders it after the step).  `normaliser`, a policy_inputs.ObsNormaliser or its
        float32 [592] table, normalises every element as (x - mean) * inv_std before the actor's masks and the cast
        (hs_pack_policy_inputs_normalized); the moments stay those of the raw rows.  Returns {name: tensor} of what was
        written."""
        from . import policy_inputs
        return policy_inputs.pack(self, actor, critic, moments, dtype, stream, normaliser)

    def pack_policy_inputs_routed(self, row_of_slot, num_policies, *, actor=None, critic=None, moments=None, moments_stride=None, tables=None,
                                  bad=None, dtype=None, stream=None):
        """pack_policy_inputs for `num_policies` policies that share this simulator, in one kernel
        (gpu_hideseek.policy_inputs.pack_routed; hs_pack_policy_inputs_routed): output row s of `actor` / `critic` is agent
        row row_of_slot[s] (int32 [rows], as league_step writes it), normalised with row s // (rows // num_policies) of
        `tables` (float32 [N, 592], or None for none), bit for bit what pack_policy_inputs gives for that row and table.
        `moments` is None, True or a float64 [N, 593] tensor or view (mom[:, t] of [N, T, 593]): policy p's moments are
        those of its slots; `moments_stride` is its stride in doubles (by default the tensor's own).  `bad`, int32 [1] or
        None, receives the number of slots whose row is out of range (their rows are zeros).  Returns {name: tensor}."""
        from . import policy_inputs
        return policy_inputs.pack_routed(self, row_of_slot, num_policies, actor, critic, moments, moments_stride, tables, bad, dtype, stream)

    def sample_actions(self, logits, *, buckets=(5, 5, 5, 2, 2), mode="draw", seed=(0, 0), counter=0, action=None,
                       log_prob=None, entropy=None, head_log_prob=None, zero_inactive=False, stream=None):
        """Turn the actor's logits [num_worlds * agents_per_world, W >= sum(buckets)] (float32, bfloat16 or float16,
        contiguous in the last dimension) into the five action heads of every agent row in one kernel
        (gpu_hideseek.action_sampling; hs_sample_actions).  mode "draw" samples with the uniforms keyed by (seed,
        counter, global agent row), "greedy" takes the first maximum, "evaluate" scores the actions already stored.
        `action` is None (in place: action_tensor(), ready for the next step) or an int32 [rows, 5] tensor; `log_prob`,
        `entropy` [rows] and `head_log_prob` [rows, 5] are each True (a new float32 tensor), a preallocated tensor (a
        slot buf[t] of a rollout buffer will do) or None.  zero_inactive zeroes the rows whose self_mask is 0.
        stream=None blocks; a torch.cuda.Stream or raw handle enqueues there without synchronising.  Returns
        {name: tensor} of the action and what was written."""
        from . import action_sampling
        return action_sampling.sample(self, logits, stream, buckets=buckets, mode=mode, seed=seed, counter=counter,
                                      action=action, log_prob=log_prob, entropy=entropy, head_log_prob=head_log_prob,
                                      zero_inactive=zero_inactive)

    def sample_actions_routed(self, logits, row_of_slot, *, buckets=(5, 5, 5, 2, 2), mode="draw", seed=(0, 0), counter=0, action_rows=None,
                              action=None, log_prob=None, entropy=None, head_log_prob=None, bad=None, stream=None):
        """sample_actions for policies that share this simulator, in one kernel (gpu_hideseek.action_sampling.sample_routed;
        hs_sample_actions_routed): `logits` [rows, W >= sum(buckets)] are indexed by SLOT and `row_of_slot` (int32 [rows], as
        league_step writes it) names each slot's agent row.  The actions go to `action_rows`, indexed by row (None: in
        place into action_tensor(), ready for the next step); `action` [rows, 5], `log_prob`, `entropy` [rows] and
        `head_log_prob` [rows, 5], each True, a tensor or None, stay indexed by slot.  Every value has the bits
        sample_actions gives the row from the same logits, seed and counter.  mode is "draw" or "greedy".  `bad`, True,
        int32 [1] or None, receives the number of slots whose row is out of range (their outputs are zeros and no row is
        written).  Returns {name: tensor}."""
        from . import action_sampling
        return action_sampling.sample_routed(self, logits, row_of_slot, stream, buckets=buckets, mode=mode, seed=seed, counter=counter,
                                             action_rows=action_rows, action=action, log_prob=log_prob, entropy=entropy,
                                             head_log_prob=head_log_prob, bad=bad)

    def compute_advantages(self, rewards, dones, values, bootstrap, *, gamma=0.998, gae_lambda=0.95, mask=None,
                           advantages=True, returns=True, moments=None, groups=None, stream=None):
        """GAE advantages and value targets of a rollout in one kernel (gpu_hideseek.advantages; hs_compute_gae, whose
        header comment states the arithmetic: IEEE f32 in a fixed order, the same bits on every call).  `rewards`
        (float32), `dones` (int32: nonzero = the episode ended with step t), `values` (float32, bfloat16 or float16: the
        critic's value of the observation the action of step t was chosen from) and `mask` (float32 self_mask of step t,
        or None: every row active) are contiguous [T, rows], [T, rows, 1] or [T, num_worlds, agents_per_world];
        `bootstrap` [rows] is the value of the observation after the last step, in the dtype of `values`.
        `advantages` and `returns` are each True (a new float32 tensor shaped like `rewards`), a preallocated tensor or
        None; `moments` likewise, [5] float64: sum and sum of squares of the advantages and of the returns and the count,
        over the active steps (advantages.moments_to_mean_std).  With `groups` = G the rows are G groups of rows / G
        consecutive rows (the slots of a population's policies) and `moments` is [G, 5], vector g with the bits of this call
        on group g's columns alone (hs_compute_gae_grouped).  stream=None blocks; a torch.cuda.Stream or raw handle
        enqueues there without synchronising.  Returns {name: tensor} of what was written."""
        from . import advantages as _advantages
        return _advantages.compute(self, rewards, dones, values, bootstrap, stream, gamma=gamma, gae_lambda=gae_lambda,
                                   mask=mask, advantages=advantages, returns=returns, moments=moments, groups=groups)

    def ppo_loss(self, logits, action, old_log_prob, advantage, *, buckets=(5, 5, 5, 2, 2), adv_moments=None, mask=None, value=None,
                 returns=None, old_value=None, clip_coef=0.2, value_loss_coef=0.5, entropy_coef=0.01, grad_scale=1.0,
                 grad_logits=True, grad_value=None, stats=True, grad_dtype=None, loss_scale=None, stream=None):
        """The PPO loss of a minibatch and its gradients in one kernel (gpu_hideseek.ppo_loss; hs_ppo_loss, whose header
        comment states the arithmetic: IEEE f32 in a fixed order).  Over the n = logits.shape[0] samples: `logits`
        [n, W >= sum(buckets)] (float32, bfloat16 or float16, contiguous in the last dimension: pass logits.detach()),
        `action` [n, 5] int32, `old_log_prob` and `advantage` [n] float32; optional `adv_moments` (the moments of
        compute_advantages: the advantage is normalised on the device), `mask` [n] float32, `value` [n] or [n, 1] with
        `returns` [n] float32 and, for the clipped value loss, `old_value` [n] float32.  `grad_logits`, `grad_value` and
        `stats` are each True (a new tensor: grad_logits shaped like `logits` in `grad_dtype`, by default the logits'
        dtype; grad_value like `value`; stats [7] float64), a preallocated tensor or None; grad_value=None means True
        with a value.  A bucket masked with -inf and an inactive sample get gradients of exactly 0.  With `loss_scale`,
        the float64 [4] state of an optim.LossScale, the gradients (not the stats) are multiplied by its scale, read on
        the device (hs_ppo_loss_scaled).  stream=None blocks;
        a torch.cuda.Stream or raw handle enqueues there without synchronising.  Returns {name: tensor} of what was
        written, plus "coefficients" for ppo_loss.attach / stats_to_metrics."""
        from . import ppo_loss as _ppo_loss
        return _ppo_loss.compute(self, logits, action, old_log_prob, advantage, stream, buckets=buckets, adv_moments=adv_moments,
                                 mask=mask, value=value, returns=returns, old_value=old_value, clip_coef=clip_coef,
                                 value_loss_coef=value_loss_coef, entropy_coef=entropy_coef, grad_scale=grad_scale,
                                 grad_logits=grad_logits, grad_value=grad_value, stats=stats, grad_dtype=grad_dtype, loss_scale=loss_scale)

    def value_head(self, logits, returns=None, *, bins=255, lo=-20.0, hi=20.0, mask=None, value=True, grad_logits=None, stats=None,
                   loss_coef=1.0, grad_scale=1.0, grad_dtype=None, value_dtype=None, loss_scale=None, stream=None):
        """The two-hot symlog critic head in one kernel (gpu_hideseek.value_head; hs_twohot_value, whose header comment
        states the arithmetic: IEEE f32 in a fixed order).  Over the n = logits.shape[0] samples: `logits`
        [n, W >= bins] (float32, bfloat16 or float16, contiguous in the last dimension: pass logits.detach()) are the
        critic's logits over `bins` bins from `lo` to `hi` in symlog space.  value = symexp(softmax(logits) . bins), the
        decoded value.  With `returns` [n] float32 also grad_logits, the gradient of
        grad_scale * loss_coef * (the mean over the active samples of the cross-entropy against the two-hot target of
        symlog(returns)), and stats [6] float64 (value_head.stats_to_metrics).  `mask` [n] float32 or None marks the
        active samples; an inactive one gets a value and gradients of exactly 0, and the count that divides is the one
        ppo_loss divides by, so the two gradients add.  Each output is True (allocated: value in `value_dtype` and
        grad_logits in `grad_dtype`, by default the logits' dtype), a preallocated tensor (for value a slot buf[t] of a
        [T, rows] buffer will do) or None; value defaults to True, grad_logits and stats to True exactly when returns
        are given.  Active samples must hold finite logits and returns that are not NaN.  With `loss_scale`, the float64
        [4] state of an optim.LossScale, grad_logits is multiplied by its scale (hs_twohot_value_scaled).  stream=None blocks; a
        torch.cuda.Stream or raw handle enqueues there without synchronising.  Returns {name: tensor} of what was
        written, plus "coefficients" for value_head.attach."""
        from . import value_head as _value_head
        return _value_head.compute(self, logits, returns, stream, bins=bins, lo=lo, hi=hi, mask=mask, value=value,
                                   grad_logits=grad_logits, stats=stats, loss_coef=loss_coef, grad_scale=grad_scale,
                                   grad_dtype=grad_dtype, value_dtype=value_dtype, loss_scale=loss_scale)

    def encode_entities(self, rows, params, *, embed_dim=64, eps=1e-6, slope=0.01, features=True, argmax=None, dtype=None, stream=None):
        """The entity encoder in one kernel (gpu_hideseek.entity_encoder; hs_entity_encode, whose header comment states
        the arithmetic: IEEE f32 in a fixed order).  `rows` [n, 296] (float32, bfloat16 or float16, contiguous) are rows of
        pack_policy_inputs; `params` the flat float32 tensor of 102 * embed_dim elements (entity_encoder.param_layout).
        Every entity of the four tables goes through its table's Dense(embed_dim), a LayerNorm (`eps`) and a leaky ReLU
        (`slope`); agents, boxes and ramps are max-pooled.  features [n, 4 * embed_dim] in `dtype` (by default the rows')
        and argmax [n, 3, embed_dim] uint8 (the first entity that attains the maximum: what the backward call needs) are
        each True (allocated), a preallocated tensor (for features a slot buf[t] of a [T, rows, 4 E] buffer will do) or
        None.  Rows and parameters must be finite.  stream=None blocks; a torch.cuda.Stream or raw handle enqueues there
        without synchronising.  Returns {name: tensor} of what was written."""
        from . import entity_encoder as _enc
        return _enc.compute(self, rows, params, stream, embed_dim=embed_dim, eps=eps, slope=slope, features=features, argmax=argmax, dtype=dtype)

    def encode_entities_backward(self, rows, params, grad_features, argmax, *, embed_dim=64, eps=1e-6, slope=0.01, grad_params=True, stream=None):
        """The gradient of the encoder's parameters in one kernel plus a fixed-order sum (hs_entity_encode_backward): from
        the rows and parameters of the forward call, the upstream `grad_features` [n, 4 * embed_dim] (float32, bfloat16 or
        float16) and the forward's `argmax`.  grad_params (True or a float32 tensor of 102 * embed_dim elements) has the
        layout of params.  No gradient with respect to the rows is computed.  The same inputs give the same bits on every
        call.  Returns {"grad_params": tensor}."""
        from . import entity_encoder as _enc
        return _enc.compute_backward(self, rows, params, grad_features, argmax, stream, embed_dim=embed_dim, eps=eps, slope=slope, grad_params=grad_params)

    def hash_encode(self, rows, params, *, eps=1e-6, features=True, bin=None, dtype=None, stream=None):
        """The SimHash encoder in one kernel (gpu_hideseek.hash_encoder; hs_hash_encode, whose header comment states the
        arithmetic: IEEE f32 in a fixed order).  `rows` [n, 296] (float32, bfloat16 or float16, contiguous, 16-byte
        aligned) are rows of pack_policy_inputs; `params` the flat float32 tensor of 10624 elements
        (hash_encoder.param_layout: proj [8, 296], table [256, 32], scale, shift).  A row's 8 projections give its bin
        (bit i set where projection i is above 0), and its features are the LayerNorm (`eps`) of the bin's table row.
        features [n, 32] in `dtype` (by default the rows') is True (allocated) or a preallocated tensor (a slot buf[t] of a
        [T, rows, 32] buffer will do); bin [n] uint8 (what the backward call needs) is True, a tensor or None.
        stream=None blocks; a torch.cuda.Stream or raw handle enqueues there without synchronising.  Returns
        {name: tensor} of what was written."""
        from . import hash_encoder as _hash
        return _hash.compute(self, rows, params, stream, eps=eps, features=features, bin=bin, dtype=dtype)

    def hash_encode_backward(self, bin, grad_features, params, *, eps=1e-6, grad_params=True, stream=None):
        """The gradient of the SimHash encoder's parameters (hs_hash_encode_backward): the upstream `grad_features` [n, 32]
        (float32, bfloat16 or float16) is summed per bin of the forward's `bin` [n] in a fixed order, and the 256 sums go
        through the LayerNorm's backward.  grad_params (True or a float32 tensor of 10624 elements) has the layout of
        params; its proj range and the table rows of bins without rows are +0.  The same inputs give the same bits on
        every call.  Returns {"grad_params": tensor}."""
        from . import hash_encoder as _hash
        return _hash.compute_backward(self, bin, grad_features, params, stream, eps=eps, grad_params=grad_params)

    def lstm_cell(self, gates, c_prev, cell_params, *, clear=None, hidden=None, eps=1e-6, y=True, h_next=True, c_next=True, y_dtype=None, stream=None):
        """The recurrent core after its gate GEMMs in one kernel (gpu_hideseek.recurrent; hs_lstm_cell, whose header
        comment states the arithmetic: IEEE f32 in a fixed order).  `gates` [n, 4 H] (float32, bfloat16 or float16,
        contiguous; order i, f, g, o) is x W_in + h W_rec, `c_prev` [n, H] float32, `cell_params` the flat float32 tensor
        bias [4 H] | gamma [H] | beta [H] (recurrent.param_layout), H one of 64, 128, 256, 512.  `clear` [n] int32 or None
        is the done export of the step just taken: a nonzero row gets h_next and c_next of exactly 0, while y is the
        LayerNorm (`eps`) of its uncleared output.  y [n, H] in `y_dtype` (by default the gates'), h_next in the gates'
        dtype and c_next float32 are each True (allocated), a preallocated tensor (for y a slot buf[t] of a [T, rows, H]
        buffer will do) or None.  stream=None blocks; a torch.cuda.Stream or raw handle enqueues there without
        synchronising.  Returns {name: tensor} of what was written."""
        from . import recurrent as _rec
        return _rec.compute(self, gates, c_prev, cell_params, stream, clear=clear, hidden=hidden, eps=eps, y=y, h_next=h_next, c_next=c_next,
                            y_dtype=y_dtype)

    def lstm_cell_backward(self, gates, c_prev, cell_params, grad_y, *, clear=None, grad_h_next=None, grad_c_next=None, hidden=None, eps=1e-6,
                           grad_gates=True, grad_c_prev=True, grad_cell_params=True, stream=None):
        """The gradients of lstm_cell in one kernel plus a fixed-order sum (hs_lstm_cell_backward): recomputed from the
        forward's gates, c_prev, cell_params and clear, with the upstream `grad_y` [n, H] (float32, bfloat16 or float16),
        `grad_h_next` (the gates' dtype) and `grad_c_next` (float32), either of which may be None for zero.  grad_gates
        [n, 4 H] in the gates' dtype, grad_c_prev [n, H] and grad_cell_params [6 H] float32 are each True, a tensor or
        None.  The same inputs give the same bits on every call.  Returns {name: tensor} of what was written."""
        from . import recurrent as _rec
        return _rec.compute_backward(self, gates, c_prev, cell_params, grad_y, stream, clear=clear, grad_h_next=grad_h_next, grad_c_next=grad_c_next,
                                     hidden=hidden, eps=eps, grad_gates=grad_gates, grad_c_prev=grad_c_prev, grad_cell_params=grad_cell_params)

    def dense_norm_act(self, z, params, *, channels=None, eps=1e-6, slope=0.01, y=True, y_dtype=None, stream=None):
        """A dense layer after its GEMM in one kernel (gpu_hideseek.mlp; hs_dense_norm_act, whose header comment states
        the arithmetic: IEEE f32 in a fixed order).  `z` [n, C] (float32, bfloat16 or float16, contiguous, 16-byte
        aligned) is x W without the bias, `params` the flat float32 tensor bias [C] | gamma [C] | beta [C]
        (mlp.param_layout), C one of 64, 128, 256, 512.  y [n, C] = leaky_relu(LayerNorm(z + bias), `slope`) in `y_dtype`
        (by default z's) is True (allocated) or a preallocated tensor.  stream=None blocks; a torch.cuda.Stream or raw
        handle enqueues there without synchronising.  Returns {"y": tensor}."""
        from . import mlp as _mlp
        return _mlp.compute(self, z, params, stream, channels=channels, eps=eps, slope=slope, y=y, y_dtype=y_dtype)

    def dense_norm_act_backward(self, z, params, grad_y, *, channels=None, eps=1e-6, slope=0.01, grad_z=True, grad_params=True, stream=None):
        """The gradients of dense_norm_act in one kernel plus a fixed-order sum (hs_dense_norm_act_backward): recomputed
        from the forward's z and params, with the upstream `grad_y` [n, C] (float32, bfloat16 or float16).  grad_z [n, C]
        in z's dtype and grad_params [3 C] float32 are each True, a tensor or None.  The same inputs give the same bits
        on every call.  Returns {name: tensor} of what was written."""
        from . import mlp as _mlp
        return _mlp.compute_backward(self, z, params, grad_y, stream, channels=channels, eps=eps, slope=slope, grad_z=grad_z,
                                     grad_params=grad_params)

    def attend_entities(self, qkv, key_mask=None, *, out=True, out_dtype=None, stream=None):
        """The attention core of the entity self-attention encoder in one kernel (gpu_hideseek.entity_attention;
        hs_entity_attend, whose header comment states the arithmetic: IEEE f32 in a fixed order).  `qkv`
        [n, 17, 3, 4, D] (float32, bfloat16 or float16, contiguous, 16-byte aligned; D 16 or 32) is the QKV GEMM's
        result viewed, `key_mask` [n, 17] uint8 (nonzero = the key counts; token 0 always does) or None.  out [n, 17, 4 D]
        in `out_dtype` (by default qkv's) is True (allocated) or a preallocated tensor.  stream=None blocks; a
        torch.cuda.Stream or raw handle enqueues there without synchronising.  Returns {"out": tensor}."""
        from . import entity_attention as _att
        return _att.compute(self, qkv, key_mask, stream, out=out, out_dtype=out_dtype)

    def attend_entities_backward(self, qkv, key_mask, grad_out, *, grad_qkv=True, stream=None):
        """The gradient of attend_entities in one kernel (hs_entity_attend_backward): recomputed from the forward's qkv
        and key_mask, with the upstream `grad_out` [n, 17, 4 D].  grad_qkv has qkv's shape and grad_out's dtype; a masked
        key's dk and dv are +0.  The same inputs give the same bits on every call.  Returns {"grad_qkv": tensor}."""
        from . import entity_attention as _att
        return _att.compute_backward(self, qkv, key_mask, grad_out, stream, grad_qkv=grad_qkv)

    def adam_step(self, params, grads, m, v, state, *, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=5.0, grad_scale=1.0,
                  zero_grad=True, stats=True, loss_scale=None, stream=None):
        """The clip by the global gradient norm and one Adam step over flat buffers in two kernels (gpu_hideseek.optim;
        hs_adam_step, whose header comment states the arithmetic: the norm in float64 and the update in IEEE f32, both in a
        fixed order).  `params`, `grads`, `m` and `v` are float32 [n], contiguous, 16-byte aligned and disjoint, updated in
        place; `state` is float64 [4] = beta1^t, beta2^t, t, skipped steps (optim.fresh_state()).  The gradients are taken as
        grads * grad_scale and scaled by max_grad_norm / norm when their norm exceeds max_grad_norm (<= 0 or None: no
        clip); a step whose norm is not finite changes nothing but the skip count.  With zero_grad the gradients are +0
        afterwards.  stats [4] float64 = norm, clip factor, skipped, t is True (allocated), a tensor or None.  With
        `loss_scale`, an optim.LossScale, the gradients are also divided by its scale, an overflow is skipped and the
        scale adjusted on the device (hs_adam_step_scaled).  stream=None
        blocks; a torch.cuda.Stream or raw handle enqueues there without synchronising.  The same inputs give the same
        bits on every call.  Returns {"stats": tensor} or {}.  optim.Adam is the torch optimiser built on this call."""
        from . import optim as _optim
        return _optim.compute(self, params, grads, m, v, state, stream, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                              max_grad_norm=max_grad_norm, grad_scale=grad_scale, zero_grad=zero_grad, stats=stats, loss_scale=loss_scale)

    def reduce_gradients(self, srcs, counts, out=None, total=None, stream=None):
        """The gradient of the mean over several shards' active samples from the shards' own flat gradient buffers, in one
        kernel (gpu_hideseek.optim; hs_reduce_gradients, whose header comment states the arithmetic: the weights
        counts[g] / sum(counts) in float64, the weighted sum in IEEE f32 in index order, a shard whose count is 0 left
        out).  `srcs` is a list of 1 to 16 float32 tensors [n], contiguous and 16-byte aligned, all on this handle's device;
        `counts` is float64 [len(srcs)].  `out` is None (allocated) or a float32 tensor [n] that is one of the sources
        or overlaps none; `total`, True or a float64 tensor [1], receives the sum of the counts.  stream=None blocks; a
        torch.cuda.Stream or raw handle enqueues there without synchronising.  The same inputs give the same bits on every
        call.  Returns {"out": tensor[, "total": tensor]}."""
        from . import optim as _optim
        return _optim.reduce_gradients(self, srcs, counts, out, total, stream)

    def gather_sequences(self, index, fields, *, chunks, chunk_steps, rows, bad=None, stream=None):
        """Cut the m sequences `index` (int32 [m] on the device; id = chunk * rows + row) out of a rollout of `chunks` x
        `chunk_steps` steps over `rows` rows, every field in one kernel (gpu_hideseek.rollout; hs_gather_sequences, whose
        header comment states the contract).  `fields` is a list of up to 16 (src, dst, per_chunk): a per-step src
        [chunks * chunk_steps, rows, ...] goes to dst [chunk_steps, m, ...] as dst[t, j] = src[k_j * chunk_steps + t, r_j],
        a per-chunk src [chunks, rows, ...] to dst [m, ...] as dst[j] = src[k_j, r_j]; dst None allocates it.  A pure copy
        of rows of a multiple of 4 bytes, bit-identical to torch indexing for every dtype; 16-byte accesses where a row is
        a multiple of 16 bytes and both bases are 16-byte aligned.  An id outside [0, chunks * rows) leaves zero rows and
        is counted in `bad` (True or an int32 [1] tensor); nothing is read out of range.  stream=None blocks; a
        torch.cuda.Stream or raw handle enqueues there without synchronising.  Returns {"fields": [dst, ...]} and "bad"
        when asked for.  rollout.Rollout.minibatch is the buffer built on this call."""
        from . import rollout as _rollout
        return _rollout.compute(self, index, fields, chunks, chunk_steps, rows, bad=bad, stream=stream)

    def episode_stats(self, state, table, *, gamma=0.998, reward=None, done=None, self_type=None, self_mask=None, episode_result=None,
                      hider_team=None, stream=None):
        """After a step: advance the per-row and per-world episode trackers `state` (episodes.new_state) and add every
        episode that ended with the step to `table` ([14] float64), in one kernel (gpu_hideseek.episodes;
        hs_episode_stats, whose header comment states the arithmetic and the table).  An input left None is the
        simulator's own export (hider_team: its team order); an explicit one is a contiguous tensor on the device.
        stream=None blocks; a torch.cuda.Stream or raw handle enqueues there without synchronising.  Returns
        {"table": table, "state": state}.  episodes.EpisodeStats is the tracker built on this call."""
        from . import episodes as _episodes
        return _episodes.compute(self, state, table, stream, gamma=gamma, reward=reward, done=done, self_type=self_type, self_mask=self_mask,
                                 episode_result=episode_result, hider_team=hider_team)

    def behaviour_stats(self, state, table, *, move_eps=0.5, positions=None, locks=None, counts=None, prep_counter=None, done=None, self_type=None,
                        self_mask=None, grabbing=None, stream=None):
        """After a step: advance the per-world behaviour trackers `state` (behaviour.new_state) and add every episode
        that ended with the step to `table` ([27] float64), in one kernel (gpu_hideseek.behaviour; hs_behaviour_stats,
        whose header comment states the arithmetic and the table): how far the boxes and ramps were moved in the
        preparation phase and after it, who had locked them when the seekers were released and at the end, how far each
        side travelled and how often it grabbed.  An input left None is the simulator's own (positions: the
        global_positions export; locks: the body metadata the lock columns of box_data / ramp_data export; counts: the
        world's boxes, ramps, hiders and seekers; grabbing: column 12 of self_data); an explicit one is a tensor on the
        device.  stream=None blocks; a torch.cuda.Stream or raw handle enqueues there without synchronising.  Returns
        {"table": table, "state": state}.  behaviour.BehaviourStats is the tracker built on this call."""
        from . import behaviour as _behaviour
        return _behaviour.compute(self, state, table, stream, move_eps=move_eps, positions=positions, locks=locks, counts=counts,
                                  prep_counter=prep_counter, done=done, self_type=self_type, self_mask=self_mask, grabbing=grabbing)

    def league_step(self, num_policies, team_size, state, counts, elo, *, k_factor=32.0, policy_assignments=None, slot=None, row_of_slot=None,
                    clear_slot=None, bad=None, done=None, self_type=None, self_mask=None, episode_result=None, hider_team=None, stream=None):
        """After a step, for a league of `num_policies` policies with `team_size` hiders and seekers per world: route every
        agent row to the policy of its side under the fixed schedule (world w plays pair w mod P^2), rank it among that
        policy's rows, add the games that ended with the step to `counts` ([P, P, 4] int64) and move the ratings `elo`
        ([P] float64), in one kernel and a one-workgroup fold (gpu_hideseek.league; hs_league_step, whose header comment
        is the contract).  `state` is league.new_state's.  policy_assignments None writes the simulator's own
        policy_assignments export; slot, row_of_slot, clear_slot (int32 [rows]) and bad (int32 [1]) are each None or a
        tensor.  An input left None is the simulator's own export (hider_team: its team order).  stream=None blocks; a
        torch.cuda.Stream or raw handle enqueues there without synchronising.  Returns {"counts", "elo", "state"} and the
        outputs given.  league.League is the evaluator built on this call."""
        from . import league as _league
        return _league.compute(self, num_policies, team_size, state, counts, elo, stream, k_factor=k_factor, policy_assignments=policy_assignments,
                               slot=slot, row_of_slot=row_of_slot, clear_slot=clear_slot, bad=bad, done=done, self_type=self_type,
                               self_mask=self_mask, episode_result=episode_result, hider_team=hider_team)

    def set_league_schedule(self, pairs, num_policies):
        """Give the handle the league schedule `pairs`, a list of (hider_policy, seeker_policy) over `num_policies`
        policies that league_step_scheduled then plays: world w plays pairs[w % len(pairs)] (hs_league_set_schedule, whose
        header comment is the contract; league.check_schedule states what makes a table valid, league.all_pairs_schedule
        and league.past_play_schedule build two).  pairs None drops the schedule.  After init(), outside an open step, and
        not while a league step of this handle is in flight; returns when the table is on the device.  Raises ValueError
        for a table that breaks a rule, before the library is involved.  league_step is not affected."""
        from . import league as _league
        return _league.set_schedule(self, pairs, num_policies)

    def league_step_scheduled(self, num_policies, team_size, state, counts, elo, *, k_factor=32.0, policy_assignments=None, slot=None, row_of_slot=None,
                              clear_slot=None, bad=None, done=None, self_type=None, self_mask=None, episode_result=None, hider_team=None, stream=None):
        """league_step under the schedule set_league_schedule gave the handle (hs_league_step_scheduled): `num_policies` is
        the schedule's, the number of worlds a multiple of its length, `counts` [N, N, 4] and `elo` [N]; everything else,
        the result included, is league_step's."""
        from . import league as _league
        return _league.compute_scheduled(self, num_policies, team_size, state, counts, elo, stream, k_factor=k_factor, policy_assignments=policy_assignments,
                                         slot=slot, row_of_slot=row_of_slot, clear_slot=clear_slot, bad=bad, done=done, self_type=self_type,
                                         self_mask=self_mask, episode_result=episode_result, hider_team=hider_team)

    def step_begin(self):
        """Enqueue one step on this handle's own stream and return (hs_step_begin); pair with step_end()."""
        _check(self._L.hs_step_begin(self._h))

    def step_end(self):
        """Wait for the step started by step_begin() and report device-side failures (hs_step_end)."""
        _check(self._L.hs_step_end(self._h))

    def step_async(self, hip_stream):
        """Enqueue one step on a caller-owned HIP stream (Manager::gpuJAXStep, mgr.cpp:1006-1022)."""
        _check(self._L.hs_step_async(self._h, C.c_void_p(int(hip_stream))))

    def _tensor(self, name):
        t = self._tensors.get(name)
        if t is None:
            d = _HsTensorDesc()
            _check(self._L.hs_get_tensor(self._h, _EXPORTS[name], C.byref(d)))
            t = self._tensors[name] = Tensor(weakref.proxy(self), d)
        return t

    # reset_tensor(), action_tensor(), ...: _tensor_getters

    def trigger_reset(self, world_idx, level_idx):
        _check(self._L.hs_trigger_reset(self._h, int(world_idx), int(level_idx)))

    def set_action(self, agent_idx, x, y, r, g, l):
        _check(self._L.hs_set_action(self._h, int(agent_idx), int(x), int(y), int(r), int(g), int(l)))

    # ---- checkpoints: Manager::saveCheckpoint / loadCheckpoint / loadCheckpoints (mgr.cpp:905-985) ----
    def save_checkpoint(self, world_idx):
        _check(self._L.hs_save_checkpoint(self._h, int(world_idx)))

    def load_checkpoint(self, world_idx):
        _check(self._L.hs_load_checkpoint(self._h, int(world_idx)))

    def load_checkpoints(self):
        """Run the LoadCheckpoints graph for the triggers currently in ckpt_ctrl_tensor()."""
        _check(self._L.hs_load_checkpoints(self._h))

    def save_checkpoints(self):
        """Run the SaveCheckpoints graph for the triggers currently in ckpt_ctrl_tensor()."""
        _check(self._L.hs_save_checkpoints(self._h))

    # ---- the XLA-callable stream functions behind sim.jax() (bindings.cpp:97-118, mgr.cpp:362-436) ----
    # `buffers`: device pointers (ints) or objects with .data_ptr(), in the reference's order
    # (include/hideseek.h hs_jax_*).  Nothing is synchronised except stream_init.
    def _stream_call(self, fn, hip_stream, buffers):
        ptrs = [int(b.data_ptr()) if hasattr(b, "data_ptr") else int(b) for b in buffers]
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        _check(fn(self._h, C.c_void_p(int(hip_stream)), arr))

    def stream_init(self, hip_stream, buffers):
        if len(buffers) != 11:
            raise ValueError("stream_init takes the 11 observation buffers")
        self._stream_call(self._L.hs_jax_init, hip_stream, buffers)

    def stream_step(self, hip_stream, buffers):
        if len(buffers) != 17:
            raise ValueError("stream_step takes actions, resets, policy_assignments, 11 observation buffers, "
                             "rewards, dones, episode_results")
        self._stream_call(self._L.hs_jax_step, hip_stream, buffers)

    def stream_save_checkpoints(self, hip_stream, buffers):
        if len(buffers) != 2:
            raise ValueError("stream_save_checkpoints takes ckpt_ctrl, ckpts")
        self._stream_call(self._L.hs_jax_save_checkpoints, hip_stream, buffers)

    def stream_load_checkpoints(self, hip_stream, buffers):
        if len(buffers) != 13:
            raise ValueError("stream_load_checkpoints takes ckpt_ctrl, ckpts, 11 observation buffers")
        self._stream_call(self._L.hs_jax_load_checkpoints, hip_stream, buffers)

    def train_interface(self):
        """Manager::trainInterface (mgr.cpp:1338-1375) bound to this simulator: {role: {name: Tensor}} with the
        reference's names and order — what `sim.jax()` hands to the learner."""
        out = {}
        for name, role, getter in train_interface():
            out.setdefault(role, {})[name] = getattr(self, getter)() if getter else None
        return out

    # ---- XLA custom calls (bindings.cpp:97-118: madrona::py::JAXInterface::buildEntry) ----
    def xla_opaque(self):
        """The descriptor an XLA custom call of this simulator carries: the 8 bytes of the native handle."""
        return int(self._h.value).to_bytes(8, "little")

    def xla_custom_call_targets(self):
        """{'init' | 'step' | 'save_ckpts' | 'load_ckpts': PyCapsule("xla._CUSTOM_CALL_TARGET")} around the native
        hs_xla_* functions (include/hideseek.h) — what xla_client.register_custom_call_target(name, capsule,
        platform="ROCM") takes."""
        new = C.pythonapi.PyCapsule_New
        new.restype = C.py_object
        new.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        return {k: new(C.cast(getattr(self._L, sym), C.c_void_p).value, b"xla._CUSTOM_CALL_TARGET", None)
                for k, sym in _native.XLA_TARGETS.items()}

    def xla_call_signatures(self):
        """Operand and result lists (name, shape, dtype) of the four custom calls, in buffer order
        (mgr.cpp:168-201, 362-436) — what a lowering rule needs besides the target and the opaque."""
        iface = self.train_interface()

        def sig(t):
            return (tuple(t.shape), t.dtype)
        obs = [(n, *sig(t)) for n, t in iface["observations"].items()]
        act = [("actions", *sig(self.action_tensor())), ("resets", *sig(self.reset_tensor())),
               ("policy_assignments", *sig(self.policy_assignments_tensor()))]
        out = [("rewards", *sig(self.reward_tensor())), ("dones", *sig(self.done_tensor())),
               ("episode_results", *sig(self.episode_result_tensor()))]
        ck = [("ckpt_ctrl", *sig(self.ckpt_ctrl_tensor())), ("ckpts", *sig(self.ckpt_tensor()))]
        return {"init": {"operands": [], "results": obs},
                "step": {"operands": act, "results": obs + out},
                "save_ckpts": {"operands": ck[:1], "results": ck[1:]},
                "load_ckpts": {"operands": ck, "results": obs}}

    def jax(self, jax_gpu):
        """bindings.cpp:97-118 (JAXInterface::buildEntry).  Everything XLA needs exists natively: the interface table
        (hs_train_interface), the four custom-call targets in XLA's own ABI (hs_xla_init / step / save_checkpoints /
        load_checkpoints — xla_custom_call_targets()), their descriptor (xla_opaque()) and their operand / result
        lists (xla_call_signatures()).  With jaxlib importable the targets are registered for the ROCm platform and
        the bundle is returned; without it (this image and the target: SURVEY §7 H8) the same bundle travels on the
        NotImplementedError, because the JAX-side lowering rules cannot be exercised here."""
        if not jax_gpu:
            raise NotImplementedError("sim.jax(jax_gpu=False): there is no CPU execution path (DESIGN.md §1)")
        bundle = {"train_interface": self.train_interface(), "targets": self.xla_custom_call_targets(),
                  "opaque": self.xla_opaque(), "signatures": self.xla_call_signatures(),
                  # one set of names per process: the targets are the same native functions for every simulator,
                  # the opaque descriptor says which one is meant
                  "target_names": {k: f"gpu_hideseek_{k}" for k in _native.XLA_TARGETS}}
        try:
            from jax.lib import xla_client
        except ImportError:
            err = NotImplementedError(
                "sim.jax(): jaxlib is not importable (SURVEY §7 H8), so the XLA custom-call targets cannot be "
                "registered here. They exist natively (hs_xla_*); the bundle a registration needs — capsules, "
                "opaque descriptor, operand / result signatures, interface table — is attached as .xla and "
                ".train_interface; stream_init / stream_step / ... call the same functions directly, and "
                "Tensor.to_jax() hands buffers over through DLPack.")
            err.train_interface = bundle["train_interface"]
            err.xla = bundle
            raise err
        global _xla_registered
        if not _xla_registered:
            for k, cap in bundle["targets"].items():
                xla_client.register_custom_call_target(bundle["target_names"][k], cap, platform="ROCM")
            _xla_registered = True
        return bundle

    def device_status(self):
        """hs_get_device_status: sticky device-side counters — candidate pairs that took the spill path of the physics
        kernel (beyond its LDS capacities; results unaffected), dropped pairs (always 0); graphs_in_use is always False;
        split_steps: blocking steps that ran as two chains of late and early octets, late_octets: the octets of their late
        groups summed over those steps (set_late_threshold)."""
        st = _native.HsDeviceStatus()
        _check(self._L.hs_get_device_status(self._h, C.byref(st)))
        return {"dropped_dd_pairs": int(st.dropped_dd_pairs), "dropped_static_pairs": int(st.dropped_static_pairs),
                "dropped_candidate_pairs": int(st.dropped_dd_pairs + st.dropped_static_pairs),
                "spilled_dd_pairs": int(st.spilled_dd_pairs), "spilled_static_pairs": int(st.spilled_static_pairs),
                "spilled_candidate_pairs": int(st.spilled_dd_pairs + st.spilled_static_pairs),
                "graphs_in_use": bool(st.graphs_in_use),
                "split_steps": int(st.split_steps), "late_octets": int(st.late_octets)}

    def set_late_threshold(self, factor):
        """hs_set_late_threshold: the one tunable of the split schedule of the blocking step().  An octet (8 worlds, one
        physics wave) whose mean time over the last two steps exceeded `factor` x the mean over all octets is in the late
        group of the next step.  0: every octet is late; float("inf"): none is.  Results do not depend on it."""
        _check(self._L.hs_set_late_threshold(self._h, float(factor)))

    def warning(self):
        """The library's last message for this thread."""
        return self._L.hs_last_error().decode()

    # ---- parity-test hooks (include/hideseek.h hs_debug_dump_*) ----
    def debug_bodies(self):
        import numpy as np
        b = np.zeros((self.num_worlds, 17, 13), np.float32)
        m = np.zeros((self.num_worlds, 17, 3), np.int32)
        _check(self._L.hs_debug_dump_bodies(self._h, b.ctypes.data, m.ctypes.data))
        return b, m

    def debug_walls(self):
        import numpy as np
        w = np.zeros((self.num_worlds, 36, 4), np.float32)
        info = np.zeros((self.num_worlds, 8), np.int32)
        _check(self._L.hs_debug_dump_walls(self._h, w.ctypes.data, info.ctypes.data))
        return w, info

    def set_profiling(self, enabled):
        _check(self._L.hs_set_profiling(self._h, int(bool(enabled))))

    def last_step_kernel_ms(self):
        out = (C.c_float * 3)()
        _check(self._L.hs_last_step_kernel_ms(self._h, C.byref(out)))
        return {"physics": out[0], "reset": out[1], "observe": out[2]}


from .sharded import ShardedSimulator  # noqa: E402
