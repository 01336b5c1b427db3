"""The reference's make_policy (scripts/jax_policy.py) as torch modules, assembled from the project's own: an actor
backbone and a separate critic backbone (BackboneSeparate), each the entity encoder (SimpleNet's first layer), the MLP of
three layers of 256 channels and the recurrent core (an LSTM of 256 hidden channels and its LayerNorm), and the two heads
on top: the multi-discrete actor's 5 + 5 + 5 + 2 + 2 logits and the two-hot critic's 255 bins.

    net = policy.make_policy(torch.bfloat16).cuda()
    state = net.init_state(rows, "cuda")
    for t in range(T):                                                   # the rollout
        sim.step()
        sim.pack_policy_inputs(actor=actor[t], critic=critic[t])
        done = sim.done_tensor().to_torch().reshape(rows)
        with torch.no_grad():
            logits, critic_logits, state = net(sim, actor[t], critic[t], state, clear=done)
    logits, critic_logits, _ = net.sequence(sim, actor, critic, state0, clears)      # a BPTT chunk, [T, rows, ...]

Composition only: this file contains no kernel call of its own.  Every piece runs its fused kernels on `sim`'s device
(entity_encoder, mlp, recurrent); with fused=False every piece runs its eager() in plain torch on the same parameters
(then `sim` is not used and may be None), for the tests and tools/mlp_bench.py.

In a chunk the encoder and the MLP do not depend on time: sequence() runs them once over the T * n flattened rows and
only the LSTM step by step.
"""
from . import entity_attention, entity_encoder, hash_encoder, mlp, recurrent
from ._request import _module_base

ENCODERS = ("simple", "attention", "hash")      # the reference's SimpleNet, its EntitySelfAttentionNet and its HashNet
BUCKETS = (5, 5, 5, 2, 2)     # the reference's action heads: move amount, move angle, rotate, grab, lock
BINS = 255                    # the two-hot critic's bins (value_head)


class Backbone(_module_base()):
    """EntityEncoder(embed) -> MLP(4 * embed, channels, layers) -> LSTMCore(channels, hidden) over k_pack's rows.  The
    compute dtype is the one the state's h carries: the encoder writes its features in it, and the GEMMs run in it.
    With encoder="attention" the backbone is entity_attention.AttentionEncoder(embed, channels) -> LSTMCore(channels,
    hidden) with no MLP in between: the reference's EntitySelfAttentionNet stands in place of all of SimpleNet, and its
    output channels feed the LSTM.  `masked` says whether the rows' entity tables carry their visibility masks (the
    actor's do, the critic's do not): the attention encoder leaves the masked-out entities out.
    With encoder="hash" it is hash_encoder.HashEncoder() -> LSTMCore(32, hidden), again with no MLP: the reference's
    HashNet stands in place of all of SimpleNet and its 32 channels feed the LSTM.  `channels`, the width that feeds the
    LSTM, must then be hash_encoder.FEATURES = 32 (make_policy passes it; the default of 256 is refused, not silently
    replaced); `embed` and `layers` are not used."""

    def __init__(self, embed=64, channels=256, layers=3, hidden=256, fused=True, generator=None, encoder="simple", masked=False):
        super().__init__()
        if encoder not in ENCODERS:
            raise ValueError(f"encoder must be one of {ENCODERS}, got {encoder!r}")
        self.fused, self.kind, self.masked = bool(fused), encoder, bool(masked)
        if encoder == "attention":
            self.encoder = entity_attention.AttentionEncoder(embed, channels, fused=fused, generator=generator)
        elif encoder == "hash":
            if channels != hash_encoder.FEATURES:
                raise ValueError(f"encoder 'hash' feeds the LSTM {hash_encoder.FEATURES} channels (hash_encoder.FEATURES): channels must be "
                                 f"{hash_encoder.FEATURES}, got {channels}")
            self.encoder = hash_encoder.HashEncoder(generator=generator)
        else:
            self.encoder = entity_encoder.EntityEncoder(embed, generator=generator)
            self.mlp = mlp.MLP(4 * embed, channels, layers, fused=fused, generator=generator)
        self.core = recurrent.LSTMCore(channels, hidden, generator=generator)

    def set_fused(self, fused):
        """Switch every piece between its kernels and its eager() on the same parameters."""
        self.fused = bool(fused)
        if self.kind == "attention":
            self.encoder.fused = self.fused
        elif self.kind == "simple":
            self.mlp.fused = self.fused
        return self

    def init_state(self, n, device, dtype=None):
        """(h [n, hidden] zeros in `dtype` (float32 by default), c [n, hidden] float32 zeros)."""
        return self.core.init_state(n, device, dtype)

    def features(self, sim, rows, dtype):
        """The encoder and the MLP over rows [n, W]: [n, channels] in `dtype`.  They carry no state."""
        if self.kind == "attention":
            return self.encoder(sim, rows, dtype, self.masked)
        if self.kind == "hash":
            if self.fused:
                return self.encoder(sim, rows, dtype)
            return hash_encoder.eager(rows, self.encoder.params, self.encoder.eps).to(dtype)
        if self.fused:
            feats = self.encoder(sim, rows, dtype)
        else:
            feats = entity_encoder.eager(rows, self.encoder.params, self.encoder.embed_dim, self.encoder.eps, self.encoder.slope).to(dtype)
        return self.mlp(sim, feats)

    def forward(self, sim, rows, state, clear=None):
        """One step: rows [n, W], state (h, c), clear [n] int32 or None -> (y [n, hidden], the new state)."""
        x = self.features(sim, rows, state[0].dtype)
        if self.fused:
            return self.core(sim, x, state, clear)
        ys, state = self._eager_steps(x.unsqueeze(0), state, None if clear is None else clear.reshape(1, -1))
        return ys[0], state

    def sequence(self, sim, rows, state, clears=None):
        """A chunk: rows [T, n, W], clears [T, n] int32 or None -> (ys [T, n, hidden], the final state).  The encoder and
        the MLP run once over the T * n flattened rows, the LSTM over the T steps."""
        T, n = rows.shape[0], rows.shape[1]
        xs = self.features(sim, rows.reshape(T * n, rows.shape[2]), state[0].dtype).reshape(T, n, -1)
        if self.fused:
            return self.core.sequence(sim, xs, state, clears)
        return self._eager_steps(xs, state, clears)

    def _eager_steps(self, xs, state, clears):
        h, c = state
        ys, (h2, c2) = recurrent.eager_sequence(xs, self.core.w_in, self.core.w_rec, self.core.cell_params, (h, c), clears, self.core.eps)
        return ys.to(h.dtype), (h2.to(h.dtype), c2)


class ActorCritic(_module_base()):
    """An actor Backbone and a separate critic Backbone (the reference's BackboneSeparate) and the two heads:
    actor_head Linear(hidden, sum(buckets)), orthogonal with gain 0.01 and a zero bias, and critic_head
    Linear(hidden, bins), zero-initialised as DreamerV3's two-hot head is, so that a fresh critic predicts 0.  Both
    initialisers are the project's choices: madrona_learn's heads are not part of the reference's tree and pin neither.
    The heads run in the dtype of the backbones' output.  state = (actor_state, critic_state), each (h, c)."""

    def __init__(self, buckets=BUCKETS, bins=BINS, dtype=None, generator=None, **backbone_kw):
        import torch
        super().__init__()
        self.buckets, self.bins = tuple(int(b) for b in buckets), int(bins)
        self.dtype = torch.float32 if dtype is None else dtype
        self.actor = Backbone(generator=generator, masked=True, **backbone_kw)
        self.critic = Backbone(generator=generator, masked=False, **backbone_kw)
        self.encoder = self.actor.kind
        hidden = self.actor.core.hidden
        self.actor_head = torch.nn.Linear(hidden, sum(self.buckets))
        self.critic_head = torch.nn.Linear(hidden, self.bins)
        with torch.no_grad():
            torch.nn.init.orthogonal_(self.actor_head.weight, gain=0.01, generator=generator)
            self.actor_head.bias.zero_()
            self.critic_head.weight.zero_()
            self.critic_head.bias.zero_()

    def set_fused(self, fused):
        """Switch both backbones between their kernels and their eager() on the same parameters."""
        self.actor.set_fused(fused)
        self.critic.set_fused(fused)
        return self

    def init_state(self, n, device, dtype=None):
        """((h, c) of the actor, (h, c) of the critic): zeros, h in `dtype` (by default the policy's compute dtype)."""
        dtype = self.dtype if dtype is None else dtype
        return self.actor.init_state(n, device, dtype), self.critic.init_state(n, device, dtype)

    @staticmethod
    def _head(head, y):
        """A head on a backbone's output, in the output's dtype."""
        import torch
        return torch.nn.functional.linear(y, head.weight.to(y.dtype), head.bias.to(y.dtype))

    def actor_logits(self, sim, rows, state, clear=None):
        """One step of the actor alone: rows [n, W], state the actor's (h, c) -> (logits [n, sum(buckets)], the new actor state)."""
        y, state = self.actor(sim, rows, state, clear)
        return self._head(self.actor_head, y), state

    def critic_logits(self, sim, rows, state, clear=None):
        """One step of the critic alone: rows [n, W], state the critic's (h, c) -> (critic_logits [n, bins], the new critic state)."""
        y, state = self.critic(sim, rows, state, clear)
        return self._head(self.critic_head, y), state

    def forward(self, sim, actor_rows, critic_rows, state, clear=None):
        """One step -> (logits [n, sum(buckets)], critic_logits [n, bins], the new state)."""
        ya, sa = self.actor(sim, actor_rows, state[0], clear)
        yc, sc = self.critic(sim, critic_rows, state[1], clear)
        return self._head(self.actor_head, ya), self._head(self.critic_head, yc), (sa, sc)

    def sequence(self, sim, actor_rows, critic_rows, state, clears=None):
        """A chunk [T, n, W] -> (logits [T, n, sum(buckets)], critic_logits [T, n, bins], the final state)."""
        ya, sa = self.actor.sequence(sim, actor_rows, state[0], clears)
        yc, sc = self.critic.sequence(sim, critic_rows, state[1], clears)
        return self._head(self.actor_head, ya), self._head(self.critic_head, yc), (sa, sc)


def make_policy(dtype=None, fused=True, generator=None, encoder="simple"):
    """An ActorCritic of the reference's sizes: embed 64, three layers of 256 channels, 256 hidden channels, heads of
    5 + 5 + 5 + 2 + 2 logits and 255 bins.  `dtype` (float32 by default) is the compute dtype the state's h carries.
    encoder="attention" builds the reference's other network instead, EntitySelfAttentionNet(num_embed_channels=128,
    num_out_channels=256, num_heads=4), in front of the same LSTM and heads; encoder="hash" its HashNet (hash_power 8,
    feature_dim 32), whose 32 channels feed the LSTM."""
    if encoder not in ENCODERS:
        raise ValueError(f"encoder must be one of {ENCODERS}, got {encoder!r}")
    if encoder == "attention":
        return ActorCritic(BUCKETS, BINS, dtype=dtype, generator=generator, embed=128, channels=256, hidden=256, fused=fused, encoder="attention")
    if encoder == "hash":
        return ActorCritic(BUCKETS, BINS, dtype=dtype, generator=generator, channels=hash_encoder.FEATURES, hidden=256, fused=fused, encoder="hash")
    return ActorCritic(BUCKETS, BINS, dtype=dtype, generator=generator, embed=64, channels=256, layers=3, hidden=256, fused=fused)
