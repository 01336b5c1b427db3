"""Where an episode starts for the trainer's LSTM state, on the CPU: the rule of gpu_hideseek.rollout (state_zero_into,
chunk_clears) on hand-written done and mask arrays, and the episode loop that tests/test_gpu_trainer*.py hold the
trainer against.

The arrays restate what the simulator exports around an episode's end (8 worlds, seed 1, teams of 1..3 + 1..3): the
observation exported with done = 1 is the first one of the next episode; a row that joins exports done = 0 with it, or a
stale done = 1 if it was in an earlier episode and left; a row that leaves keeps done = 1 while it is out; a row that
stays out exports nothing new.  A row's memory is modelled by a sum of distinct powers of two, one per slot, so the
value that reaches a forward names every slot it remembers.
"""
import pytest
import torch

from gpu_hideseek import rollout

KINDS = ("stay", "join", "rejoin", "leave", "out")
T, K = 8, 2                   # one rollout: two chunks of four slots
L = T // K
SLOTS = 2 * T                 # two rollouts in a row


def exports(boundary, slots=SLOTS):
    """(clear, mask) [slots, 5] int32 / float32 of one row of every kind, the episode's first observation in slot
    `boundary`; clear[t] is the done export that comes with the observation of slot t."""
    clear = torch.zeros(slots, len(KINDS), dtype=torch.int32)
    mask = torch.zeros(slots, len(KINDS), dtype=torch.float32)
    t = torch.arange(slots)
    mask[:, 0] = 1.0
    clear[boundary, 0] = 1                                    # stay: done with the step that ended its episode, 0 again after
    mask[:, 1] = (t >= boundary).float()                      # join: never a done
    mask[:, 2] = (t >= boundary).float()
    clear[:, 2] = (t <= boundary).int()                       # rejoin: the stale done of the episode it left, up to its first step
    mask[:, 3] = (t < boundary).float()
    clear[:, 3] = (t >= boundary).int()                       # leave: its last done stays in the export
    return clear, mask


def remembered(boundary, slots=SLOTS):
    """[slots, 5] int64: what the forward of slot t must receive, as the sum of 2^s over the slots s < t of the same
    episode in which the row was active too; 0 at an episode's first active slot.  -1 where the row is out (not checked)."""
    _, mask = exports(boundary, slots)
    want = torch.full((slots, len(KINDS)), -1, dtype=torch.int64)
    for r in range(len(KINDS)):
        for t in range(slots):
            if mask[t, r] != 0:
                first = boundary if t >= boundary else 0
                want[t, r] = sum(1 << s for s in range(first, t) if mask[s, r] != 0)
    return want


def collect_model(clear, mask):
    """The carried state as collect() treats it, over rollouts of T slots: after every step (the closing step of a
    rollout is the one that leads to the next rollout's slot 0) the rule zeroes rows; a forward adds 2^t, for rows that
    are out as well, as the policy runs on every row.  Returns (what each forward received, the chunk-start states)."""
    state = torch.zeros(clear.shape[1], dtype=torch.int64)
    got, starts = [], []
    for t in range(clear.shape[0]):
        zero = rollout.state_zero_into(clear[t], mask[t], mask[t - 1] if t else mask[t])
        state = torch.where(zero, torch.zeros_like(state), state)
        if t % L == 0:
            starts.append(state.clone())
        got.append(state.clone())
        state = state + (1 << t)
    return torch.stack(got), torch.stack(starts)


def update_model(clear, mask, starts):
    """What each forward receives in the update: per chunk from its stored start, the recurrent core's meaning of clear
    (the state carried OUT of a step is zero where it is set) under chunk_clears()."""
    got = []
    for k in range(clear.shape[0] // L):
        sl = slice(k * L, (k + 1) * L)
        clears = rollout.chunk_clears(clear[sl], mask[sl])
        assert clears.dtype == torch.int32 and clears.shape == clear[sl].shape and not clears[-1].any()
        state = starts[k].clone()
        for i in range(L):
            got.append(state.clone())
            state = torch.where(clears[i] != 0, torch.zeros_like(state), state + (1 << (k * L + i)))
    return torch.stack(got)


@pytest.mark.parametrize("boundary", list(range(1, SLOTS)))
def test_the_state_into_an_episodes_first_slot_is_zero_and_carried_otherwise(boundary):
    """Every place of the boundary in two rollouts: mid-chunk, a chunk's first and last slot, the second rollout's slot 0."""
    clear, mask = exports(boundary)
    want = remembered(boundary)
    active = want >= 0
    assert (want[boundary][[0, 1, 2]] == 0).all() and (want[boundary - 1][[0, 3]] == (1 << (boundary - 1)) - 1).all()
    got, starts = collect_model(clear, mask)
    assert torch.equal(got[active], want[active]), (got, want)
    assert torch.equal(starts, got[::L])
    again = update_model(clear, mask, starts)
    assert torch.equal(again[active], want[active]), (again, want)
    # a row that is out carries zero into every forward, in both paths
    assert not got[~active].any() and not again[~active].any()


def test_the_rule_on_single_rows():
    z = lambda c, m, b: bool(rollout.state_zero_into(torch.tensor([c]), torch.tensor([float(m)]), torch.tensor([float(b)]))[0])  # noqa: E731
    assert not z(0, 1, 1)                         # inside an episode
    assert z(1, 1, 1)                             # done with this observation: the episode's first
    assert z(0, 1, 0)                             # joins: no done
    assert z(1, 0, 1) and z(0, 0, 0) and z(1, 0, 0)          # out, whatever the stale done says
    one = rollout.chunk_clears(torch.ones(1, 3, dtype=torch.int32), torch.ones(1, 3))
    assert one.shape == (1, 3) and not one.any()


# ---- the episode loop: the reference of the GPU tests ----
def zero_in(mask, critic):
    """The loop's own rule, from what a slot stores and from neither done nor clear: zero the state into slot t where the
    row is out or its observation is an episode's first (prep_counter = 96).  Column 0 of a packed row is
    prep_counter / 96 (hs_k_pack.h), which no normaliser touches; it must be a whole count in [0, 96]."""
    p = critic[..., 0].double() * 96.0
    prep = p.round()
    assert float((p - prep).abs().max()) < 1e-4 and float(prep.min()) >= 0 and float(prep.max()) <= 96, (p.min(), p.max())
    return (mask == 0) | (prep == 96)


def episode_loop(net, actor, critic, zero, state):
    """net (eager pieces, on the CPU) over slots [S, n, 296] from `state`, with no clear: (logits [S, n, .],
    critic_logits [S, n, .], the state each forward received)."""
    lg, cl, received = [], [], []
    for t in range(actor.shape[0]):
        z = zero[t].unsqueeze(1)
        state = tuple(tuple(torch.where(z, torch.zeros_like(x), x) for x in s) for s in state)
        received.append(state)
        a, c, state = net(None, actor[t], critic[t], state, None)
        lg.append(a)
        cl.append(c)
    return torch.stack(lg), torch.stack(cl), received


def toy_policy():
    from gpu_hideseek import policy as P
    net = P.ActorCritic(generator=torch.Generator().manual_seed(21), embed=32, channels=64, layers=2, hidden=64, fused=False).double()
    with torch.no_grad():
        net.critic_head.weight.copy_(0.05 * torch.randn(net.critic_head.weight.shape, generator=torch.Generator().manual_seed(22)))
    return net


def trainer_paths(net, actor, critic, clear, mask, chunk):
    """The trainer's two paths on the CPU: the chunk-start states as collect() carries them (the rule after every step,
    a forward with no clear), then every chunk's logits as the update recomputes them from those states
    (net.sequence under chunk_clears)."""
    state = net.init_state(actor.shape[1], "cpu", torch.float64)
    starts = []
    for t in range(actor.shape[0]):
        z = rollout.state_zero_into(clear[t], mask[t], mask[t - 1] if t else mask[t]).unsqueeze(1)
        state = tuple(tuple(torch.where(z, torch.zeros_like(x), x) for x in s) for s in state)
        if t % chunk == 0:
            starts.append(state)
        _, _, state = net(None, actor[t], critic[t], state, None)
    lg, cl = [], []
    for k, s0 in enumerate(starts):
        sl = slice(k * chunk, (k + 1) * chunk)
        a, c, _ = net.sequence(None, actor[sl], critic[sl], s0, rollout.chunk_clears(clear[sl], mask[sl]))
        lg.append(a)
        cl.append(c)
    return torch.cat(lg), torch.cat(cl)


@pytest.mark.parametrize("boundary", [2, 3, 4])       # a chunk's last slot, a chunk's first slot, mid-chunk
def test_no_input_before_the_boundary_reaches_a_logit_after_it(boundary):
    """A 2-chunk toy sequence (6 slots in chunks of 3, a row of every kind) through the trainer's two paths in float64:
    a central difference of a logit at the episode's first slot in an input of the slot before is exactly zero, and in
    an input of the same episode it is not; the paths agree with the episode loop."""
    S, chunk, n, eps = 6, 3, len(KINDS), 1e-3
    net = toy_policy()
    g = torch.Generator().manual_seed(5 + boundary)
    actor, critic = (torch.randn(S, n, 296, generator=g, dtype=torch.float64) for _ in range(2))
    clear, mask = exports(boundary, S)

    def logits(t_in, row, delta):
        a, c = actor.clone(), critic.clone()
        a[t_in, row] += delta
        c[t_in, row] += delta
        with torch.no_grad():
            return trainer_paths(net, a, c, clear, mask, chunk)

    def sensitivity(t_in, t_out, row):
        (pa, pc), (ma, mc) = logits(t_in, row, eps), logits(t_in, row, -eps)
        return float(((pa - ma)[t_out, row] / (2 * eps)).abs().max()), float(((pc - mc)[t_out, row] / (2 * eps)).abs().max())

    stay, leave = KINDS.index("stay"), KINDS.index("leave")
    assert sensitivity(boundary - 1, boundary, stay) == (0.0, 0.0)                      # across the boundary: nothing
    assert all(s == (0.0, 0.0) for s in (sensitivity(t, boundary, stay) for t in range(boundary - 1)))
    for t_in, t_out, row in ((boundary, boundary + 1, stay), (boundary, S - 1, stay), (0, boundary - 1, stay), (0, boundary - 1, leave),
                             (boundary, boundary + 1, KINDS.index("join")), (boundary, S - 1, KINDS.index("rejoin"))):
        sa, sc = sensitivity(t_in, t_out, row)
        assert sa > 1e-6 and sc > 1e-6, (t_in, t_out, row, sa, sc)                       # inside an episode, chunk starts included
    # what a row that is out saw before it joins does not reach its first slot either
    for row in (KINDS.index("join"), KINDS.index("rejoin")):
        assert sensitivity(boundary - 1, boundary, row) == (0.0, 0.0)
    # and the two paths are the episode loop, which knows neither done nor clear
    first = torch.zeros(S, n, dtype=torch.bool)
    first[boundary] = True
    with torch.no_grad():
        la, lc, _ = episode_loop(net, actor, critic, (mask == 0) | first, net.init_state(n, "cpu", torch.float64))
        ta, tc = trainer_paths(net, actor, critic, clear, mask, chunk)
    active = mask != 0
    # (sequence() runs the encoder and the MLP over all slots at once: float64 rounding of another batching, no more)
    assert float((ta - la)[active].abs().max()) < 1e-12 and float((tc - lc)[active].abs().max()) < 1e-12
