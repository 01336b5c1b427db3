"""What the training drivers share, as far as it can be checked without a GPU: league.Table's refusals and its packed
table, the policy's actor-only and critic-only steps against forward(), episodes.step_trackers, and the two small helpers
of gpu_hideseek.rollout the drivers zero and snapshot their carried LSTM states with."""
import pytest
import torch


class _Sim:
    """8 worlds of 2 + 2 agents; it has no set_league_schedule: a refusal comes before the schedule is set."""
    num_worlds, agents_per_world, gpu_id = 8, 4, 0


def test_the_league_table_refuses_the_shape_then_k_factor_before_anything_touches_a_device():
    from gpu_hideseek import league as G
    bad = [
        (dict(P=0), "num_policies"), (dict(P=17), "num_policies"), (dict(P=True), "num_policies"), (dict(k=1), "team_size"), (dict(k=2.0), "team_size"),
        (dict(P=3), "multiple of num_policies\\^2"),
        (dict(P=0, k=1, k_factor=0.0), "num_policies"),                      # the policies before the teams before k_factor
        (dict(k=1, k_factor=0.0), "team_size"), (dict(P=3, k_factor=0.0), "multiple of num_policies\\^2"),
        (dict(k_factor=0.0), "k_factor"), (dict(k_factor=float("nan")), "k_factor"), (dict(k_factor=float("inf")), "k_factor"),
        # with a schedule the shape rule is the group's: P = 3 passes it with G = 8, and 8 worlds are no multiple of G = 3
        (dict(P=3, schedule=[(0, 1)] * 8, k_factor=0.0), "k_factor"), (dict(schedule=[(0, 1)] * 3), "multiple of the schedule's group = 3"),
        (dict(schedule=[(0, 1)] * 257), "group must be an integer in"), (dict(schedule=[(0, 1)] * 3, k_factor=0.0), "multiple of the schedule's group = 3"),
    ]
    for kw, what in bad:
        kw = dict(dict(P=2, k=2, k_factor=G.DEFAULT_K_FACTOR, schedule=None), **kw)
        with pytest.raises(ValueError, match=what):
            G.Table(_Sim(), kw["P"], kw["k"], kw["k_factor"], kw["schedule"])


@pytest.mark.parametrize("P", (1, 2, 3, 16))
def test_the_packed_tables_views_alias_one_buffer(P):
    from gpu_hideseek import league as G
    words = P * P * 4 + P + 1
    table = torch.zeros(words, dtype=torch.int64)
    counts, elo, bad_total = G.table_views(table, P)
    assert (counts.shape, counts.dtype) == ((P, P, 4), torch.int64) and (elo.shape, elo.dtype) == ((P,), torch.float64)
    assert (bad_total.shape, bad_total.dtype) == ((1,), torch.int64)
    base = table.data_ptr()
    assert counts.data_ptr() == base and elo.data_ptr() == base + 8 * P * P * 4 and bad_total.data_ptr() == base + 8 * (P * P * 4 + P)
    assert counts.numel() + elo.numel() + bad_total.numel() == words
    counts[P - 1, P - 1, 3] = 7
    elo.fill_(G.INITIAL_ELO)
    bad_total += 2
    assert table[P * P * 4 - 1] == 7 and table[-1] == 2
    assert table[P * P * 4:-1].view(torch.float64).tolist() == [1500.0] * P and not table[:P * P * 4 - 1].any()
    assert set(G.Table.TENSORS) == {"slot", "row_of_slot", "clear_slot", "bad", "world", "_table", "counts", "elo", "bad_total"}


def test_actor_logits_and_critic_logits_are_the_halves_of_forward():
    from gpu_hideseek import policy as P
    net = P.make_policy(fused=False, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        net.critic_head.weight.copy_(0.05 * torch.randn(net.critic_head.weight.shape, generator=torch.Generator().manual_seed(22)))
    n, rng = 7, torch.Generator().manual_seed(4)
    actor, critic = torch.randn(n, 296, generator=rng), torch.randn(n, 296, generator=rng)
    state = tuple((torch.randn(n, 256, generator=rng), torch.randn(n, 256, generator=rng)) for _ in range(2))
    for clear in (None, torch.tensor([0, 1, 0, 0, 1, 0, 0], dtype=torch.int32)):
        with torch.no_grad():
            logits, critic_logits, (sa, sc) = net(None, actor, critic, state, clear)
            a, a_state = net.actor_logits(None, actor, state[0], clear)
            c, c_state = net.critic_logits(None, critic, state[1], clear)
        assert bool(logits.any()) and bool(critic_logits.any())
        assert torch.equal(a, logits) and torch.equal(c, critic_logits)
        for got, want in zip(a_state + c_state, sa + sc):
            assert torch.equal(got, want)
    # a chunk of one step runs the same heads
    with torch.no_grad():
        seq, seq_critic, _ = net.sequence(None, actor.unsqueeze(0), critic.unsqueeze(0), state, None)
        logits, critic_logits, _ = net(None, actor, critic, state, None)
    assert torch.equal(seq[0], logits) and torch.equal(seq_critic[0], critic_logits)


def test_step_trackers_steps_none_one_and_lists_once_and_in_order():
    from gpu_hideseek.episodes import step_trackers
    calls = []

    class Tracker:
        def __init__(self, name):
            self.name = name

        def step(self):
            calls.append(self.name)

    step_trackers()
    step_trackers(None, None)
    assert calls == []
    step_trackers(Tracker("a"), None)
    assert calls == ["a"]
    step_trackers(None, [Tracker("b"), Tracker("c")], Tracker("d"), (Tracker("e"),), [])
    assert calls == ["a", "b", "c", "d", "e"]


def test_zero_where_and_snapshot_state():
    from gpu_hideseek import rollout

    class Sim:
        num_worlds, agents_per_world, gpu_id = 2, 3, 0

    xs = [torch.ones(4, 3), torch.full((4, 2), 2.0, dtype=torch.bfloat16)]
    rollout.zero_where(torch.tensor([True, False, False, True]), *xs)
    assert xs[0][:, 0].tolist() == [0.0, 1.0, 1.0, 0.0] and xs[1][:, 1].tolist() == [0.0, 2.0, 2.0, 0.0]
    buf = rollout.Rollout(Sim(), 4, 2, hidden=5, device="cpu")
    state = tuple((torch.full((6, 5), float(10 * b + 1)), torch.full((6, 5), float(10 * b + 2))) for b in range(2))
    buf.snapshot_state(1, state)
    for name, want in (("actor_h", 1.0), ("actor_c", 2.0), ("critic_h", 11.0), ("critic_c", 12.0)):
        assert not getattr(buf, name)[0].any() and bool((getattr(buf, name)[1] == want).all())
    part = tuple((h[:2] + 100, c[:2] + 100) for h, c in state)
    buf.snapshot_state(0, part, slice(2, 4))
    assert bool((buf.actor_h[0, 2:4] == 101.0).all()) and not buf.actor_h[0, :2].any() and not buf.actor_h[0, 4:].any()
    assert bool((buf.critic_c[0, 2:4] == 112.0).all()) and bool((buf.critic_c[1] == 12.0).all())
