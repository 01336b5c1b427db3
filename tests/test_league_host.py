"""What can be checked of the league (include/hideseek.h: hs_league_step; gpu_hideseek.league) without a GPU: the
refusals of league.request, the schedule, the properties of the routing and of the ratings as league.host_step restates
them in numpy, print_elos, and the agreement of the ctypes mirror with the header.  tests/test_gpu_league.py compares the
kernel with host_step on the synthetic steps made here."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = np.int32
RESULTS = np.array([1.0, 0.0, 0.5, 0.25, np.nan], np.float32)
ELO_TOL = 1e-6            # Elo points.  A pair's update carries a few ulp of E times k_factor * n, about 32 * 64 * 1e-15; at
#                           most 24 steps x 240 pairs of them accumulate, about 1e-8: two orders of margin remain.


def new_state(worlds):
    return dict(world_hider_team=np.zeros(worlds, I32), world_phase=np.zeros(worlds, I32))


def synthetic_steps(worlds, P, k, steps, seed):
    """`steps` calls' inputs for worlds x 2k rows: every world carries one done on all its rows and ends with probability
    1/6 per step (several worlds, and with worlds > P^2 several of one pair, in one step); at an end its rows are dealt
    anew into k hiders and k seekers in a random order and its team index is drawn; results come from RESULTS; some
    worlds are malformed for a step (one hider too many, or a masked row)."""
    rng = np.random.default_rng(seed)
    A = 2 * k
    types = np.tile((np.arange(A) < k).astype(I32), (worlds, 1))
    team = np.zeros(worlds, I32)
    out = []
    for _ in range(steps):
        ended = rng.random(worlds) < 1 / 6
        for w in np.flatnonzero(ended):
            types[w] = rng.permutation(types[w])
            team[w] = rng.integers(0, 2)
        st, mask = types.copy(), np.ones((worlds, A), np.float32)
        for w in np.flatnonzero(rng.random(worlds) < 0.08):
            if rng.random() < 0.5:
                st[w, np.flatnonzero(st[w] == 0)[0]] = 7          # k + 1 hiders, and a self_type that is not 1
            else:
                mask[w, rng.integers(0, A)] = 0.0
        out.append(dict(done=np.repeat(ended.astype(I32), A), self_type=st.reshape(-1).copy(), self_mask=mask.reshape(-1),
                        episode_result=rng.choice(RESULTS, (worlds, 2)).astype(np.float32), hider_team=team.copy()))
    return out


def host_run(worlds, P, k, calls, k_factor=32.0):
    """host_step over `calls` from a fresh state: (per-call results, state, counts, elo after every call)."""
    from gpu_hideseek import league as G
    st, counts, elo = new_state(worlds), np.zeros((P, P, 4), np.int64), np.full(P, 1500.0)
    res, elos = [], []
    for c in calls:
        r = G.host_step(st, counts, elo, P, k, c["done"], c["self_type"], c["self_mask"], c["episode_result"], c["hider_team"], k_factor)
        r.update(world_hider_team=st["world_hider_team"].copy(), world_phase=st["world_phase"].copy(), counts=counts.copy())
        res.append(r)
        elos.append(elo.copy())
    return res, st, counts, elos


# ---- the schedule and the routing ----
@pytest.mark.parametrize("worlds,P", [(1, 1), (8, 2), (27, 3), (256, 16)])
def test_schedule_gives_every_ordered_pair_the_same_number_of_worlds(worlds, P):
    from gpu_hideseek import league as G
    hp, sp = G.schedule(worlds, P)
    pairs = {}
    for h, s in zip(hp, sp):
        pairs[h, s] = pairs.get((h, s), 0) + 1
    assert pairs == {(i, j): worlds // (P * P) for i in range(P) for j in range(P)}
    for bad in ((7, 2), (4, 0), (4, 17), (0, 1)):
        with pytest.raises(ValueError, match="multiple"):
            G.schedule(*bad)


@pytest.mark.parametrize("worlds,P,k", [(1, 1, 1), (8, 2, 1), (18, 3, 3), (32, 4, 2)])
def test_routing_is_the_stable_sort_by_policy_and_survives_flips_and_malformed_worlds(worlds, P, k):
    from gpu_hideseek import league as G
    A, R = 2 * k, worlds * 2 * k
    calls = synthetic_steps(worlds, P, k, 30, seed=worlds)
    res, _, _, _ = host_run(worlds, P, k, calls)
    hp, sp = G.schedule(worlds, P)
    owned, bad_seen = None, 0
    for c, r in zip(calls, res):
        pol, slot = r["policy_assignments"], r["slot"]
        assert sorted(slot.tolist()) == list(range(R))
        inverse = np.empty(R, I32)
        inverse[np.argsort(pol, kind="stable")] = np.arange(R, dtype=I32)
        assert np.array_equal(slot, inverse)
        assert np.array_equal(r["row_of_slot"][slot], np.arange(R)) and np.array_equal(r["clear_slot"][slot], c["done"])
        assert np.bincount(pol, minlength=P).tolist() == [R // P] * P
        for p in range(P):
            assert ((slot[pol == p] >= p * (R // P)) & (slot[pol == p] < (p + 1) * (R // P))).all()
        # the policies of a world are those of its pair, and its set of slots never changes
        sets = [frozenset(slot[w * A:(w + 1) * A].tolist()) for w in range(worlds)]
        assert owned is None or sets == owned
        owned = sets
        st, mask = c["self_type"].reshape(worlds, A), c["self_mask"].reshape(worlds, A)
        malformed = ((st != 0).sum(1) != k) | (mask == 0).any(1)
        assert r["bad"] == int(malformed.sum())
        bad_seen += r["bad"]
        for w in range(worlds):
            side = (np.arange(A) < k) if malformed[w] else st[w] != 0
            assert np.array_equal(pol[w * A:(w + 1) * A], np.where(side, hp[w], sp[w]))
    assert bad_seen > 0 or worlds == 1
    assert len({tuple(c["self_type"]) for c in calls}) > 5 or worlds == 1


def test_a_malformed_world_raises_bad_and_still_yields_a_permutation():
    from gpu_hideseek import league as G
    P, k, worlds = 2, 2, 4
    R = worlds * 2 * k
    types = np.tile(np.array([1, 0, 1, 0], I32), worlds)
    ones, zero = np.ones(R, np.float32), np.zeros(R, I32)
    args = dict(episode_result=np.zeros((worlds, 2), np.float32), hider_team=np.zeros(worlds, I32))
    for name, st, mask in (("k + 1 hiders", np.where(np.arange(R) == 5, 1, types), ones), ("a masked row", types, np.where(np.arange(R) == 10, 0, ones))):
        r = G.host_step(new_state(worlds), np.zeros((P, P, 4), np.int64), np.full(P, 1500.0), P, k, zero, st.astype(I32), mask.astype(np.float32), **args)
        assert r["bad"] == 1 and sorted(r["slot"].tolist()) == list(range(R)), name
        w = 1 if name.startswith("k") else 2
        hp, sp = G.schedule(worlds, P)
        assert r["policy_assignments"][w * 4:(w + 1) * 4].tolist() == [hp[w], hp[w], sp[w], sp[w]], name


# ---- the table and the ratings ----
def _one_step(P, worlds, results, ended, elo=None, phase=1, k_factor=32.0, hider_team=0):
    """A step of worlds x 2 rows in which the worlds `ended` end with `results` [worlds] for the hiders (team index
    hider_team, latched when phase is 1)."""
    from gpu_hideseek import league as G
    st = dict(world_hider_team=np.full(worlds, hider_team, I32), world_phase=np.full(worlds, phase, I32))
    counts, elo = np.zeros((P, P, 4), np.int64), np.full(P, 1500.0) if elo is None else np.array(elo, np.float64)
    er = np.zeros((worlds, 2), np.float32)
    er[:, hider_team] = results
    er[:, 1 - hider_team] = 1.0 - np.asarray(results, np.float32)
    done = np.repeat(np.asarray(ended, I32), 2)
    G.host_step(st, counts, elo, P, 1, done, np.tile(np.array([1, 0], I32), worlds), np.ones(2 * worlds, np.float32), er, np.zeros(worlds, I32), k_factor)
    return counts, elo, st


def test_one_hider_win_between_equal_ratings_moves_them_by_half_the_k_factor_exactly():
    for kf in (32.0, 10.0):
        counts, elo, _ = _one_step(2, 4, [1.0] * 4, [0, 1, 0, 0], k_factor=kf)          # world 1: hiders 0, seekers 1
        assert counts[0, 1].tolist() == [1, 0, 0, 0] and counts.sum() == 1
        assert elo.tolist() == [1500.0 + kf / 2, 1500.0 - kf / 2]
    counts, elo, _ = _one_step(2, 4, [0.0] * 4, [0, 0, 1, 0])                           # world 2: hiders 1, seekers 0; the seekers win
    assert counts[1, 0].tolist() == [0, 1, 0, 0] and elo.tolist() == [1516.0, 1484.0]
    counts, elo, _ = _one_step(2, 4, [0.5] * 4, [0, 1, 1, 0])                           # two draws between equals
    assert counts[0, 1, 2] == 1 and counts[1, 0, 2] == 1 and elo.tolist() == [1500.0, 1500.0]
    # the latched team index picks the column of episode_result
    counts, elo, _ = _one_step(2, 4, [1.0] * 4, [0, 1, 0, 0], hider_team=1)
    assert counts[0, 1].tolist() == [1, 0, 0, 0] and elo.tolist() == [1516.0, 1484.0]


def test_self_matches_games_without_an_outcome_and_unlatched_worlds_move_nothing():
    start = [1400.0, 1650.0]
    counts, elo, _ = _one_step(2, 4, [1.0, 0.0, 0.5, 0.0], [1, 0, 0, 1], elo=start)      # worlds 0 and 3 play (0, 0) and (1, 1)
    assert counts[0, 0].tolist() == [1, 0, 0, 0] and counts[1, 1].tolist() == [0, 1, 0, 0] and elo.tolist() == start
    for x in (0.25, np.nan, 2.0, -1.0):
        counts, elo, _ = _one_step(2, 4, [x] * 4, [1, 1, 1, 1], elo=start)
        assert counts[:, :, 3].tolist() == [[1, 1], [1, 1]] and counts.sum() == 4 and elo.tolist() == start
    counts, elo, st = _one_step(2, 4, [1.0] * 4, [1, 1, 1, 1], elo=start, phase=0)       # nothing latched: not booked, latched now
    assert counts.sum() == 0 and elo.tolist() == start and st["world_phase"].tolist() == [1] * 4
    counts, elo, _ = _one_step(2, 4, [1.0] * 4, [1, 1, 1, 1], elo=start, hider_team=0)
    assert counts[:, :, 0].tolist() == [[1, 1], [1, 1]] and elo.tolist() != start
    # a latched team index outside {0, 1}: played, no outcome
    from gpu_hideseek import league as G
    st = dict(world_hider_team=np.full(4, 5, I32), world_phase=np.ones(4, I32))
    counts, elo = np.zeros((2, 2, 4), np.int64), np.array(start)
    G.host_step(st, counts, elo, 2, 1, np.ones(8, I32), np.tile(np.array([1, 0], I32), 4), np.ones(8, np.float32), np.ones((4, 2), np.float32), np.zeros(4, I32))
    assert counts[:, :, 3].sum() == 4 and elo.tolist() == start and st["world_hider_team"].tolist() == [0] * 4


def test_ratings_are_batched_by_step_and_their_sum_stays():
    # two games of one pair in one step are rated against the ratings before it: twice one game's move
    _, one, _ = _one_step(2, 8, [1.0] * 8, [0, 1, 0, 0, 0, 0, 0, 0], elo=[1500.0, 1600.0])
    _, two, _ = _one_step(2, 8, [1.0] * 8, [0, 1, 0, 0, 0, 1, 0, 0], elo=[1500.0, 1600.0])
    assert abs((two[0] - 1500.0) - 2 * (one[0] - 1500.0)) < 1e-12 and one[0] > 1500.0 + 16.0
    E = 1.0 / (1.0 + 10.0 ** (100.0 / 400.0))
    assert abs(one[0] - (1500.0 + 32.0 * (1.0 - E))) < 1e-12 and abs(one[1] - (1600.0 - 32.0 * (1.0 - E))) < 1e-12
    for worlds, P, k in ((8, 2, 1), (261, 3, 3), (256, 16, 1)):
        _, _, counts, elos = host_run(worlds, P, k, synthetic_steps(worlds, P, k, 24, seed=P))
        assert counts[:, :, :3].sum() > 0 and counts[:, :, 3].sum() > 0
        for e in elos:
            assert abs(e.sum() - P * 1500.0) <= ELO_TOL
        assert P == 1 or max(abs(elos[-1] - 1500.0)) > 1.0


def test_synthetic_steps_cover_what_they_are_for():
    calls = synthetic_steps(261, 3, 3, 24, seed=3)
    res, _, counts, _ = host_run(261, 3, 3, calls)
    ends = np.stack([c["done"].reshape(261, 6)[:, 0] for c in calls])
    assert (ends.sum(1) > 9).all()                                        # several worlds end in one step
    pair = np.arange(261) % 9
    assert max(np.bincount(pair[ends[t] != 0], minlength=9).max() for t in range(24)) > 2       # several of one pair
    assert sum(r["bad"] for r in res) > 100 and (counts > 0).all()
    assert len({tuple(c["hider_team"]) for c in calls}) > 10 and len({tuple(c["self_type"]) for c in calls}) > 10


# ---- print_elos ----
def test_print_elos_prints_four_to_a_line():
    from gpu_hideseek import league as G
    out = io.StringIO()
    G.print_elos(np.array([1500.0, 1512.345, 987.6, 1500.0, 2000.0, 1.0]), file=out)
    lines = out.getvalue().splitlines()
    assert len(lines) == 2
    assert lines[0].split("       ")[:4] == ["  0:  1500.00", "  1:  1512.35", "  2:   987.60", "  3:  1500.00"]
    assert lines[1].rstrip() == "  4:  2000.00         5:     1.00"
    assert G.hider_win_rates([[[3, 1, 0, 9], [0, 0, 0, 2]]]) == [[0.75, 0.0]]


# ---- request() ----
class _Sim:
    num_worlds, agents_per_world, gpu_id = 8, 4, 0


def test_request_refuses_before_the_library_is_called():
    import torch
    from gpu_hideseek import league as G
    W, A = _Sim.num_worlds, _Sim.agents_per_world
    R = W * A
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)        # noqa: E731

    def call(P=2, k=2, state=None, counts=None, elo=None, sim=None, **kw):
        st = G.new_state(W, "cpu")
        st.update(state or {})
        counts = torch.zeros(P, P, 4, dtype=torch.int64) if counts is None and isinstance(P, int) and not isinstance(P, bool) and 0 < P < 99 else counts
        elo = torch.full((P,), 1500.0, dtype=torch.float64) if elo is None and isinstance(P, int) and not isinstance(P, bool) and 0 < P < 99 else elo
        return G.compute(sim or _Sim(), P, k, st, counts, elo, **kw)

    class Odd(_Sim):
        num_worlds = 6

    buf = torch.zeros(256, dtype=torch.int64)
    bad = [
        (dict(P=0), "num_policies"), (dict(P=17), "num_policies"), (dict(P=2.0), "num_policies"), (dict(P=True), "num_policies"),
        (dict(k=0), "team_size"), (dict(k=1), "team_size"), (dict(k=3), "team_size"), (dict(k=2.0), "team_size"),
        (dict(P=3), "multiple of num_policies\\^2"), (dict(P=4), "multiple"), (dict(sim=Odd()), "multiple"),
        (dict(k_factor=0.0), "k_factor"), (dict(k_factor=-1.0), "k_factor"), (dict(k_factor=float("nan")), "k_factor"), (dict(k_factor=float("inf")), "k_factor"),
        (dict(state=dict(extra=i32(W))), "state must be"), (dict(state=dict(world_phase=i32(R))), "world_phase.*shape"),
        (dict(state=dict(world_hider_team=torch.zeros(W))), "world_hider_team.*dtype"),
        (dict(counts=torch.zeros(2, 2, 3, dtype=torch.int64)), "counts.*shape"), (dict(counts=torch.zeros(2, 2, 4, dtype=torch.int32)), "counts.*dtype"),
        (dict(counts=[0] * 16), "counts must be"), (dict(elo=torch.zeros(3, dtype=torch.float64)), "elo.*shape"), (dict(elo=torch.zeros(2)), "elo.*dtype"),
        (dict(elo=[1500.0] * 2), "elo must be"),
        (dict(done=torch.zeros(R)), "done.*dtype"), (dict(self_type=torch.zeros(R, dtype=torch.int64)), "self_type.*dtype"),
        (dict(self_mask=i32(R)), "self_mask.*dtype"), (dict(done=i32(R + 1)), "done.*shape"), (dict(self_mask=torch.zeros(2 * R)[::2]), "self_mask.*not contiguous"),
        (dict(episode_result=torch.zeros(W, 3)), "episode_result.*shape"), (dict(hider_team=torch.zeros(W)), "hider_team.*dtype"),
        (dict(slot=torch.zeros(R)), "slot.*dtype"), (dict(row_of_slot=i32(R - 1)), "row_of_slot.*shape"), (dict(clear_slot=[0] * R), "clear_slot"),
        (dict(policy_assignments=torch.zeros(R, dtype=torch.int64)), "policy_assignments.*dtype"), (dict(bad=i32(2)), "bad.*shape"),
        (dict(bad=torch.zeros(1, dtype=torch.int64)), "bad.*dtype"),
        # outputs in an input's or in each other's storage
        (dict(slot=buf.view(torch.int32)[:R], done=buf.view(torch.int32)[R - 1:2 * R - 1]), "slot overlaps done"),
        (dict(slot=buf.view(torch.int32)[:R], row_of_slot=buf.view(torch.int32)[R - 1:2 * R - 1]), "row_of_slot overlaps slot"),
        (dict(counts=buf[:16].view(2, 2, 4), elo=buf[15:17].view(torch.float64)), "elo overlaps counts"),
        (dict(state=dict(world_phase=buf.view(torch.int32)[:W]), bad=buf.view(torch.int32)[W - 1:W]), "bad overlaps world_phase"),
        (dict(clear_slot=buf.view(torch.int32)[:R], hider_team=buf.view(torch.int32)[R - 1:R - 1 + W]), "clear_slot overlaps hider_team"),
    ]
    for kw, what in bad:
        with pytest.raises(ValueError, match=what):
            call(**kw)
    # int64 counts and float64 ratings at an address that is 4 mod 8
    raw = bytearray(8 * 20)
    off = 4 if torch.frombuffer(raw, dtype=torch.uint8).data_ptr() % 8 == 0 else 8
    with pytest.raises(ValueError, match="counts must be 8-byte aligned"):
        call(counts=torch.frombuffer(raw, dtype=torch.int64, offset=off, count=16).view(2, 2, 4))
    with pytest.raises(ValueError, match="elo must be 8-byte aligned"):
        call(elo=torch.frombuffer(raw, dtype=torch.float64, offset=off, count=2))
    # well formed, on the wrong device: every accepted shape gets as far as the device check
    for shape in ((R,), (R, 1), (W, A)):
        with pytest.raises(ValueError, match="done must be on cuda:0: it is on cpu"):
            call(done=i32(shape), self_type=i32(shape), self_mask=torch.zeros(shape), episode_result=torch.zeros(W, 2), hider_team=i32(W),
                 slot=i32(shape), row_of_slot=i32(shape), clear_slot=i32(shape), policy_assignments=i32(shape), bad=i32(1))
    with pytest.raises(ValueError, match="world_hider_team must be on cuda:0: it is on cpu"):
        call()
    for kw, what in ((dict(mode="best"), "mode"), (dict(k_factor=0.0), "k_factor")):
        with pytest.raises(ValueError, match=what):
            G.League(_Sim(), [(None, None)] * 2, 2, **kw)
    with pytest.raises(ValueError, match="multiple of num_policies\\^2"):
        G.League(_Sim(), [(None, None)] * 3, 2)
    with pytest.raises(ValueError, match="policies must be"):
        G.League(_Sim(), [], 2)


# ---- the header ----
def test_header_mirror_and_symbols_agree(hideseek_lib):
    from gpu_hideseek import league as G
    src = open(os.path.join(ROOT, "include", "hideseek.h")).read()
    flat = " ".join(src.split())
    assert "int32_t hs_league_step(hs_sim *sim, const hs_league_request *req);" in flat
    assert "int32_t hs_league_step_async(hs_sim *sim, void *hip_stream, const hs_league_request *req);" in flat
    enums = dict(re.findall(r"(HS_LEAGUE_[A-Z_]+) = (\d+)", src))
    assert enums == {"HS_LEAGUE_MAX_POLICIES": "16", "HS_LEAGUE_OUTCOMES": "4", "HS_LEAGUE_HIDERS_WIN": "0", "HS_LEAGUE_SEEKERS_WIN": "1",
                     "HS_LEAGUE_DRAW": "2", "HS_LEAGUE_NO_OUTCOME": "3"}
    assert (G.MAX_POLICIES, G.OUTCOMES, G.HIDERS_WIN, G.SEEKERS_WIN, G.DRAW, G.NO_OUTCOME) == (16, 4, 0, 1, 2, 3)
    body = re.search(r"typedef struct hs_league_request \{(.*?)\} hs_league_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in G.HsLeagueRequest._fields_]
    want = dict(done=0, self_type=8, self_mask=16, episode_result=24, hider_team=32, num_policies=40, team_size=44, k_factor=48, policy_assignments=56,
                slot=64, row_of_slot=72, clear_slot=80, world_hider_team=88, world_phase=96, bad=104, counts=112, elo=120)
    assert C.sizeof(G.HsLeagueRequest) == 128
    assert {n: getattr(G.HsLeagueRequest, n).offset for n in want} == want
    L = C.CDLL(hideseek_lib)
    assert hasattr(L, "hs_league_step") and hasattr(L, "hs_league_step_async")
