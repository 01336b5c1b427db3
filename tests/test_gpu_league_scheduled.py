"""The league kernel on a schedule table (sim.set_league_schedule, sim.league_step_scheduled; hs_league_set_schedule,
hs_league_step_scheduled, csrc/hs_k_league.h) on the GPU: with the all-pairs table against hs_league_step on a twin handle,
bit for bit; with the pool's schedules against league.host_step(pairs=) after every call, and a second run bit for bit; the
refusals of the C ABI, which write nothing; and hs_league_step on a handle that has a schedule set.  Synthetic inputs
through explicit pointers, as tests/test_gpu_league.py makes them; the simulator is only the handle."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_league as TL
import test_league_host as H
from test_gpu_league import INPUTS, ROUTING, STEPS
from test_league_host import ELO_TOL

pytestmark = pytest.mark.gpu

STATE = ("world_hider_team", "world_phase")


def _device_calls(calls):
    import torch
    return {n: torch.from_numpy(np.stack([c[n] for c in calls])).cuda() for n in INPUTS}


# ---- the all-pairs table is hs_league_step ----
@pytest.mark.parametrize("P,k,worlds", [(2, 1, 4), (3, 3, 261), (16, 1, 256)], ids=["P2-k1-4", "P3-k3-261", "P16-k1-256"])
def test_the_all_pairs_table_has_the_bits_of_the_fixed_schedule_after_every_call(P, k, worlds):
    import torch
    from gpu_hideseek import league as G
    dev = _device_calls(H.synthetic_steps(worlds, P, k, STEPS, seed=100 + P))
    fixed, tabled = TL._sim(worlds, k), TL._sim(worlds, k)
    try:
        fixed.init()
        tabled.init()
        assert tabled.set_league_schedule(G.all_pairs_schedule(P), P) == G.all_pairs_schedule(P)
        a, b = TL._outputs(worlds, 2 * k, P, fill=-3), TL._outputs(worlds, 2 * k, P, fill=-3)
        for t in range(STEPS):
            step = {n: dev[n][t] for n in INPUTS}
            fixed.league_step(P, k, a[1], a[2], a[3], **a[0], **step)
            tabled.league_step_scheduled(P, k, b[1], b[2], b[3], **b[0], **step)
            for n in (*ROUTING, "bad"):
                assert torch.equal(a[0][n], b[0][n]), (t, n)
            for n in STATE:
                assert torch.equal(a[1][n], b[1][n]), (t, n)
            assert torch.equal(a[2], b[2]), t
            assert torch.equal(a[3].view(torch.int64), b[3].view(torch.int64)), (t, a[3].tolist(), b[3].tolist())
        assert int(a[2].sum()) > 0 and (P == 1 or float((a[3] - 1500.0).abs().max()) > 1.0)
    finally:
        fixed.close()
        tabled.close()


# ---- the pool's schedules against the restatement ----
# (T, Q, k, worlds, fill): the smallest; G = 6 and 42 worlds per workgroup, 7 workgroups, the last one partial; G = 15, which
# does not divide 42, so groups straddle workgroups; N = 16 and G = 240, every lane of the fold; repeated (t, t) pairs
POOLS = [(1, 1, 1, 2, "cross"), (2, 1, 3, 264, "cross"), (3, 2, 3, 270, "cross"), (15, 1, 1, 240, "cross"), (2, 1, 3, 264, "self")]


def _run(sim, N, k, worlds, dev, want=None):
    out, st, counts, elo = TL._outputs(worlds, 2 * k, N, fill=-3)
    elos = []
    for t in range(STEPS):
        sim.league_step_scheduled(N, k, st, counts, elo, **out, **{n: dev[n][t] for n in INPUTS})
        elos.append(elo.cpu().numpy())
        if want is None:
            continue
        w = want[t]
        for n in ROUTING:
            assert np.array_equal(out[n].cpu().numpy(), w[n]), (t, n)
        for n in STATE:
            assert np.array_equal(st[n].cpu().numpy(), w[n]), (t, n)
        assert int(out["bad"].item()) == w["bad"], t
        assert np.array_equal(counts.cpu().numpy(), w["counts"]), t
        err = float(np.abs(elos[-1] - w["elo"]).max())
        print(f"N {N} k {k} worlds {worlds} step {t}: max |elo - host| = {err:.3e} (bound {ELO_TOL:.0e})")
        assert err <= ELO_TOL, (t, elos[-1], w["elo"])
    return elos, counts.cpu().numpy()


@pytest.mark.parametrize("T,Q,k,worlds,fill", POOLS, ids=[f"T{t}-Q{q}-k{k}-{w}-{f}" for t, q, k, w, f in POOLS])
def test_pool_schedules_equal_the_restatement_after_every_call_and_repeat_bit_for_bit(T, Q, k, worlds, fill):
    from gpu_hideseek import league as G
    N = T + Q
    pairs = G.past_play_schedule(T, Q, fill)
    calls = H.synthetic_steps(worlds, N, k, STEPS, seed=300 + 16 * T + Q)
    st, counts, elo = H.new_state(worlds), np.zeros((N, N, 4), np.int64), np.full(N, 1500.0)
    want = []
    for c in calls:
        r = G.host_step(st, counts, elo, N, k, c["done"], c["self_type"], c["self_mask"], c["episode_result"], c["hider_team"], pairs=pairs)
        r.update(world_hider_team=st["world_hider_team"].copy(), world_phase=st["world_phase"].copy(), counts=counts.copy(), elo=elo.copy())
        want.append(r)
    dev = _device_calls(calls)
    sim = TL._sim(worlds, k)
    try:
        sim.init()
        sim.set_league_schedule(pairs, N)
        first, got = _run(sim, N, k, worlds, dev, want)
        second, _ = _run(sim, N, k, worlds, dev)
        for a, b in zip(first, second):
            assert np.array_equal(a.view(np.int64), b.view(np.int64))
        present = np.zeros((N, N), bool)
        for i, j in pairs:
            present[i, j] = True
        assert got.sum() > 0                                               # games were booked at all
        assert (got[~present] == 0).all() and (got[T:, T:] == 0).all()     # and none where the table has no pair
        if fill == "self":
            assert got[0, 0].sum() > 0 and got[1, 1].sum() > 0 and got[0, 1].sum() == 0
    finally:
        sim.close()


# ---- refusals ----
def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import league as G
    INVALID = 1
    T, Q, k, worlds = 2, 1, 2, 12
    N, A = T + Q, 2 * k
    rows = worlds * A
    pairs = G.past_play_schedule(T, Q)
    f32 = lambda n: torch.full((n + 8,), -7.0, device="cuda")                        # noqa: E731
    i32 = lambda n: torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")       # noqa: E731
    bufs = dict(done=i32(rows), self_type=i32(rows), self_mask=f32(rows), episode_result=f32(2 * worlds), hider_team=i32(worlds),
                policy_assignments=i32(rows), slot=i32(rows), row_of_slot=i32(rows), clear_slot=i32(rows), world_hider_team=i32(worlds),
                world_phase=i32(worlds), bad=i32(1), counts=torch.full((N * N * 4 + 2,), -7, dtype=torch.int64, device="cuda"),
                elo=torch.full((N + 2,), -7.0, dtype=torch.float64, device="cuda"))
    names = [f[0] for f in G.HsLeagueRequest._fields_]

    def req(**kw):
        p = {n: t.data_ptr() for n, t in bufs.items()}
        p.update(num_policies=N, team_size=k, k_factor=32.0)
        p.update(kw)
        return G.HsLeagueRequest(*(p[n] for n in names))

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in bufs.values())

    def step(sim, r, stream=False):
        p = C.byref(r) if r is not None else None
        if stream:
            return sim._L.hs_league_step_scheduled_async(sim._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p)
        return sim._L.hs_league_step_scheduled(sim._h, p)

    def setter(sim, table, group=None, n=N):
        flat = (C.c_int32 * max(1, 2 * len(table)))(*(x for pair in table for x in pair))
        return sim._L.hs_league_set_schedule(sim._h, flat if table else None, len(table) if group is None else group, n)

    def message(sim):
        return sim._L.hs_last_error().decode()

    sim = TL._sim(worlds, k)
    try:
        assert setter(sim, pairs) == INVALID and "before hs_init" in message(sim)
        sim.init()
        # a step before any schedule is set
        for stream in (False, True):
            assert step(sim, req(), stream) == INVALID and "no schedule is set" in message(sim) and message(sim).startswith("hs_league_step_scheduled")
        with pytest.raises(ValueError, match="no schedule is set"):
            sim.league_step_scheduled(N, k, G.new_state(worlds, "cuda"), torch.zeros(N, N, 4, dtype=torch.int64, device="cuda"),
                                      torch.zeros(N, dtype=torch.float64, device="cuda"))
        assert untouched()
        # every rule of a table through the C ABI; the schedule stays unset after each
        ok = [(0, 1), (1, 0)]
        for name, args, what in (("irregular", dict(table=[(0, 1), (0, 1), (1, 1)], n=2), "not regular"), ("irregular N", dict(table=[(0, 1)], n=3), "not regular"),
                                 ("entry", dict(table=[(0, 1), (1, 3)], n=3), "out of range"), ("negative entry", dict(table=[(0, -1), (1, 0)], n=2), "out of range"),
                                 ("G 257", dict(table=ok * 128 + [(0, 0)], n=2), "group must be"), ("G -1", dict(table=ok, group=-1, n=2), "group must be"),
                                 ("N 17", dict(table=ok, n=17), "num_policies must be in"), ("N 0", dict(table=ok, n=0), "num_policies must be in"),
                                 ("null pairs", dict(table=[], group=2, n=2), "null pairs")):
            assert setter(sim, **args) == INVALID, name
            assert what in message(sim) and message(sim).startswith("hs_league_set_schedule"), (name, message(sim))
            assert step(sim, req()) == INVALID and "no schedule is set" in message(sim), name
        assert untouched()
        sim.step_begin()
        assert setter(sim, pairs) == INVALID and "open step" in message(sim)
        sim.step_end()
        assert setter(sim, pairs) == 0
        sim.step_begin()
        assert step(sim, req()) == INVALID and "open step" in message(sim)
        sim.step_end()
        # a refused table leaves the one that is set in place: the shape rules below are still those of G = 6, N = 3
        assert setter(sim, [(0, 1)], n=3) == INVALID
        bad = {"null request": (None, "null request"), "N 2": (req(num_policies=2), "num_policies must equal the schedule's"),
               "N 4": (req(num_policies=4), "num_policies must equal the schedule's"), "null counts": (req(counts=None), "null counts"),
               "k 3": (req(team_size=3), "team_size"), "k_factor 0": (req(k_factor=0.0), "k_factor"),
               "slot +1": (req(slot=bufs["slot"].data_ptr() + 1), "aligned"), "clear_slot in done": (req(clear_slot=bufs["done"].data_ptr()), "clear_slot overlaps done")}
        for stream in (False, True):
            for name, (r, what) in bad.items():
                assert step(sim, r, stream) == INVALID, (name, stream)
                assert what in message(sim) and message(sim).startswith("hs_league_step_scheduled"), (name, message(sim))
        assert untouched()
        # worlds not a multiple of G: 12 worlds, G = 8
        assert setter(sim, G.past_play_schedule(2, 2), n=4) == 0
        assert step(sim, req(num_policies=4)) == INVALID and "multiple of the schedule's group" in message(sim)
        sim._league_schedule = (8, 4)
        with pytest.raises(ValueError, match="multiple of the schedule's group = 8"):
            sim.league_step_scheduled(4, k, G.new_state(worlds, "cuda"), torch.zeros(4, 4, 4, dtype=torch.int64, device="cuda"),
                                      torch.zeros(4, dtype=torch.float64, device="cuda"))
        assert untouched()
        # the table that fits runs, and group = 0 drops it again
        assert setter(sim, pairs) == 0
        bufs["self_type"][:rows] = torch.tensor([1, 1, 0, 0], dtype=torch.int32, device="cuda").repeat(worlds)
        bufs["self_mask"].fill_(1.0)
        bufs["done"].zero_()
        bufs["counts"].zero_()
        bufs["world_phase"].zero_()
        bufs["elo"].fill_(1500.0)
        assert step(sim, req(slot=None, row_of_slot=None, clear_slot=None, bad=None)) == 0
        torch.cuda.synchronize()
        assert bufs["policy_assignments"][:rows].cpu().tolist() == [p for w in range(worlds) for i, j in [pairs[w % 6]] for p in (i, i, j, j)]
        assert all(bool((bufs[n] == -7).all()) for n in ("slot", "row_of_slot", "clear_slot", "bad")) and bufs["world_phase"][:worlds].cpu().tolist() == [1] * worlds
        for n in ("policy_assignments", "world_phase", "world_hider_team"):
            bufs[n].fill_(-7)
        kept = {n: bufs[n].clone() for n in ("counts", "elo")}
        assert setter(sim, [], group=0, n=0) == 0
        assert step(sim, req()) == INVALID and "no schedule is set" in message(sim)
        torch.cuda.synchronize()
        assert all(torch.equal(bufs[n], kept[n]) for n in kept) and all(bool((bufs[n] == -7).all()) for n in bufs if n not in kept and n not in ("self_type", "self_mask", "done"))
        sim._league_schedule = (6, 3)
        sim.set_league_schedule(None, 0)                                   # the Python face of the same
        assert sim._league_schedule is None
    finally:
        sim.close()


# ---- the setter leaves hs_league_step alone ----
def test_the_fixed_schedule_step_is_unchanged_on_a_handle_with_a_schedule_set():
    from gpu_hideseek import league as G
    P, k, worlds = 3, 3, 261
    calls = H.synthetic_steps(worlds, P, k, STEPS, seed=100 + P)
    want = H.host_run(worlds, P, k, calls)
    sim = TL._sim(worlds, k)
    try:
        sim.init()
        sim.set_league_schedule(G.past_play_schedule(2, 1), 3)            # set, never stepped: its G = 6 does not even divide 261
        TL._run(sim, P, k, worlds, _device_calls(calls), want)
    finally:
        sim.close()
