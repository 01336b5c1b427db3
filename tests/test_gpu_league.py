"""The league kernel on the GPU (sim.league_step, hs_league_step, csrc/hs_k_league.h) against league.host_step: synthetic
inputs through explicit pointers, compared after every call; a second run bit for bit; the simulator's own exports through
null pointers; the refusals of the C ABI.  The simulator is only the handle, made with matching worlds and teams."""
import ctypes as C

import numpy as np
import pytest

import test_league_host as H
from test_league_host import ELO_TOL

pytestmark = pytest.mark.gpu

# (P, k, worlds): one world; the smallest league; A = 6 gives 42 worlds per 256-lane workgroup, so 261 = 9 * 29 worlds are 7
# workgroups, the last one partial with idle tail lanes; every lane of the fold for P = 16, one world per pair
SHAPES = [(1, 1, 1), (2, 1, 4), (3, 3, 261), (8, 1, 64), (16, 1, 256)]
STEPS = 24
INPUTS = ("done", "self_type", "self_mask", "episode_result", "hider_team")
ROUTING = ("policy_assignments", "slot", "row_of_slot", "clear_slot")


def _sim(worlds, k, flags=0, seed=0):
    import gpu_hideseek
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=flags, rand_seed=seed,
        min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=1)


def _outputs(worlds, A, P, fill=0):
    import torch
    from gpu_hideseek import league as G
    i32 = lambda n: torch.full((n,), fill, dtype=torch.int32, device="cuda")       # noqa: E731
    out = {k: i32(worlds * A) for k in ROUTING}
    out["bad"] = i32(1)
    return out, G.new_state(worlds, "cuda"), torch.zeros(P, P, 4, dtype=torch.int64, device="cuda"), torch.full((P,), 1500.0, dtype=torch.float64, device="cuda")


def _run(sim, P, k, worlds, dev, want=None):
    """The STEPS synthetic calls through the kernel; with `want` (host_run's results) everything is compared after every
    call.  Returns the ratings after every call, as numpy."""
    out, st, counts, elo = _outputs(worlds, 2 * k, P, fill=-3)
    elos = []
    for t in range(STEPS):
        sim.league_step(P, k, st, counts, elo, **out, **{n: dev[n][t] for n in INPUTS})
        elos.append(elo.cpu().numpy())
        if want is None:
            continue
        w, e = want[0][t], want[3][t]
        for n in ROUTING:
            assert np.array_equal(out[n].cpu().numpy(), w[n]), (P, k, worlds, t, n)
        for n in ("world_hider_team", "world_phase"):
            assert np.array_equal(st[n].cpu().numpy(), w[n]), (P, k, worlds, t, n)
        assert int(out["bad"].item()) == w["bad"], (P, k, worlds, t)
        assert np.array_equal(counts.cpu().numpy(), w["counts"]), (P, k, worlds, t)
        err = float(np.abs(elos[-1] - e).max())
        print(f"P {P} k {k} worlds {worlds} step {t}: max |elo - host| = {err:.3e} (bound {ELO_TOL:.0e})")
        assert err <= ELO_TOL, (P, k, worlds, t, elos[-1], e)
    return elos


@pytest.mark.parametrize("P,k,worlds", SHAPES, ids=[f"P{p}-k{k}-{w}" for p, k, w in SHAPES])
def test_synthetic_steps_equal_the_restatement_after_every_call_and_repeat_bit_for_bit(P, k, worlds):
    import torch
    calls = H.synthetic_steps(worlds, P, k, STEPS, seed=100 + P)
    want = H.host_run(worlds, P, k, calls)
    assert want[2].sum() > 0 or worlds == 1
    dev = {n: torch.from_numpy(np.stack([c[n] for c in calls])).cuda() for n in INPUTS}
    sim = _sim(worlds, k)
    sim.init()
    assert sim.agents_per_world == 2 * k
    first = _run(sim, P, k, worlds, dev, want)
    second = _run(sim, P, k, worlds, dev)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
    assert P == 1 or float(np.abs(first[-1] - 1500.0).max()) > 1.0
    sim.close()


def test_null_pointers_take_the_simulators_exports_and_write_its_policy_assignments():
    import torch
    import gpu_hideseek
    P, k, worlds = 2, 3, 16
    sim = _sim(worlds, k, flags=int(gpu_hideseek.SimFlags.RandomFlipTeams), seed=11)
    sim.init()
    for _ in range(3):
        sim.step()
    rows = worlds * 2 * k
    get = lambda n: getattr(sim, n + "_tensor")().to_torch().reshape(rows, -1)[:, 0].cpu().numpy().copy()      # noqa: E731
    types = get("self_type")
    out, st, counts, elo = _outputs(worlds, 2 * k, P, fill=-3)
    sim.league_step(P, k, st, counts, elo, **out)
    own = sim.policy_assignments_tensor().to_torch().reshape(rows)
    own.fill_(-5)
    out2, st2, counts2, elo2 = _outputs(worlds, 2 * k, P, fill=-3)
    del out2["policy_assignments"]
    res = sim.league_step(P, k, st2, counts2, elo2, **out2)
    assert "policy_assignments" not in res and torch.equal(own, out["policy_assignments"])
    for n in ("slot", "row_of_slot", "clear_slot", "bad"):
        assert torch.equal(out[n], out2[n]), n
    from gpu_hideseek import league as G
    hst = H.new_state(worlds)
    want = G.host_step(hst, np.zeros((P, P, 4), np.int64), np.full(P, 1500.0), P, k, get("done"), types, get("self_mask"),
                       sim.episode_result_tensor().to_torch().cpu().numpy(), (types.reshape(worlds, -1)[:, 0] == 0).astype(np.int32))
    assert want["bad"] == 0 and int(out["bad"].item()) == 0
    assert np.array_equal(own.cpu().numpy(), want["policy_assignments"]) and np.array_equal(out["slot"].cpu().numpy(), want["slot"])
    assert np.array_equal(st["world_hider_team"].cpu().numpy(), hst["world_hider_team"]) and st["world_phase"].cpu().tolist() == [1] * worlds
    assert len(set(types.reshape(worlds, -1)[:, 0].tolist())) == 2          # teams were flipped in some worlds
    sim.close()


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import league as G
    from lockstep import EXT_SKIP_OBSERVATIONS
    INVALID, UNSUPPORTED = 1, 3
    P, k, worlds = 2, 2, 8
    A = 2 * k
    rows = worlds * A
    f32 = lambda n: torch.full((n + 8,), -7.0, device="cuda")                        # noqa: E731
    i32 = lambda n: torch.full((n + 8,), -7, dtype=torch.int32, device="cuda")       # noqa: E731
    bufs = dict(done=i32(rows), self_type=i32(rows), self_mask=f32(rows), episode_result=f32(2 * worlds), hider_team=i32(worlds),
                policy_assignments=i32(rows), slot=i32(rows), row_of_slot=i32(rows), clear_slot=i32(rows), world_hider_team=i32(worlds),
                world_phase=i32(worlds), bad=i32(1), counts=torch.full((P * P * 4 + 2,), -7, dtype=torch.int64, device="cuda"),
                elo=torch.full((P + 2,), -7.0, dtype=torch.float64, device="cuda"))
    big = i32(4 * rows)
    names = [f[0] for f in G.HsLeagueRequest._fields_]

    def req(**kw):
        p = {n: t.data_ptr() for n, t in bufs.items()}
        p.update(num_policies=P, team_size=k, k_factor=32.0)
        p.update(kw)
        return G.HsLeagueRequest(*(p[n] for n in names))

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == -7).all()) for t in (*bufs.values(), big))

    def call(sim, r, stream=False):
        p = C.byref(r) if r is not None else None
        if stream:
            return sim._L.hs_league_step_async(sim._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p)
        return sim._L.hs_league_step(sim._h, p)

    def message(sim):
        return sim._L.hs_last_error().decode()

    sim = _sim(worlds, k)
    for stream in (False, True):
        assert call(sim, req(), stream) == INVALID and "before hs_init" in message(sim)
    assert untouched()
    sim.init()
    nan, inf = float("nan"), float("inf")
    bad = {"null request": (None, "null request"), "null counts": (req(counts=None), "null counts"), "null elo": (req(elo=None), "null elo"),
           "null world_phase": (req(world_phase=None), "null state pointer"), "null world_hider_team": (req(world_hider_team=None), "null state pointer"),
           "P 0": (req(num_policies=0), "num_policies"), "P 17": (req(num_policies=17), "num_policies"), "P 3": (req(num_policies=3), "multiple"),
           "P 4": (req(num_policies=4), "multiple"), "k 0": (req(team_size=0), "team_size"), "k 1": (req(team_size=1), "team_size"),
           "k 3": (req(team_size=3), "team_size"), "k_factor 0": (req(k_factor=0.0), "k_factor"), "k_factor -1": (req(k_factor=-1.0), "k_factor"),
           "k_factor nan": (req(k_factor=nan), "k_factor"), "k_factor inf": (req(k_factor=inf), "k_factor"),
           "done +2": (req(done=bufs["done"].data_ptr() + 2), "aligned"), "slot +1": (req(slot=bufs["slot"].data_ptr() + 1), "aligned"),
           "bad +2": (req(bad=bufs["bad"].data_ptr() + 2), "aligned"), "counts +4": (req(counts=bufs["counts"].data_ptr() + 4), "8-byte"),
           "elo +4": (req(elo=bufs["elo"].data_ptr() + 4), "8-byte"),
           "slot = row_of_slot": (req(slot=big.data_ptr(), row_of_slot=big.data_ptr() + 4 * (rows - 1)), "row_of_slot overlaps slot"),
           "clear_slot in done": (req(clear_slot=bufs["done"].data_ptr()), "clear_slot overlaps done"),
           "elo in counts": (req(elo=bufs["counts"].data_ptr() + 8 * (P * P * 4 - 1)), "elo overlaps counts"),
           "bad in world_phase": (req(bad=bufs["world_phase"].data_ptr() + 4), "bad overlaps world_phase"),
           "world team in result": (req(world_hider_team=bufs["episode_result"].data_ptr() + 4 * (2 * worlds - 1)), "world_hider_team overlaps episode_result"),
           "the sim's own done": (req(done=None, slot=sim.done_tensor().to_torch().data_ptr()), "slot overlaps done"),
           "the sim's own policy_assignments": (req(policy_assignments=None, slot=sim.policy_assignments_tensor().to_torch().data_ptr()), "slot overlaps policy_assignments")}
    before = sim.policy_assignments_tensor().to_torch().clone()
    for stream in (False, True):
        for name, (r, what) in bad.items():
            assert call(sim, r, stream) == INVALID, (name, stream)
            assert what in message(sim) and message(sim).startswith("hs_league_step"), (name, message(sim))
    assert untouched() and torch.equal(before, sim.policy_assignments_tensor().to_torch())
    sim.step_begin()
    assert call(sim, req()) == INVALID and "open step" in message(sim)
    sim.step_end()
    assert untouched()
    # the optional outputs may be null
    bufs["self_type"][:rows] = torch.tensor([1, 1, 0, 0], dtype=torch.int32, device="cuda").repeat(worlds)
    bufs["self_mask"].fill_(1.0)
    bufs["done"].zero_()
    bufs["counts"].zero_()
    bufs["world_phase"].zero_()
    bufs["elo"].fill_(1500.0)
    assert call(sim, req(slot=None, row_of_slot=None, clear_slot=None, bad=None)) == 0
    torch.cuda.synchronize()
    hp, sp = G.schedule(worlds, P)
    assert bufs["policy_assignments"][:rows].cpu().tolist() == [p for w in range(worlds) for p in (hp[w], hp[w], sp[w], sp[w])]
    assert all(bool((bufs[n] == -7).all()) for n in ("slot", "row_of_slot", "clear_slot", "bad")) and bufs["world_phase"][:worlds].cpu().tolist() == [1] * worlds
    sim.close()
    # no observations: the null form is refused, the explicit one works
    skip = _sim(worlds, k, flags=EXT_SKIP_OBSERVATIONS)
    skip.init()
    for n in ("self_type", "self_mask"):
        assert call(skip, req(**{n: None})) == UNSUPPORTED and "HS_FLAG_EXT_SKIP_OBSERVATIONS" in message(skip)
    assert call(skip, req()) == 0
    torch.cuda.synchronize()
    assert int(bufs["bad"][0].item()) == 0 and sorted(bufs["slot"][:rows].cpu().tolist()) == list(range(rows))
    skip.close()
