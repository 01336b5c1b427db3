"""The routed pack on the GPU (sim.pack_policy_inputs_routed, hs_pack_policy_inputs_routed, csrc/hs_k_pack_routed.h)
against the pack kernels it stands for: on a stepped simulator, with row_of_slot from hs_league_step and a random
normaliser state per policy, output row s is bit for bit row row_of_slot[s] of pack_policy_inputs(normaliser=table of the
slot's policy); the moments per policy against a float64 sum over that policy's rows; slots without a row; the refusals
of the Python face and of the C ABI."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROW, MOMENTS, TABLE = 296, 593, 592
EPS = 1e-5
# name: (N, worlds, agents per team, steps driven).  R / N slots per policy, in blocks of 32:
#   n3: 36 = a full block and a partial one per policy, the policies' boundaries (36, 72) off the block grid
#   n2: 64 = whole blocks;   n1: slot == row, the unrouted call
#   cap: 12 288 = 384 blocks per policy against 1024 / 4 = 256 workgroups: the first 128 take a second block
SHAPES = {"n3": (3, 18, 3, 12), "n2": (2, 32, 2, 12), "n1": (1, 5, 3, 12), "cap": (4, 8192, 3, 1)}
DTYPES = ("float32", "bfloat16", "float16")


def _bits(t):
    import torch
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _tables(N, seed):
    """[N, 592] tables of N normalisers with random states, each kept in its row of the one buffer."""
    import torch
    from gpu_hideseek import policy_inputs as P
    rng = np.random.default_rng(seed)
    buf = torch.empty(N, TABLE, dtype=torch.float32, device="cuda")
    norms = []
    for p in range(N):
        norm = P.ObsNormaliser(0, decay=0.9, eps=EPS, table=buf[p])
        assert norm.table.data_ptr() == buf[p].data_ptr()
        mean, var = rng.normal(0.0, 2.0, ROW), rng.uniform(0.01, 9.0, ROW)
        norm.load_state_dict({"state": torch.from_numpy(np.concatenate([mean, var + mean * mean, [1.0]])), "decay": 0.9, "eps": EPS})
        norms.append(norm)
    assert bool((buf[:, ROW:] != 1.0).any(dim=1).all())
    return buf, norms


@pytest.fixture(scope="module")
def scenes():
    """Per shape: a simulator driven for some steps, the routing hs_league_step gives it, N random tables, and (made once
    per dtype, on demand) the reference rows.  Shared and left unchanged by the tests."""
    import torch
    import gpu_hideseek
    from gpu_hideseek import league as G
    made = {}

    def get(name):
        if name in made:
            return made[name]
        N, worlds, k, steps = SHAPES[name]
        sim = gpu_hideseek.HideAndSeekSimulator(
            exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=int(gpu_hideseek.SimFlags.RandomFlipTeams),
            rand_seed=3, min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=N)
        sim.init()
        act = sim.action_tensor().to_torch()
        g = torch.Generator(device=act.device).manual_seed(11)
        for _ in range(steps):
            act[:, 0:2] = torch.randint(-5, 5, (act.shape[0], 2), device=act.device, dtype=torch.int32, generator=g)
            sim.step()
        R = worlds * 2 * k
        ros = torch.full((R,), -1, dtype=torch.int32, device="cuda")
        sim.league_step(N, k, G.new_state(worlds, "cuda"), torch.zeros(N, N, 4, dtype=torch.int64, device="cuda"),
                        torch.full((N,), 1500.0, dtype=torch.float64, device="cuda"), row_of_slot=ros)
        assert sorted(ros.tolist()) == list(range(R))
        assert N == 1 or ros.tolist() != list(range(R))
        tables, norms = _tables(N, seed=7 + N)
        s = dict(sim=sim, N=N, R=R, m=R // N, ros=ros, tables=tables, norms=norms, want={})

        def want(dtype, normalised=True):
            """{"actor", "critic"}: the rows the routed pack must write, from N unrouted packs and an index."""
            key = (dtype, normalised)
            if key not in s["want"]:
                out = {}
                for p in range(N):
                    res = sim.pack_policy_inputs(actor=True, critic=True, dtype=getattr(torch, dtype), normaliser=norms[p] if normalised else None)
                    rows = ros[p * s["m"]:(p + 1) * s["m"]].long()
                    for side in ("actor", "critic"):
                        out.setdefault(side, []).append(res[side][rows])
                s["want"][key] = {side: torch.cat(v) for side, v in out.items()}
            return s["want"][key]
        s["rows"] = want
        made[name] = s
        return s
    yield get
    for s in made.values():
        s["sim"].close()


# ---- (a) the rows ----
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_are_the_bits_of_the_unrouted_pack_under_the_slots_policy(scenes, shape, dtype):
    import torch
    s = scenes(shape)
    want = s["rows"](dtype)
    got = s["sim"].pack_policy_inputs_routed(s["ros"], s["N"], actor=True, critic=True, tables=s["tables"], dtype=getattr(torch, dtype))
    for side in ("actor", "critic"):
        bad = (_bits(got[side]) != _bits(want[side])).any(dim=1).nonzero().flatten()
        assert not len(bad), (shape, dtype, side, len(bad), int(bad[0]))
    assert not _same_bits(got["actor"], got["critic"])            # the masks did something
    if s["N"] > 1:                                                # and so did the tables: block 0 under table 1 differs
        other = s["sim"].pack_policy_inputs(critic=True, dtype=getattr(torch, dtype), normaliser=s["norms"][1])["critic"]
        assert not _same_bits(other[s["ros"][:s["m"]].long()], got["critic"][:s["m"]])


def test_one_policy_is_the_unrouted_call_moments_included(scenes):
    import torch
    s = scenes("n1")
    sim = s["sim"]
    assert s["ros"].tolist() == list(range(s["R"]))
    a = sim.pack_policy_inputs(actor=True, critic=True, moments=True, normaliser=s["norms"][0])
    b = sim.pack_policy_inputs_routed(s["ros"], 1, actor=True, critic=True, moments=True, tables=s["tables"])
    assert _same_bits(a["actor"], b["actor"]) and _same_bits(a["critic"], b["critic"])
    assert b["moments"].shape == (1, MOMENTS) and _same_bits(a["moments"], b["moments"][0])


@pytest.mark.parametrize("shape", ["n3", "n2"])
def test_each_output_alone_mixed_dtypes_and_no_tables(scenes, shape):
    import torch
    s = scenes(shape)
    sim, N, R, ros, tables = s["sim"], s["N"], s["R"], s["ros"], s["tables"]
    f32, bf16 = s["rows"]("float32"), s["rows"]("bfloat16")
    sentinel = torch.full((R, ROW), -7.0, device="cuda")
    got = sim.pack_policy_inputs_routed(ros, N, actor=sentinel.clone(), tables=tables)
    assert set(got) == {"actor"} and _same_bits(got["actor"], f32["actor"])
    got = sim.pack_policy_inputs_routed(ros, N, critic=sentinel.clone().to(torch.bfloat16), tables=tables)
    assert set(got) == {"critic"} and _same_bits(got["critic"], bf16["critic"])
    got = sim.pack_policy_inputs_routed(ros, N, actor=sentinel.clone().to(torch.bfloat16), critic=sentinel.clone(), tables=tables)
    assert _same_bits(got["actor"], bf16["actor"]) and _same_bits(got["critic"], f32["critic"])
    both = sim.pack_policy_inputs_routed(ros, N, critic=True, moments=True, tables=tables)
    only = sim.pack_policy_inputs_routed(ros, N, moments=True, tables=tables)
    none = sim.pack_policy_inputs_routed(ros, N, moments=True)
    assert set(only) == {"moments"} and _same_bits(only["moments"], both["moments"]) and _same_bits(none["moments"], both["moments"])
    # null tables: the plain pack
    for dtype in DTYPES:
        want = s["rows"](dtype, normalised=False)
        got = sim.pack_policy_inputs_routed(ros, N, actor=True, critic=True, dtype=getattr(torch, dtype))
        assert _same_bits(got["actor"], want["actor"]) and _same_bits(got["critic"], want["critic"]), dtype
    # on a stream, into a slot of a rollout buffer
    buf = torch.zeros(3, R, ROW, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    sim.pack_policy_inputs_routed(ros, N, actor=buf[1], tables=tables, stream=st)
    st.synchronize()
    assert _same_bits(buf[1], f32["actor"]) and not bool(buf[0].any()) and not bool(buf[2].any())


# ---- (b) the moments ----
@pytest.mark.parametrize("shape", list(SHAPES))
def test_moments_per_policy_against_float64_repeat_bit_for_bit_and_keep_their_stride(scenes, shape):
    import torch
    s = scenes(shape)
    sim, N, R, m, ros = s["sim"], s["N"], s["R"], s["m"], s["ros"]
    T = 3
    mom = torch.full((N, T, MOMENTS), -7.0, dtype=torch.float64, device="cuda")
    sim.pack_policy_inputs_routed(ros, N, critic=True, moments=mom[:, 1], moments_stride=T * MOMENTS, tables=s["tables"])
    assert bool((mom[:, 0] == -7).all()) and bool((mom[:, 2] == -7).all())          # the doubles between the vectors
    again = torch.full((N, T, MOMENTS), -7.0, dtype=torch.float64, device="cuda")
    sim.pack_policy_inputs_routed(ros, N, moments=again[:, 1])                      # the stride is the view's own by default
    assert _same_bits(mom, again)
    got = mom[:, 1].cpu().numpy()
    x = sim.pack_policy_inputs(critic=True)["critic"].cpu().numpy().astype(np.float64)           # the plain f32 critic rows
    mask = sim.self_mask_tensor().to_torch().reshape(R).cpu().numpy().astype(np.float64)
    rows = ros.cpu().numpy()
    u = 2.0 ** -52
    for p in range(N):
        mine = rows[p * m:(p + 1) * m]
        xm, mm = x[mine], mask[mine][:, None]
        assert got[p, 2 * ROW] == mm.sum(), (shape, p)                              # the count: exact
        for name, off, terms in (("sum m x", 0, mm * xm), ("sum m x x", ROW, mm * xm * xm)):
            want, bound = terms.sum(axis=0), m * u * np.abs(terms).sum(axis=0)
            err = np.abs(got[p, off:off + ROW] - want)
            worst = int(np.argmax(err - bound * (err > 0)))
            print(f"{shape} policy {p} {name}: max error {err.max():.3e}, worst column {worst}: {err[worst]:.3e} (bound {bound[worst]:.3e})")
            assert bool((err <= bound).all()), (shape, p, name, worst, err[worst], bound[worst])
    assert bool(np.isfinite(got).all()) and float(got[:, 2 * ROW].sum()) == mask.sum() > 0


# ---- (c) slots without a row ----
def test_out_of_range_rows_give_zero_rows_and_are_counted(scenes):
    import torch
    s = scenes("n3")
    sim, N, R, m, tables = s["sim"], s["N"], s["R"], s["m"], s["tables"]
    ros = s["ros"].clone()
    holes = {0: -1, 33: R, 35: 2 ** 31 - 1, 40: -2 ** 31, 71: R + 5, R - 1: -7}      # in both blocks of policy 0, in 1 and 2
    for slot, v in holes.items():
        ros[slot] = v
    idx = torch.tensor(sorted(holes), device="cuda")
    keep = torch.ones(R, dtype=torch.bool, device="cuda")
    keep[idx] = False
    bad = torch.full((1,), 99, dtype=torch.int32, device="cuda")
    for dtype in DTYPES:
        want = s["rows"](dtype)
        got = sim.pack_policy_inputs_routed(ros, N, actor=True, critic=True, moments=True, tables=tables, bad=bad, dtype=getattr(torch, dtype))
        assert int(bad.item()) == len(holes)
        for side in ("actor", "critic"):
            assert not bool(_bits(got[side][idx]).any()), (dtype, side)               # all-zero bits, whatever the table
            assert _same_bits(got[side][keep], want[side][keep]), (dtype, side)
    clean = sim.pack_policy_inputs_routed(s["ros"], N, moments=True, bad=bad)["moments"]
    assert int(bad.item()) == 0                                                       # zeroed by the call
    mask = sim.self_mask_tensor().to_torch().reshape(R)
    per = [sum(1 for slot in holes if slot // m == p and float(mask[s["ros"][slot]]) != 0.0) for p in range(N)]
    assert (clean[:, 2 * ROW] - got["moments"][:, 2 * ROW]).tolist() == per and sum(per) > 0
    # a routing with no row at all
    ros.fill_(-1)
    got = sim.pack_policy_inputs_routed(ros, N, critic=True, moments=True, tables=tables, bad=bad)
    assert int(bad.item()) == R and not bool(_bits(got["critic"]).any()) and not bool(_bits(got["moments"]).any())


# ---- (d) the refusals ----
def test_the_python_face_refuses_before_the_library_is_called(scenes):
    import torch
    s = scenes("n3")
    sim, N, R, ros, tables = s["sim"], s["N"], s["R"], s["ros"], s["tables"]
    f32 = lambda *shape: torch.zeros(*shape, device="cuda")        # noqa: E731
    raw = torch.zeros(N * TABLE + 8, device="cuda")
    mom = torch.zeros(N, 2, MOMENTS, dtype=torch.float64, device="cuda")
    shared = torch.zeros(R * ROW + R, device="cuda")
    cases = [
        (dict(num_policies=0), "num_policies"), (dict(num_policies=17), "num_policies"), (dict(num_policies=2.0), "num_policies"),
        (dict(num_policies=True), "num_policies"), (dict(num_policies=5), "multiple of num_policies"),
        (dict(actor=None), "no output requested"),
        (dict(actor=f32(R - 1, ROW)), "actor.*shape"), (dict(actor=f32(R, ROW).double()), "actor.*dtype"), (dict(critic=f32(R, 2 * ROW)[:, ::2]), "critic.*contiguous"),
        (dict(actor=f32(R * ROW + 1)[1:].view(R, ROW)), "actor.*16-byte"), (dict(actor=torch.zeros(R, ROW)), "actor.*on cpu"),
        (dict(dtype=torch.float64), "dtype must be one of"),
        (dict(row_of_slot=ros[:-1]), "row_of_slot.*shape"), (dict(row_of_slot=ros.long()), "row_of_slot.*dtype"), (dict(row_of_slot=ros.tolist()), "row_of_slot must be"),
        (dict(row_of_slot=ros.cpu()), "row_of_slot must be on"),
        (dict(tables=tables[:2]), "tables.*shape"), (dict(tables=tables.double()), "tables.*dtype"), (dict(tables=raw[1:1 + N * TABLE].view(N, TABLE)), "tables must be 16-byte aligned"),
        (dict(tables=tables.cpu()), "tables must be on"), (dict(tables=s["norms"][0]), "tables must be"),
        (dict(moments=torch.zeros(N, MOMENTS, device="cuda")), "moments.*dtype"), (dict(moments=mom[:, 0, :-1]), "moments.*shape"),
        (dict(moments=torch.zeros(MOMENTS, dtype=torch.float64, device="cuda")), "moments.*shape"),
        (dict(moments=torch.zeros(N, 2 * MOMENTS, dtype=torch.float64, device="cuda")[:, ::2]), "moments.*stride"),
        (dict(moments=torch.zeros(N, MOMENTS, dtype=torch.float64)), "moments.*on cpu"),
        (dict(moments=mom[:, 0], moments_stride=MOMENTS), "moments_stride is 593"), (dict(moments=True, moments_stride=MOMENTS - 1), "moments_stride must be"),
        (dict(moments=True, moments_stride=593.0), "moments_stride must be"),
        (dict(bad=torch.zeros(2, dtype=torch.int32, device="cuda")), "bad.*shape"), (dict(bad=torch.zeros(1, device="cuda")), "bad.*dtype"),
        (dict(actor=shared[:R * ROW].view(R, ROW), row_of_slot=shared.view(torch.int32)[R * ROW - 4:R * ROW - 4 + R]), "actor overlaps row_of_slot"),
        (dict(actor=shared[:R * ROW].view(R, ROW), critic=shared[R:R + R * ROW].view(R, ROW)), "critic overlaps actor"),
        (dict(critic=raw.new_zeros(R, ROW), tables=None, actor=None, bad=ros[:1]), "bad overlaps row_of_slot"),
    ]
    for kw, what in cases:
        args = dict(row_of_slot=ros, num_policies=N, actor=True, tables=tables)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            sim.pack_policy_inputs_routed(args.pop("row_of_slot"), args.pop("num_policies"), **args)


def test_the_c_abi_refuses_and_writes_nothing(scenes):
    import torch
    import gpu_hideseek
    from gpu_hideseek import policy_inputs as P
    from gpu_hideseek._native import load
    INVALID, F32, BF16 = 1, 1, 3
    s = scenes("n3")
    sim, N, R, tables = s["sim"], s["N"], s["R"], s["tables"]
    L, h = sim._L, sim._h
    out = torch.full((2 * R * ROW + 8,), -7.0, device="cuda")
    mom = torch.full((2 * N * MOMENTS + 8,), -7.0, dtype=torch.float64, device="cuda")       # room for a stride of 2 x 593
    idx = torch.cat([s["ros"], torch.full((8,), -7, dtype=torch.int32, device="cuda")])
    tab = torch.cat([tables.flatten(), torch.full((8,), -7.0, device="cuda")])
    o, c2, m, i, t = out.data_ptr(), out.data_ptr() + 4 * R * ROW, mom.data_ptr(), idx.data_ptr(), tab.data_ptr()
    b = i + 4 * R
    before = [x.clone() for x in (out, mom, idx, tab)]

    def calls(req):
        r = C.byref(req) if req is not None else None
        return L.hs_pack_policy_inputs_routed(h, r), L.hs_pack_policy_inputs_routed_async(h, None, r)

    def refused(fields, what, code=INVALID, sim_handle=None):
        req = P.HsPackRoutedRequest(*fields) if fields is not None else None
        hh = h if sim_handle is None else sim_handle
        r = C.byref(req) if req is not None else None
        for rc in (L.hs_pack_policy_inputs_routed(hh, r), L.hs_pack_policy_inputs_routed_async(hh, None, r)):
            assert rc == code, (what, rc)
            msg = load().hs_last_error().decode()
            assert "hs_pack_policy_inputs_routed" in msg and what in msg, (what, msg)
        torch.cuda.synchronize()
        for x, y in zip((out, mom, idx, tab), before):
            assert torch.equal(x, y), what

    S = MOMENTS
    for fields, what in (
            ((None, F32, None, F32, i, N, t, None, S, b), "every output is null"),
            ((o, 2, None, F32, i, N, t, m, S, b), "dtype"), ((None, F32, c2, 0, i, N, t, m, S, b), "dtype"),
            ((o, F32, c2, F32, None, N, t, m, S, b), "null row_of_slot"),
            ((o, F32, c2, F32, i, 0, t, m, S, b), "num_policies"), ((o, F32, c2, F32, i, -1, t, m, S, b), "num_policies"),
            ((o, F32, c2, F32, i, 17, t, m, S, b), "num_policies"), ((o, F32, c2, F32, i, 5, t, m, S, b), "multiple of num_policies"),
            ((o, F32, c2, F32, i, N, t, m, S - 1, b), "moments_stride"), ((o, F32, c2, F32, i, N, t, m, 0, b), "moments_stride"),
            ((o, F32, c2, F32, i, N, t, m, -S, b), "moments_stride"),
            ((o + 8, F32, c2, F32, i, N, t, m, S, b), "outputs must be 16-byte aligned"), ((o, BF16, c2 + 2, BF16, i, N, t, m, S, b), "outputs must be 16-byte aligned"),
            ((o, F32, c2, F32, i, N, t + 4, m, S, b), "tables must be 16-byte aligned"), ((o, F32, c2, F32, i, N, t + 8, m, S, b), "tables must be 16-byte aligned"),
            ((o, F32, c2, F32, i, N, t, m + 4, S, b), "moments must be 8-byte aligned"),
            ((o, F32, c2, F32, i + 2, N, t, m, S, b), "row_of_slot and bad must be 4-byte aligned"),
            ((o, F32, c2, F32, i, N, t, m, S, b + 1), "row_of_slot and bad must be 4-byte aligned"),
            ((o, F32, o + 16, F32, i, N, t, m, S, b), "critic overlaps actor"), ((o, F32, c2 - 16, F32, i, N, t, m, S, b), "critic overlaps actor"),
            ((o, F32, c2, F32, o + 4 * R * ROW - 4, N, t, m, S, b), "actor overlaps row_of_slot"),
            ((o, F32, c2, F32, i, N, c2 + 16, m, S, b), "critic overlaps tables"),
            ((o, F32, c2, F32, i, N, t, o + 8 * 5, S, b), "moments overlaps actor"),
            ((None, F32, None, F32, i, N, t, m, 2 * S, m + 8 * 2 * S + 4), "bad overlaps moments"),
            ((o, F32, c2, F32, i, N, t, m, S, i + 4), "bad overlaps row_of_slot")):
        refused(fields, what)
    refused(None, "null request")
    # the accepted call writes its own ranges and nothing else
    ok = P.HsPackRoutedRequest(o, F32, c2, F32, i, N, t, m, S, b)
    assert calls(ok) == (0, 0)
    torch.cuda.synchronize()
    assert bool((out[:2 * R * ROW] != -7).any()) and bool((out[2 * R * ROW:] == -7).all()) and bool((mom[N * S:] == -7).all())
    assert int(idx[R]) == 0 and bool((idx[R + 1:] == -7).all()) and torch.equal(tab, before[3])
    assert _same_bits(out[:R * ROW].view(R, ROW), s["rows"]("float32")["actor"])
    # before hs_init, inside an open step, without observations
    k = SHAPES["n3"][2]
    kw = dict(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=SHAPES["n3"][1], rand_seed=3, min_hiders=k, max_hiders=k,
              min_seekers=k, max_seekers=k, num_pbt_policies=N)
    fresh = gpu_hideseek.HideAndSeekSimulator(sim_flags=0, **kw)
    fields = (o, F32, c2, F32, i, N, t, m, S, b)
    before = [x.clone() for x in (out, mom, idx, tab)]
    refused(fields, "before hs_init", sim_handle=fresh._h)
    fresh.init()
    fresh.step_begin()
    refused(fields, "open step", sim_handle=fresh._h)
    fresh.step_end()
    fresh.close()
    blind = gpu_hideseek.HideAndSeekSimulator(sim_flags=int(gpu_hideseek.SimFlags.ExtSkipObservations), **kw)
    blind.init()
    refused(fields, "HS_FLAG_EXT_SKIP_OBSERVATIONS", code=3, sim_handle=blind._h)
    blind.close()


# ---- League.act() on the routed pack ----
def test_league_act_gives_the_bits_of_the_per_policy_packs_and_gathers():
    """Two leagues over two simulators with the same seed, one on the routed pack and one forced onto the path of a league
    with several dtypes (a pack and a gather per policy): the same logits and actions, bit for bit, across several steps."""
    import torch
    import gpu_hideseek
    from gpu_hideseek import league, policy
    from gpu_hideseek.policy_inputs import NORM_STATE, ObsNormaliser
    N, worlds, k = 3, 18, 3
    F = gpu_hideseek.SimFlags
    nets = [policy.make_policy(generator=torch.Generator().manual_seed(20 + p)).cuda() for p in range(N)]
    norm = ObsNormaliser(0)
    norm.load_state_dict({"state": torch.rand(NORM_STATE, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) + 0.5, "decay": norm.decay, "eps": norm.eps})
    policies = list(zip(nets, [norm, None, norm]))
    runs = []
    for routed in (True, False):
        sim = gpu_hideseek.HideAndSeekSimulator(
            exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=int(F.RandomFlipTeams | F.UseFixedWorld | F.ZeroAgentVelocity),
            rand_seed=5, min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=N)
        sim.init()
        lg = league.League(sim, policies, k, mode="draw", seed=2)
        assert lg.routed
        if not routed:
            lg.routed = False
            lg.gathered = {nets[0].dtype: torch.zeros(1, lg.block, ROW, dtype=nets[0].dtype, device="cuda")}
        seen = []
        lg.run(6, on_step=lambda i, lg: seen.append((lg.logits.clone(), sim.action_tensor().to_torch().clone())))
        runs.append(seen)
        sim.close()
    for (la, aa), (lb, ab) in zip(*runs):
        assert _same_bits(la, lb) and torch.equal(aa, ab)
    assert bool((runs[0][0][0] != runs[0][-1][0]).any())
