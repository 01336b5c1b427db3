"""The routed sampler on the GPU (sim.sample_actions_routed, hs_sample_actions_routed, csrc/hs_k_sample_routed.h) against
sim.sample_actions on the logits gathered back to rows by torch indexing: bit for bit, for every routing, dtype, stride,
mode and bucket layout, on 36 worlds x (3 + 3) (R = 216 = 6 x 32 + 24: the last block of 32 slots is partial) and on one
world x (1 + 1) (R = 2)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED, COUNTER = (0x1234567, 0x9abcdef0), 41
DTYPES = ("float32", "bfloat16", "float16")
BUCKETS = ((5, 5, 5, 2, 2), (16, 1, 3, 2, 7))
ALL = dict(action=True, log_prob=True, entropy=True, head_log_prob=True)
SLOT_SHAPES = dict(action=(5,), log_prob=(), entropy=(), head_log_prob=(5,))


@pytest.fixture(scope="module")
def sims():
    """{R: an initialised simulator of R agent rows}: 36 x (3 + 3) and 1 x (1 + 1)."""
    import gpu_hideseek
    made = {}
    for worlds, k in ((36, 3), (1, 1)):
        s = gpu_hideseek.HideAndSeekSimulator(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=0, rand_seed=3,
                                              min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=1)
        s.init()
        made[worlds * 2 * k] = s
    yield made
    for s in made.values():
        s.close()


def _routings(R):
    """{name: row_of_slot (numpy int32 [R], a permutation)}."""
    from gpu_hideseek import league
    out = {"identity": np.arange(R), "reversal": np.arange(R)[::-1].copy(), "random": np.random.default_rng(R).permutation(R)}
    if R == 216:
        worlds, k = 36, 3
        for P in (2, 3, 6):
            rng = np.random.default_rng(10 + P)
            first_hides = rng.random(worlds) < 0.5                            # seeded random sides: which team of a world hides
            self_type = np.where(first_hides[:, None], np.arange(2 * k)[None, :] < k, np.arange(2 * k)[None, :] >= k).astype(np.int32).reshape(-1)
            st = {"world_hider_team": np.zeros(worlds, np.int32), "world_phase": np.zeros(worlds, np.int32)}
            r = league.host_step(st, np.zeros((P, P, 4), np.int64), np.full(P, 1500.0), P, k, np.zeros(R, np.int32), self_type, np.ones(R, np.float32),
                                 np.zeros((worlds, 2), np.float32), np.zeros(worlds, np.int32))
            assert r["bad"] == 0 and sorted(r["row_of_slot"].tolist()) == list(range(R))
            out[f"league{P}"] = r["row_of_slot"]
    return {k: np.ascontiguousarray(v, np.int32) for k, v in out.items()}


def _logits(R, L, dtype, seed, stride=None):
    """Slot-order logits [R, L] of `dtype` on the device (inside a [R, stride] buffer of NaN with a stride), 3 N(0, 1)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = (3.0 * torch.randn(R, L, generator=g)).to(getattr(torch, dtype)).cuda()
    if stride is None:
        return x
    buf = torch.full((R, stride), float("nan"), dtype=x.dtype, device="cuda")
    buf[:, :L] = x
    return buf[:, :L]


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _check(sim, by_slot, ros, buckets, mode, tag, seed=SEED, counter=COUNTER):
    """One routed call with every output against sample_actions on by_row[ros[s]] = by_slot[s]."""
    import torch
    R = by_slot.shape[0]
    row_of_slot = torch.from_numpy(ros).cuda()
    slot_of_row = torch.empty(R, dtype=torch.long, device="cuda")
    slot_of_row[row_of_slot.long()] = torch.arange(R, device="cuda")
    by_row = by_slot[slot_of_row].contiguous()
    ref_rows = torch.full((R, 5), -7, dtype=torch.int32, device="cuda")
    ref = sim.sample_actions(by_row, buckets=buckets, mode=mode, seed=seed, counter=counter, action=ref_rows, log_prob=True, entropy=True, head_log_prob=True)
    rows = torch.full((R, 5), -9, dtype=torch.int32, device="cuda")
    out = sim.sample_actions_routed(by_slot, row_of_slot, buckets=buckets, mode=mode, seed=seed, counter=counter, action_rows=rows, bad=True, **ALL)
    assert out["action_rows"] is rows and int(out["bad"].item()) == 0, tag
    assert torch.equal(rows, ref_rows), tag
    assert (rows >= 0).all().item() and (rows < torch.tensor(buckets, device="cuda")).all().item(), tag
    for k in SLOT_SHAPES:
        assert tuple(out[k].shape) == (R,) + SLOT_SHAPES[k], (tag, k)
        assert torch.equal(_bits(out[k]), _bits(ref[k][row_of_slot.long()])), (tag, k)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_routing_gives_sample_actions_bits(sims, dtype):
    for R in (216, 2):
        for i, (name, ros) in enumerate(_routings(R).items()):
            for mode in ("draw", "greedy"):
                _check(sims[R], _logits(R, 19, dtype, 100 + i), ros, BUCKETS[0], mode, (R, name, dtype, mode))


@pytest.mark.parametrize("buckets", BUCKETS)
def test_stride_bucket_layouts_and_a_masked_logit(sims, buckets):
    import torch
    L = sum(buckets)
    for R in (216, 2):
        ros = _routings(R)["league2" if R == 216 else "reversal"]
        for dtype in DTYPES:
            by_slot = _logits(R, L, dtype, 7, stride=L + 5)                # 24 over L = 19
            assert by_slot.stride(0) == L + 5 and not by_slot.is_contiguous()
            by_slot[::3, 0] = float("-inf")                                # a masked bucket in head 0 of every third slot
            by_slot[1, buckets[0]:buckets[0] + buckets[1]] = float("-inf")
            by_slot[1, buckets[0]] = 0.5                                   # one finite logit left in head 1
            for mode in ("draw", "greedy"):
                out = _check(sims[R], by_slot, ros, buckets, mode, (R, dtype, mode, buckets))
                assert torch.isfinite(out["log_prob"]).all().item() and torch.isfinite(out["entropy"]).all().item()
                if buckets[0] > 1:
                    assert (out["action"][::3, 0] != 0).all().item()       # the masked bucket is never taken
                assert out["action"][1, 1].item() == 0


def test_two_calls_give_the_same_bits_and_the_draw_follows_seed_and_counter(sims):
    import torch
    R = 216
    ros = _routings(R)["league3"]
    by_slot = _logits(R, 19, "float32", 9)
    a = _check(sims[R], by_slot, ros, BUCKETS[0], "draw", "first")
    b = _check(sims[R], by_slot, ros, BUCKETS[0], "draw", "second")
    for k in SLOT_SHAPES:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    c = _check(sims[R], by_slot, ros, BUCKETS[0], "draw", "counter", counter=COUNTER + 1)
    d = _check(sims[R], by_slot, ros, BUCKETS[0], "draw", "seed", seed=(SEED[0], SEED[1] + 1))
    assert not torch.equal(a["action"], c["action"]) and not torch.equal(a["action"], d["action"])
    # the draw does not depend on the routing: the same logits per ROW under another routing give the same row actions
    other = _routings(R)["random"]
    row_of_slot, other_t = torch.from_numpy(ros).cuda().long(), torch.from_numpy(other).cuda().long()
    by_row = torch.empty_like(by_slot)
    by_row[row_of_slot] = by_slot
    rows_a, rows_b = (torch.zeros(R, 5, dtype=torch.int32, device="cuda") for _ in range(2))
    sims[R].sample_actions_routed(by_slot, torch.from_numpy(ros).cuda(), seed=SEED, counter=COUNTER, action_rows=rows_a, log_prob=True)
    sims[R].sample_actions_routed(by_row[other_t].contiguous(), torch.from_numpy(other).cuda(), seed=SEED, counter=COUNTER, action_rows=rows_b, log_prob=True)
    assert torch.equal(rows_a, rows_b)


def test_bad_slots_write_zeros_and_no_row(sims):
    import torch
    R = 216
    sim = sims[R]
    ros = _routings(R)["random"].copy()
    where = [5, 100, 215]                                                  # a full block, another, and the partial last one
    orphans = ros[where].copy()
    ros[where] = [-1, R, 2 ** 31 - 1]
    by_slot = _logits(R, 19, "float32", 11)
    row_of_slot = torch.from_numpy(ros).cuda()
    rows = torch.full((R, 5), -9, dtype=torch.int32, device="cuda")
    bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")           # zeroed by the call
    out = sim.sample_actions_routed(by_slot, row_of_slot, seed=SEED, counter=COUNTER, action_rows=rows, bad=bad, **ALL)
    assert bad.item() == 3
    for k in SLOT_SHAPES:
        assert not _bits(out[k][where]).any().item(), k                    # all-zero bits
    assert (rows[torch.from_numpy(orphans).long().cuda()] == -9).all().item()
    # every other slot is what the well-formed routing gives
    good = np.setdiff1d(np.arange(R), where)
    full = _routings(R)["random"]
    ref = _check(sim, by_slot, full, BUCKETS[0], "draw", "reference")
    g = torch.from_numpy(good).cuda()
    for k in SLOT_SHAPES:
        assert torch.equal(_bits(out[k][g]), _bits(ref[k][g])), k
    named = torch.from_numpy(full[good]).long().cuda()
    assert torch.equal(rows[named], ref["action"][g])


def test_a_null_action_rows_writes_the_export(sims):
    import torch
    for R in (216, 2):
        sim = sims[R]
        ros = _routings(R)["reversal"]
        by_slot = _logits(R, 19, "bfloat16", 13)
        export = sim.action_tensor().to_torch()
        export.fill_(-3)
        out = sim.sample_actions_routed(by_slot, torch.from_numpy(ros).cuda(), seed=SEED, counter=COUNTER)      # no other output: what League.act does
        assert out["action_rows"].data_ptr() == export.data_ptr()
        given = _check(sim, by_slot, ros, BUCKETS[0], "draw", "export")
        assert torch.equal(export.reshape(R, 5), given["action_rows"])


def test_the_library_refuses():
    """What only the C ABI can tell: evaluate, a flag, overlaps with the export, and every output null with action_rows."""
    import ctypes as C
    import torch
    import gpu_hideseek
    from gpu_hideseek import action_sampling as A
    from gpu_hideseek._native import check
    k = 1
    sim = gpu_hideseek.HideAndSeekSimulator(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=2, sim_flags=0, rand_seed=3,
                                            min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=1)
    try:
        sim.init()
        R = 4
        logits = torch.zeros(R, 19, device="cuda")
        ros = torch.arange(R, dtype=torch.int32, device="cuda")
        lp = torch.zeros(R, device="cuda")
        export = sim.action_tensor().to_torch()

        def refused(what, **change):
            _, req = A.request_routed(R, 0, logits, ros, log_prob=lp)
            for name, v in change.items():
                setattr(req, name, v)
            with pytest.raises(Exception, match=what):
                check(sim._L.hs_sample_actions_routed(sim._h, C.byref(req)))
        refused("mode must be HS_SAMPLE_DRAW or HS_SAMPLE_GREEDY", mode=2)
        refused("flags must be 0", flags=1)
        refused("null row_of_slot", row_of_slot=None)
        refused("null logits", logits=None)
        refused("4-byte aligned", log_prob=lp.data_ptr() + 2)
        refused("logits_stride", logits_stride=18)
        refused("action overlaps action_rows", action=export.data_ptr())                    # the export, named by null
        refused("action_rows overlaps row_of_slot", action_rows=ros.data_ptr())
        refused("log_prob overlaps logits", log_prob=logits.data_ptr())
        refused("every slot-order output is null", action_rows=export.data_ptr(), log_prob=None)
        _, ok = A.request_routed(R, 0, logits, ros, log_prob=lp)
        check(sim._L.hs_sample_actions_routed(sim._h, C.byref(ok)))
    finally:
        sim.close()
