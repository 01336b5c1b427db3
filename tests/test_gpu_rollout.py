"""The minibatch gather on the GPU (hs_gather_sequences, gpu_hideseek.rollout) at the chunk lengths, row widths, grids and
request shapes the trainer uses and at those where a loop of csrc/hs_k_gather.h makes one trip more.  A pure copy: every
comparison is torch.equal on byte views against torch indexing (rollout.gather_eager; test_rollout_host.expected zeroes
the rows of the ids out of range), over sources of every bit pattern, NaNs included.

The tests down to test_the_library_refuses_what_python_cannot_see run at one small geometry: K = 2 chunks of L = 3 steps
over n = 7 rows, m = 5 ids of which one is repeated, over fields of 4, 20 and 592 bytes per row, a per-chunk field of 512
and one of 1024, and a 592-byte field whose base lies 4 bytes past a 16-byte boundary and so moves as dwords; and a source
past 2^31 bytes.

The tests behind them put every dst and `bad` between guard bytes (_Guards) and assert that those are unchanged, take
kGatherInFlight, kGatherMaxGrid, kGatherWaves, kGatherVec and the 64 lanes out of the header's text
(test_rollout_host.kernel_constants) and assert with them the trip they claim.  What each is the first to reach:
  test_chunk_lengths                        gather_wide's `t0 += kGatherInFlight`: a second and a third pass (L = 5, 8, 9), the
                                            ragged pass whose `t0 + q < rows` is false for some q (L = 5, 9; L = 1, 2), a
                                            chunk of one step; `p += 64` a second time (1184 bytes); `perChunk` in
                                            gather_narrow (rows = 1, row0 = s)
  test_row_widths                           `p = lane; p < pieces`: 1 piece (63 lanes idle), 63, 64, 65 (a second trip of
                                            one lane), 128 and 129 (a third); the same rows as dwords because of the dst
                                            alone (launch_gather's `wide`); 600 and 24 bytes: aligned, narrow by `% kGatherVec`;
                                            gather_narrow's `e += 64` up to 41 times
  test_grid_stride                          k_gather's `u += stride`: the grid at its cap, three trips of a wave and a last
                                            one that not every wave makes; `!ok` in a second and third trip, in every slot;
                                            INT32_MIN and INT32_MAX as ids; atomicAdd from hundreds of waves
  test_wide_only_and_narrow_only            `units = nWide * m` with no narrow slot; nWide == 0: the narrow slot is slot 0
                                            and counts; `a.bad` null with bad ids
  test_sixteen_fields_in_request_order      launch_gather's two passes over a full table that interleaves the classes
  test_one_dword                            units = 1: one wave, one lane's store
  test_trainer_geometry                     L = 5 and K = 8 over the 13 fields of Rollout, float32 rows of 1184 bytes and
                                            hidden = 512 (2048-byte rows), two parts of a permutation into one `out`
  test_destination_past_two_to_the_31       `((int64_t)(t0 + q) * m + j) * rb` past 2^31 on the dst side, in gather_wide;
                                            hundreds of trips of `u += stride`
  test_the_seeded_sweep                     src and dst shifted independently by 0, 4, 8, 12; rows of 8, 48 and 1040 bytes;
                                            K = 1, n = 1, m = 1 and whatever 40 seeded mixtures of all of the above hold
  test_every_refusal_of_the_library         every `return c.bad(...)` of check_gather (hideseek.hip)"""
import pytest

import test_rollout_host as H

pytestmark = pytest.mark.gpu

K, L, N, M = 2, 3, 7, 5
IDS = [9, 0, 13, 9, 6]            # 9 twice; 13 = K N - 1, the last sequence; 6 = the last row of chunk 0


@pytest.fixture(scope="module")
def sim():
    import gpu_hideseek
    s = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=2, sim_flags=0, rand_seed=1,
        min_hiders=2, max_hiders=2, min_seekers=1, max_seekers=1, num_pbt_policies=1)
    s.init()
    yield s
    s.close()


def _random(shape, dtype, g):
    import torch
    if dtype == torch.int32:
        return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32).cuda()
    # every bit pattern of the type, NaNs included: the comparison is on bytes
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)
    return (bits.view(torch.float32) if dtype == torch.float32 else (bits >> 16).to(torch.int16).view(dtype)).cuda()


@pytest.fixture(scope="module")
def sources():
    """[(name, src, per_chunk, row bytes)] on the device."""
    import torch
    g = torch.Generator().manual_seed(11)
    T = K * L
    shifted = torch.empty(T * N * 296 + 2, dtype=torch.bfloat16, device="cuda")
    shifted.copy_(_random((T * N * 296 + 2,), torch.bfloat16, g))
    out = [("f32 4", _random((T, N), torch.float32, g), False, 4),
           ("i32 20", _random((T, N, 5), torch.int32, g), False, 20),
           ("bf16 592", _random((T, N, 296), torch.bfloat16, g), False, 592),
           ("bf16 512 per chunk", _random((K, N, 256), torch.bfloat16, g), True, 512),
           ("f32 1024 per chunk", _random((K, N, 256), torch.float32, g), True, 1024),
           ("bf16 592 shifted by 4 bytes", shifted[2:].view(T, N, 296), False, 592)]
    assert out[2][1].data_ptr() % 16 == 0 and out[5][1].data_ptr() % 16 == 4
    return out


def _bytes(t):
    import torch
    return t.contiguous().view(-1).view(torch.uint8)


def _fields(sources, dsts=None):
    return [(src, None if dsts is None else dsts[i], pc) for i, (_, src, pc, _) in enumerate(sources)]


def _expected(sources, index):
    from gpu_hideseek import rollout
    return [rollout.gather_eager(index, src, K, L, N, pc) for _, src, pc, _ in sources]


def test_bit_identical_to_torch_indexing(sim, sources):
    import torch
    from gpu_hideseek import rollout
    index = torch.tensor(IDS, dtype=torch.int32, device="cuda")
    res = sim.gather_sequences(index, _fields(sources), chunks=K, chunk_steps=L, rows=N, bad=True)
    assert res["bad"].item() == 0
    for (name, src, pc, rb), got, want in zip(sources, res["fields"], _expected(sources, index)):
        assert got.dtype == src.dtype and got.shape == want.shape == ((M,) if pc else (L, M)) + tuple(src.shape[2:]), name
        assert rollout._tail_bytes(src) == rb and torch.equal(_bytes(got), _bytes(want)), name
    # the rows by the id formula, once by hand: dst[t, j] = src[k L + t, r]
    for j, (k, r, steps) in enumerate(rollout.sequence_rows(IDS, K, L, N)):
        for t, step in enumerate(steps):
            assert torch.equal(_bytes(res["fields"][2][t, j]), _bytes(sources[2][1][step, r]))
        assert torch.equal(_bytes(res["fields"][4][j]), _bytes(sources[4][1][k, r]))
    # one sequence
    one = torch.tensor([13], dtype=torch.int32, device="cuda")
    res = sim.gather_sequences(one, _fields(sources), chunks=K, chunk_steps=L, rows=N)
    assert "bad" not in res
    for (name, _, pc, _), got, want in zip(sources, res["fields"], _expected(sources, one)):
        assert got.shape[0 if pc else 1] == 1 and torch.equal(_bytes(got), _bytes(want)), name


def test_ids_out_of_range_leave_zero_rows_and_are_counted(sim, sources):
    import torch
    ids = [K * N, 3, -1, 9, 3]
    index = torch.tensor(ids, dtype=torch.int32, device="cuda")
    valid = torch.tensor([0, 3, 0, 9, 3], dtype=torch.int32, device="cuda")
    dsts = [torch.full(((M,) if pc else (L, M)) + tuple(src.shape[2:]), 1, dtype=src.dtype, device="cuda") for _, src, pc, _ in sources]
    bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    res = sim.gather_sequences(index, _fields(sources, dsts), chunks=K, chunk_steps=L, rows=N, bad=bad)
    assert res["bad"] is bad and bad.item() == 2
    for (name, _, pc, _), got, want in zip(sources, res["fields"], _expected(sources, valid)):
        want = want.clone()
        if pc:
            want[[0, 2]] = 0
        else:
            want[:, [0, 2]] = 0
        assert torch.equal(_bytes(got), _bytes(want)), name
        assert not _bytes(got[[0, 2]] if pc else got[:, [0, 2]]).any().item(), name


def test_the_async_form_on_a_side_stream(sim, sources):
    import torch
    index = torch.tensor(IDS, dtype=torch.int32, device="cuda")
    want = _expected(sources, index)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    res = sim.gather_sequences(index, _fields(sources), chunks=K, chunk_steps=L, rows=N, bad=True, stream=stream)
    stream.synchronize()
    assert res["bad"].item() == 0
    for (name, _, _, _), got, w in zip(sources, res["fields"], want):
        assert torch.equal(_bytes(got), _bytes(w)), name


def test_a_rollout_minibatch_reuses_its_outputs(sim):
    import torch
    from gpu_hideseek import rollout
    buf = rollout.Rollout(sim, K * L, K, dtype=torch.bfloat16, rows=N)
    g = torch.Generator().manual_seed(12)
    for t in buf.tensors().values():
        t.copy_(_random(tuple(t.shape), t.dtype, g) if t.dtype != torch.float64 else torch.randn(t.shape, generator=g, dtype=torch.float64))
    index = torch.tensor(IDS, dtype=torch.int32, device="cuda")
    mb = buf.minibatch(index)
    want = buf.minibatch_eager(index)
    assert list(mb) == list(rollout.PER_STEP + rollout.PER_CHUNK)
    assert mb["actor"].shape == (L, M, 296) and mb["actor"].dtype == mb["critic_h"].dtype == torch.bfloat16 and mb["critic_c"].dtype == torch.float32
    for k in mb:
        assert mb[k].shape == want[k].shape and torch.equal(_bytes(mb[k]), _bytes(want[k])), k
    ptrs = {k: t.data_ptr() for k, t in mb.items()}
    other = torch.tensor([1, 2, 3, 4, 5], dtype=torch.int32, device="cuda")
    allocations = torch.cuda.memory_stats()["allocation.all.allocated"]          # a count that only grows: frees elsewhere do not hide one
    again = buf.minibatch(other, out=mb)
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocations
    assert {k: t.data_ptr() for k, t in again.items()} == ptrs and all(again[k] is mb[k] for k in mb)
    want = buf.minibatch_eager(other)
    for k in mb:
        assert torch.equal(_bytes(mb[k]), _bytes(want[k])), k
    with pytest.raises(ValueError, match="dst must be a contiguous"):
        buf.minibatch(other[:3], out=mb)


def test_byte_offsets_past_two_to_the_31(sim):
    """A per-step source just over 2^31 bytes: 2 steps of 1 048 600 rows of 1024 bytes.  Row (1, r) starts at byte
    (1 048 600 + r) * 1024, which is past 2^31 for r > 1 048 552: the last three rows of step 1 lie there."""
    import torch
    n, W = 1048600, 256
    src = torch.empty(2, n, W, dtype=torch.int32, device="cuda")
    assert src.numel() * 4 > 2 ** 31 and (n + n - 3) * 1024 > 2 ** 31
    g = torch.Generator().manual_seed(13)
    known = _random((2, 3, W), torch.int32, g)
    src[:, -3:] = known
    index = torch.tensor([n - 1, n - 3, n - 2], dtype=torch.int32, device="cuda")
    narrow = torch.arange(2 * n, dtype=torch.int32, device="cuda").view(2, n)
    res = sim.gather_sequences(index, [(src, None, False), (narrow, None, False)], chunks=1, chunk_steps=2, rows=n, bad=True)
    assert res["bad"].item() == 0
    got = res["fields"][0]
    assert got.shape == (2, 3, W)
    assert torch.equal(got, known[:, [2, 0, 1]])
    assert res["fields"][1].tolist() == [[n - 1, n - 3, n - 2], [2 * n - 1, 2 * n - 3, 2 * n - 2]]


def test_the_library_refuses_what_python_cannot_see(sim):
    """The library's own check, reached through the raw request: a row_bytes that is no multiple of 4."""
    import ctypes as C
    import torch
    from gpu_hideseek import rollout
    index = torch.tensor(IDS, dtype=torch.int32, device="cuda")
    src = torch.zeros(K * L, N, 2, device="cuda")
    res, req = rollout.request(0, index, [(src, None, False)], K, L, N)
    req.fields[0].row_bytes = 6
    rc = sim._L.hs_gather_sequences(sim._h, C.byref(req))
    assert rc == 1 and "row_bytes" in sim.warning()
    req.fields[0].row_bytes = 8
    req.fields[0].dst = src.data_ptr()
    assert sim._L.hs_gather_sequences(sim._h, C.byref(req)) == 1 and "overlaps" in sim.warning()


# ---- the chunk lengths, row widths, grids and request shapes of training ----
GUARD = 256                                     # bytes of PATTERN on either side of every dst and of bad, at least
PATTERN = 0xA5


class _Guards:
    """Every output of a call inside a larger buffer of PATTERN bytes: empty() cuts a tensor out of one, `shift` bytes
    past a 16-byte boundary and filled with ones; intact() asserts that nothing outside the tensors has changed."""

    def __init__(self):
        self.kept = []

    def empty(self, shape, dtype, shift=0, fill=1):
        import torch
        nbytes = torch.empty((), dtype=dtype).element_size()
        for d in shape:
            nbytes *= int(d)
        raw = torch.empty(GUARD + 16 + nbytes + GUARD, dtype=torch.uint8, device="cuda")
        raw.fill_(PATTERN)
        lead = GUARD + (shift - raw.data_ptr() - GUARD) % 16
        t = raw[lead:lead + nbytes].view(dtype).view(tuple(shape))
        t.fill_(fill)
        assert t.data_ptr() % 16 == shift and lead >= GUARD and raw.numel() - lead - nbytes >= GUARD
        self.kept.append((raw, lead, nbytes))
        return t

    def intact(self, note=""):
        for i, (raw, lead, nbytes) in enumerate(self.kept):
            assert (raw[:lead] == PATTERN).all().item(), f"{note}: bytes in front of output {i} were written"
            assert (raw[lead + nbytes:] == PATTERN).all().item(), f"{note}: bytes behind output {i} were written"


def _row_bytes(t):
    from gpu_hideseek import rollout
    return rollout._tail_bytes(t)


def _shifted(t, shift):
    """A copy of `t` whose base lies `shift` bytes past a 16-byte boundary."""
    import torch
    nbytes = t.numel() * t.element_size()
    raw = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    lead = (shift - raw.data_ptr()) % 16
    out = raw[lead:lead + nbytes].view(t.dtype).view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == shift
    return out


def _gather(sim, K, L, n, ids, specs, bad=True, stream=None, note=""):
    """One call over `specs` = [(src, per_chunk, dst shift)] with guarded outputs, compared field by field with
    H.expected.  Returns (the deal of the work as H.geometry tells it, the dsts)."""
    import torch
    index = torch.tensor(ids, dtype=torch.int32, device="cuda")
    m = len(ids)
    gone = [j for j, s in enumerate(ids) if not 0 <= s < K * n]
    guards = _Guards()
    dsts = [guards.empty(((m,) if pc else (L, m)) + tuple(src.shape[2:]), src.dtype, shift) for src, pc, shift in specs]
    count = guards.empty((1,), torch.int32, fill=77) if bad else None
    want = [H.expected(ids, src, K, L, n, pc) for src, pc, _ in specs]
    torch.cuda.synchronize()
    res = sim.gather_sequences(index, [(src, d, pc) for (src, pc, _), d in zip(specs, dsts)], chunks=K, chunk_steps=L, rows=n, bad=count, stream=stream)
    if stream is not None:
        stream.synchronize()
    assert len(res["fields"]) == len(specs) and all(a is b for a, b in zip(res["fields"], dsts)), note
    if bad:
        assert res["bad"] is count and count.item() == len(gone), (note, count.item(), len(gone))
    else:
        assert "bad" not in res, note
    for i, ((src, pc, shift), got, w) in enumerate(zip(specs, dsts, want)):
        what = f"{note}: field {i} ({_row_bytes(src)} bytes, {'per chunk' if pc else 'per step'}, dst + {shift})"
        assert got.shape == w.shape and got.dtype == w.dtype, what
        assert torch.equal(_bytes(got), _bytes(w)), what
        if gone:
            assert not _bytes(got[gone] if pc else got[:, gone]).any().item(), what
    guards.intact(note)
    return H.geometry([(_row_bytes(src), src.data_ptr(), d.data_ptr()) for (src, _, _), d in zip(specs, dsts)], m), dsts


PASSES = {1: (0, 1), 2: (0, 2), 4: (1, 0), 5: (1, 1), 8: (2, 0), 9: (2, 1)}       # L: full passes of the rows in flight, rows of the ragged one


@pytest.mark.parametrize("L", sorted(PASSES))
def test_chunk_lengths(sim, L):
    """L = 5 is TrainConfig's (T = 40, K = 8), L = 4 test_gpu_trainer's."""
    import torch
    c = H.kernel_constants()
    assert divmod(L, c.in_flight) == PASSES[L]
    K, n = 2, 7
    g = torch.Generator().manual_seed(100 + L)
    specs = [(_random((K * L, n, 296), torch.bfloat16, g), False, 0), (_random((K * L, n, 296), torch.float32, g), False, 0),
             (_random((K * L, n), torch.float32, g), False, 0), (_random((K * L, n, 5), torch.int32, g), False, 0),
             (_random((K, n, 256), torch.bfloat16, g), True, 0), (_random((K, n), torch.float32, g), True, 0)]
    assert [_row_bytes(s) for s, _, _ in specs] == [592, 1184, 4, 20, 512, 4] and 1184 // c.vec == 74 > c.lanes
    geo, _ = _gather(sim, K, L, n, IDS, specs, note=f"L = {L}")
    assert geo.wide == [True, True, False, False, True, False] and geo.units == 4 * len(IDS)


PIECES = {16: 1, 1008: 63, 1024: 64, 1040: 65, 2048: 128, 2064: 129, 600: None, 24: None}      # row bytes: 16-byte pieces (None: no multiple of 16)


@pytest.mark.parametrize("width", list(PIECES))
def test_row_widths(sim, width):
    """A width as a per-step field at L = 5 and as a per-chunk field; then the same two with the dst 4 bytes past a
    16-byte boundary and the src on one, which move as dwords and give the same bytes.  2048 bytes is a float32 state of
    Rollout(hidden=512)."""
    import torch
    c = H.kernel_constants()
    K, L, n = 2, 5, 7
    g = torch.Generator().manual_seed(width)
    step, chunk = _random((K * L, n, width // 4), torch.float32, g), _random((K, n, width // 2), torch.bfloat16, g)
    assert _row_bytes(step) == _row_bytes(chunk) == width and step.data_ptr() % 16 == chunk.data_ptr() % 16 == 0
    geo, aligned = _gather(sim, K, L, n, IDS, [(step, False, 0), (chunk, True, 0)], note=f"{width} bytes")
    if PIECES[width] is None:
        assert width % c.vec and width % 4 == 0 and geo.wide == [False, False]
        return
    assert width // c.vec == PIECES[width] and geo.wide == [True, True]
    assert -(-PIECES[width] // c.lanes) == {1: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 3}[PIECES[width]]          # trips of `p += 64`
    geo, shifted = _gather(sim, K, L, n, IDS, [(step, False, 4), (chunk, True, 4)], note=f"{width} bytes, dst + 4")
    assert geo.wide == [False, False] and geo.units == len(IDS)
    for a, b in zip(aligned, shifted):
        assert torch.equal(_bytes(a), _bytes(b))


def _six_fields(K, L, n, g):
    """Four wide fields and two narrow ones."""
    import torch
    return [(_random((K * L, n, 296), torch.bfloat16, g), False, 0), (_random((K * L, n), torch.float32, g), False, 0),
            (_random((K, n, 256), torch.bfloat16, g), True, 0), (_random((K * L, n, 296), torch.float32, g), False, 0),
            (_random((K * L, n, 5), torch.int32, g), False, 0), (_random((K, n, 256), torch.float32, g), True, 0)]


def test_grid_stride(sim):
    """units = 5 slots x 3400 ids = 17 000 > 2 x 8192: every wave makes two trips of `u += stride`, the first 616 a
    third.  A tenth of the ids are out of range on both sides; each j is met in one trip or another by the waves of the
    five slots, and the test asserts that bad ones are met in a first, a second and a third."""
    import torch
    c = H.kernel_constants()
    K, L, n, m = 2, 5, 50, 3400
    g = torch.Generator().manual_seed(31)
    ids = torch.randint(0, K * n, (m,), generator=g).tolist()
    assert len(set(ids)) < m
    where = torch.randperm(m, generator=g)[:m // 10].tolist()
    values = [-2 ** 31, 2 ** 31 - 1, -1, K * n] + H.outside(K * n)
    for i, j in enumerate(where):
        ids[j] = values[i % len(values)]
    assert {-2 ** 31, 2 ** 31 - 1, -1, K * n} <= set(ids)
    specs = _six_fields(K, L, n, g)
    geo, dsts = _gather(sim, K, L, n, ids, specs, note="blocking")
    assert geo.n_wide == 4 and geo.slots == 5 and geo.stride == c.max_grid * c.waves
    assert geo.units > 2 * c.max_grid * c.waves and geo.units % geo.stride and geo.trips == 3
    assert {(slot * m + j) // geo.stride for slot in range(geo.slots) for j in where} == {0, 1, 2}
    assert {(slot * m + j) // geo.stride for slot in range(geo.n_wide) for j in where} == {0, 1}           # the third trip's are narrow units
    kept = [_bytes(d).clone() for d in dsts]
    geo, dsts = _gather(sim, K, L, n, ids, specs, stream=torch.cuda.Stream(), note="on a side stream")
    assert geo.trips == 3 and all(torch.equal(_bytes(d), k) for d, k in zip(dsts, kept))


@pytest.mark.parametrize("bad_ids", [False, True])
@pytest.mark.parametrize("count", [False, True])
@pytest.mark.parametrize("kind", ["wide", "narrow"])
def test_wide_only_and_narrow_only(sim, kind, count, bad_ids):
    import torch
    K, L, n = 2, 5, 7
    g = torch.Generator().manual_seed(41)
    if kind == "wide":
        specs = [(_random((K * L, n, 296), torch.bfloat16, g), False, 0), (_random((K, n, 256), torch.bfloat16, g), True, 0),
                 (_random((K * L, n, 296), torch.float32, g), False, 0)]
    else:
        specs = [(_random((K * L, n), torch.float32, g), False, 0), (_random((K * L, n, 5), torch.int32, g), False, 0),
                 (_random((K, n), torch.int32, g), True, 0), (_random((K * L, n, 296), torch.bfloat16, g), False, 4)]
    ids = [K * n, 3, -2 ** 31, 9, 3, 2 ** 31 - 1, 13] if bad_ids else [12, 3, 0, 9, 3, 13, 6]
    geo, _ = _gather(sim, K, L, n, ids, specs, bad=count, note=f"{kind} fields only")
    if kind == "wide":
        assert geo.wide == [True] * 3 and geo.slots == 3 and geo.units == 3 * len(ids)
    else:
        assert geo.wide == [False] * 4 and geo.n_wide == 0 and geo.slots == 1 and geo.units == len(ids)


def test_sixteen_fields_in_request_order(sim):
    """All HS_GATHER_MAX_FIELDS fields, wide and narrow, per step and per chunk, in an order that interleaves the classes:
    the kernel takes the wide ones first, and the results come back in the order of the request."""
    import torch
    from gpu_hideseek import rollout
    K, L, n = 2, 5, 7
    g = torch.Generator().manual_seed(51)
    step, chunk = (lambda *tail: (K * L, n) + tail), (lambda *tail: (K, n) + tail)
    bf16, f32, i32 = torch.bfloat16, torch.float32, torch.int32
    specs = [(_random(step(), f32, g), False, 0), (_random(step(296), bf16, g), False, 0), (_random(chunk(), i32, g), True, 0), (_random(chunk(256), bf16, g), True, 0),
             (_random(step(296), bf16, g), False, 4), (_random(step(296), bf16, g), False, 0), (_random(step(5), i32, g), False, 0), (_random(chunk(256), f32, g), True, 0),
             (_random(chunk(256), f32, g), True, 8), (_random(step(296), f32, g), False, 0), (_random(step(), i32, g), False, 0), (_random(chunk(256), bf16, g), True, 0),
             (_random(step(150), f32, g), False, 0), (_random(step(4), f32, g), False, 0), (_random(chunk(6), bf16, g), True, 0), (_random(step(296), bf16, g), False, 0)]
    assert len(specs) == rollout.MAX_FIELDS == 16
    for ids in (IDS, [K * n, 3, -1, 9, 3]):
        geo, _ = _gather(sim, K, L, n, ids, specs, note="16 fields")
        assert geo.wide == [False, True, False, True, False, True, False, True, False, True, False, True, False, True, False, True]
        assert geo.slots == 9 and geo.units == 9 * len(ids)


def test_one_dword(sim):
    import torch
    g = torch.Generator().manual_seed(61)
    for s in (13, 0, 14):
        geo, _ = _gather(sim, 2, 3, 7, [s], [(_random((6, 7), torch.float32, g), False, 0)], note=f"one id {s}")
        assert geo.units == 1 and geo.stride == H.kernel_constants().waves


@pytest.mark.parametrize("dtype, hidden", [("float32", 256), ("bfloat16", 256), ("bfloat16", 64), ("float32", 512)])
def test_trainer_geometry(sim, dtype, hidden):
    """TrainConfig's T = 40 and K = 8 with 36 rows in place of 96 000: the 288 sequences of a device permutation in two
    parts, both gathered into one `out`, and between them every row of `actor` exactly once."""
    import torch
    from gpu_hideseek import rollout
    c = H.kernel_constants()
    dtype = getattr(torch, dtype)
    buf = rollout.Rollout(sim, 40, 8, dtype, hidden, rows=36)
    T, K, L, n = 40, 8, 5, 36
    assert (buf.chunk_steps, buf.sequences) == (L, K * n) == (5, 288) and divmod(L, c.in_flight) == (1, 1)
    g = torch.Generator().manual_seed(71)
    for t in buf.tensors().values():
        t.copy_(_random(tuple(t.shape), t.dtype, g) if t.dtype != torch.float64 else torch.randn(t.shape, generator=g, dtype=torch.float64))
    rows = buf.actor.view(T * n, -1).view(torch.int32)                     # the first dword of a row of actor is its number: the rows are distinct
    rows[:, 0] = torch.arange(T * n, dtype=torch.int32, device="cuda")
    widths = {k: rollout._tail_bytes(getattr(buf, k)) for k in rollout.PER_STEP + rollout.PER_CHUNK}
    assert widths["actor"] == 296 * buf.actor.element_size() and widths["actor_c"] == 4 * hidden
    if (dtype, hidden) == (torch.float32, 512):
        assert widths["actor"] // c.vec == 74 > c.lanes and widths["critic_c"] // c.vec == 128 == 2 * c.lanes
    perm = torch.randperm(buf.sequences, device="cuda", generator=torch.Generator(device="cuda").manual_seed(72)).to(torch.int32)
    parts = rollout.epoch_parts(perm, 2)
    m = 144
    guards = _Guards()
    out = {k: guards.empty(((m,) if k in rollout.PER_CHUNK else (L, m)) + tuple(getattr(buf, k).shape[2:]), getattr(buf, k).dtype)
           for k in rollout.PER_STEP + rollout.PER_CHUNK}
    seen = []
    for part in parts:
        assert part.shape == (m,)
        mb = buf.minibatch(part, out=out)
        want = buf.minibatch_eager(part)
        assert list(mb) == list(want) and all(mb[k] is out[k] for k in out)
        for k in mb:
            assert mb[k].shape == want[k].shape and torch.equal(_bytes(mb[k]), _bytes(want[k])), k
        guards.intact(f"part of {m}")
        seen.append(mb["actor"].clone())
    both = torch.cat(seen, dim=1).view(T * n, -1).view(torch.int32)
    assert torch.equal(both[both[:, 0].long().argsort()], rows), "the two parts hold every row of actor once"
    geo = H.geometry([(widths[k], getattr(buf, k).data_ptr(), out[k].data_ptr()) for k in out], m, c)
    assert geo.wide == [widths[k] % c.vec == 0 for k in out] and geo.n_wide == 6 and geo.units == 7 * m


def test_destination_past_two_to_the_31(sim):
    """The mirror of test_byte_offsets_past_two_to_the_31: a source of 6 rows and a dst [2, 1 048 600, 256] int32 of
    2 147 532 800 bytes.  Row (t, j) of the dst starts at byte (t m + j) 1024: step 1 starts past 2^30 and its last 48 rows
    start at 2^31 and behind it.  units = 2 m: every wave goes round `u += stride` 256 times.  The expected dst is not built: step 1 is
    compared in slices of 2^17 ids, step 0 in its first and last slice."""
    import torch
    c = H.kernel_constants()
    K, L, n, m, W, S = 1, 2, 3, 1048600, 256, 2 ** 17
    assert 2 * m * 1024 > 2 ** 31 and (2 * m - 48) * 1024 == 2 ** 31 and m * 1024 > 2 ** 30
    g = torch.Generator().manual_seed(81)
    wide, narrow = _random((L, n, W), torch.int32, g), _random((L, n), torch.int32, g)
    ids = torch.randint(0, n, (m,), generator=g)
    ids[-3:] = torch.tensor([2, 0, 1])
    index = ids.to(torch.int32).cuda()
    guards = _Guards()
    dst, small, count = guards.empty((L, m, W), torch.int32), guards.empty((L, m), torch.int32), guards.empty((1,), torch.int32, fill=77)
    assert dst.numel() * 4 > 2 ** 31 and dst.data_ptr() % 16 == 0
    geo = H.geometry([(1024, wide.data_ptr(), dst.data_ptr()), (4, narrow.data_ptr(), small.data_ptr())], m, c)
    assert geo.wide == [True, False] and geo.units == 2 * m and geo.trips > 200
    res = sim.gather_sequences(index, [(wide, dst, False), (narrow, small, False)], chunks=K, chunk_steps=L, rows=n, bad=count)
    assert res["fields"][0] is dst and res["fields"][1] is small and count.item() == 0
    guards.intact("a dst past 2^31 bytes")
    rows = index.long()
    for t, a in [(1, a) for a in range(0, m, S)] + [(0, 0), (0, m - S)]:
        assert torch.equal(dst[t, a:a + S], wide[t][rows[a:a + S]]), (t, a)
    assert torch.equal(dst[1, -3:], wide[1][[2, 0, 1]])
    assert torch.equal(small, narrow[:, rows])
    del dst, small, res, guards
    torch.cuda.empty_cache()


def test_the_seeded_sweep(sim):
    """The 40 configurations of test_rollout_host.gather_configs, whose reference test_rollout_host pins on the CPU."""
    import torch
    g = torch.Generator().manual_seed(91)
    for cfg in H.gather_configs():
        K, L, n = cfg["K"], cfg["L"], cfg["n"]
        specs = [(_shifted(_random(H.source_shape(f, K, L, n), getattr(torch, f["dtype"]), g), f["src_shift"]), f["per_chunk"], f["dst_shift"]) for f in cfg["fields"]]
        geo, _ = _gather(sim, K, L, n, cfg["ids"], specs, note=str(cfg))
        assert geo.wide == [f["row_bytes"] % 16 == 0 and f["src_shift"] == f["dst_shift"] == 0 for f in cfg["fields"]], cfg


def test_every_refusal_of_the_library(sim):
    """Every refusal of check_gather, through the raw request in both forms: each returns HS_ERR_INVALID_ARG, the message
    names the entry point and the cause, and every dst and `bad` keeps its bytes."""
    import ctypes as C
    import torch
    from gpu_hideseek import rollout
    INVALID = 1
    index = torch.tensor(IDS, dtype=torch.int32, device="cuda")
    srcs = [torch.ones(K * L, N, 4, device="cuda"), torch.ones(K, N, 2, dtype=torch.int32, device="cuda")]
    guards = _Guards()
    dsts = [guards.empty((L, M, 4), torch.float32), guards.empty((M, 2), torch.int32)]
    count = guards.empty((1,), torch.int32, fill=77)
    _, base = rollout.request(0, index, [(srcs[0], dsts[0], False), (srcs[1], dsts[1], True)], K, L, N, bad=count)
    saved = [_bytes(t).clone() for t in dsts + [count]]
    stream = torch.cuda.Stream()

    def refused(cause, **change):
        for form in ("hs_gather_sequences", "hs_gather_sequences_async"):
            req = rollout.HsGatherRequest.from_buffer_copy(base)
            for k, v in change.items():
                if "_" in k and k.split("_")[0] in ("f0", "f1"):
                    setattr(req.fields[int(k[1])], k[3:], v)
                else:
                    setattr(req, k, v)
            args = (sim._h, C.byref(req)) if form == "hs_gather_sequences" else (sim._h, C.c_void_p(stream.cuda_stream), C.byref(req))
            assert getattr(sim._L, form)(*args) == INVALID, (cause, change)
            assert sim.warning().startswith("hs_gather_sequences: ") and cause in sim.warning(), (cause, change, sim.warning())
            torch.cuda.synchronize()
            assert all(torch.equal(_bytes(t), s) for t, s in zip(dsts + [count], saved)), (cause, change)
            guards.intact(cause)

    P = lambda t: t.data_ptr()                                             # noqa: E731
    assert sim._L.hs_gather_sequences(sim._h, None) == INVALID and "hs_gather_sequences: null request" in sim.warning()
    refused("null index", index=None)
    for size in ("m", "chunks", "chunk_steps", "rows"):
        refused("m, chunks, chunk_steps and rows must be at least 1", **{size: 0})
    refused("chunks * rows must stay below 2^31", chunks=2 ** 16, rows=2 ** 15)
    refused("num_fields must be in [1, HS_GATHER_MAX_FIELDS]", num_fields=0)
    refused("num_fields must be in [1, HS_GATHER_MAX_FIELDS]", num_fields=rollout.MAX_FIELDS + 1)
    refused("field 0: null src or dst", f0_src=None)
    refused("field 1: null src or dst", f1_dst=None)
    for row_bytes in (0, 6, rollout.MAX_ROW_BYTES + 4):
        refused("field 1: row_bytes must be a multiple of 4 in [4, HS_GATHER_MAX_ROW_BYTES]", f1_row_bytes=row_bytes)
    refused("field 0: src and dst must be 4-byte aligned", f0_src=P(srcs[0]) + 2)
    refused("field 1: src and dst must be 4-byte aligned", f1_dst=P(dsts[1]) + 2)
    refused("index and bad must be 4-byte aligned", index=P(index) + 2)
    refused("index and bad must be 4-byte aligned", bad=P(count) + 2)
    refused("field 0: dst overlaps index", f0_dst=P(index))
    refused("field 0: dst overlaps the src of field 1", f0_dst=P(srcs[1]))
    refused("field 1: dst overlaps the dst of field 0", f1_dst=P(dsts[0]) + 16)
    refused("bad overlaps the dst of field 0", bad=P(dsts[0]) + 4)
    # and the request itself is good: the same bytes as torch indexing, the guards untouched
    assert sim._L.hs_gather_sequences(sim._h, C.byref(base)) == 0 and count.item() == 0
    for src, dst, pc in ((srcs[0], dsts[0], False), (srcs[1], dsts[1], True)):
        assert torch.equal(_bytes(dst), _bytes(H.expected(IDS, src, K, L, N, pc)))
    guards.intact("the request as it was built")
