"""The minibatch gather on the GPU (hs_gather_sequences, gpu_hideseek.rollout): K = 2 chunks of L = 3 steps over n = 7 rows,
m = 5 ids of which one is repeated, over fields of 4, 20 and 592 bytes per row, a per-chunk field of 512 and one of 1024,
and a 592-byte field whose base lies 4 bytes past a 16-byte boundary and so moves as dwords.  A pure copy: every comparison
is torch.equal on byte views against torch indexing."""
import pytest

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
