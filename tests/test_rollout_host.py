"""The rollout buffer and the minibatch gather without a GPU (gpu_hideseek.rollout, hs_gather_sequences): the refusals of
request(), Rollout() and epoch_parts() before the library is involved, minibatch_eager() on a hand-written buffer against
the id formula s = k n + r, an epoch's parts as a partition of the sequence ids, and the header against the ctypes mirror.
The last part is shared with tests/test_gpu_rollout.py: the kernel's constants out of the header's text, launch_gather's
deal of the work restated, the 40 seeded configurations of the sweep, and the reference of every GPU comparison, which is
pinned here against a plain loop over rollout.sequence_rows."""
import ctypes as C
import os
import re

import pytest
import torch

K, L, N = 2, 3, 4


class _Sim:
    """What Rollout() reads of a simulator."""
    gpu_id, num_worlds, agents_per_world = 0, 2, 2


def _src(lead, tail=(), dtype=torch.float32):
    return torch.zeros((lead, N) + tail, dtype=dtype)


def _index(m=5):
    return torch.zeros(m, dtype=torch.int32)


def _request(index, fields, **kw):
    from gpu_hideseek import rollout
    return rollout.request(0, index, fields, kw.pop("chunks", K), kw.pop("chunk_steps", L), kw.pop("rows", N), **kw)


# ---- refusals ----
@pytest.mark.parametrize("what, index, fields", [
    ("index must be a contiguous int32", torch.zeros(5, dtype=torch.int64), [(_src(K * L), None, False)]),
    ("index must be a contiguous int32", torch.zeros(5, 1, dtype=torch.int32), [(_src(K * L), None, False)]),
    ("index must be a contiguous int32", torch.zeros(10, dtype=torch.int32)[::2], [(_src(K * L), None, False)]),
    ("src must be a contiguous tensor of shape (6, 4, ...)", _index(), [(_src(K * L + 1), None, False)]),
    ("src must be a contiguous tensor of shape (2, 4, ...)", _index(), [(_src(K * L), None, True)]),                       # a per-chunk field has K leading rows
    ("it is not contiguous", _index(), [(_src(K * L, (8,))[:, :, ::2], None, False)]),
    ("a row must be a multiple of 4 bytes", _index(), [(_src(K * L, (3,), torch.bfloat16), None, False)]),                  # 6 bytes
    ("a row must be a multiple of 4 bytes", _index(), [(_src(K * L, (), torch.float16), None, False)]),                     # 2 bytes
    ("dst must be a contiguous torch.float32 tensor of shape (3, 5, 2)", _index(), [(_src(K * L, (2,)), torch.zeros(3, 5, 3), False)]),
    ("dst must be a contiguous torch.float32 tensor of shape (5, 2)", _index(), [(_src(K, (2,)), torch.zeros(3, 5, 2), True)]),
    ("its dtype is torch.int32", _index(), [(_src(K * L, (2,)), torch.zeros(3, 5, 2, dtype=torch.int32), False)]),
    ("src must be 4-byte aligned", _index(), [(torch.zeros(K * L * N * 2 + 1, dtype=torch.bfloat16)[1:].view(K * L, N, 2), None, False)]),
    ("dst must be 4-byte aligned", _index(), [(_src(K * L, (2,), torch.bfloat16), torch.zeros(L * 5 * 2 + 1, dtype=torch.bfloat16)[1:].view(L, 5, 2), False)]),
    ("between 1 and 16 fields", _index(), [(_src(K * L), None, False)] * 17),
    ("between 1 and 16 fields", _index(), []),
    ("must be (src, dst or None, per_chunk)", _index(), [(_src(K * L), None)]),
])
def test_a_bad_field_or_index_is_refused(what, index, fields):
    with pytest.raises(ValueError) as e:
        _request(index, fields)
    assert what in str(e.value), str(e.value)


def test_overlapping_outputs_are_refused():
    src, dst = _src(K * L, (2,)), torch.zeros(L, 5, 2)
    with pytest.raises(ValueError, match="field 1: dst overlaps field 0: dst"):
        _request(_index(), [(src, dst, False), (_src(K * L, (2,)), dst, False)])
    with pytest.raises(ValueError, match="field 0: dst overlaps field 0: src"):
        _request(_index(), [(src, src.view(-1)[:L * 5 * 2].view(L, 5, 2), False)])
    idx = torch.zeros(L * 5 * 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="field 0: dst overlaps index"):
        _request(idx[:5], [(_src(K * L, (2,), torch.int32), idx.view(L, 5, 2), False)])
    with pytest.raises(ValueError, match="bad overlaps"):
        _request(idx[:5], [(src, None, False)], bad=idx[2:3])
    with pytest.raises(ValueError, match=r"bad must be a contiguous int32 tensor of shape \(1,\)"):
        _request(_index(), [(src, None, False)], bad=torch.zeros(2, dtype=torch.int32))


def test_sizes_are_refused():
    from gpu_hideseek import rollout
    f = [(_src(K * L), None, False)]
    for kw, what in ((dict(chunks=0), "chunks must be a positive integer"), (dict(chunk_steps=-1), "chunk_steps must be a positive integer"),
                     (dict(rows=True), "rows must be a positive integer"), (dict(chunks=2 ** 16, rows=2 ** 15), "must stay below 2^31")):
        with pytest.raises(ValueError) as e:
            _request(_index(), f, **kw)
        assert what in str(e.value)
    with pytest.raises(ValueError, match=r"steps \(7\) must be a multiple of chunks \(2\)"):
        rollout.Rollout(_Sim(), 7, 2, device="cpu")
    with pytest.raises(ValueError, match="dtype must be"):
        rollout.Rollout(_Sim(), 6, 2, dtype=torch.float64, device="cpu")
    with pytest.raises(ValueError, match="do not divide into 3 minibatches"):
        rollout.epoch_parts(torch.randperm(K * N), 3)
    with pytest.raises(ValueError, match="num_minibatches must be a positive integer"):
        rollout.epoch_parts(torch.randperm(K * N), 0)


def test_a_config_that_does_not_fit_is_refused():
    from gpu_hideseek import trainer
    cfg = trainer.TrainConfig()
    assert (cfg.steps_per_update, cfg.num_bptt_chunks, cfg.num_minibatches, cfg.num_epochs, cfg.lr, cfg.gamma, cfg.gae_lambda, cfg.clip_coef,
            cfg.value_loss_coef, cfg.entropy_coef, cfg.max_grad_norm, cfg.dtype, cfg.seed, cfg.normalise_obs) == (
        40, 8, 2, 4, 1e-4, 0.998, 0.95, 0.2, 1.0, 0.01, 5.0, None, 5, True)             # scripts/jax_train.py's defaults
    trainer.check_config(cfg, 96000)
    for kw, rows, what in ((dict(steps_per_update=41), 6, "must be a multiple of num_bptt_chunks"), (dict(num_minibatches=3), 7, "do not divide into 3 minibatches"),
                           (dict(num_bptt_chunks=0), 6, "num_bptt_chunks must be a positive integer"), (dict(num_epochs=1.5), 6, "num_epochs must be a positive integer")):
        with pytest.raises(ValueError, match=what):
            trainer.check_config(trainer.TrainConfig(**kw), rows)


def test_nothing_reaches_the_library_on_a_cpu_request():
    """A request of CPU tensors passes every check of shape, dtype, alignment and overlap and is refused for its device:
    the last check, and still before the library."""
    with pytest.raises(ValueError, match="must be on cuda:0"):
        _request(_index(), [(_src(K * L, (2,)), None, False)])


# ---- the id formula ----
def _hand_written():
    """A K = 2, L = 3, n = 4 buffer whose every element names its place: per-step value 100 t + 10 r + c, per-chunk
    1000 + 100 k + 10 r + c."""
    from gpu_hideseek import rollout
    buf = rollout.Rollout(_Sim(), K * L, K, hidden=2, device="cpu")
    assert (buf.steps, buf.chunks, buf.chunk_steps, buf.rows, buf.sequences) == (6, 2, 3, 4, 8)
    t, r = torch.arange(K * L).view(-1, 1, 1), torch.arange(N).view(1, -1, 1)
    for name in rollout.PER_STEP:
        x = getattr(buf, name)
        c = torch.arange(x[0, 0].numel()).view(1, 1, -1)
        x.copy_((100 * t + 10 * r + c).view(x.shape).to(x.dtype))
    k = torch.arange(K).view(-1, 1, 1)
    for name in rollout.PER_CHUNK:
        x = getattr(buf, name)
        x.copy_((1000 + 100 * k + 10 * r + torch.arange(2).view(1, 1, -1)).to(x.dtype))
    return buf


def test_minibatch_eager_gives_the_rows_of_the_id_formula():
    from gpu_hideseek import rollout
    buf = _hand_written()
    ids = [5, 0, 7, 5, 3]                                   # 5 = chunk 1 of row 1, twice; 3 = chunk 0 of row 3; 7 = chunk 1 of row 3
    assert [(k, r, ts) for k, r, ts in rollout.sequence_rows(ids, K, L, N)] == [(1, 1, [3, 4, 5]), (0, 0, [0, 1, 2]), (1, 3, [3, 4, 5]),
                                                                               (1, 1, [3, 4, 5]), (0, 3, [0, 1, 2])]
    mb = buf.minibatch_eager(torch.tensor(ids, dtype=torch.int32))
    assert set(mb) == set(rollout.PER_STEP + rollout.PER_CHUNK)
    assert mb["actor"].shape == (L, 5, 296) and mb["action"].shape == (L, 5, 5) and mb["clear"].shape == (L, 5) and mb["critic_c"].shape == (5, 2)
    assert mb["actor"].dtype == torch.float32 and mb["action"].dtype == mb["clear"].dtype == torch.int32
    for j, (k, r, ts) in enumerate(rollout.sequence_rows(ids, K, L, N)):
        for t, step in enumerate(ts):
            assert mb["log_prob"][t, j].item() == 100 * step + 10 * r
            assert mb["clear"][t, j].item() == 100 * step + 10 * r
            assert mb["action"][t, j].tolist() == [100 * step + 10 * r + c for c in range(5)]
            assert mb["critic"][t, j, 295].item() == 100 * step + 10 * r + 295
        for name in rollout.PER_CHUNK:
            assert mb[name][j].tolist() == [1000 + 100 * k + 10 * r, 1000 + 100 * k + 10 * r + 1], name
    with pytest.raises(ValueError, match="outside"):
        rollout.sequence_rows([8], K, L, N)


def test_the_parts_of_an_epoch_hold_every_sequence_once():
    from gpu_hideseek import rollout
    g = torch.Generator().manual_seed(0)
    for total, parts in ((8, 2), (8, 1), (84, 4), (12, 12)):
        perm = torch.randperm(total, generator=g).to(torch.int32)
        cut = rollout.epoch_parts(perm, parts)
        assert len(cut) == parts and all(c.shape == (total // parts,) for c in cut)
        assert sorted(torch.cat(cut).tolist()) == list(range(total))
        assert all(c.data_ptr() == perm.data_ptr() + 4 * i * (total // parts) for i, c in enumerate(cut)), "views of the permutation, no copies"


def test_the_field_table_of_a_minibatch():
    from gpu_hideseek import rollout
    buf = _hand_written()
    table = buf.fields()
    assert len(table) == len(rollout.PER_STEP) + len(rollout.PER_CHUNK) <= rollout.MAX_FIELDS
    assert [pc for _, _, pc in table] == [False] * 9 + [True] * 4 and all(d is None for _, d, _ in table)
    assert table[0][0] is buf.actor and table[-1][0] is buf.critic_c
    out = buf.minibatch_eager(torch.tensor([1, 2], dtype=torch.int32))
    assert all(d is out[k] for (_, d, _), k in zip(buf.fields(out), rollout.PER_STEP + rollout.PER_CHUNK))
    # the widths the kernel's two paths are for: 16-byte pieces for the rows and the states, dwords for the rest
    big = rollout.Rollout(_Sim(), 6, 2, dtype=torch.bfloat16, device="cpu")
    widths = {k: rollout._tail_bytes(getattr(big, k)) for k in rollout.PER_STEP + rollout.PER_CHUNK}
    assert widths == dict(actor=592, critic=592, action=20, log_prob=4, value=4, advantage=4, returns=4, mask=4, clear=4,
                          actor_h=512, actor_c=1024, critic_h=512, critic_c=1024)
    assert big.moments.shape == (6, 593) and big.moments.dtype == torch.float64 and big.done.dtype == torch.int32 and big.actor_c.dtype == torch.float32


# ---- the header ----
CTYPES = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "double": C.c_double}


def _struct_fields(src, name, known):
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.replace("const", "").split()
        if words:
            for part in " ".join(words[1:]).split(","):
                part = part.strip()
                array = re.fullmatch(r"(\w+)\[(\w+)\]", part)
                if array:
                    fields.append((array.group(1), known[words[0]] * known[array.group(2)]))
                else:
                    fields.append((part.lstrip("*").strip(), C.c_void_p if part.startswith("*") else known[words[0]]))
    return fields


def test_header_states_the_request(hideseek_lib):
    """include/hideseek.h declares the two entry points, the ctypes mirrors agree with it field by field in name and type,
    and the kernel's constants are the module's."""
    from gpu_hideseek import _native, rollout
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hideseek.h")).read()
    for name, value in (("HS_GATHER_MAX_FIELDS", rollout.MAX_FIELDS), ("HS_GATHER_MAX_ROW_BYTES", rollout.MAX_ROW_BYTES)):
        assert re.search(rf"{name} = (\d+)", src).group(1) == str(value), name
    assert re.search(r"int32_t hs_gather_sequences\(hs_sim \*\w*, const hs_gather_request \*\w*\);", src)
    assert re.search(r"int32_t hs_gather_sequences_async\(hs_sim \*\w*, void \*hip_stream, const hs_gather_request \*\w*\);", src)
    known = dict(CTYPES, HS_GATHER_MAX_FIELDS=rollout.MAX_FIELDS)
    field = _struct_fields(src, "hs_gather_field", known)
    assert field == list(rollout.HsGatherField._fields_), field
    F = rollout.HsGatherField
    assert C.sizeof(F) == 24 and F.dst.offset == 8 and F.row_bytes.offset == 16 and F.per_chunk.offset == 20
    known["hs_gather_field"] = rollout.HsGatherField
    fields = _struct_fields(src, "hs_gather_request", known)
    mirror = list(rollout.HsGatherRequest._fields_)
    assert [f[0] for f in fields] == [f[0] for f in mirror] == ["index", "m", "chunks", "chunk_steps", "rows", "num_fields", "reserved", "bad", "fields"]
    assert all(a[1] is b[1] or (C.sizeof(a[1]) == C.sizeof(b[1]) == 24 * 16 and a[1]._type_ is b[1]._type_) for a, b in zip(fields, mirror))
    R = rollout.HsGatherRequest
    assert C.sizeof(R) == 424 and R.m.offset == 8 and R.chunks.offset == 12 and R.chunk_steps.offset == 16 and R.rows.offset == 20
    assert R.num_fields.offset == 24 and R.bad.offset == 32 and R.fields.offset == 40
    lib = C.CDLL(hideseek_lib)
    assert hasattr(lib, "hs_gather_sequences") and hasattr(lib, "hs_gather_sequences_async")
    assert "hs_gather_sequences" in open(_native.__file__).read()
    for phrase in ("s = k n + r", "dst[t][j] = src[k_j L + t][r_j]", "dst[j] = src[k_j][r_j]", "never reads outside a source"):
        assert phrase in src, phrase
    csrc = os.path.join(root, "marl-hideandseek_amd", "csrc")
    kernel, host = (open(os.path.join(csrc, f)).read() for f in ("hs_k_gather.h", "hideseek.hip"))
    assert int(re.search(r"kGatherMaxFields = (\d+);", kernel).group(1)) == rollout.MAX_FIELDS
    assert int(re.search(r"kGatherVec = (\d+);", kernel).group(1)) == rollout.VEC
    assert "HS_GATHER_MAX_FIELDS == hs::kGatherMaxFields" in host
    # a bandwidth kernel: no LDS, and the one atomic is the count of the bad ids
    assert "__shared__" not in kernel and len(re.findall(r"atomic\w*\(", kernel)) == 1 and "atomicAdd(a.bad, 1)" in kernel
    assert len(re.findall(r"__global__", kernel)) == len(re.findall(r"template <int kThreads = kGatherThreads>\n__global__", kernel)) == 1


# ---- what tests/test_gpu_rollout.py shares: the kernel's constants, its deal of the work, the seeded configurations ----
class _Constants:
    pass


def kernel_constants():
    """kGatherInFlight, kGatherMaxGrid, kGatherWaves, kGatherVec and the 64 lanes of a wave, out of the text of
    csrc/hs_k_gather.h: a test that claims a trip count asserts it with these, so that a changed constant fails it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "marl-hideandseek_amd", "csrc", "hs_k_gather.h")).read()
    c = _Constants()
    threads = int(re.search(r"kGatherThreads = (\d+);", text).group(1))
    c.lanes = int(re.search(r"kGatherWaves = kGatherThreads / (\d+);", text).group(1))
    c.waves = threads // c.lanes
    c.in_flight = int(re.search(r"kGatherInFlight = (\d+);", text).group(1))
    c.max_grid = int(re.search(r"kGatherMaxGrid = (\d+);", text).group(1))
    c.vec = int(re.search(r"kGatherVec = (\d+);", text).group(1))
    # the strides of the three lane loops and of the grid are written with the same numbers
    for phrase in (f"p += {c.lanes})", f"e += {c.lanes})", f"threadIdx.x % {c.lanes}", f"threadIdx.x / {c.lanes}", "t0 += kGatherInFlight", "gridDim.x * kGatherWaves",
                   "u += stride"):
        assert phrase in text, phrase
    return c


class _Geometry:
    pass


def geometry(fields, m, c=None):
    """launch_gather's deal of a request, restated: `fields` is [(row_bytes, src address, dst address)].  .wide[i] says
    whether field i moves as kGatherVec-byte pieces, .slots is the wide fields plus one for all the narrow ones, .units
    = slots * m, .stride the waves of the capped grid and .trips how often the busiest wave goes round `u += stride`."""
    c = c or kernel_constants()
    g = _Geometry()
    g.wide = [rb % c.vec == 0 and src % c.vec == 0 and dst % c.vec == 0 for rb, src, dst in fields]
    g.n_wide = sum(g.wide)
    g.slots = g.n_wide + (1 if g.n_wide < len(fields) else 0)
    g.units = g.slots * m
    g.stride = min(-(-g.units // c.waves), c.max_grid) * c.waves
    g.trips = -(-g.units // g.stride)
    return g


SWEEP_ROW_BYTES = (4, 8, 20, 48, 512, 592, 1040)
SWEEP_SHIFTS = (0, 4, 8, 12)
SWEEP_DTYPES = {"float32": 4, "bfloat16": 2, "int32": 4}


def outside(total):
    """Ids that are no sequence of a rollout of `total`, on both sides."""
    return [-1, total, total + 1, -total, -2 ** 31, 2 ** 31 - 1]


def gather_configs(count=40, seed=20260):
    """The seeded sweep: `count` configurations from one numpy generator.  K in [1, 4], L in [1, 9], n in [1, 70], m in
    [1, 300]; 1 to 16 fields of a row width out of SWEEP_ROW_BYTES, per step or per chunk, src and dst each shifted by
    0, 4, 8 or 12 bytes from a 16-byte boundary; ids that repeat, 0 to 3 of them out of range."""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for number in range(count):
        K, L, n, m = (int(rng.integers(lo, hi + 1)) for lo, hi in ((1, 4), (1, 9), (1, 70), (1, 300)))
        fields = []
        for _ in range(int(rng.integers(1, 17))):
            fields.append(dict(row_bytes=int(rng.choice(SWEEP_ROW_BYTES)), per_chunk=bool(rng.integers(2)), dtype=str(rng.choice(sorted(SWEEP_DTYPES))),
                               src_shift=int(rng.choice(SWEEP_SHIFTS)), dst_shift=int(rng.choice(SWEEP_SHIFTS))))
        ids = [int(s) for s in rng.integers(0, K * n, m)]
        bad = min(int(rng.integers(0, 4)), m)
        for j, s in zip(rng.choice(m, bad, replace=False), rng.choice(outside(K * n), bad)):
            ids[int(j)] = int(s)
        out.append(dict(number=number, K=K, L=L, n=n, m=m, fields=fields, ids=ids, bad=bad))
    return out


def source_shape(field, K, L, n):
    """The shape of the src of a field of gather_configs()."""
    elements = field["row_bytes"] // SWEEP_DTYPES[field["dtype"]]
    return (K if field["per_chunk"] else K * L, n) + (() if elements == 1 else (elements,))


def random_bits(shape, dtype, g):
    """A CPU tensor of every bit pattern of the type, NaNs included."""
    bits = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)
    return bits if dtype == torch.int32 else bits.view(torch.float32) if dtype == torch.float32 else (bits >> 16).to(torch.int16).view(dtype)


def expected(ids, src, chunks, chunk_steps, rows, per_chunk):
    """The reference of every comparison: rollout.gather_eager (torch indexing) on the device of `src`, the ids out of
    range replaced by a valid one and their rows zeroed."""
    from gpu_hideseek import rollout
    idx = torch.as_tensor(ids).long()
    ok = (idx >= 0) & (idx < chunks * rows)
    valid = torch.where(ok, idx, torch.zeros_like(idx)).to(torch.int32).to(src.device)
    want = rollout.gather_eager(valid, src, chunks, chunk_steps, rows, per_chunk).clone()
    gone = (~ok).nonzero().flatten().to(src.device)
    if per_chunk:
        want[gone] = 0
    else:
        want[:, gone] = 0
    return want


def _by_the_formula(ids, src, chunks, chunk_steps, rows, per_chunk):
    """The same as bytes [L, m, row bytes] (or [m, row bytes]) by a plain loop over rollout.sequence_rows."""
    import numpy as np
    from gpu_hideseek import rollout
    a = src.contiguous().view(-1).view(torch.uint8).numpy().reshape(src.shape[0], rows, -1)
    dst = np.zeros(((len(ids),) if per_chunk else (chunk_steps, len(ids))) + (a.shape[2],), np.uint8)
    for j, s in enumerate(ids):
        if 0 <= s < chunks * rows:
            (k, r, steps), = rollout.sequence_rows([s], chunks, chunk_steps, rows)
            if per_chunk:
                dst[j] = a[k, r]
            else:
                for t, step in enumerate(steps):
                    dst[t, j] = a[step, r]
    return dst


def test_the_constants_and_the_deal_of_the_work():
    c = kernel_constants()
    assert (c.lanes, c.waves, c.in_flight, c.max_grid, c.vec) == (64, 4, 4, 2048, 16)
    g = geometry([(592, 0x1000, 0x2000), (4, 0x1000, 0x2000), (592, 0x1004, 0x2000), (592, 0x1000, 0x2004), (600, 0x1000, 0x2000), (16, 0x10, 0x20)], 5, c)
    assert g.wide == [True, False, False, False, False, True] and (g.n_wide, g.slots, g.units, g.stride, g.trips) == (2, 3, 15, 16, 1)
    g = geometry([(16, 0, 0)] * 3, 3400, c)
    assert (g.slots, g.units, g.stride, g.trips) == (3, 10200, 8192, 2)
    g = geometry([(4, 0, 0)] * 3, 9, c)
    assert (g.n_wide, g.slots, g.units, g.stride) == (0, 1, 9, 12)


def test_the_sweep_reaches_what_it_is_for():
    """The 40 configurations are the same on every machine, and between them they hold every row width, shift and count
    of bad ids, requests of wide fields only and of narrow fields only, 16 fields, and chunks of one, two and three
    passes of the rows in flight."""
    c = kernel_constants()
    configs = gather_configs()
    assert len(configs) == 40 and configs == gather_configs()
    fields = [f for cfg in configs for f in cfg["fields"]]
    assert {f["row_bytes"] for f in fields} == set(SWEEP_ROW_BYTES)
    assert {(f["src_shift"], f["dst_shift"]) for f in fields} == {(a, b) for a in SWEEP_SHIFTS for b in SWEEP_SHIFTS}
    assert {f["per_chunk"] for f in fields} == {False, True} and {f["dtype"] for f in fields} == set(SWEEP_DTYPES)
    assert {cfg["bad"] for cfg in configs} == {0, 1, 2, 3} and {len(cfg["fields"]) for cfg in configs} >= {1, 16}
    assert all(1 <= cfg["K"] <= 4 and 1 <= cfg["L"] <= 9 and 1 <= cfg["n"] <= 70 and 1 <= cfg["m"] <= 300 for cfg in configs)
    assert {-(-cfg["L"] // c.in_flight) for cfg in configs} == {1, 2, 3}
    assert all(sum(not 0 <= s < cfg["K"] * cfg["n"] for s in cfg["ids"]) == cfg["bad"] for cfg in configs)
    assert any(len(set(cfg["ids"])) < cfg["m"] for cfg in configs), "ids repeat"
    kinds = {frozenset(geometry([(f["row_bytes"], f["src_shift"], f["dst_shift"]) for f in cfg["fields"]], cfg["m"], c).wide) for cfg in configs}
    assert kinds == {frozenset([True]), frozenset([False]), frozenset([True, False])}


def test_gather_eager_is_the_id_formula_on_the_sweep():
    """The reference of the GPU tests, pinned without a GPU: for the 40 configurations, expected() (gather_eager with
    the bad ids' rows zeroed) on CPU tensors is, byte for byte, a plain Python loop over rollout.sequence_rows."""
    import numpy as np
    g = torch.Generator().manual_seed(7)
    for cfg in gather_configs():
        K, L, n = cfg["K"], cfg["L"], cfg["n"]
        for i, f in enumerate(cfg["fields"]):
            src = random_bits(source_shape(f, K, L, n), getattr(torch, f["dtype"]), g)
            want = expected(cfg["ids"], src, K, L, n, f["per_chunk"])
            assert want.dtype == src.dtype and want.shape == ((cfg["m"],) if f["per_chunk"] else (L, cfg["m"])) + tuple(src.shape[2:]), (cfg, i)
            got = want.contiguous().view(-1).view(torch.uint8).numpy()
            assert np.array_equal(got, _by_the_formula(cfg["ids"], src, K, L, n, f["per_chunk"]).reshape(-1)), (cfg, i)
