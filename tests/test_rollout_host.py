"""The rollout buffer and the minibatch gather without a GPU (gpu_hideseek.rollout, hs_gather_sequences): the refusals of
request(), Rollout() and epoch_parts() before the library is involved, minibatch_eager() on a hand-written buffer against
the id formula s = k n + r, an epoch's parts as a partition of the sequence ids, and the header against the ctypes mirror."""
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
