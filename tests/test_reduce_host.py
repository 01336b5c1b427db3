"""The gradient reduction without a GPU (gpu_hideseek.optim.host_reduce / reduce_request, hs_reduce_gradients): the ctypes
mirror against include/hideseek.h and the layout hideseek.hip asserts, the numpy restatement of the header's arithmetic on
the cases that pin its wording (one shard is the identity, a shard with a zero count is left out and not multiplied by 0,
all counts zero give +0, the weights are float64 quotients rounded once, the sums float32 in index order), and the
refusals of reduce_request() before the library is involved."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

MAX_SHARDS = 16                                               # asserted against module, header and kernel below
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_header_states_the_request():
    from gpu_hideseek import optim
    src = open(os.path.join(ROOT, "include", "hideseek.h")).read()

    def const(name):
        return int(re.search(rf"{name} = (\d+)", src).group(1))
    assert const("HS_REDUCE_MAX_SHARDS") == MAX_SHARDS == optim.REDUCE_MAX_SHARDS
    assert re.search(r"int32_t hs_reduce_gradients\(hs_sim \*\w*, const hs_grad_reduce_request \*\w*\);", src)
    assert re.search(r"int32_t hs_reduce_gradients_async\(hs_sim \*\w*, void \*hip_stream, const hs_grad_reduce_request \*\w*\);", src)
    body = re.search(r"typedef struct hs_grad_reduce_request \{(.*?)\} hs_grad_reduce_request;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert decls == ["const float *src[HS_REDUCE_MAX_SHARDS]", "const double *count", "float *dst", "int64_t n", "int32_t shards", "double *total"], decls
    R = optim.HsGradReduceRequest
    assert [f[0] for f in R._fields_] == ["src", "count", "dst", "n", "shards", "total"]
    assert R._fields_[0][1] is C.c_void_p * MAX_SHARDS and R._fields_[3][1] is C.c_int64 and R._fields_[4][1] is C.c_int32
    assert all(R._fields_[i][1] is C.c_void_p for i in (1, 2, 5))
    offsets = dict(src=0, count=128, dst=136, n=144, shards=152, total=160)
    assert C.sizeof(R) == 168 and {k: getattr(R, k).offset for k in offsets} == offsets
    # the same numbers in the static_assert of the host file, and the kernel's constant
    csrc = os.path.join(ROOT, "marl-hideandseek_amd", "csrc")
    host, kernel = (open(os.path.join(csrc, f)).read() for f in ("hideseek.hip", "hs_k_reduce.h"))
    assert "sizeof(hs_grad_reduce_request) == 168" in host and "HS_REDUCE_MAX_SHARDS == hs::kReduceMaxShards" in host
    for k, v in offsets.items():
        assert k == "src" or f"offsetof(hs_grad_reduce_request, {k}) == {v}" in host, k
    assert int(re.search(r"kReduceMaxShards = (\d+);", kernel).group(1)) == MAX_SHARDS
    assert "atomic" not in kernel.replace("No atomics", "") and "__shared__" not in kernel
    assert len(re.findall(r"__global__", kernel)) == len(re.findall(r"template <int kThreads = kAdamThreads>\n__global__", kernel)) == 1
    # the stated arithmetic, in the header's text
    for phrase in ("w_g = (float)(c_g / C)", "acc = w_a * x_a;   acc = acc + w_g * x_g;   dst = acc", "If every count is 0, dst is +0",
                   "over the shards with c_g != 0"):
        assert phrase in src, phrase


def test_one_shard_is_the_identity():
    from gpu_hideseek import optim
    rng = np.random.default_rng(3)
    x = rng.standard_normal(1027).astype(np.float32)
    x[:6] = [0.0, -0.0, 1e-45, -1e-40, np.inf, np.nan]                  # signed zeros, denormals and the non-finite keep their bits
    for c in (1.0, 3.0, 1e300, 5e-324, -2.0):
        out, total = optim.host_reduce([x], [c])
        assert out.dtype == np.float32 and np.array_equal(bits(out), bits(x)) and total == c, c


def test_a_zero_count_shard_is_left_out():
    from gpu_hideseek import optim
    rng = np.random.default_rng(4)
    a, b, c = (rng.standard_normal(33).astype(np.float32) for _ in range(3))
    bad = b.copy()
    bad[5], bad[6] = np.inf, np.nan
    out, total = optim.host_reduce([a, bad, c], [3.0, 0.0, 1.0])
    want, _ = optim.host_reduce([a, c], [3.0, 1.0])
    assert np.isfinite(out).all() and np.array_equal(bits(out), bits(want)) and total == 4.0
    # a leading zero count: the first product is the first COUNTED shard's, taken as it is (-0 stays -0)
    z = np.full(4, -0.0, np.float32)
    out, _ = optim.host_reduce([bad[:4], z, z], [0.0, 1.0, 0.0])
    assert np.array_equal(bits(out), bits(z))
    # counted, an infinity and a NaN propagate; a NaN count makes everything NaN
    out, _ = optim.host_reduce([a, bad], [1.0, 1.0])
    assert np.isinf(out[5]) and np.isnan(out[6]) and np.isfinite(np.delete(out, [5, 6])).all()
    out, total = optim.host_reduce([a, b], [np.nan, 1.0])
    assert np.isnan(out).all() and np.isnan(total)


def test_all_counts_zero_give_plus_zero():
    from gpu_hideseek import optim
    x = np.array([np.inf, -1.0, np.nan, -0.0, 2.0], np.float32)
    for G in (1, 2, 16):
        out, total = optim.host_reduce([x] * G, [0.0] * G)
        assert out.dtype == np.float32 and out.shape == x.shape and not bits(out).any() and total == 0.0
    out, _ = optim.host_reduce([x, x], [0.0, -0.0])                    # -0 is 0
    assert not bits(out).any()


def test_the_stated_order_and_roundings():
    """Element by element in Python: float64 counts and quotients, a weight rounded to float32 once, float32 products
    and sums in index order."""
    from gpu_hideseek import optim
    rng = np.random.default_rng(5)
    f32 = np.float32
    for G, counts in ((2, [7.0, 9.0]), (3, [100.0, 1.0, 37.0]), (5, [3.0, 0.0, 3.0, 1e6, 11.0])):
        xs = [rng.standard_normal(19).astype(f32) * f32(10.0 ** rng.integers(-3, 4)) for _ in range(G)]
        out, total = optim.host_reduce(xs, counts)
        C_ = 0.0
        for c in counts:
            if c != 0.0:
                C_ = C_ + c
        assert total == C_
        for i in range(19):
            acc = None
            for g in range(G):
                if counts[g] == 0.0:
                    continue
                p = f32(f32(counts[g] / C_) * xs[g][i])
                acc = p if acc is None else f32(acc + p)
            assert bits(acc) == bits(out[i]), (G, i)
    # equal counts: the weights are exactly 1 / G for a power of two, and the order of the sum still matters elsewhere
    a, b = np.array([1e8], f32), np.array([1.0], f32)
    x, _ = optim.host_reduce([a, -a, b], [1.0, 1.0, 1.0])
    y, _ = optim.host_reduce([a, b, -a], [1.0, 1.0, 1.0])
    assert x[0] != y[0]
    with pytest.raises(ValueError):
        optim.host_reduce([a, b], [1.0])
    with pytest.raises(ValueError):
        optim.host_reduce([a] * 17, [1.0] * 17)


def test_request_refuses_before_the_library_is_called():
    from gpu_hideseek import optim

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    n = 40
    good = dict(srcs=[torch.zeros(n), torch.zeros(n), torch.zeros(n)], counts=torch.zeros(3, dtype=torch.float64))

    def call(**kw):
        a = dict(good, **kw)
        return optim.reduce_gradients(Sim(), a.pop("srcs"), a.pop("counts"), **a)

    def off(by=1):
        t = torch.zeros(n + 8)[by:by + n]
        assert t.is_contiguous() and t.data_ptr() % 16
        return t

    for bad in (torch.zeros(n), [], None, [torch.zeros(n)] * 17, 3):
        with pytest.raises(ValueError, match="srcs must be a list of 1 to 16"):
            call(srcs=bad)
    for bad in (torch.zeros(0), torch.zeros(()), torch.zeros(2, 3)):
        with pytest.raises(ValueError, match=r"srcs\[0\] must be .* shape"):
            call(srcs=[bad, torch.zeros(n)])
    with pytest.raises(ValueError, match=r"srcs\[0\] must be a torch tensor"):
        call(srcs=[None, torch.zeros(n), torch.zeros(n)])
    for bad, what in ((torch.zeros(n, dtype=torch.float64), "dtype"), (torch.zeros(n, dtype=torch.bfloat16), "dtype"), (torch.zeros(n + 1), "shape"),
                      (torch.zeros(n, 1), "shape"), (torch.zeros(2 * n)[::2], "contiguous"), (off(1), "16-byte aligned"), (off(2), "16-byte aligned"),
                      (None, r"srcs\[2\] must be a torch tensor")):
        with pytest.raises(ValueError, match=what):
            call(srcs=good["srcs"][:2] + [bad])
        if bad is not None:
            with pytest.raises(ValueError, match="out must be|out overlaps" if what != "16-byte aligned" else what):
                call(out=bad)
    for bad, what in ((torch.zeros(3), "dtype"), (torch.zeros(2, dtype=torch.float64), "shape"), (torch.zeros(6, dtype=torch.float64)[::2], "contiguous"),
                      (None, "counts must")):
        with pytest.raises(ValueError, match=what):
            call(counts=bad)
    for bad, what in ((torch.zeros(1), "dtype"), (torch.zeros(2, dtype=torch.float64), "shape"), (2.0, "total must")):
        with pytest.raises(ValueError, match=what):
            call(total=bad)
    with pytest.raises(ValueError, match="out must be True, None or a torch tensor"):
        call(out=2.0)
    # overlaps: out may be one source itself and nothing else
    shared = torch.zeros(2 * n)
    with pytest.raises(ValueError, match=r"out overlaps srcs\[1\] without being it"):
        call(srcs=[good["srcs"][0], shared[:n], good["srcs"][2]], out=shared[8:8 + n])
    with pytest.raises(ValueError, match="out is more than one of the sources"):
        call(srcs=[shared[:n], good["srcs"][1], shared[:n]], out=shared[:n])
    with pytest.raises(ValueError, match="out overlaps counts"):
        call(counts=shared.view(torch.float64)[:3], out=shared[:n])
    both = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError, match="total overlaps counts"):
        call(counts=both[:3], total=both[2:3])
    with pytest.raises(ValueError, match=r"total overlaps srcs\[0\]"):
        call(total=good["srcs"][0].view(torch.float64)[:1])
    with pytest.raises(ValueError, match="total overlaps out"):
        call(out=shared[:n], total=shared.view(torch.float64)[1:2])
    # well-formed tensors on the wrong device come last
    for ok in (dict(), dict(out=good["srcs"][0]), dict(out=good["srcs"][2], total=torch.zeros(1, dtype=torch.float64)), dict(out=torch.zeros(n)),
               dict(srcs=[torch.zeros(1)], counts=torch.zeros(1, dtype=torch.float64))):
        with pytest.raises(ValueError, match="on cpu"):
            call(**ok)
    res, req = None, None
    with pytest.raises(ValueError, match="on cpu"):
        res, req = optim.reduce_request(0, good["srcs"], good["counts"])
    assert res is None and req is None
