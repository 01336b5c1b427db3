"""The gradient reduction on the GPU (sim.reduce_gradients, hs_reduce_gradients, csrc/hs_k_reduce.h) against
optim.host_reduce, the numpy restatement of include/hideseek.h, bit for bit: one element, a short quad, a full one, a full
and a short one, idle lanes, more than one workgroup and a second grid-stride trip; 1, 2, 3, 8 and 16 shards; counts that
are equal, unequal, zero for one shard and zero for all; dst as the first and as the last source; signed zeros, denormals
and non-finite values; a NaN count; total; determinism; the stream form; and the refusals of the C ABI."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THREADS, VEC, STEP_MAX_GRID = 256, 4, 2048                    # hs_k_adam.h: the shape k_reduce shares with k_adam_step
SIZES = (1, 3, 4, 5, 1023, 2 * THREADS * VEC + 3)
SHARDS = (1, 2, 3, 8, 16)
SECOND_TRIP = STEP_MAX_GRID * THREADS * VEC + 4               # one full quad past the largest grid's first trip
GUARD = 64


def _sim(worlds=4, agents=4, seed=0):
    import gpu_hideseek
    k = agents // 2
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=0, rand_seed=seed,
        min_hiders=k, max_hiders=k, min_seekers=k, max_seekers=k, num_pbt_policies=1)


@pytest.fixture(scope="module")
def sim():
    s = _sim()
    s.init()
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def _sources(n, G):
    """G read-only float32 arrays [n] of mixed magnitudes."""
    rng = np.random.default_rng([n % 100003, G, 17])
    out = []
    for g in range(G):
        a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3)).astype(np.float32)
        a.setflags(write=False)
        out.append(a)
    return out


def counts_of(G):
    """{name: counts}: equal, unequal, one shard with none, nobody with any."""
    unequal = [float(7 + 13 * g % 11 + 100 * (g % 3)) for g in range(G)]
    one_zero = list(unequal)
    one_zero[G // 2] = 0.0
    return {"equal": [48.0] * G, "unequal": unequal, "one zero": one_zero, "all zero": [0.0] * G}


def _u(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, tag):
    g, w = _u(got), _u(want)
    assert g.shape == w.shape and np.array_equal(g, w), (tag, int((g != w).sum()), g.size)


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype)).cuda()


def _guarded(n):
    """(the whole buffer, its first n elements): GUARD elements of -7 behind them."""
    import torch
    whole = torch.full((n + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    return whole, whole[:n]


@pytest.mark.parametrize("G", SHARDS)
@pytest.mark.parametrize("n", SIZES)
def test_parity_with_the_restatement(sim, n, G):
    import torch
    from gpu_hideseek import optim
    xs = _sources(n, G)
    dev = [_dev(x) for x in xs]
    for name, counts in counts_of(G).items():
        want, C_ = optim.host_reduce(xs, counts)
        whole, out = _guarded(n)
        res = sim.reduce_gradients(dev, _dev(counts, np.float64), out=out, total=True)
        _same(res["out"], want, (n, G, name))
        assert res["out"] is out and bool((whole[n:] == -7).all()), (n, G, name)
        assert res["total"].cpu().tolist() == [C_] == [sum(counts)]
        if not any(counts):                                                   # with one shard, "one zero" is that too
            assert not _u(out).any()
        elif G == 1:
            _same(out, xs[0], (n, "identity"))
    for x, d in zip(xs, dev):                                             # the sources are only read
        _same(d, x, (n, G, "source"))


def test_a_second_grid_stride_trip(sim):
    from gpu_hideseek import optim
    n, G = SECOND_TRIP, 2
    assert -(-(-(-n // VEC)) // THREADS) > STEP_MAX_GRID
    xs = _sources(n, G)
    counts = [1000.0, 24.0]
    want, _ = optim.host_reduce(xs, counts)
    whole, out = _guarded(n)
    sim.reduce_gradients([_dev(x) for x in xs], _dev(counts, np.float64), out=out)
    _same(out, want, "second trip")
    assert bool((whole[n:] == -7).all())


@pytest.mark.parametrize("G", (2, 3, 16))
def test_dst_may_be_one_of_the_sources(sim, G):
    from gpu_hideseek import optim
    n = SIZES[-1]
    xs = _sources(n, G)
    counts = counts_of(G)["unequal"]
    want, _ = optim.host_reduce(xs, counts)
    for alias in (0, G - 1):
        dev = [_dev(x) for x in xs]
        whole, own = _guarded(n)
        own.copy_(dev[alias])
        dev[alias] = own
        res = sim.reduce_gradients(dev, _dev(counts, np.float64), out=own)
        _same(res["out"], want, (G, "alias", alias))
        assert bool((whole[n:] == -7).all())
        for g in range(G):
            if g != alias:
                _same(dev[g], xs[g], (G, alias, "source", g))


def test_special_values(sim):
    from gpu_hideseek import optim
    n = 1023
    a, b, c = (np.array(x) for x in _sources(n, 3))
    a[:8] = [-0.0, -0.0, 0.0, 1e-45, -1e-40, 1e-38, np.inf, 3.0]
    b[:8] = [-0.0, 0.0, -0.0, 1e-45, 1e-40, -1e-38, 1.0, np.nan]
    c[:8] = [-0.0, 0.0, 0.0, -1e-45, 2e-40, 1e-38, 2.0, 1.0]
    for counts in ([5.0, 3.0, 8.0], [1.0, 1.0, 1.0], [4.0, 4.0, 0.0]):
        want, _ = optim.host_reduce([a, b, c], counts)
        out = sim.reduce_gradients([_dev(a), _dev(b), _dev(c)], _dev(counts, np.float64))["out"]
        _same(out, want, ("special", counts))
        got = out.cpu().numpy()
        assert np.isinf(got[6]) and np.isnan(got[7]) and np.isfinite(got[8:]).all()
    assert _u(want)[0] == 0x80000000                                       # -0 of every counted shard stays -0
    # a shard with no samples is left out, whatever it holds: not multiplied by 0
    poison = np.full(n, np.inf, np.float32)
    poison[::2] = np.nan
    rest = _sources(n, 2)
    want, _ = optim.host_reduce([rest[0], poison, rest[1]], [9.0, 0.0, 3.0])
    out = sim.reduce_gradients([_dev(rest[0]), _dev(poison), _dev(rest[1])], _dev([9.0, 0.0, 3.0], np.float64))["out"]
    _same(out, want, "zero-count shard")
    assert np.isfinite(out.cpu().numpy()).all()
    _same(out, optim.host_reduce(rest, [9.0, 3.0])[0], "as if it were not there")
    # a NaN count: every weight is NaN, and so is the gradient (hs_adam_step then skips)
    res = sim.reduce_gradients([_dev(rest[0]), _dev(rest[1])], _dev([np.nan, 3.0], np.float64), total=True)
    assert np.isnan(res["out"].cpu().numpy()).all() and np.isnan(res["total"].item())


def test_determinism_total_and_the_stream_form(sim):
    import torch
    from gpu_hideseek import optim
    n, G = SIZES[-1], 8
    xs = _sources(n, G)
    counts = counts_of(G)["one zero"]
    want, C_ = optim.host_reduce(xs, counts)
    dev, cnt = [_dev(x) for x in xs], _dev(counts, np.float64)
    first = sim.reduce_gradients(dev, cnt, total=True)
    again = sim.reduce_gradients(dev, cnt, total=True)
    _same(first["out"], want, "first")
    _same(again["out"], want, "again")
    assert first["out"].data_ptr() != again["out"].data_ptr() and first["total"].item() == again["total"].item() == C_
    total = torch.full((3,), -7.0, dtype=torch.float64, device="cuda")
    assert "total" not in sim.reduce_gradients(dev, cnt)
    sim.reduce_gradients(dev, cnt, total=total[1:2])
    assert total.cpu().tolist() == [-7.0, C_, -7.0]
    # on a side stream, and on a raw handle: enqueued without waiting
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = sim.reduce_gradients(dev, cnt, stream=side)["out"]
    side.synchronize()
    _same(out, want, "side stream")
    whole, out = _guarded(n)
    sim.reduce_gradients(dev, cnt, out=out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _same(out, want, "raw handle")
    # inside on_current_stream() a call without a stream is enqueued on torch's current one
    from gpu_hideseek._request import on_current_stream
    with torch.cuda.stream(side), on_current_stream():
        out = sim.reduce_gradients(dev, cnt)["out"]
    side.synchronize()
    _same(out, want, "current stream")


def test_the_c_abi_refuses_and_writes_nothing():
    import torch
    from gpu_hideseek import optim
    INVALID = 1
    n, G = 37, 3
    xs = _sources(n, G)
    src = [torch.cat([_dev(x), torch.full((GUARD,), -7.0, device="cuda")]) for x in xs]
    dst = torch.full((n + GUARD,), -7.0, device="cuda")
    count = torch.tensor([5.0, 3.0, 8.0, -7.0], dtype=torch.float64, device="cuda")
    total = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    everything = src + [dst, count, total]
    saved = [t.clone() for t in everything]
    P = lambda t: t.data_ptr()                                              # noqa: E731
    assert all(P(t) % 16 == 0 for t in everything)

    def req(srcs=tuple(P(t) for t in src), count=P(count), dst=P(dst), n=n, shards=G, total=P(total)):
        r = optim.HsGradReduceRequest()
        for g, p in enumerate(srcs):
            r.src[g] = p
        r.count, r.dst, r.n, r.shards, r.total = count, dst, n, shards, total
        return r

    def untouched():
        torch.cuda.synchronize()
        return all(np.array_equal(_u(a), _u(b)) for a, b in zip(everything, saved))

    def call(s, r, stream=False):
        if stream:
            return s._L.hs_reduce_gradients_async(s._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), None if r is None else C.byref(r))
        return s._L.hs_reduce_gradients(s._h, None if r is None else C.byref(r))

    def message(s):
        return s._L.hs_last_error().decode()

    s = _sim()
    for stream in (False, True):
        assert call(s, req(), stream) == INVALID and "before hs_init" in message(s)
    assert untouched()
    s.init()
    a, b, c = (P(t) for t in src)
    bad = {
        "null request": (None, "null request"),
        "null dst": (req(dst=None), "null dst"), "null count": (req(count=None), "null count"),
        "null src 0": (req(srcs=(None, b, c)), "null src[0]"), "null src 2": (req(srcs=(a, b, None)), "null src[2]"),
        "a source short": (req(srcs=(a, b)), "null src[2]"),
        "shards 0": (req(shards=0), "shards must"), "shards -1": (req(shards=-1), "shards must"), "shards 17": (req(shards=17), "shards must"),
        "n 0": (req(n=0), "n must"), "n -1": (req(n=-1), "n must"), "n 2^31": (req(n=2 ** 31), "n must"), "n 2^40": (req(n=2 ** 40), "n must"),
        "src +4": (req(srcs=(a, b + 4, c)), "src[1] must be 16-byte aligned"), "src +8": (req(srcs=(a + 8, b, c)), "src[0] must be 16-byte aligned"),
        "dst +4": (req(dst=P(dst) + 4), "dst must be 16-byte aligned"), "dst +12": (req(dst=P(dst) + 12), "dst must be 16-byte aligned"),
        "count +4": (req(count=P(count) + 4), "8-byte aligned"), "total +4": (req(total=P(total) + 4), "8-byte aligned"),
        "dst in src 1": (req(dst=b + 16), "dst overlaps src[1] without being it"), "src 2 in dst": (req(srcs=(a, b, P(dst) + 32)), "dst overlaps src[2] without being it"),
        "dst is two sources": (req(srcs=(a, b, a), dst=a), "more than one"),
        "count in dst": (req(count=P(dst) + 8), "count overlaps dst"), "total in dst": (req(total=P(dst) + 16), "total overlaps dst"),
        "total in count": (req(total=P(count) + 8), "total overlaps count"), "total in src": (req(total=c), "total overlaps src[2]"),
    }
    for what, (r, msg) in bad.items():
        for stream in (False, True):
            assert call(s, r, stream) == INVALID, what
            assert msg in message(s), (what, message(s))
    assert untouched()
    s.step_begin()
    for stream in (False, True):
        assert call(s, req(), stream) == INVALID and "open step" in message(s)
    s.step_end()
    assert untouched()
    # the call does write, and only its own ranges; a null total, a source past `shards` and dst as a source are accepted
    want, C_ = optim.host_reduce(xs, [5.0, 3.0, 8.0])
    assert call(s, req()) == 0
    torch.cuda.synchronize()
    _same(dst[:n], want, "C ABI")
    assert bool((dst[n:] == -7).all()) and total.cpu().tolist() == [C_, -7.0, -7.0, -7.0] and all(bool((t[n:] == -7).all()) for t in src)
    want2, _ = optim.host_reduce(xs[:2], [5.0, 3.0])
    assert call(s, req(srcs=(a, b, 4), shards=2, total=None, dst=a), stream=True) == 0
    torch.cuda.synchronize()
    _same(src[0][:n], want2, "in place")
    assert bool((src[0][n:] == -7).all()) and total.cpu().tolist() == [C_, -7.0, -7.0, -7.0]
    s.close()
