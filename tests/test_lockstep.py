"""oracle/lockstep.py, the protocol of every GPU-vs-oracle parity test, checked with two oracle sides (no GPU)."""
import numpy as np

import lockstep


def _lockstep(a, b, steps):
    """Both sides through the "bench" stream, as Pair.drive writes it: columns 0-1 of a copy of a's actions."""
    draw, cols = lockstep.stream("bench")
    for s in range(steps):
        act = a.tensor("action").copy()
        act[:, list(cols)] = draw(s, act.shape[0])
        a.tensor("action")[:] = act
        b.tensor("action")[:] = act
        a.step()
        b.step()


def test_same_configuration_stays_bit_equal(oracle):
    a, b = lockstep.make_ref(6, seed=3, threads=1), lockstep.make_ref(6, seed=3, threads=3)
    a.init(); b.init()
    assert lockstep.diff(a, b) == []
    _lockstep(a, b, 4)
    assert lockstep.diff(a, b) == []
    lockstep.check(a, b, "after 4 steps")


def test_different_seeds_are_reported_where_they_differ(oracle):
    a, b = lockstep.make_ref(4, seed=1), lockstep.make_ref(4, seed=2)
    a.init(); b.init()
    bad = lockstep.diff(a, b)
    assert bad
    what, count, first, va, vb = bad[0]
    # the first differing tensor in NAMES order, its mismatch count, the first index and both values at it
    diffs = [n for n in lockstep.NAMES if not np.array_equal(lockstep.bits(a.tensor(n)), lockstep.bits(b.tensor(n)))]
    assert what == diffs[0]
    x, y = lockstep.bits(a.tensor(what)), lockstep.bits(b.tensor(what))
    assert count == int((x != y).sum()) and count > 0
    assert first == np.argwhere(x != y)[0].tolist()
    assert x[tuple(first)] != y[tuple(first)]
    assert (va, vb) == (a.tensor(what)[tuple(first)], b.tensor(what)[tuple(first)])
    assert {"bodies", "walls"} <= {m[0] for m in bad}
    try:
        lockstep.check(a, b, "seeds 1 / 2")
    except AssertionError as e:
        assert str(e).startswith("seeds 1 / 2: ") and what in str(e) and str(first) in str(e)
    else:
        raise AssertionError("check() passed on different seeds")


def test_bits_tells_signed_zeros_and_nan_payloads_apart():
    z = np.array([0.0, -0.0], np.float32)
    assert z[0] == z[1] and lockstep.bits(z)[0] != lockstep.bits(z)[1]
    nans = np.array([0x7FC00000, 0x7FC00001], np.int32).view(np.float32)
    assert lockstep.bits(nans)[0] != lockstep.bits(nans)[1]
    ints = np.arange(3, dtype=np.int32)
    assert lockstep.bits(ints).dtype == np.int32
    assert lockstep.diff(_Side(z[:1]), _Side(z[1:]), names=["x"], bodies=False, walls=False)[0][:3] == ("x", 1, [0])


class _Side:
    def __init__(self, x):
        self.x = x

    def tensor(self, name):
        return self.x
