"""The scalar core (marl-hideandseek_amd/csrc/hs_core.h) as the DEVICE compiler reads it, against the host compile, bit
for bit.  Both evaluate the probe table csrc/hs_core_probe.h: hs_debug_core_eval (k_core_eval, one case per lane) and the
oracle's hsref_core_eval.  The inputs are those of tests/test_core_float64.py, which pins the host compile to float64: they
stay inside the callers' domains, so no case makes a NaN or an out-of-range float-to-int conversion.  All 16 output words
of every case are compared as uint32; no difference is allowed.  When a lock-step test breaks, this file says whether the
core moved or the code above it."""
import ctypes as C

import numpy as np
import pytest

from test_core_float64 import OPS, all_inputs, op_of, subset, table

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 257, 65536)       # around the wave, around the 256-lane workgroup, many workgroups
POISON = np.uint32(0xDEADBEEF)
GUARD = 64                                      # rows of 16 words behind the n cases
HS_OK, HS_ERR_INVALID_ARG = 0, 1


@pytest.fixture(scope="module")
def native():
    import gpu_hideseek
    L = gpu_hideseek._native.load()
    L.hs_debug_core_eval.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.hs_debug_core_eval.restype = C.c_int32
    return L


def device(L, op, x):
    """hs_debug_core_eval on [n, 16] words into a poisoned buffer with a guard region: the results as uint32."""
    x = np.ascontiguousarray(x)
    n = len(x)
    out = np.full((n + GUARD, 16), POISON, np.uint32)
    assert L.hs_debug_core_eval(int(op), n, x.ctypes.data, out.ctypes.data) == HS_OK
    assert np.all(out[n:] == POISON), "wrote behind the n cases"
    return out[:n]


def sized(x, n):
    """n rows of a table: special cases and an even sample of it, repeated if the table is shorter."""
    return np.resize(subset(x, n), (n, 16))


@pytest.mark.parametrize("name", sorted(all_inputs()))
def test_device_and_host_compile_agree_word_for_word(native, oracle, name):
    op, x = op_of(name), table(name)["x"]
    runs = [sized(x, n) for n in SIZES] + [x[i:i + (1 << 20)] for i in range(0, len(x), 1 << 20)]      # the sizes, then every input
    for xs in runs:
        dev = device(native, op, xs)
        ref = oracle.core_eval(op, xs).view(np.uint32)
        differ = dev != ref
        assert not differ.any(), (name, len(xs), int(differ.sum()), "words differ; first case:", xs[np.argwhere(differ)[0][0]].tolist(),
                                  dev[np.argwhere(differ)[0][0]].tolist(), ref[np.argwhere(differ)[0][0]].tolist())


def test_every_op_of_the_table_is_compared():
    assert {op_of(n) for n in all_inputs()} == set(OPS.values())


def test_refusals_write_nothing(native):
    x = np.ones((4, 16), np.float32)
    out = np.full((4 + GUARD, 16), POISON, np.uint32)
    L = native
    for op, n, pin, pout in ((0, 4, None, out.ctypes.data), (0, 4, x.ctypes.data, None), (0, 0, x.ctypes.data, out.ctypes.data),
                             (0, -1, x.ctypes.data, out.ctypes.data), (0, (1 << 20) + 1, x.ctypes.data, out.ctypes.data),
                             (-1, 4, x.ctypes.data, out.ctypes.data), (len(OPS), 4, x.ctypes.data, out.ctypes.data)):
        assert L.hs_debug_core_eval(op, n, pin, pout) == HS_ERR_INVALID_ARG, (op, n)
        assert np.all(out == POISON) and np.all(x == 1)
    assert L.hs_debug_core_eval(len(OPS) - 1, 4, x.ctypes.data, out.ctypes.data) == HS_OK          # the last op is known
    assert np.all(out[4:] == POISON) and not np.any(out[:4] == POISON)
