"""bench.py --dump-outputs: what the timed path computed in its last step, as .npy files two builds can be compared by.
On the CPU box dump_outputs() runs on a stand-in simulator whose tensors have the exports' real dtypes and shapes
(oracle/hs_ref.TENSORS) at the benchmark's 16 000 worlds, which is more than the 64 MB budget holds; the -m gpu test
runs the benchmark itself twice and compares the files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


class _View:
    def __init__(self, a):
        self.a = a

    def to_torch(self):
        import torch
        return torch.from_numpy(self.a)


class _FakeSim:
    """The getters bench.dump_outputs() reads, filled with seeded random values of each export's dtype and shape."""

    def __init__(self, oracle, N, A=4, world_offset=0):
        self.num_worlds, self.agents_per_world, self.world_offset = N, A, world_offset
        rng = np.random.default_rng(1)
        self.arrays = {}
        for name, (_, dt, tail, per_agent) in oracle.TENSORS.items():
            shape = ((N * A) if per_agent else N,) + tuple(tail)
            self.arrays[name] = (rng.integers(-2**31, 2**31 - 1, size=shape, dtype=np.int64).astype(dt)
                                 if np.dtype(dt).kind in "iu" else rng.standard_normal(shape).astype(dt))

    def __getattr__(self, getter):
        if getter.endswith("_tensor") and getter[:-len("_tensor")] in self.arrays:
            return lambda: _View(self.arrays[getter[:-len("_tensor")]])
        raise AttributeError(getter)


def _dumped(sim, d):
    bench.dump_outputs(sim, str(d))
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _expected_names():
    import gpu_hideseek
    return {n for n, role, _ in gpu_hideseek.train_interface() if role in bench.DUMP_ROLES} | {"world_index"}


def test_dump_of_16000_worlds_is_a_fixed_sample_within_64_mb(oracle, tmp_path):
    sim = _FakeSim(oracle, 16000)
    out = _dumped(sim, tmp_path / "a")
    assert set(out) == _expected_names()
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in out) <= 64 * 10**6
    w = out["world_index"]
    assert w.dtype == np.float64 and 0 < len(w) < 16000
    assert np.all(np.diff(w) > 0) and w[0] >= 0 and w[-1] < 16000
    assert len(w) > 10000, "the budget holds most of the 16 000 worlds"
    import gpu_hideseek
    getters = {n: g for n, _, g in gpu_hideseek.train_interface()}
    worlds = w.astype(np.int64)
    for name, a in out.items():
        if name == "world_index":
            continue
        src = sim.arrays[getters[name][:-len("_tensor")]]
        assert a.dtype == (np.float64 if src.dtype.kind in "iu" else np.float32), name
        r = src.shape[0] // 16000
        assert np.array_equal(a, src[(worlds[:, None] * r + np.arange(r)).reshape(-1)].astype(a.dtype)), name
    # the same worlds every time
    again = _dumped(sim, tmp_path / "b")
    assert all(np.array_equal(out[n], again[n]) for n in out)


def test_dump_of_a_small_run_holds_every_world(oracle, tmp_path):
    sim = _FakeSim(oracle, 77, world_offset=154)
    out = _dumped(sim, tmp_path)
    assert np.array_equal(out["world_index"], np.arange(154, 231, dtype=np.float64))
    assert out["self_data"].shape == (77 * 4, 13) and out["episode_results"].shape == (77, 2)
    assert np.array_equal(out["dones"], sim.arrays["done"].astype(np.float64))


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_dumped_outputs_repeat(tmp_path):
    """Two plain runs with the same arguments: identical inputs, so identical outputs; the line keeps the headline fields
    and none of what --full adds."""
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "12", "--warmup", "2", "--worlds-per-gpu", "2048",
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    out = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert out["steps"] == 12 and out["ms_per_step"] > 0 and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert abs(out["value"] - 2048 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]
    for k in ("roofline", "cpu_baseline", "device_status", "ms_per_step_percentiles"):
        assert k not in out, k
    a, b = sorted(os.listdir(tmp_path / "a")), sorted(os.listdir(tmp_path / "b"))
    assert a == b and "self_data.npy" in a and "rewards.npy" in a and "world_index.npy" in a
    for f in a:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.all(np.isfinite(x)), f
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f
    assert np.array_equal(np.load(tmp_path / "a" / "world_index.npy"), np.arange(2048))
