"""ORACLE — TEST INFRASTRUCTURE ONLY.

Lock-step runs of the HIP simulator against the CPU oracle (hs_ref.RefSim): both start from the same seeds, the same
actions are written to both, both are stepped, and the exported tensors plus the body and wall state are compared bit
for bit.  Used by tests/, __graft_entry__.smoke() and tools/parity_run.py; never by the product package.

A *side* is anything with tensor(name) -> ndarray, bodies() and walls(): a RefSim, or a GpuSide over a
HideAndSeekSimulator.  torch and gpu_hideseek are imported only where a GPU is needed.
"""
import hashlib
import os

import numpy as np

import hs_ref

# the exported tensors the oracle restates, and the observations in the JAX buffer order (mgr.cpp:168-201)
NAMES = ["reset", "prep_counter", "action", "self_data", "self_type", "self_mask", "agent_data", "box_data",
         "ramp_data", "visible_agents_mask", "visible_boxes_mask", "visible_ramps_mask", "lidar", "seed",
         "reward", "done", "global_positions", "episode_result"]
OBS = ["prep_counter", "self_data", "self_type", "self_mask", "lidar", "agent_data", "box_data", "ramp_data",
       "visible_agents_mask", "visible_boxes_mask", "visible_ramps_mask"]

EXT_SKIP_OBSERVATIONS = 1 << 16     # SimFlags.ExtSkipObservations: the oracle's skip_observations
EXT_RENDER = 1 << 17                # SimFlags.ExtRender: no oracle counterpart (RefSim.render() renders on request)


def bits(a):
    """float32 as int32, so that -0.0 != 0.0 and NaN payloads count; other dtypes unchanged."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def oracle_threads():
    """OMP_NUM_THREADS when set, else the CPU affinity; at most 16.  The oracle gives each thread a contiguous range of
    worlds (hs_ref_sim.hpp parallel), so its results do not depend on this."""
    n = os.environ.get("OMP_NUM_THREADS", "").split(",")[0].strip()
    if not n.isdigit():
        n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return max(1, min(int(n), 16))


def _mismatch(what, x, y):
    if x.shape != y.shape:
        return (what, "shape", None, x.shape, y.shape)
    bx, by = bits(x), bits(y)
    if np.array_equal(bx, by):
        return None
    idx = np.argwhere(bx != by)
    first = tuple(idx[0])
    return (what, len(idx), idx[0].tolist(), x[first], y[first])


def diff(a, b, names=NAMES, bodies=True, walls=True):
    """Where sides a and b differ, bitwise: a list of (what, count, first index, value in a, value in b)."""
    pairs = [(n, a.tensor(n), b.tensor(n)) for n in names]
    if bodies:
        (ab, am), (bb, bm) = a.bodies(), b.bodies()
        pairs += [("body_meta", am, bm), ("bodies", ab, bb)]
    if walls:
        (aw, ai), (bw, bi) = a.walls(), b.walls()
        pairs += [("world_info", ai, bi), ("walls", aw, bw)]
    return [m for m in (_mismatch(*p) for p in pairs) if m]


def _fail(tag, bad):
    return f"{tag}: {len(bad)} mismatching: " + "; ".join(map(str, bad[:4]))


def check(a, b, tag, names=NAMES, bodies=True, walls=True):
    """Assert that sides a and b are bit-equal; the message names the first differing elements."""
    bad = diff(a, b, names, bodies, walls)
    assert not bad, _fail(tag, bad)


class GpuSide:
    """A HideAndSeekSimulator as a side, restricted to worlds [lo, lo + n) (per-agent rows scaled by the agent count).
    `views` replaces exported tensors by caller-owned buffers of the same layout (the stream entry points)."""

    def __init__(self, sim, lo=0, n=None, views=None):
        self.sim, self.lo = sim, lo
        self.n = sim.num_worlds - lo if n is None else n
        self._views = dict(views or {})

    def view(self, name):
        """The torch view of exported tensor `name`, all worlds."""
        if name not in self._views:
            self._views[name] = getattr(self.sim, name + "_tensor")().to_torch()
        return self._views[name]

    def tensor(self, name):
        _, _, tail, per_agent = hs_ref.TENSORS[name]
        k = self.sim.agents_per_world if per_agent else 1
        rows = self.view(name)[self.lo * k:(self.lo + self.n) * k]
        return rows.cpu().numpy().reshape((self.n * k,) + tail)

    def bodies(self):
        b, m = self.sim.debug_bodies()
        return b[self.lo:self.lo + self.n], m[self.lo:self.lo + self.n]

    def walls(self):
        w, info = self.sim.debug_walls()
        return w[self.lo:self.lo + self.n], info[self.lo:self.lo + self.n]


def make_ref(worlds, flags=0, seed=0, hiders=(2, 2), seekers=(2, 2), world_offset=0, threads=None):
    """The oracle of the simulator made with the same arguments (not initialised)."""
    return hs_ref.RefSim(worlds, sim_flags=flags & 0xFFFF, rand_seed=seed, min_hiders=hiders[0], max_hiders=hiders[1],
                         min_seekers=seekers[0], max_seekers=seekers[1], world_offset=world_offset,
                         skip_observations=bool(flags & EXT_SKIP_OBSERVATIONS), threads=threads or oracle_threads())


def stream(kind, seed=1234):
    """A recurring action stream as (draw, cols): draw(step, rows) gives the values of columns `cols` (None: all five).
    "bench": moves in [-5, 5) on columns 0-1 (scripts/benchmark.py:82-84); "full": every bucket incl. grab / lock
    (jax_train.py:146-148 style); "none": no actions written."""
    rng = np.random.default_rng(seed)
    if kind == "bench":
        return (lambda s, rows: rng.integers(-5, 5, size=(rows, 2))), (0, 1)
    if kind == "full":
        return (lambda s, rows: np.stack([rng.integers(0, 11, rows), rng.integers(0, 11, rows), rng.integers(0, 11, rows),
                                          rng.integers(0, 2, rows), rng.integers(0, 2, rows)], axis=1)), None
    if kind == "none":
        return None, None
    raise ValueError(f"unknown action stream {kind!r}")


def hashed(mods, shift=0, first_row=0):
    """A stateless stream over global agent rows: column c of row g at step s is
    (((g * 2654435761 + (s + 1) * 40503 * (c + 1)) & 0x7FFFFFFF) >> 8) % mods[c] - shift, in int64."""
    mods = np.asarray(mods, np.int64)
    c = np.arange(1, len(mods) + 1, dtype=np.int64)

    def draw(s, rows):
        g = np.arange(first_row, first_row + rows, dtype=np.int64)[:, None]
        return (((g * 2654435761 + (s + 1) * 40503 * c) & 0x7FFFFFFF) >> 8) % mods - shift
    return draw


class Pair:
    """The HIP simulator (`sim`, seen through `gpu`) and the oracle (`ref`) made from one set of arguments; the debug
    level is written to both reset tensors before init.  `render` = (width, height) turns the batch renderer on."""

    def __init__(self, worlds, flags=0, seed=0, hiders=(2, 2), seekers=(2, 2), level=0, world_offset=0, render=None,
                 threads=None, init=True):
        import gpu_hideseek
        view = {} if render is None else dict(enable_batch_renderer=True, batch_render_width=render[0],
                                              batch_render_height=render[1])
        self.sim = gpu_hideseek.HideAndSeekSimulator(
            exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=flags, rand_seed=seed,
            min_hiders=hiders[0], max_hiders=hiders[1], min_seekers=seekers[0], max_seekers=seekers[1],
            num_pbt_policies=1, world_offset=world_offset, **view)
        self.ref = make_ref(worlds, flags, seed, hiders, seekers, world_offset, threads)
        self.gpu = GpuSide(self.sim)
        self.rows = worlds * self.ref.A
        if level:
            self.ref.tensor("reset")[:] = level
            self.gpu.view("reset")[:] = level
        if init:
            self.sim.init()
            self.ref.init()

    def act(self, actions, cols=None):
        """Write `actions` (int array, or draw(step, rows) already called) into columns `cols` (None: all) of a copy of
        the oracle's current actions, and that copy to both sides."""
        import torch
        a = self.ref.tensor("action").copy()
        if cols is None:
            a[:] = actions
        else:
            a[:, list(cols)] = actions
        self.ref.tensor("action")[:] = a
        dst = self.gpu.view("action")
        dst.copy_(torch.from_numpy(a).to(dst.device))

    def step(self, actions=None, cols=None):
        """act() unless `actions` is None, then one step of both sides."""
        if actions is not None:
            self.act(actions, cols)
        self.sim.step()
        self.ref.step()

    def check(self, tag, names=NAMES, bodies=True, walls=True):
        check(self.gpu, self.ref, tag, names, bodies, walls)

    def check_views(self, width, height, tag):
        """The agent views in depth_tensor() / rgb_tensor() against the oracle's render of the current state."""
        d = self.sim.depth_tensor().to_torch().cpu().numpy()
        c = self.sim.rgb_tensor().to_torch().cpu().numpy()
        rd, rc = self.ref.render(width, height)
        assert c.dtype == np.uint8, c.dtype
        bad = [m for m in (_mismatch("rgb", c, rc), _mismatch("depth", d, rd)) if m]
        assert not bad, _fail(tag, bad)
        return d, c

    def drive(self, steps, actions="bench", cols=None, seed=1234, every=1, names=NAMES, bodies=True, walls=True,
              digest=False):
        """`steps` lock steps with actions from stream(actions, seed) or draw(step, rows) into `cols`; check() after every
        `every`-th step and the last.  With `digest`, returns a sha256 of the GPU body state at the checked steps."""
        if isinstance(actions, str):
            actions, cols = stream(actions, seed)
        h = hashlib.sha256() if digest else None
        for s in range(steps):
            self.step(None if actions is None else actions(s, self.rows), cols)
            if (s + 1) % every == 0 or s == steps - 1:
                self.check(f"step {s}", names, bodies, walls)
                if h:
                    h.update(self.sim.debug_bodies()[0].tobytes())
        return h.hexdigest() if h else None
