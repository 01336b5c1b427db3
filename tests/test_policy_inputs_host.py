"""Policy inputs, the parts that need no GPU (gpu_hideseek.policy_inputs, hs_pack_policy_inputs): the layout table, the
zero-copy views, argument validation, and a numpy restatement of the packed row (pack_rows, independent of the product;
tests/test_gpu_policy_inputs.py holds the kernel to it bit for bit) applied to oracle runs: its values are finite, and
the visibility masks of those runs do hide non-zero data, so that the actor's masking is really exercised."""
import numpy as np
import pytest
import torch

import lockstep

ROW = 296
SELF = ["prep_counter", "self_data", "self_type", "lidar"]
ENTITIES = [("agent_data", "visible_agents_mask"), ("box_data", "visible_boxes_mask"), ("ramp_data", "visible_ramps_mask")]
# (flags, hiders, seekers, action stream): 3+3 "full", the benchmark's 2+2, variable team sizes (inactive rows)
CONFIGS = {"3+3": (13, (3, 3), (3, 3), "full"), "2+2": (0, (2, 2), (2, 2), "bench"), "var": (13, (1, 3), (1, 3), "full")}


def pack_rows(t, actor):
    """The packed rows [R, 296] f32 of the observation tensors `t` (name -> array, rows in agent-row order): column 0
    prep_counter / 96 as one f32 division, then self_data, self_type, lidar, and the entity tables, each multiplied in f32
    by its visibility mask for the actor."""
    R = t["prep_counter"].shape[0]
    cols = [t["prep_counter"].reshape(R, 1).astype(np.float32) / np.float32(96.0),
            t["self_data"].reshape(R, 13).astype(np.float32),
            t["self_type"].reshape(R, 1).astype(np.float32),
            t["lidar"].reshape(R, 30).astype(np.float32)]
    for data, mask in ENTITIES:
        d = t[data].astype(np.float32)
        d = d.reshape(R, d.shape[-2], d.shape[-1])
        if actor:
            with np.errstate(invalid="ignore"):
                d = d * t[mask].astype(np.float32).reshape(R, d.shape[1], 1)
        cols.append(d.reshape(R, -1))
    out = np.concatenate(cols, axis=1)
    assert out.dtype == np.float32 and out.shape == (R, ROW)
    return out


def moments_of(t):
    """float64 [593]: sum m x, sum m x x over the rows for every column of the critic row, and sum m (m = self_mask)."""
    x = pack_rows(t, False).astype(np.float64)
    m = t["self_mask"].reshape(-1, 1).astype(np.float64)
    return np.concatenate([(m * x).sum(0), (m * x * x).sum(0), [m.sum()]])


def obs_of(side):
    return {n: np.array(side.tensor(n)) for n in lockstep.OBS}


def run_oracle(cfg, steps, worlds=64, seed=5):
    flags, hiders, seekers, kind = CONFIGS[cfg]
    ref = lockstep.make_ref(worlds, flags, seed, hiders, seekers)
    ref.init()
    draw, cols = lockstep.stream(kind)
    snaps = {0: obs_of(ref)}
    for s in range(steps):
        a = draw(s, worlds * ref.A)
        if cols is None:
            ref.tensor("action")[:] = a
        else:
            ref.tensor("action")[:, list(cols)] = a
        ref.step()
        if s + 1 in (1, steps):
            snaps[s + 1] = obs_of(ref)
    return snaps


def test_layout_covers_the_row_once(oracle):
    from gpu_hideseek import policy_inputs as P
    seen = np.zeros(ROW, int)
    prev = 0
    for name, (lo, hi, shape) in P.LAYOUT.items():
        assert lo == prev, name                   # in column order, no gap
        seen[lo:hi] += 1
        assert hi - lo == int(np.prod(shape)), name
        assert tuple(shape) == tuple(oracle.TENSORS[name][2]), name
        prev = hi
    assert prev == ROW == P.ROW and (seen == 1).all()
    assert P.MOMENTS == 2 * ROW + 1
    assert list(P.LAYOUT) == SELF + [d for d, _ in ENTITIES]
    assert P.MASKS == dict(ENTITIES)
    for data, mask in ENTITIES:                   # one mask per entity of the table
        assert oracle.TENSORS[mask][2] == (oracle.TENSORS[data][2][0], 1)
    assert P.TABLES["self"][:2] == (0, P.LAYOUT["agent_data"][0])


def test_views_share_storage():
    from gpu_hideseek import policy_inputs as P
    R = 6
    x = torch.arange(R * ROW, dtype=torch.float32).reshape(R, ROW)
    v = P.views(x)
    assert {k: tuple(t.shape) for k, t in v.items()} == {"self": (R, 45), "agents": (R, 5, 14), "boxes": (R, 9, 17),
                                                         "ramps": (R, 2, 14)}
    first = {"self": 0, "agents": 45, "boxes": 115, "ramps": 268}
    for k, t in v.items():
        assert t.untyped_storage().data_ptr() == x.untyped_storage().data_ptr(), k
        assert t.data_ptr() == x.data_ptr() + 4 * first[k], k
        assert float(t.reshape(R, -1)[0, 0]) == first[k] and float(t.reshape(R, -1)[2, 1]) == 2 * ROW + first[k] + 1
    assert float(v["boxes"][1, 3, 2]) == ROW + 115 + 3 * 17 + 2
    v["ramps"][0, 1, 13] = -1.0
    assert float(x[0, 295]) == -1.0
    buf = torch.zeros(4, R, ROW, dtype=torch.bfloat16)      # a rollout buffer: views of a slot and of the whole buffer
    assert P.views(buf[2])["agents"].data_ptr() == buf[2].data_ptr() + 2 * 45
    assert tuple(P.views(buf)["boxes"].shape) == (4, R, 9, 17)
    with pytest.raises(ValueError):
        P.views(torch.zeros(R, ROW - 1))


def test_restatement_is_the_concatenation():
    rng = np.random.default_rng(0)
    R = 7
    t = {"prep_counter": rng.integers(0, 97, (R, 1)).astype(np.int32), "self_data": rng.normal(size=(R, 13)).astype(np.float32),
         "self_type": rng.integers(0, 2, (R, 1)).astype(np.int32), "lidar": rng.random((R, 30)).astype(np.float32),
         "self_mask": np.ones((R, 1), np.float32)}
    for (d, m), shape in zip(ENTITIES, ((5, 14), (9, 17), (2, 14))):
        t[d] = rng.normal(size=(R,) + shape).astype(np.float32)
        t[m] = rng.integers(0, 2, (R, shape[0], 1)).astype(np.float32)
    c, a = pack_rows(t, False), pack_rows(t, True)
    assert c[3, 0] == np.float32(t["prep_counter"][3, 0]) / np.float32(96) and c[3, 14] == t["self_type"][3, 0]
    assert np.array_equal(c[:, 1:14], t["self_data"]) and np.array_equal(c[:, 15:45], t["lidar"])
    assert np.array_equal(c[:, 115:268].reshape(R, 9, 17), t["box_data"])
    assert np.array_equal(a[:, :45], c[:, :45])
    assert a[2, 45 + 3 * 14 + 5] == t["agent_data"][2, 3, 5] * t["visible_agents_mask"][2, 3, 0]
    assert a[5, 268 + 14 + 13] == t["ramp_data"][5, 1, 13] * t["visible_ramps_mask"][5, 1, 0]
    neg = {**t, "box_data": -np.abs(t["box_data"]) - 1, "visible_boxes_mask": np.zeros((R, 9, 1), np.float32)}
    assert (lockstep.bits(pack_rows(neg, True)[:, 115:268]) == np.int32(-2 ** 31)).all()        # -x * 0 = -0: a product
    mom = moments_of(t)
    assert mom[592] == R and np.isclose(mom[20], c[:, 20].astype(np.float64).sum())


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_oracle_rows_are_finite_and_masks_bite(oracle, cfg):
    snaps = run_oracle(cfg, 130)
    for step, t in snaps.items():
        for actor in (False, True):
            assert np.isfinite(pack_rows(t, actor)).all(), (cfg, step, actor)
        assert np.isfinite(moments_of(t)).all()
        for _, m in ENTITIES:
            assert np.isin(t[m], (0.0, 1.0)).all(), (cfg, step, m)
        assert np.isin(t["self_mask"], (0.0, 1.0)).all()
    # the division column is exercised inside the preparation phase only
    for step in (0, 1):
        col0 = pack_rows(snaps[step], False)[:, 0]
        active = snaps[step]["self_mask"].reshape(-1) > 0
        assert (col0[active] != 0).all() and (col0 <= 1).all(), (cfg, step)
    t = snaps[130]
    assert (t["prep_counter"] == 0).all()                                 # the seekers are released
    hidden = shown = total = 0
    for d, m in ENTITIES:
        mask = np.broadcast_to(t[m].reshape(t[d].shape[0], -1, 1), t[d].reshape(t[d].shape[0], t[m].shape[-2], -1).shape)
        data = t[d].reshape(mask.shape)
        hidden += int(((mask == 0) & (data != 0)).sum())
        shown += int((mask == 1).sum())
        total += data.size
    print(f"{cfg}: mask 0 over non-zero data {hidden / total:.3%}, mask 1 {shown / total:.3%}")
    assert hidden >= 0.01 * total and shown >= 0.01 * total, (cfg, hidden, shown, total)
    if cfg == "var":
        assert (t["self_mask"] == 0).any()


def test_outputs_are_validated_before_the_library_is_called(monkeypatch):
    from gpu_hideseek import policy_inputs as P

    class Lib:                                   # any call into the library fails the test
        def __getattr__(self, name):
            raise AssertionError(f"library function {name} called")

    class Sim:
        num_worlds, agents_per_world, gpu_id = 8, 4, 0
        _L, _h = Lib(), None
    R = 32
    good = torch.zeros(R, ROW)
    for bad, what in ((torch.zeros(R, ROW - 1), "shape"), (torch.zeros(R + 1, ROW), "shape"), (torch.zeros(R * ROW), "shape"),
                      (torch.zeros(R, ROW, dtype=torch.float64), "dtype"), (torch.zeros(R, ROW, dtype=torch.int32), "dtype"),
                      (torch.zeros(ROW, R).t(), "contiguous"), (torch.zeros(R, 2 * ROW)[:, :ROW], "contiguous")):
        for name in ("actor", "critic"):
            with pytest.raises(ValueError, match=what):
                P.pack(Sim(), **{name: bad})
    for bad, what in ((torch.zeros(592, dtype=torch.float64), "shape"), (torch.zeros(593), "dtype"),
                      (torch.zeros(2 * 593, dtype=torch.float64)[::2], "contiguous")):
        with pytest.raises(ValueError, match=what):
            P.pack(Sim(), critic=None, moments=bad)
    with pytest.raises(ValueError, match="on cpu"):           # a well-formed tensor on the wrong device
        P.pack(Sim(), actor=good)
    with pytest.raises(ValueError, match="no output"):
        P.pack(Sim())
    with pytest.raises(ValueError, match="dtype"):
        P.pack(Sim(), actor=True, dtype=torch.float64)
    with pytest.raises(ValueError):
        P.pack(Sim(), actor="yes")


def test_moments_to_mean_var():
    from gpu_hideseek import policy_inputs as P
    rng = np.random.default_rng(1)
    x = rng.normal(2.0, 3.0, size=(50, ROW))
    m = (rng.random(50) < 0.7).astype(np.float64)[:, None]
    mom = torch.from_numpy(np.concatenate([(m * x).sum(0), (m * x * x).sum(0), [m.sum()]]))
    count, mean, var = P.moments_to_mean_var(mom)
    sel = x[m[:, 0] > 0]
    assert count.dtype == mean.dtype == var.dtype == torch.float64 and float(count) == len(sel)
    assert np.allclose(mean.numpy(), sel.mean(0), rtol=1e-12, atol=1e-12)
    assert np.allclose(var.numpy(), sel.var(0), rtol=1e-9, atol=1e-12)
    count, mean, var = P.moments_to_mean_var(torch.zeros(593, dtype=torch.float64))
    assert float(count) == 0 and not mean.any() and not var.any()
    with pytest.raises(ValueError):
        P.moments_to_mean_var(torch.zeros(592, dtype=torch.float64))


def test_header_states_the_request(hideseek_lib):
    """The ctypes mirror of hs_pack_request and the constants agree with include/hideseek.h."""
    import ctypes as C
    import os
    import re
    from gpu_hideseek import policy_inputs as P
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hideseek.h")).read()
    assert re.search(r"HS_PACK_ROW = (\d+)", src).group(1) == str(P.ROW)
    assert re.search(r"HS_PACK_MOMENTS = (\d+)", src).group(1) == str(P.MOMENTS)
    for name, code in (("F32", 1), ("BF16", 3), ("F16", 4)):
        assert re.search(rf"HS_DTYPE_{name} = (\d+)", src).group(1) == str(code)
    assert P._DTYPES == {"float32": 1, "bfloat16": 3, "float16": 4}
    assert C.sizeof(P.HsPackRequest) == 40 and P.HsPackRequest.moments.offset == 32 and P.HsPackRequest.critic.offset == 16
    L = C.CDLL(hideseek_lib)
    assert hasattr(L, "hs_pack_policy_inputs") and hasattr(L, "hs_pack_policy_inputs_async")
