"""Grouped advantages on the GPU (sim.compute_advantages(groups=G), hs_compute_gae_grouped, csrc/hs_k_gae.h): R = 216 rows in
G in {1, 2, 3, 6} groups of m = 216, 108, 72, 36 rows (three of them no multiple of the 64 rows of a workgroup), T in
{1, 8, 9, 17} around the register block of 8.  Advantages and returns are the ungrouped call's bit for bit; the moments of
group g are, bit for bit, those of compute_advantages on a second handle of m rows given the group's columns made
contiguous; G = 1 gives the ungrouped moments of the same handle."""
import numpy as np
import pytest

from test_advantages_host import GAMMA, LAMBDA, inputs

pytestmark = pytest.mark.gpu

AGENTS, WORLDS = 6, 36
R = AGENTS * WORLDS
GROUPS = (1, 2, 3, 6)
STEPS = (1, 8, 9, 17)


@pytest.fixture(scope="module")
def sims():
    """{rows: an initialised simulator}: 216 rows and the 108, 72 and 36 of a group (18, 12 and 6 worlds)."""
    import gpu_hideseek
    made = {}
    for worlds in sorted({WORLDS // g for g in GROUPS}):
        s = gpu_hideseek.HideAndSeekSimulator(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=0, rand_seed=1,
                                              min_hiders=3, max_hiders=3, min_seekers=3, max_seekers=3, num_pbt_policies=1)
        s.init()
        made[worlds * AGENTS] = s
    yield made
    for s in made.values():
        s.close()


def _device(x, dtype):
    import torch
    out = {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}
    out["value"], out["bootstrap"] = (out[k].to(getattr(torch, dtype)) for k in ("value", "bootstrap"))
    return out


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("masked", (True, False))
@pytest.mark.parametrize("dtype", ("float32", "bfloat16"))
def test_grouped_moments_are_each_groups_own_call(sims, dtype, masked):
    import torch
    sim = sims[R]
    for T in STEPS:
        x = inputs(T, R, dtype, masked=masked, seed=5, p_done=0.15)          # dones, and NaN behind the mask
        assert (x["done"] != 0).any()
        d = _device(x, dtype)
        args = (d["reward"], d["done"], d["value"], d["bootstrap"])
        kw = dict(gamma=GAMMA, gae_lambda=LAMBDA, mask=d["mask"])
        plain = sim.compute_advantages(*args, moments=True, **kw)
        for G in GROUPS:
            tag = (dtype, masked, T, G)
            m = R // G
            out = sim.compute_advantages(*args, moments=True, groups=G, **kw)
            assert tuple(out["moments"].shape) == (G, 5) and out["moments"].dtype == torch.float64, tag
            assert torch.equal(_bits(out["advantages"]), _bits(plain["advantages"])) and torch.equal(_bits(out["returns"]), _bits(plain["returns"])), tag
            if G == 1:
                assert torch.equal(_bits(out["moments"][0]), _bits(plain["moments"])), tag
            for g in range(G):
                cols = slice(g * m, (g + 1) * m)
                own = sims[m].compute_advantages(*(t[:, cols].contiguous() for t in args[:3]), d["bootstrap"][cols].contiguous(), gamma=GAMMA, gae_lambda=LAMBDA,
                                                 mask=None if d["mask"] is None else d["mask"][:, cols].contiguous(), moments=True)
                assert torch.equal(_bits(out["moments"][g]), _bits(own["moments"])), (tag, g, out["moments"][g].tolist(), own["moments"].tolist())
                assert torch.equal(_bits(out["advantages"][:, cols]), _bits(own["advantages"])), (tag, g)
            # the count of every group is the number of its active pairs, and the groups add up
            active = np.ones((T, R)) if x["mask"] is None else (x["mask"] != 0)
            assert out["moments"][:, 4].tolist() == [float(active[:, g * m:(g + 1) * m].sum()) for g in range(G)], tag


def test_moments_alone_given_tensors_and_two_calls(sims):
    """moments without advantages and returns, into a given [G, 5] tensor; advantages alone without moments; the same bits
    on a second call."""
    import torch
    sim, T, G = sims[R], 9, 3
    d = _device(inputs(T, R, "float32", masked=True, seed=6), "float32")
    args = (d["reward"], d["done"], d["value"], d["bootstrap"])
    full = sim.compute_advantages(*args, mask=d["mask"], moments=True, groups=G)
    mom = torch.full((G, 5), -1.0, dtype=torch.float64, device="cuda")
    only = sim.compute_advantages(*args, mask=d["mask"], advantages=None, returns=None, moments=mom, groups=G)
    assert set(only) == {"moments"} and only["moments"] is mom and torch.equal(_bits(mom), _bits(full["moments"]))
    adv = sim.compute_advantages(*args, mask=d["mask"], returns=None, groups=G)
    assert set(adv) == {"advantages"} and torch.equal(_bits(adv["advantages"]), _bits(full["advantages"]))
    again = sim.compute_advantages(*args, mask=d["mask"], moments=True, groups=G)
    assert all(torch.equal(_bits(again[k]), _bits(full[k])) for k in full)


def test_the_library_refuses():
    import ctypes as C
    import torch
    from gpu_hideseek import advantages as A
    from gpu_hideseek._native import check
    import gpu_hideseek
    sim = gpu_hideseek.HideAndSeekSimulator(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=6, sim_flags=0, rand_seed=1,
                                            min_hiders=3, max_hiders=3, min_seekers=3, max_seekers=3, num_pbt_policies=1)
    try:
        sim.init()
        T, rows = 4, 36
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")       # noqa: E731
        x = (z(T, rows), z(T, rows, dt=torch.int32), z(T, rows), z(rows))
        mom = z(3, 5, dt=torch.float64)

        def refused(what, groups=None, **change):
            _, req = A.request(6, 6, 0, *x, moments=mom, groups=3)
            if groups is not None:
                req.groups = groups
            for name, v in change.items():
                setattr(req.gae, name, v)
            with pytest.raises(Exception, match=what):
                check(sim._L.hs_compute_gae_grouped(sim._h, C.byref(req)))
        refused("groups must be in", groups=0)
        refused("groups must be in", groups=17)
        refused("multiple of groups", groups=5)
        refused("null reward", reward=None)
        refused("steps must be in", steps=0)
        refused("moments must be 8-byte aligned", moments=mom.data_ptr() + 4)
        # the moments range is G vectors: the third one overlaps here, the first does not
        both = z(T * rows + 32, dt=torch.float64)                  # room for either, so both pointers stay inside one allocation
        refused("moments overlaps advantage", advantage=both.data_ptr() + 2 * 5 * 8, moments=both.data_ptr())
    finally:
        sim.close()
