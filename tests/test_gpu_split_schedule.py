"""The split schedule of the blocking step (csrc/hideseek.hip launch_step): step() runs the late and
the early octets as two k_physics -> k_observe chains on two streams, step_async() on a caller's stream keeps the one
chain.  Both must leave the same bits in every tensor of train_interface() and in debug_bodies() after every step, at
every threshold, and device_status() must show which steps ran split and how many octets were late."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BALANCE_PERIOD = 32          # hs_k_balance.h kBalancePeriod: the step with the deal keeps the one chain


def _sim(n, hiders=2, seekers=2, **kw):
    import gpu_hideseek
    args = dict(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=0, rand_seed=11,
                min_hiders=hiders, max_hiders=hiders, min_seekers=seekers, max_seekers=seekers, num_pbt_policies=1)
    args.update(kw)
    return gpu_hideseek.HideAndSeekSimulator(**args)


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _tensors(sim):
    return [(f"{role}/{name}", t.to_torch()) for role, d in sim.train_interface().items() for name, t in d.items() if t is not None]


def _run(n, steps, hiders=2, seekers=2, threshold=None, profile_every=0, sim_flags=0):
    """Steps a split simulator and a serial one side by side under the same random move / grab / lock actions and
    compares them after every step.  Returns the split simulator's device_status() after every step."""
    import torch
    a, b = _sim(n, hiders, seekers, sim_flags=sim_flags), _sim(n, hiders, seekers, sim_flags=sim_flags)
    if threshold is not None:
        a.set_late_threshold(threshold)
    a.init(); b.init()
    act_a, act_b = a.action_tensor().to_torch(), b.action_tensor().to_torch()
    ta, tb = _tensors(a), _tensors(b)
    assert len(ta) == len(tb) > 10
    side = torch.cuda.Stream()
    gen = torch.Generator(device="cuda"); gen.manual_seed(3)
    rows = act_a.shape[0]
    status = []
    for i in range(steps):
        act = torch.cat([torch.randint(0, 11, (rows, 3), generator=gen, device="cuda", dtype=torch.int32),
                         torch.randint(0, 2, (rows, 2), generator=gen, device="cuda", dtype=torch.int32)], dim=1)
        act_a.copy_(act); act_b.copy_(act)
        profiled = profile_every > 0 and i % profile_every == 0
        if profile_every > 0:
            a.set_profiling(profiled)
        a.step()
        side.wait_stream(torch.cuda.current_stream())
        b.step_async(side.cuda_stream)
        side.synchronize()
        if profiled:
            ms = a.last_step_kernel_ms()
            assert ms["physics"] > 0 and (ms["observe"] > 0 or sim_flags), (i, ms)
        for (name, x), (_, y) in zip(ta, tb):
            assert torch.equal(_bits(x), _bits(y)), (i, name)
        (ba, ma), (bb, mb) = a.debug_bodies(), b.debug_bodies()
        assert np.array_equal(ba.view(np.int32), bb.view(np.int32)) and np.array_equal(ma, mb), (i, "bodies")
        status.append(a.device_status())
    st_b = b.device_status()
    assert st_b["split_steps"] == 0 and st_b["late_octets"] == 0, "step_async keeps the one chain"
    return status


def _late_per_step(status):
    """(ran split, late octets) of every step, from the sticky counters."""
    out, prev = [], {"split_steps": 0, "late_octets": 0}
    for st in status:
        out.append((st["split_steps"] - prev["split_steps"], st["late_octets"] - prev["late_octets"]))
        prev = st
    return out


def test_split_and_serial_steps_agree_over_an_episode_and_eight_deals():
    """20 worlds = two full octets and a half-empty one (slots without a world), 260 steps: past the regeneration of
    every level at step 240 and eight deals of the worlds."""
    steps = 260
    status = _run(20, steps)
    assert status[-1]["split_steps"] == steps - steps // BALANCE_PERIOD
    per = _late_per_step(status)
    assert all(split in (0, 1) and 0 <= late <= 3 * split for split, late in per), per
    assert any(split == 1 and 0 < late < 3 for split, late in per), "no step with both groups non-empty"


@pytest.mark.parametrize("threshold, late_octets", [(float("inf"), 0), (0.0, 3)])
def test_thresholds_at_the_extremes(threshold, late_octets):
    """Nobody late / everybody late: one launch of each pair finds no octet to serve."""
    steps = 40
    status = _run(20, steps, threshold=threshold)
    assert status[-1]["split_steps"] == steps - steps // BALANCE_PERIOD
    per = _late_per_step(status)
    # (the groups of the first two steps were formed before any physics wave had been timed: all early)
    assert all(late == late_octets * split for split, late in per[2:]), per
    assert all(late == 0 for _, late in per[:2]), per


def test_profiled_steps_keep_the_one_chain_between_split_steps():
    steps, every = 40, 3
    status = _run(20, steps, profile_every=every)
    per = _late_per_step(status)
    # the 32nd step carries the deal; step i is profiled when i % 3 == 0
    expect = [0 if i % every == 0 or (i + 1) % BALANCE_PERIOD == 0 else 1 for i in range(steps)]
    assert [split for split, _ in per] == expect


def test_three_hiders_and_three_seekers():
    """k_physics<3> and k_observe<320>."""
    steps = 40
    status = _run(16, steps, hiders=3, seekers=3)
    assert status[-1]["split_steps"] == steps - steps // BALANCE_PERIOD


def test_skipped_observations_are_never_split():
    status = _run(16, 40, sim_flags=1 << 16)
    assert status[-1]["split_steps"] == 0 and status[-1]["late_octets"] == 0


def test_the_threshold_is_checked():
    sim = _sim(16)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            sim.set_late_threshold(bad)
    sim.set_late_threshold(1.25)
