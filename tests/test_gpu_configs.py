"""BASELINE.json configs[3] and configs[4] on ONE GPU, against the oracle.

configs[3] = 131 072 worlds sharded over 8 GPUs: a rank is a 16 384-world handle with a `world_offset`; the last
rank (offset 114 688) is run here for 245 steps, i.e. across the lock-step level regeneration of step 240.
configs[4] = 16 000 worlds as scripts/jax_train.py drives them: flags RandomFlipTeams|UseFixedWorld|
ZeroAgentVelocity, seed 5, 3 hiders + 3 seekers, actions from the real bucket ranges [0,5)^3 x [0,2)^2
(scripts/jax_train.py:69-81,146-148), through the stream entry point with caller-owned buffers
(Manager::gpuJAXStep, src/mgr.cpp:379-398, 1006-1022).

Full-size runs are checked through size-independent properties (finite state, the done / prep-counter /
reward timeline, seed rows = {episode, GLOBAL world id}) AND against the oracle on EVERY world, bit for bit: the oracle
steps the whole batch beside the GPU on up to 16 host threads (no sampled ranges).  configs[1] — the
benchmark batch, 16 000 worlds x 245 steps across the lock-step regeneration — is here as well.
"""
import numpy as np
import pytest

from lockstep import OBS, GpuSide, Pair, check, hashed

pytestmark = pytest.mark.gpu


def test_config3_last_shard_of_131072_worlds(oracle):
    import torch
    N, A, OFF, STEPS = 16384, 4, 114688, 245
    # the oracle runs the WHOLE shard beside the GPU (every world, not sampled ranges)
    p = Pair(N, world_offset=OFF)
    sim = p.sim
    moves = hashed((10, 10), shift=5, first_row=OFF * A)
    done, prep, reward = p.gpu.view("done"), p.gpu.view("prep_counter"), p.gpu.view("reward")
    for s in range(STEPS):
        p.step(moves(s, p.rows), cols=(0, 1))
        if s % 7 == 6:                 # every 7th step: body state and the observations that feed a policy, every world
            p.check(s, names=("self_data", "lidar", "box_data", "reward"), walls=False)
        # timeline (sim.cpp:806-841, 448-464): every world is in lock-step
        if s in (0, 50, 94, 95, 200, 238, 239, 240, 244):
            ep_step = s % 240          # curEpisodeStep the step ran with
            assert (done == (1 if ep_step == 239 else 0)).all(), s
            after = (ep_step + 1) % 240
            assert (prep == max(96 - after, 0)).all(), s
            if ep_step < 95:
                assert (reward == 0).all(), s
            else:
                assert (reward != 0).all(), s
    body, meta = sim.debug_bodies()
    assert np.isfinite(body).all()
    lidar = sim.lidar_tensor().to_torch()
    assert torch.isfinite(lidar).all() and (lidar >= 0).all() and (lidar <= 200).all()
    seed = sim.seed_tensor().to_torch().cpu().numpy().reshape(N, A, 2)
    assert (seed[:, :, 0] == 1).all(), "second episode after the regeneration at step 240"
    assert (seed[:, :, 1] == (OFF + np.arange(N))[:, None]).all(), "seed rows carry GLOBAL world ids (sim.cpp:107-111)"
    assert (sim.debug_walls()[1][:, 6] == STEPS % 240).all()
    p.check("end", names=OBS + ["reward", "done", "global_positions", "episode_result", "seed"])
    assert sim.device_status()["dropped_candidate_pairs"] == 0


def test_config4_jax_train_workload_through_stream_step(oracle):
    import torch
    N, A, STEPS = 16000, 6, 245
    p = Pair(N, flags=13, seed=5, hiders=(3, 3), seekers=(3, 3), init=False)
    sim = p.sim
    assert sim.agents_per_world == A
    dev = torch.device("cuda", 0)
    R = N * A
    own = {k: getattr(sim, k + "_tensor")().to_torch() for k in OBS + ["reward", "done", "episode_result"]}
    obs = [torch.zeros_like(own[k]) for k in OBS]
    rew, done, epres = (torch.zeros_like(own[k]) for k in ("reward", "done", "episode_result"))
    act = torch.zeros(R, 5, dtype=torch.int32, device=dev)
    resets = torch.zeros(N, 1, dtype=torch.int32, device=dev)
    pol = torch.zeros(R, 1, dtype=torch.int32, device=dev)
    strm = torch.cuda.Stream()
    sim.stream_init(strm.cuda_stream, obs)
    p.ref.init()                                 # the oracle runs every world beside the GPU
    names = OBS + ["reward", "done", "episode_result"]
    buffers = GpuSide(sim, views=dict(zip(names, obs + [rew, done, epres])))    # the caller-owned outputs as a side
    buckets = hashed((5, 5, 5, 2, 2))            # actions_num_buckets (scripts/jax_train.py:146-148)
    grabbed = 0
    for s in range(STEPS):
        a = buckets(s, R).astype(np.int32)
        p.ref.tensor("action")[:] = a
        act.copy_(torch.from_numpy(a).to(dev))
        p.ref.step()
        strm.wait_stream(torch.cuda.current_stream())
        sim.stream_step(strm.cuda_stream, [act, resets, pol] + obs + [rew, done, epres])
        strm.synchronize()
        if s in (0, 94, 95, 150, 239, 240, 244):
            ep_step = s % 240
            assert (done == (1 if ep_step == 239 else 0)).all(), s
            assert (obs[0] == max(96 - (ep_step + 1) % 240, 0)).all(), s
            assert torch.isfinite(obs[1]).all() and torch.isfinite(obs[4]).all(), s
            assert ((rew == 0).all() if ep_step < 95 else (rew != 0).all()), s
            grabbed += int(obs[1][:, 12].sum().item())
            check(buffers, p.ref, s, names=names, bodies=False, walls=False)
    assert grabbed > 0, "grab joints were live at some checked step"
    body, meta = sim.debug_bodies()
    assert np.isfinite(body).all()
    # quaternions stay normalised in ZeroAgentVelocity mode (240 N m torques): |q|^2 within 1e-3 of 1
    q2 = (body[:, :, 3:7] ** 2).sum(axis=2)
    live = meta[:, :, 0] >= 0
    assert np.abs(q2[live] - 1).max() < 1e-3
    # UseFixedWorld: every world holds the same wall layout
    walls, info = sim.debug_walls()
    assert (walls == walls[0]).all() and (info[:, 0] == info[0, 0]).all()
    p.check("end", names=(), walls=False)
    assert sim.device_status()["dropped_candidate_pairs"] == 0


def test_config1_benchmark_batch_every_world_against_the_oracle(oracle):
    """BASELINE.json configs[1]: 16 000 worlds, 2 hiders + 2 seekers, flags 0, seed 0, move actions in [-5, 4] on columns
    0-1 (scripts/benchmark.py:21-35, 82-84), 245 steps — across the regeneration of every level at step 240.  Every exported
    tensor, body and wall of every world against the oracle at every 7th step and at the end."""
    N, STEPS = 16000, 245
    p = Pair(N)
    moves = hashed((10, 10), shift=5)
    names = OBS + ["reward", "done", "global_positions", "episode_result", "seed", "action"]
    checked = 0
    for s in range(STEPS):
        p.step(moves(s, p.rows), cols=(0, 1))
        if s % 7 == 6 or s == STEPS - 1:
            p.check(s, names=names)
            checked += 1
    assert checked == 35
    st = p.sim.device_status()
    assert st["dropped_candidate_pairs"] == 0
