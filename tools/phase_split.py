"""Per-phase time of k_physics and per-section time of k_observe, separately for the preparation phase of an episode
(episode steps 0 .. 94: no reward rays) and the rest (95 .. 238), over two episodes of the benchmark workload.

Needs the timing build of the library (python marl-hideandseek_amd/build.py --timing):
  HS_LIB_PATH=$PWD/marl-hideandseek_amd/lib/libhideseek_timing.so python tools/phase_split.py
"""
import os, sys, ctypes as C, numpy as np, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "marl-hideandseek_amd"))
import gpu_hideseek
N = 16000
sim = gpu_hideseek.HideAndSeekSimulator(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=N, sim_flags=0, rand_seed=0,
    min_hiders=2, max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1)
act = sim.action_tensor().to_torch()
torch.manual_seed(0)
sim.init()
nb = (N + 7) // 8
L = sim._L
L.hs_debug_phase_ticks.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
L.hs_debug_observe_ticks.argtypes = [C.c_void_p, C.c_void_p]
def read():
    torch.cuda.synchronize()
    out = np.zeros((nb, 10), np.int64); L.hs_debug_phase_ticks(sim._h, out.ctypes.data, nb)
    ob = np.zeros(16, np.int64); L.hs_debug_observe_ticks(sim._h, ob.ctypes.data)
    return out, ob
names = ["pre", "integrate", "detect", "sat", "dd_pos", "body_pos", "dd_vel", "body_vel", "post+store", "load"]
onames = ["stage(+wait)", "agent table", "ray setup", "walls", "planes", "cull(+barrier)", "hull tests", "ray results", "obs rows"]
marks = [0, 95, 239, 240 + 95, 240 + 239]
snaps = [read()]
s = 0
for m in marks[1:]:
    while s < m:
        sim.step(); act[:, :2] = torch.randint(-5, 5, (N * 4, 2), dtype=torch.int32, device="cuda"); s += 1
    snaps.append(read())
print("lib", os.environ.get("HS_LIB_PATH"))
for k in range(1, len(marks)):
    n = marks[k] - marks[k - 1]
    us = (snaps[k][0] - snaps[k - 1][0]) / 100.0 / n
    print(f"-- steps [{marks[k-1]}, {marks[k]}): us per wave and step, mean / max over {nb} waves")
    print("   " + "  ".join(f"{nm} {us[:, i].mean():.2f}/{us[:, i].max():.2f}" for i, nm in enumerate(names)) + f"  total {us.sum(axis=1).mean():.1f}/{us.sum(axis=1).max():.1f}")
    ob = (snaps[k][1] - snaps[k - 1][1]) / 100.0 / n / (N * 3)
    print("   k_observe us per wave and launch: " + "  ".join(f"{nm} {ob[i]:.2f}" for i, nm in enumerate(onames)) + f"  sum {ob[:9].sum():.2f}")
