"""Rays/s of the spectator cameras (hs_render_cameras, csrc/hs_k_spectate.h), culled and with HS_SPECTATE_NO_CULL.

    python tools/spectate_bench.py [--window 1.0] [--json out.json] [--cases top1024,mosaic256,agents64]

  top1024    one 1024 x 1024 top-down camera on each of 64 worlds
  mosaic256  256 worlds x 256 x 256 top-down (a training-monitor mosaic)
  agents64   every agent view of 16 000 worlds at 64 x 64 as spectator cameras, next to hs_render (k_render) on the
             same pixels

Each call is blocking (camera upload, launch, synchronise).  After warm-up, the variants alternate; each timing is a
window of repeated calls at least --window seconds long, and the median of --rounds windows is reported.  The culled
and unculled outputs (and, for agents64, k_render's) are compared bit for bit.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402
from gpu_hideseek import spectate as S  # noqa: E402


def make_sim(n, render=None, steps=120):
    kw = {} if render is None else dict(enable_batch_renderer=True, batch_render_width=render[0],
                                        batch_render_height=render[1])
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=0, rand_seed=0, min_hiders=2,
        max_hiders=2, min_seekers=2, max_seekers=2, num_pbt_policies=1, **kw)
    sim.init()
    act = sim.action_tensor().to_torch()
    g = torch.Generator(device=act.device).manual_seed(0)
    for _ in range(steps):
        act[:, 0:2] = torch.randint(-5, 5, (act.shape[0], 2), device=act.device, dtype=torch.int32, generator=g)
        sim.step()
    return sim


def window(fn, seconds):
    torch.cuda.synchronize()
    k, t0 = 0, time.perf_counter()
    while True:
        fn()
        k += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt / k, k


def bench_case(name, sim, cams, W, H, args, k_render=False):
    arr = S.camera_array(cams)
    V = arr.size
    outs = {e: sim.spectate(arr, W, H, hit=True, exact=e) for e in (False, True)}
    variants = {"culled": lambda: sim.spectate(arr, W, H, hit=True, out=outs[False]),
                "no_cull": lambda: sim.spectate(arr, W, H, hit=True, out=outs[True], exact=True)}
    if k_render:
        variants["hs_render"] = sim.render
    for fn in variants.values():                   # warm-up
        for _ in range(2):
            fn()
    times = {k: [] for k in variants}
    calls = {k: 0 for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            dt, n = window(fn, args.window)
            times[k].append(dt)
            calls[k] += n
    same = all(torch.equal(outs[False][k].view(torch.int32) if k != "rgb" else outs[False][k],
                           outs[True][k].view(torch.int32) if k != "rgb" else outs[True][k]) for k in outs[False])
    res = {"case": name, "cameras": V, "width": W, "height": H, "pixels": V * W * H, "culled_equals_no_cull": bool(same)}
    for k, ts in times.items():
        med = statistics.median(ts)
        res[k] = {"ms": med * 1e3, "ms_windows": [t * 1e3 for t in ts], "calls": calls[k],
                  "g_rays_per_s": V * W * H / med / 1e9}
    if k_render:                                   # cameras in view order: world * A + agent
        d = sim.depth_tensor().to_torch().reshape(-1, H, W)
        c = sim.rgb_tensor().to_torch().reshape(-1, H, W, 4)
        res["equals_hs_render"] = bool(torch.equal(outs[False]["depth"].view(torch.int32), d.view(torch.int32))
                                       and torch.equal(outs[False]["rgb"], c))
    res["speedup_culled_vs_no_cull"] = res["no_cull"]["ms"] / res["culled"]["ms"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="top1024,mosaic256,agents64")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    want = args.cases.split(",")
    results = []
    if "top1024" in want:
        sim = make_sim(64)
        results.append(bench_case("top1024", sim, [S.top_down(w) for w in range(64)], 1024, 1024, args))
        sim.close()
    if "mosaic256" in want:
        sim = make_sim(256)
        results.append(bench_case("mosaic256", sim, [S.top_down(w) for w in range(256)], 256, 256, args))
        sim.close()
    if "agents64" in want:
        n = 16000
        sim = make_sim(n, render=(64, 64))
        bodies = sim.debug_bodies()[0]
        A = sim.agents_per_world                   # 2 + 2: every agent is active, rows w * A + a
        cams = [S.agent_camera(bodies, w, a) for w in range(n) for a in range(A)]
        results.append(bench_case("agents64", sim, cams, 64, 64, args, k_render=True))
        sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "rounds": args.rounds}
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"meta": meta, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
