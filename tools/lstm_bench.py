"""Time of the recurrent core's kernels (sim.lstm_cell / lstm_cell_backward, csrc/hs_k_lstm.h) next to the eager
composition a torch learner writes today (recurrent.eager, with backward() for the update) on the same device, and next
to a plain device-to-device copy of as many bytes as the forward call moves (cycling through more than 256 MB of buffers,
so that it runs at the HBM rate and not out of the last-level cache).  The gate GEMMs are not part of either side: both
start from the same gates.

    python tools/lstm_bench.py [--sizes 96000,16384] [--calls 20] [--rounds 3] [--out profiles/lstm_bench.txt]

At n = 96 000 rows (the rollout: 16 000 worlds x 6 agents) and n = 16 384 (one minibatch), H = 256: gates, y and h in
bf16 and f32, the forward alone and the forward plus the backward.  Each variant is timed with device events around
--calls enqueued calls after warm-up; fused, eager and copy alternate inside each of --rounds rounds and the median
window is reported with the spread (max - min) of the windows.  Algorithmic bytes of the forward = gates, c_prev and
clear read once + y, h_next and c_next written once.  Before timing, the fused outputs of the first 2051 rows are
compared once with the float64 restatement of tests/test_lstm_cell_host.py, within the bound it derives for those rows.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402
from gpu_hideseek import recurrent as N  # noqa: E402

HID = 256
COPY_SET = 1 << 29        # bytes the copy baseline cycles through: twice the last-level cache
VARIANTS = [(dt, back) for dt in (torch.bfloat16, torch.float32) for back in (False, True)]


def make_sim():
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=64, sim_flags=0, rand_seed=0, min_hiders=3,
        max_hiders=3, min_seekers=3, max_seekers=3, num_pbt_policies=1)
    sim.init()
    return sim


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls      # ms per call


def bench_variant(sim, n, dtype, back, args):
    import numpy as np
    import test_lstm_cell_host as H
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n % 1000)
    gates = (2.0 * torch.randn(n, 4 * HID, device=dev, generator=g)).to(dtype)
    c_prev = torch.randn(n, HID, device=dev, generator=g)
    params = torch.cat([0.1 * torch.randn(4 * HID, device=dev, generator=g), 1.0 + 0.2 * torch.randn(HID, device=dev, generator=g),
                        0.1 * torch.randn(HID, device=dev, generator=g)])
    clear = (torch.rand(n, device=dev, generator=g) < 0.25).to(torch.int32)
    gy, gh, gc = (torch.randn(n, HID, device=dev, generator=g) / n for _ in range(3))
    gy, gh = gy.to(dtype), gh.to(dtype)
    y, hn = torch.empty(n, HID, dtype=dtype, device=dev), torch.empty(n, HID, dtype=dtype, device=dev)
    cn = torch.empty(n, HID, device=dev)
    gg, gcp, gp = torch.empty(n, 4 * HID, dtype=dtype, device=dev), torch.empty(n, HID, device=dev), torch.empty(N.PARAM_ROWS * HID, device=dev)
    stream = torch.cuda.current_stream()
    leaves = [gates.clone().requires_grad_(True), c_prev.clone().requires_grad_(True), params.clone().requires_grad_(True)]

    def fused():                          # enqueue only, like the eager ops: the events see device time
        sim.lstm_cell(gates, c_prev, params, clear=clear, y=y, h_next=hn, c_next=cn, stream=stream)
        if back:
            sim.lstm_cell_backward(gates, c_prev, params, gy, clear=clear, grad_h_next=gh, grad_c_next=gc, grad_gates=gg, grad_c_prev=gcp,
                                   grad_cell_params=gp, stream=stream)

    def eager():
        if back:
            for t in leaves:
                t.grad = None
            ey, eh, ec = N.eager(leaves[0], leaves[1], leaves[2], clear)
            torch.autograd.backward([ey.to(dtype), eh.to(dtype), ec], [gy, gh, gc])
        else:
            with torch.no_grad():
                ey, eh, ec = N.eager(gates, c_prev, params, clear)
                ey.to(dtype), eh.to(dtype)

    esz = gates.element_size()
    nbytes = n * (4 * HID * esz + HID * 4 + 4 + 2 * HID * esz + HID * 4)
    pairs = [(torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev))
             for _ in range(max(2, -(-COPY_SET // nbytes)))]
    turn = [0]

    def copy():
        src, dst = pairs[turn[0] % len(pairs)]
        turn[0] += 1
        dst.copy_(src)

    variants = {"fused": fused, "eager": eager, "copy": copy}
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    name = str(dtype).replace("torch.", "")
    # the fused y against float64 eager on the first rows: the bound the host tests derive, from these very rows
    m = min(n, 2051)
    x = dict(gates=gates[:m].float().cpu().numpy(), c_prev=c_prev[:m].cpu().numpy(), params=params.cpu().numpy(), clear=clear[:m].cpu().numpy())
    f32, f64 = (H.forward(ft, x["gates"], x["c_prev"], x["params"], x["clear"], HID) for ft in (np.float32, np.float64))
    rel, absolute = H.ROUNDING[name]
    agree = True
    for k, t in (("y", y), ("h_next", hn), ("c_next", cn)):
        tol = 4.0 * float(np.abs(f32[k].astype(np.float64) - f64[k]).max())
        r, a = (rel, absolute) if k != "c_next" else (0.0, 0.0)
        err = np.abs(t[:m].double().cpu().numpy() - f64[k])
        agree = agree and bool((err <= tol + r * np.abs(f64[k]) + a).all())
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    res = {"variant": f"{name}/{'forward+backward' if back else 'forward'}", "n": n, "hidden": HID, "algorithmic_bytes_forward": nbytes,
           "copy_buffer_pairs": len(pairs), "fused_agrees_with_float64": agree}
    for k, ts in times.items():
        res[k] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}
    res["fused_bytes_per_s"] = nbytes / (res["fused"]["ms"] * 1e-3)
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["fused_over_copy"] = res["fused"]["ms"] / res["copy"]["ms"]
    res["faster_than_eager_beyond_both_spreads"] = res["eager"]["ms"] - res["fused"]["ms"] > max(res["eager"]["spread_ms"], res["fused"]["spread_ms"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="96000,16384")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_bench.txt"))
    args = ap.parse_args()
    sim = make_sim()
    results = []
    for n in args.sizes.split(","):
        for dt, back in VARIANTS:
            results.append(bench_variant(sim, int(n), dt, back, args))
            torch.cuda.empty_cache()
    sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "hidden": HID, "calls_per_window": args.calls, "rounds": args.rounds}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n")
        for r in results:
            f.write(json.dumps(r) + "\n")
        f.write("\n%-7s %-26s %10s %8s %10s %8s %10s %8s %14s %13s %10s\n" % (
            "n", "variant", "fused ms", "spread", "eager ms", "spread", "copy ms", "spread", "eager / fused", "fused / copy", "fused GB/s"))
        for r in results:
            f.write("%-7d %-26s %10.4f %8.4f %10.4f %8.4f %10.4f %8.4f %14.1f %13.2f %10.0f\n" % (
                r["n"], r["variant"], r["fused"]["ms"], r["fused"]["spread_ms"], r["eager"]["ms"], r["eager"]["spread_ms"], r["copy"]["ms"],
                r["copy"]["spread_ms"], r["eager_over_fused"], r["fused_over_copy"], r["fused_bytes_per_s"] / 1e9))
    if not all(r["fused_agrees_with_float64"] for r in results):
        sys.exit("the fused outputs differ from the float64 restatement beyond the derived bound")


if __name__ == "__main__":
    main()
