"""Time of the dense layer's kernels (sim.dense_norm_act / dense_norm_act_backward, csrc/hs_k_dense.h) next to the eager
composition a torch learner writes today (mlp.eager, with backward() for the update) on the same device, and next to a
plain device-to-device copy of as many bytes as the forward call moves (cycling through more than 256 MB of buffers, so
that it runs at the HBM rate and not out of the last-level cache).  The GEMM is not part of either side: both start
from the same z.  Then one pair of rows for the whole backbone: policy.Backbone.forward (encoder, three layers, LSTM,
GEMMs included) with fused=True and with fused=False, the number that stands next to the simulator's step.

    python tools/mlp_bench.py [--sizes 96000,16384] [--calls 20] [--rounds 3] [--out profiles/mlp_bench.txt]

At n = 96 000 rows (the rollout: 16 000 worlds x 6 agents) and n = 16 384 (one minibatch), C = 256: z and y in bf16 and
f32, the forward alone and the forward plus the backward.  Each variant is timed with device events around --calls
enqueued calls after warm-up; fused, eager and copy alternate inside each of --rounds rounds and the median window is
reported with the spread (max - min) of the windows.  Algorithmic bytes of the forward = z read once + y written once.
Before timing, the fused y of the first 2051 rows is compared once with the float64 restatement of
tests/test_mlp_host.py, within the bound it derives for those rows.
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
from gpu_hideseek import mlp as M  # noqa: E402
from gpu_hideseek import policy as P  # noqa: E402

CH = 256
COPY_SET = 1 << 29        # bytes the copy baseline cycles through: twice the last-level cache
VARIANTS = [(dt, back) for dt in (torch.bfloat16, torch.float32) for back in (False, True)]
BACKBONE_ROWS = 96000


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


def measure(variants, args):
    """{name: {ms, ms_windows, spread_ms, calls_per_window}}: the variants alternate inside each round."""
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    return {k: {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls} for k, ts in times.items()}


def bench_variant(sim, n, dtype, back, args):
    import numpy as np
    import test_mlp_host as H
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n % 1000)
    z = torch.randn(n, CH, device=dev, generator=g).to(dtype)
    params = torch.cat([0.1 * torch.randn(CH, device=dev, generator=g), 1.0 + 0.2 * torch.randn(CH, device=dev, generator=g),
                        0.1 * torch.randn(CH, device=dev, generator=g)])
    gy = (torch.randn(n, CH, device=dev, generator=g) / n).to(dtype)
    y, gz, gp = torch.empty(n, CH, dtype=dtype, device=dev), torch.empty(n, CH, dtype=dtype, device=dev), torch.empty(M.PARAM_ROWS * CH, device=dev)
    stream = torch.cuda.current_stream()
    leaves = [z.clone().requires_grad_(True), params.clone().requires_grad_(True)]

    def fused():                          # enqueue only, like the eager ops: the events see device time
        sim.dense_norm_act(z, params, y=y, stream=stream)
        if back:
            sim.dense_norm_act_backward(z, params, gy, grad_z=gz, grad_params=gp, stream=stream)

    def eager():
        if back:
            for t in leaves:
                t.grad = None
            M.eager(leaves[0], leaves[1]).to(dtype).backward(gy)
        else:
            with torch.no_grad():
                M.eager(z, params).to(dtype)

    esz = z.element_size()
    nbytes = n * 2 * CH * esz
    pairs = [(torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev))
             for _ in range(max(2, -(-COPY_SET // nbytes)))]
    turn = [0]

    def copy():
        src, dst = pairs[turn[0] % len(pairs)]
        turn[0] += 1
        dst.copy_(src)

    res = {"variant": f"{str(dtype).replace('torch.', '')}/{'forward+backward' if back else 'forward'}", "n": n, "channels": CH,
           "algorithmic_bytes_forward": nbytes, "copy_buffer_pairs": len(pairs)}
    res.update(measure({"fused": fused, "eager": eager, "copy": copy}, args))
    # the fused y against the float64 restatement on the first rows: the bound the host tests derive, from these very rows
    name = str(dtype).replace("torch.", "")
    m = min(n, 2051)
    f32, f64 = (H.forward(ft, z[:m].float().cpu().numpy(), params.cpu().numpy(), CH)["y"] for ft in (np.float32, np.float64))
    rel, absolute = H.ROUNDING[name]
    err = np.abs(y[:m].double().cpu().numpy() - f64)
    res["fused_agrees_with_float64"] = bool((err <= 4.0 * float(np.abs(f32.astype(np.float64) - f64).max()) + rel * np.abs(f64) + absolute).all())
    res["fused_bytes_per_s"] = nbytes / (res["fused"]["ms"] * 1e-3)
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["fused_over_copy"] = res["fused"]["ms"] / res["copy"]["ms"]
    res["faster_than_eager_beyond_both_spreads"] = res["eager"]["ms"] - res["fused"]["ms"] > max(res["eager"]["spread_ms"], res["fused"]["spread_ms"])
    print(json.dumps(res), flush=True)
    return res


def bench_backbone(sim, n, args):
    """policy.Backbone.forward on n bf16 rows, one rollout step without autograd: every kernel and every GEMM of the
    backbone, with the project's kernels (fused=True) and with the eager pieces on the same parameters (fused=False)."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(7)
    rows = torch.randn(n, 296, device=dev, generator=g).to(torch.bfloat16)
    clear = (torch.rand(n, device=dev, generator=g) < 0.01).to(torch.int32)
    net = P.Backbone().to(dev)
    state = net.init_state(n, dev, torch.bfloat16)

    def run(flag):
        def fn():
            net.set_fused(flag)
            with torch.no_grad():
                net(sim if flag else None, rows, state, clear)
        return fn

    res = {"variant": "bfloat16/Backbone.forward", "n": n}
    res.update(measure({"fused": run(True), "eager": run(False)}, args))
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["faster_than_eager_beyond_both_spreads"] = res["eager"]["ms"] - res["fused"]["ms"] > max(res["eager"]["spread_ms"], res["fused"]["spread_ms"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="96000,16384")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_bench.txt"))
    args = ap.parse_args()
    sim = make_sim()
    results = []
    for n in args.sizes.split(","):
        for dt, back in VARIANTS:
            results.append(bench_variant(sim, int(n), dt, back, args))
            torch.cuda.empty_cache()
    backbone = bench_backbone(sim, BACKBONE_ROWS, args)
    sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "channels": CH, "calls_per_window": args.calls, "rounds": args.rounds}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n")
        for r in results + [backbone]:
            f.write(json.dumps(r) + "\n")
        f.write("\n%-7s %-26s %10s %8s %10s %8s %10s %8s %14s %13s %10s\n" % (
            "n", "variant", "fused ms", "spread", "eager ms", "spread", "copy ms", "spread", "eager / fused", "fused / copy", "fused GB/s"))
        for r in results:
            f.write("%-7d %-26s %10.4f %8.4f %10.4f %8.4f %10.4f %8.4f %14.1f %13.2f %10.0f\n" % (
                r["n"], r["variant"], r["fused"]["ms"], r["fused"]["spread_ms"], r["eager"]["ms"], r["eager"]["spread_ms"], r["copy"]["ms"],
                r["copy"]["spread_ms"], r["eager_over_fused"], r["fused_over_copy"], r["fused_bytes_per_s"] / 1e9))
        r = backbone
        f.write("%-7d %-26s %10.4f %8.4f %10.4f %8.4f %10s %8s %14.1f\n" % (
            r["n"], r["variant"], r["fused"]["ms"], r["fused"]["spread_ms"], r["eager"]["ms"], r["eager"]["spread_ms"], "-", "-", r["eager_over_fused"]))
    if not all(r["fused_agrees_with_float64"] for r in results):
        sys.exit("the fused y differs from the float64 restatement beyond the derived bound")


if __name__ == "__main__":
    main()
