"""Time of the entity encoder kernels (sim.encode_entities / encode_entities_backward, csrc/hs_k_embed.h) next to the
eager composition a torch learner writes today (entity_encoder.eager, with backward() for the update) on the same device,
and next to a plain device-to-device copy of as many bytes as the forward call moves (cycling through more than 256 MB of
buffers, so that it runs at the HBM rate and not out of the last-level cache).

    python tools/embed_bench.py [--sizes 96000,16384] [--calls 20] [--rounds 3] [--out profiles/embed_bench.txt]

At n = 96 000 rows (the rollout: 16 000 worlds x 6 agents) and n = 16 384 (one minibatch), E = 64: rows and features in
bf16 and f32, the forward alone and the forward plus the backward.  Each variant is timed with device events around
--calls enqueued calls after warm-up; fused, eager and copy alternate inside each of --rounds rounds and the median
window is reported with the spread (max - min) of the windows.  Algorithmic bytes of the forward = rows read once +
features written once.  Before timing, the fused and the eager features are compared once within the tolerances
tests/test_entity_encoder_host.py derives.
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
from gpu_hideseek import entity_encoder as N  # noqa: E402
from gpu_hideseek import policy_inputs as P  # noqa: E402

E = 64
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
    import test_entity_encoder_host as H
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n % 1000)
    rows = torch.randn(n, P.ROW, device=dev, generator=g)
    for name in P.MASKS:                                      # a third of the pooled entities masked, as an actor sees them
        lo, hi, (NE, K) = P.LAYOUT[name]
        keep = (torch.rand(n, NE, 1, device=dev, generator=g) >= 1.0 / 3.0).float()
        rows[:, lo:hi] = (rows[:, lo:hi].view(n, NE, K) * keep).view(n, NE * K)
    rows = rows.to(dtype)
    params = N.init_params(E, torch.Generator().manual_seed(0)).to(dev)
    up = (torch.randn(n, 4 * E, device=dev, generator=g) / n).to(dtype)
    feats = torch.empty(n, 4 * E, dtype=dtype, device=dev)
    argmax = torch.empty(n, 3, E, dtype=torch.uint8, device=dev)
    gp = torch.empty(N.PARAM_ROWS * E, device=dev)
    stream = torch.cuda.current_stream()
    leaf = params.clone().requires_grad_(True)

    def fused():                          # enqueue only, like the eager ops: the events see device time
        sim.encode_entities(rows, params, embed_dim=E, features=feats, argmax=argmax if back else None, stream=stream)
        if back:
            sim.encode_entities_backward(rows, params, up, argmax, embed_dim=E, grad_params=gp, stream=stream)

    def eager():
        if back:
            leaf.grad = None
            N.eager(rows, leaf, E).to(dtype).backward(up)
        else:
            with torch.no_grad():
                N.eager(rows, params, E).to(dtype)

    esz = rows.element_size()
    nbytes = n * (P.ROW + 4 * E) * esz
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
    rel, absolute = (2 * r for r in H.ROUNDING[name])                   # both sides round to the narrow type
    with torch.no_grad():
        want = N.eager(rows, params, E).double()
        tol = torch.tensor(H.feature_tolerance(E), device=dev).repeat_interleave(E)[None, :]
        agree = bool((((feats.double() - want).abs() - (2 * tol + rel * want.abs() + absolute)).max() <= 0).item())
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    res = {"variant": f"{name}/{'forward+backward' if back else 'forward'}", "n": n, "embed_dim": E, "algorithmic_bytes_forward": nbytes,
           "copy_buffer_pairs": len(pairs), "fused_agrees_with_eager": agree}
    for k, ts in times.items():
        res[k] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}
    res["fused_bytes_per_s"] = nbytes / (res["fused"]["ms"] * 1e-3)
    res["fused_fma_per_s"] = n * P.ROW * E * (3 if back else 1) / (res["fused"]["ms"] * 1e-3)
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["fused_over_copy"] = res["fused"]["ms"] / res["copy"]["ms"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="96000,16384")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "embed_bench.txt"))
    args = ap.parse_args()
    sim = make_sim()
    results = []
    for n in args.sizes.split(","):
        for dt, back in VARIANTS:
            results.append(bench_variant(sim, int(n), dt, back, args))
            torch.cuda.empty_cache()
    sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "embed_dim": E, "calls_per_window": args.calls, "rounds": args.rounds}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n")
        for r in results:
            f.write(json.dumps(r) + "\n")
        f.write("\n%-7s %-26s %10s %8s %10s %8s %10s %8s %14s %13s %10s %10s\n" % (
            "n", "variant", "fused ms", "spread", "eager ms", "spread", "copy ms", "spread", "eager / fused", "fused / copy", "fused GB/s", "Gfma/s"))
        for r in results:
            f.write("%-7d %-26s %10.4f %8.4f %10.4f %8.4f %10.4f %8.4f %14.1f %13.2f %10.0f %10.0f\n" % (
                r["n"], r["variant"], r["fused"]["ms"], r["fused"]["spread_ms"], r["eager"]["ms"], r["eager"]["spread_ms"], r["copy"]["ms"],
                r["copy"]["spread_ms"], r["eager_over_fused"], r["fused_over_copy"], r["fused_bytes_per_s"] / 1e9, r["fused_fma_per_s"] / 1e9))
    if not all(r["fused_agrees_with_eager"] for r in results):
        sys.exit("the fused and the eager features differ beyond the derived tolerances")


if __name__ == "__main__":
    main()
