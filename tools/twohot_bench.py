"""Time of the two-hot critic head kernel (sim.value_head, csrc/hs_k_twohot.h) next to the eager composition a torch
learner writes today (value_head.decode for the rollout; value_head.eager_loss and backward() for the update) on the same
device, and next to a plain device-to-device copy of as many bytes as the call moves (cycling through more than 256 MB
of buffers, so that it runs at the HBM rate and not out of the last-level cache).

    python tools/twohot_bench.py [--sizes 1920000,96000] [--calls 20] [--rounds 3] [--out profiles/twohot_bench.txt]

At n = 1 920 000 and n = 96 000 samples, B = 255 bins over [-20, 20]: logits in bf16 and f32, for the decode (value
alone) and for the loss (value, grad_logits and stats under a mask).  Each variant is timed with device events around
--calls enqueued calls after warm-up; fused, eager and copy alternate inside each of --rounds rounds and the median
window is reported with the spread (max - min) of the windows.  Algorithmic bytes = logits read once (+ returns and
mask) + value (+ grad_logits) written once.  Before timing, the fused and the eager results are compared once within
the tolerances tests/test_value_head_host.py derives.
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
from gpu_hideseek import value_head as V  # noqa: E402

B, LO, HI = 255, -20.0, 20.0
COPY_SET = 1 << 29        # bytes the copy baseline cycles through: twice the last-level cache
VARIANTS = [(dt, loss) for dt in (torch.bfloat16, torch.float32) for loss in (False, True)]


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


def bench_variant(sim, n, dtype, loss, args):
    import test_value_head_host as H
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n % 1000)
    returns = torch.randn(n, device=dev, generator=g) * torch.exp(9.0 * torch.rand(n, device=dev, generator=g) - 3.0)
    pos = (V.symlog(returns * (1 + 0.3 * torch.randn(n, device=dev, generator=g))).clamp(LO, HI) - LO) / ((HI - LO) / (B - 1))
    logits = 3.0 * torch.randn(n, B, device=dev, generator=g)
    logits += 12.0 * torch.exp(-0.5 * ((torch.arange(B, device=dev)[None, :] - pos[:, None]) / 1.5) ** 2)
    logits = logits.to(dtype)
    mask = (torch.rand(n, device=dev, generator=g) < 0.8).float() if loss else None
    value = torch.empty(n, dtype=dtype, device=dev)
    grad = torch.empty(n, B, dtype=dtype, device=dev) if loss else None
    stats = torch.empty(V.STATS, dtype=torch.float64, device=dev) if loss else None
    stream = torch.cuda.current_stream()
    leaf = logits.clone().requires_grad_(True)
    bins = V.bins(B, LO, HI, device=dev)

    def fused():                          # enqueue only, like the eager ops: the events see device time
        sim.value_head(logits, returns if loss else None, bins=B, lo=LO, hi=HI, mask=mask, value=value, grad_logits=grad if loss else None,
                       stats=stats if loss else None, stream=stream)

    def eager():
        if loss:
            leaf.grad = None
            V.eager_loss(leaf, returns, mask, B, LO, HI).backward()
        else:
            with torch.no_grad():
                V.symexp(torch.softmax(logits.float(), dim=-1) @ bins)

    esz = logits.element_size()
    nbytes = n * (B * esz + esz + ((B * esz + 8) if loss else 0))
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
    tol = H.tolerances(n)
    name = str(dtype).replace("torch.", "")
    rel, absolute = (2 * r for r in H.ROUNDING[name])                   # both sides round to the narrow type
    with torch.no_grad():
        want = V.decode(logits, B, LO, HI).double()
        on = mask != 0 if loss else torch.ones(n, dtype=torch.bool, device=dev)
        errv = ((value.double() - want).abs() - (2 * tol["y"] * (1 + want.abs()) + rel * want.abs() + absolute))[on].max().item()
        agree = errv <= 0
        if loss:
            ge = leaf.grad.double()
            errg = ((grad.double() - ge).abs() - (rel * ge.abs() + absolute)).max().item()
            agree = agree and errg <= 2 * tol["grad_logits"]
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    res = {"variant": f"{name}/{'loss' if loss else 'decode'}", "n": n, "algorithmic_bytes": nbytes, "copy_buffer_pairs": len(pairs), "fused_agrees_with_eager": bool(agree)}
    for k, ts in times.items():
        res[k] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}
    res["fused_bytes_per_s"] = nbytes / (res["fused"]["ms"] * 1e-3)
    res["fused_expf_per_s"] = n * B / (res["fused"]["ms"] * 1e-3)
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["fused_over_copy"] = res["fused"]["ms"] / res["copy"]["ms"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="1920000,96000")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twohot_bench.txt"))
    args = ap.parse_args()
    sim = make_sim()
    results = []
    for n in args.sizes.split(","):
        for dt, loss in VARIANTS:
            results.append(bench_variant(sim, int(n), dt, loss, args))
            torch.cuda.empty_cache()
    sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "bins": [B, LO, HI], "calls_per_window": args.calls, "rounds": args.rounds}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n")
        for r in results:
            f.write(json.dumps(r) + "\n")
        f.write("\n%-9s %-18s %10s %8s %10s %8s %10s %8s %14s %13s %10s %12s\n" % (
            "n", "variant", "fused ms", "spread", "eager ms", "spread", "copy ms", "spread", "eager / fused", "fused / copy", "fused GB/s", "Gexpf/s"))
        for r in results:
            f.write("%-9d %-18s %10.4f %8.4f %10.4f %8.4f %10.4f %8.4f %14.1f %13.2f %10.0f %12.1f\n" % (
                r["n"], r["variant"], r["fused"]["ms"], r["fused"]["spread_ms"], r["eager"]["ms"], r["eager"]["spread_ms"], r["copy"]["ms"],
                r["copy"]["spread_ms"], r["eager_over_fused"], r["fused_over_copy"], r["fused_bytes_per_s"] / 1e9, r["fused_expf_per_s"] / 1e9))
    if not all(r["fused_agrees_with_eager"] for r in results):
        sys.exit("the fused and the eager results differ beyond the derived tolerances")


if __name__ == "__main__":
    main()
