"""Time of a minibatch gather (rollout.Rollout.minibatch: hs_gather_sequences, csrc/hs_k_gather.h — every field of the
rollout in one launch) next to the same result by torch indexing (Rollout.minibatch_eager: an index expansion and a
launch or more per field) and next to a plain device-to-device copy of as many bytes as the minibatch holds.

    python tools/gather_bench.py [--steps 40] [--chunks 8] [--rows 96000] [--calls 20] [--out profiles/gather_bench.txt]

At the training shape: T = 40 steps in K = 8 chunks over n = 96 000 agent rows (16 000 worlds x 6 agents), bfloat16,
m = K n / 2 sequences of a fresh device-side permutation per call.  The variants alternate; every call of every variant is
timed with device events of its own (a call runs for milliseconds) after two warm-up calls each, and the median of the
--calls calls is reported with their spread (max - min).  The fused call writes into kept tensors (out=); the eager one
allocates its results, as torch indexing does.  The copy moves one contiguous buffer of the minibatch's size into another.
Bytes of a minibatch = the rows it holds, read once and written once.  Before timing, the fused result is compared with
the eager one byte for byte.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402
from gpu_hideseek import rollout  # noqa: E402


def make_sim():
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=64, sim_flags=0, rand_seed=0, min_hiders=3,
        max_hiders=3, min_seekers=3, max_seekers=3, num_pbt_policies=1)
    sim.init()
    return sim


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--rows", type=int, default=96000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_bench.txt"))
    args = ap.parse_args()
    if args.calls < 20:
        sys.exit("--calls must be at least 20")
    sim = make_sim()
    dev = torch.device("cuda", 0)
    buf = rollout.Rollout(sim, args.steps, args.chunks, torch.bfloat16, rows=args.rows)
    g = torch.Generator(device=dev).manual_seed(0)
    for t in buf.tensors().values():                       # bytes worth comparing: every field its own values
        if t.dtype == torch.int32:
            t.copy_(torch.randint(0, 2 ** 31 - 1, t.shape, device=dev, generator=g, dtype=torch.int32))
        else:
            t.copy_(torch.randn(t.shape, device=dev, generator=g, dtype=torch.float32))
    m = buf.sequences // 2
    stream = torch.cuda.current_stream()
    perm = lambda: torch.randperm(buf.sequences, device=dev, generator=g, dtype=torch.int32)[:m]      # noqa: E731
    index = perm()
    out = buf.minibatch(index)
    want = buf.minibatch_eager(index)
    same = all(torch.equal(out[k].view(-1).view(torch.uint8), want[k].contiguous().view(-1).view(torch.uint8)) for k in out)
    nbytes = sum(t.numel() * t.element_size() for t in out.values())
    del want
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    src.random_(0, 255)
    state = {"index": index}
    variants = {"fused": lambda: buf.minibatch(state["index"], out=out, stream=stream),
                "eager": lambda: buf.minibatch_eager(state["index"]),
                "copy": lambda: dst.copy_(src)}
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.calls):
        state["index"] = perm()
        torch.cuda.synchronize()
        for k, fn in variants.items():
            times[k].append(timed(fn))
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "steps": args.steps, "chunks": args.chunks, "rows": args.rows,
           "dtype": "bfloat16", "m": m, "fields": len(out), "minibatch_bytes": nbytes, "rollout_bytes": sum(t.numel() * t.element_size() for t in buf.tensors().values()),
           "fused_is_the_eager_result_byte_for_byte": same, "calls": args.calls}
    for k, ts in times.items():
        res[k] = {"ms": statistics.median(ts), "spread_ms": max(ts) - min(ts), "ms_calls": ts}
        res[k + "_bytes_per_s"] = 2 * nbytes / (res[k]["ms"] * 1e-3)                   # read once and written once
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["fused_no_slower_than_eager"] = res["fused"]["ms"] <= res["eager"]["ms"]
    res["fused_share_of_the_copy_rate"] = res["copy"]["ms"] / res["fused"]["ms"]
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n\n")
        f.write("T = %d, K = %d, n = %d, bfloat16, m = %d sequences, %d fields, %.3f GB per minibatch (read once, written once)\n" % (
            args.steps, args.chunks, args.rows, m, len(out), nbytes / 1e9))
        f.write("%-8s %10s %10s %12s\n" % ("variant", "median ms", "spread ms", "GB/s moved"))
        for k in variants:
            f.write("%-8s %10.3f %10.3f %12.0f\n" % (k, res[k]["ms"], res[k]["spread_ms"], res[k + "_bytes_per_s"] / 1e9))
        f.write("eager / fused = %.2f; the fused gather runs at %.0f %% of the plain copy's rate\n" % (res["eager_over_fused"], 100 * res["fused_share_of_the_copy_rate"]))
    sim.close()
    if not same:
        sys.exit("Rollout.minibatch differs from minibatch_eager")


if __name__ == "__main__":
    main()
