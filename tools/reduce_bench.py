"""Two measurements of data-parallel training over shards (trainer.ShardedTrainer, optim.reduce_gradients).

    python tools/reduce_bench.py kernel [--shards 2,4,8] [--calls 20] [--rounds 5] [--out profiles/reduce_bench.txt]
    python tools/reduce_bench.py train [--num-worlds 16000] [--updates 3] [--out profiles/sharded_trainer_bench.txt]

kernel: the time of hs_reduce_gradients (csrc/hs_k_reduce.h) at the policy's flat length (policy.make_policy(): 1 532 992
float32) for 2, 4 and 8 shards on one device, in place into the first source as the trainer calls it, next to what torch
writes for the same sum, torch.stack(srcs).mul(w[:, None]).sum(0), and next to a plain device-to-device copy of as many
bytes as the call moves, (G + 1) * 4 n, cycling through more than 256 MB of buffers so that it runs at the HBM rate and
not out of the last-level cache.  Each variant is timed with device events around --calls enqueued calls after warm-up; the
variants alternate inside each of --rounds rounds and the median window is reported with the spread (max - min) of the
windows, as tools/adam_bench.py does.  Before timing, one call is compared bit for bit with optim.host_reduce.

train: one device, the same session, alternating update by update: trainer.Trainer over one simulator of --num-worlds worlds
(the single-device loop, which this change leaves as it was) and trainer.ShardedTrainer over a ShardedSimulator([0, 0]) of
twice half as many, both bfloat16 with tools/train.py's flags and defaults and with phase events.  On one device nothing
can get faster: what is measured is the overhead of the sharded loop (twice the launches at half the rows, the staging
copies and the reduction).  Scaling over real devices is not measured here.
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
from gpu_hideseek import optim, trainer  # noqa: E402
from gpu_hideseek import policy as P  # noqa: E402
from gpu_hideseek.sharded import ShardedSimulator  # noqa: E402

COPY_SET = 1 << 29        # bytes the copy baseline cycles through: twice the last-level cache


def sim_kw(worlds, flags=0, seed=0):
    return dict(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, num_worlds=worlds, sim_flags=flags, rand_seed=seed, min_hiders=3, max_hiders=3,
                min_seekers=3, max_seekers=3, num_pbt_policies=1)


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
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    return {k: {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts)} for k, ts in times.items()}


def bench_kernel(sim, n, G, args):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    g = torch.Generator(device=dev).manual_seed(G)
    srcs = [torch.randn(n, device=dev, generator=g) for _ in range(G)]
    counts = torch.tensor([float(1000 + 37 * i) for i in range(G)], dtype=torch.float64, device=dev)
    want, _ = optim.host_reduce([x.cpu().numpy() for x in srcs], counts.cpu().numpy())
    got = sim.reduce_gradients(srcs, counts)["out"]
    res = {"shards": G, "flat_length": n, "algorithmic_bytes": (G + 1) * 4 * n,
           "call_is_the_restatement_bit_for_bit": bool((got.cpu().numpy().view("uint32") == want.view("uint32")).all())}
    w = (counts / counts.sum()).float()
    nbytes = res["algorithmic_bytes"]
    pairs = [(torch.empty(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)) for _ in range(max(2, -(-COPY_SET // nbytes)))]
    turn = [0]

    def copy():
        src, dst = pairs[turn[0] % len(pairs)]
        turn[0] += 1
        dst.copy_(src)

    variants = {"call": lambda: sim.reduce_gradients(srcs, counts, out=srcs[0], stream=stream),       # in place, as the trainer calls it
                "torch": lambda: torch.stack(srcs).mul(w[:, None]).sum(0), "copy": copy}
    res.update(measure(variants, args))
    res["call_bytes_per_s"] = nbytes / (res["call"]["ms"] * 1e-3)
    res["call_over_copy"] = res["call"]["ms"] / res["copy"]["ms"]
    res["torch_over_call"] = res["torch"]["ms"] / res["call"]["ms"]
    print(json.dumps(res), flush=True)
    return res


def job_kernel(args):
    sim = gpu_hideseek.HideAndSeekSimulator(gpu_id=0, **sim_kw(64))
    sim.init()
    n = optim.flatten(P.make_policy(fused=False, generator=torch.Generator().manual_seed(1)).named_parameters(), "cpu").params.numel()
    results = [bench_kernel(sim, n, int(G), args) for G in args.shards.split(",")]
    sim.close()
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "calls_per_window": args.calls, "rounds": args.rounds}}) + "\n")
        for r in results:
            f.write(json.dumps(r) + "\n")
        f.write("\n%-7s %11s %10s %8s %10s %8s %10s %8s %13s %12s %10s\n" % ("shards", "flat length", "call ms", "spread", "torch ms", "spread", "copy ms",
                                                                           "spread", "torch / call", "call / copy", "call GB/s"))
        for r in results:
            f.write("%-7d %11d %10.4f %8.4f %10.4f %8.4f %10.4f %8.4f %13.1f %12.2f %10.0f\n" % (
                r["shards"], r["flat_length"], r["call"]["ms"], r["call"]["spread_ms"], r["torch"]["ms"], r["torch"]["spread_ms"], r["copy"]["ms"],
                r["copy"]["spread_ms"], r["torch_over_call"], r["call_over_copy"], r["call_bytes_per_s"] / 1e9))
    if not all(r["call_is_the_restatement_bit_for_bit"] for r in results):
        sys.exit("reduce_gradients differs from host_reduce")


def job_train(args):
    F = gpu_hideseek.SimFlags
    flags = F.RandomFlipTeams | F.UseFixedWorld | F.ZeroAgentVelocity
    cfg = trainer.TrainConfig(dtype=torch.bfloat16)
    plain = gpu_hideseek.HideAndSeekSimulator(gpu_id=0, **sim_kw(args.num_worlds, flags, cfg.seed))
    plain.init()
    ssim = ShardedSimulator([0, 0], **sim_kw(args.num_worlds, flags, cfg.seed))
    ssim.init()
    runs = {"trainer": trainer.Trainer(plain, cfg), "sharded_trainer_0_0": trainer.ShardedTrainer(ssim, cfg)}
    runs["trainer"].phases = trainer.PhaseTimer()
    runs["sharded_trainer_0_0"].phases = trainer.PhaseTimer(trainer.SHARDED_PHASES)
    wall = {k: [] for k in runs}
    spans = {k: {p: 0.0 for p in tr.phases.names} for k, tr in runs.items()}
    for i in range(args.updates + 1):                                  # the first round warms up
        for k, tr in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = tr.update_iter()
            got = tr.phases.totals()
            ms = 1e3 * (time.perf_counter() - t0)
            print(f"  round {i}: {k}: {ms:.1f} ms, loss {m['loss']:.4f}", flush=True)
            if i > 0:
                wall[k].append(ms)
                for p, v in got.items():
                    spans[k][p] += v / args.updates
    med = {k: statistics.median(v) for k, v in wall.items()}
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "num_worlds": args.num_worlds, "updates": args.updates, "wall_ms_windows": wall,
           "wall_ms_median": med, "wall_ms_spread": {k: max(v) - min(v) for k, v in wall.items()}, "phases_ms_per_update": spans,
           "sharded_over_trainer": med["sharded_trainer_0_0"] / med["trainer"]}
    lines = ["%d worlds x (3 + 3) agents, bfloat16, T = 40, K = 8, 2 minibatches x 4 epochs; %d updates each after 1 warm-up update, alternating" % (
        args.num_worlds, args.updates), "%-26s %16s %22s" % ("ms per update", "Trainer", "ShardedTrainer [0, 0]")]
    for p in trainer.SHARDED_PHASES:
        lines.append("%-26s %16s %22.2f" % (p, "%.2f" % spans["trainer"][p] if p in spans["trainer"] else "-", spans["sharded_trainer_0_0"][p]))
    lines.append("%-26s %16.2f %22.2f" % ("wall (median)", med["trainer"], med["sharded_trainer_0_0"]))
    lines.append("%-26s %16.2f %22.2f" % ("wall spread (max - min)", res["wall_ms_spread"]["trainer"], res["wall_ms_spread"]["sharded_trainer_0_0"]))
    lines.append("ShardedTrainer [0, 0] / Trainer: %.3f.  One device: the overhead of the sharded loop, not a speed-up; scaling over several devices is not measured." %
                 res["sharded_over_trainer"])
    print("\n".join(lines))
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n\n" + "\n".join(lines) + "\n")
    plain.close()
    ssim.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("job", choices=("kernel", "train"))
    ap.add_argument("--shards", default="2,4,8")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--num-worlds", type=int, default=16000)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "reduce_bench.txt" if args.job == "kernel" else "sharded_trainer_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    (job_kernel if args.job == "kernel" else job_train)(args)


if __name__ == "__main__":
    main()
