"""Time of the behaviour tracker (behaviour.BehaviourStats.step, csrc/hs_k_behaviour.h) next to the same update written
from torch eager ops on the same device (behaviour.eager_step), and next to a plain device-to-device copy of as many
bytes as the kernel touches; and the wall time per update of tools/train.py --phases with and without --behaviour-stats.

    python tools/behaviour_bench.py [--worlds 16000] [--calls 200] [--rounds 3] [--train-updates 6] [--out profiles/behaviour_stats_bench.txt]

At --worlds x (3+3) agents, on the exports of a simulator stepped into its second episode with random actions (grab and
lock drawn too), so that the worlds are tracked and the table holds finished episodes.  Each variant is timed with device
events around --calls enqueued calls after warm-up; fused, eager and copy alternate inside each of --rounds rounds and the
median window is reported with the spread (max - min) of the windows.  Bytes touched per world of a running episode =
positions, last_pos, the 11 body metadata words, counts, the slot, phase, n_side, travel, grab, agent_steps and per row
self_mask, was_active, done, self_type and grabbing read once, one prep_counter + last_pos, last_locks, travel, grab,
agent_steps and was_active written once: 712 bytes with 6 rows.  The eager state is compared with the fused one once, after
the same calls from the same start.
With --train-updates N > 0, tools/train.py --bf16 --phases runs N + 1 updates four times in child processes, alternating
with and without --behaviour-stats, and the wall time per update of each run is recorded.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402
from gpu_hideseek import behaviour, replay  # noqa: E402

INPUTS = ("positions", "locks", "counts", "prep_counter", "done", "self_type", "self_mask", "grabbing")


def make_sim(n, agents=3):
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=int(gpu_hideseek.SimFlags.RandomFlipTeams), rand_seed=0,
        min_hiders=agents, max_hiders=agents, min_seekers=agents, max_seekers=agents, num_pbt_policies=1)
    sim.init()
    return sim


def exports(sim):
    """The inputs of the explicit form from the exports alone: the locks from the lock columns of box_data / ramp_data of
    each world's lowest active row, the counts from the checkpoint records."""
    W, A = sim.num_worlds, sim.agents_per_world
    rows = W * A
    get = lambda n: getattr(sim, n + "_tensor")().to_torch()          # noqa: E731
    mask = get("self_mask").reshape(W, A)
    first = (mask != 0).to(torch.int32).argmax(1) + torch.arange(W, device=mask.device) * A
    box, ramp = get("box_data").reshape(rows, 9, 17)[first], get("ramp_data").reshape(rows, 2, 14)[first]
    lock = lambda x, c: (x[:, :, c] != 0).to(torch.int32) + 2 * (x[:, :, c + 1] != 0).to(torch.int32)    # noqa: E731
    get("ckpt_ctrl").fill_(1)
    sim.save_checkpoints()
    rec = get("ckpt").reshape(W, replay.CHECKPOINT_BYTES)[:, -16:].contiguous().view(torch.int32)         # numHiders, numSeekers, numBoxes, numRamps
    return dict(positions=get("global_positions").reshape(W, 17, 2), locks=torch.cat([lock(box, 15), lock(ramp, 12)], 1).contiguous(),
                counts=rec[:, [2, 3, 0, 1]].contiguous(), prep_counter=get("prep_counter").reshape(rows), done=get("done").reshape(rows),
                self_type=get("self_type").reshape(rows), self_mask=mask.reshape(rows), grabbing=get("self_data").reshape(rows, 13)[:, 12])


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls      # ms per call


def bench_kernel(args):
    sim = make_sim(args.worlds)
    A, W = sim.agents_per_world, sim.num_worlds
    bh = behaviour.BehaviourStats(sim).arm(from_start=True)
    st_e, table_e = behaviour.new_state(W, A, bh.device), torch.zeros_like(bh.table)      # no world armed: the first eager call starts them as well
    x = exports(sim)
    behaviour.eager_step(st_e, table_e, A, *(x[k] for k in INPUTS), move_eps=bh.move_eps)
    g = torch.Generator(device="cuda").manual_seed(3)
    action = sim.action_tensor().to_torch()
    hi = torch.tensor([5, 5, 5, 2, 2], device="cuda")
    for _ in range(245):                  # through the first episode's end: finished episodes in the table
        action.copy_((torch.rand(action.shape, generator=g, device="cuda") * hi).to(torch.int32).clamp_(max=hi - 1))
        sim.step()
        bh.step()
        x = exports(sim)
        behaviour.eager_step(st_e, table_e, A, *(x[k] for k in INPUTS), move_eps=bh.move_eps)
    torch.cuda.synchronize()
    differ = [k for k in bh.state if not torch.equal(bh.state[k].view(torch.int32), st_e[k].view(torch.int32))]
    exact = [i for i in range(behaviour.STATS) if i not in (3, 4, 12, 13, 21, 24)]        # counts and sums of integers
    same_counts = bool(torch.equal(bh.table[exact], table_e[exact]))
    rel = float(((bh.table - table_e).abs() / bh.table.abs().clamp(min=1e-300)).max())
    nbytes = W * ((360 + 20 * A + 4) + (204 + 4 * A))     # read + written: 484 + 228 with 6 rows
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    x = exports(sim)
    variants = {"fused": bh.step, "eager": lambda: behaviour.eager_step(st_e, table_e, A, *(x[k] for k in INPUTS), move_eps=bh.move_eps),
                "copy": lambda: dst.copy_(src)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    res = {"worlds": W, "rows": W * A, "bytes_touched": nbytes, "eager_state_arrays_that_differ_from_fused": differ, "eager_counts_equal_fused": same_counts,
           "largest_relative_table_difference": rel, "world_episodes_in_table": float(bh.table[0])}
    for k, ts in times.items():
        res[k] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["fused_over_copy"] = res["fused"]["ms"] / res["copy"]["ms"]
    sim.close()
    print(json.dumps(res), flush=True)
    return res


def bench_train(args):
    """[{behaviour_stats, wall ms per update, phases}] of four tools/train.py --phases runs."""
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, tracked in enumerate((True, False, True, False)):
            path = os.path.join(tmp, f"run{i}.txt")
            cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--num-worlds", str(args.worlds), "--num-updates", str(args.train_updates + 1), "--bf16",
                   "--phases", "--out", path] + (["--behaviour-stats"] if tracked else [])
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
            with open(path) as f:
                head = json.loads(f.readline())
            out.append({"behaviour_stats": tracked, "wall_ms_per_update": head["wall_ms_per_update"], "updates": head["updates"],
                        "phases_ms_per_update": head["phases_ms_per_update"]})
            print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=16000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--train-updates", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "behaviour_stats_bench.txt"))
    args = ap.parse_args()
    meta = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "worlds": args.worlds, "agents_per_world": 6, "calls_per_window": args.calls,
            "rounds": args.rounds}
    r = bench_kernel(args)
    runs = bench_train(args) if args.train_updates > 0 else []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n" + json.dumps(r) + "\n")
        for t in runs:
            f.write(json.dumps(t) + "\n")
        f.write("\n%-10s %10s %12s\n" % ("variant", "ms", "spread ms"))
        for k in ("fused", "eager", "copy"):
            f.write("%-10s %10.4f %12.4f\n" % (k, r[k]["ms"], r[k]["spread_ms"]))
        f.write("eager / fused %.1f;  fused / copy of %d bytes %.2f\n" % (r["eager_over_fused"], r["bytes_touched"], r["fused_over_copy"]))
        if runs:
            f.write("\ntools/train.py --bf16 --phases, %d worlds, %d updates after 1 warm-up update, in the order run\n" % (args.worlds, args.train_updates))
            f.write("%-18s %20s %16s\n" % ("--behaviour-stats", "wall ms per update", "sim ms per update"))
            for t in runs:
                f.write("%-18s %20.2f %16.2f\n" % ("yes" if t["behaviour_stats"] else "no", t["wall_ms_per_update"], t["phases_ms_per_update"]["sim"]))
            on = [t["wall_ms_per_update"] for t in runs if t["behaviour_stats"]]
            off = [t["wall_ms_per_update"] for t in runs if not t["behaviour_stats"]]
            f.write("mean with %.2f ms, without %.2f ms: %+.2f ms per update; run-to-run spread with %.2f ms, without %.2f ms; %d tracker calls per update\n" % (
                statistics.mean(on), statistics.mean(off), statistics.mean(on) - statistics.mean(off), max(on) - min(on), max(off) - min(off), 40))


if __name__ == "__main__":
    main()
