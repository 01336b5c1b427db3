"""Time of the episode tracker (episodes.EpisodeStats.step, csrc/hs_k_episode.h) next to the same update written from
torch eager ops on the same device, and next to a plain device-to-device copy of as many bytes as the kernel touches;
and the wall time per update of tools/train.py --phases with and without --episode-stats.

    python tools/episode_bench.py [--worlds 16000] [--calls 200] [--rounds 3] [--train-updates 6] [--out profiles/episode_stats_bench.txt]

At --worlds x (3+3) agents, on the exports of a simulator stepped into its second episode, so that the rows are tracked.
The eager update is the contract of include/hideseek.h op for op: the selects of the row update, the ten masked f64 sums
and the four world counters, the restart writes and the worlds' latch.  Each is timed with device events around --calls
enqueued calls after warm-up; fused, eager and copy alternate inside each of --rounds rounds and the median window is
reported with the spread (max - min) of the windows.  Bytes touched = reward, done, self_mask and the six row state
arrays read once + ret, disc, gpow and len written once (a tracked row that does not restart).  The eager state is
compared with the fused one once, after the same calls from the same start: equal bit for bit.
With --train-updates N > 0, tools/train.py --bf16 --phases runs N + 1 updates four times in child processes, alternating
with and without --episode-stats, and the wall time per update of each run is recorded.
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
from gpu_hideseek import episodes  # noqa: E402

GAMMA = 0.998


def make_sim(n, agents=3):
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=int(gpu_hideseek.SimFlags.RandomFlipTeams), rand_seed=0,
        min_hiders=agents, max_hiders=agents, min_seekers=agents, max_seekers=agents, num_pbt_policies=1)
    sim.init()
    return sim


def eager_step(st, table, A, reward, done, self_type, mask, result, hider_team, gamma):
    """hs_episode_stats from eager ops, in place on `st` and `table`."""
    phase = st["phase"]
    was = phase == episodes.TRACKED
    g = torch.tensor(gamma, dtype=torch.float32, device=reward.device)
    R = torch.where(was, reward, torch.zeros_like(reward))
    ret = torch.where(was, st["ret"] + R, st["ret"])
    disc = torch.where(was, st["disc"] + st["gpow"] * R, st["disc"])
    gpow = torch.where(was, st["gpow"] * g, st["gpow"])
    length = torch.where(was, st["len"] + 1, st["len"])
    ended = was & (done != 0)
    hider = st["type"] != 0
    r64 = ret.double()
    terms = torch.stack([torch.ones_like(r64), r64, r64 * r64, disc.double(), length.double()])          # [5, rows]
    sums = [(terms * (ended & (hider == bool(side))).double()).sum(1) for side in (0, 1)]
    restart = (done != 0) | ((phase != episodes.WAITING) & (~was | (mask == 0)))
    worlds = hider_team.shape[0]
    w_end, w_restart = ended.view(worlds, A).any(1), restart.view(worlds, A).any(1)
    h = st["world_hider_team"]
    known = w_end & (st["world_phase"] == 1) & ((h == 0) | (h == 1))
    x = result.gather(1, h.clamp(0, 1).long().unsqueeze(1))[:, 0]
    counters = torch.stack([(known & (x == 1.0)).sum(), (known & (x == 0.0)).sum(), (known & (x == 0.5)).sum(), w_end.sum()]).double()
    table += torch.cat(sums + [counters])
    zero, one = torch.zeros_like(ret), torch.ones_like(ret)
    st["ret"].copy_(torch.where(restart, zero, ret))
    st["disc"].copy_(torch.where(restart, zero, disc))
    st["gpow"].copy_(torch.where(restart, one, gpow))
    st["len"].copy_(torch.where(restart, torch.zeros_like(length), length))
    st["type"].copy_(torch.where(restart, self_type, st["type"]))
    st["phase"].copy_(torch.where(restart, (mask != 0).to(phase.dtype), phase))
    latch = w_end | w_restart
    st["world_hider_team"].copy_(torch.where(latch, hider_team, h))
    st["world_phase"].copy_(torch.where(latch, torch.ones_like(h), st["world_phase"]))


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
    rows = W * A
    ep = episodes.EpisodeStats(sim, gamma=GAMMA).arm(from_start=True)
    st_e, table_e = episodes.new_state(W, A, ep.device), torch.zeros_like(ep.table)      # every row out: the first eager call arms as well

    def exports():
        get = lambda n, k: getattr(sim, n + "_tensor")().to_torch().reshape(k, -1)       # noqa: E731
        x = dict(reward=get("reward", rows)[:, 0], done=get("done", rows)[:, 0], self_type=get("self_type", rows)[:, 0], mask=get("self_mask", rows)[:, 0],
                 result=get("episode_result", W))
        x["hider_team"] = (x["self_type"].view(W, A)[:, 0] == 0).to(torch.int32)
        return x
    x = exports()
    eager_step(st_e, table_e, A, x["reward"], x["done"], x["self_type"], x["mask"], x["result"], x["hider_team"], GAMMA)      # the arming call
    for _ in range(245):                  # through the first episode's end: flipped teams, finished episodes in the table
        sim.step()
        ep.step()
        x = exports()
        eager_step(st_e, table_e, A, x["reward"], x["done"], x["self_type"], x["mask"], x["result"], x["hider_team"], GAMMA)
    torch.cuda.synchronize()
    same = all(torch.equal(ep.state[k].view(torch.int32), st_e[k].view(torch.int32)) for k in ep.state)
    exact = [0, 1, 2, 4, 5, 6, 7, 9, 10, 11, 12, 13]          # counts and sums of integers: the same in any order of addition
    same_counts = bool(torch.equal(ep.table[exact], table_e[exact]))
    nbytes = rows * 4 * (3 + 6 + 4)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    x = exports()
    variants = {"fused": ep.step, "eager": lambda: eager_step(st_e, table_e, A, x["reward"], x["done"], x["self_type"], x["mask"], x["result"], x["hider_team"], GAMMA),
                "copy": lambda: dst.copy_(src)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    res = {"rows": rows, "bytes_touched": nbytes, "eager_state_equals_fused_bit_for_bit": bool(same), "eager_counts_equal_fused": same_counts,
           "episodes_in_table": float(ep.table[0] + ep.table[5])}
    for k, ts in times.items():
        res[k] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["fused_over_copy"] = res["fused"]["ms"] / res["copy"]["ms"]
    sim.close()
    print(json.dumps(res), flush=True)
    return res


def bench_train(args):
    """[(label, wall ms per update, ms per update of the "sim" phase)] of four tools/train.py --phases runs."""
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, tracked in enumerate((True, False, True, False)):
            path = os.path.join(tmp, f"run{i}.txt")
            cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--num-worlds", str(args.worlds), "--num-updates", str(args.train_updates + 1), "--bf16",
                   "--phases", "--out", path] + (["--episode-stats"] if tracked else [])
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
            with open(path) as f:
                head = json.loads(f.readline())
            out.append({"episode_stats": tracked, "wall_ms_per_update": head["wall_ms_per_update"], "updates": head["updates"],
                        "phases_ms_per_update": head["phases_ms_per_update"]})
            print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=16000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--train-updates", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_stats_bench.txt"))
    args = ap.parse_args()
    meta = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "worlds": args.worlds, "agents_per_world": 6, "calls_per_window": args.calls,
            "rounds": args.rounds}
    r = bench_kernel(args)
    runs = bench_train(args) if args.train_updates > 0 else []
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
            f.write("%-16s %20s %16s\n" % ("--episode-stats", "wall ms per update", "sim ms per update"))
            for t in runs:
                f.write("%-16s %20.2f %16.2f\n" % ("yes" if t["episode_stats"] else "no", t["wall_ms_per_update"], t["phases_ms_per_update"]["sim"]))
            on = statistics.mean(t["wall_ms_per_update"] for t in runs if t["episode_stats"])
            off = statistics.mean(t["wall_ms_per_update"] for t in runs if not t["episode_stats"])
            f.write("mean with %.2f ms, without %.2f ms: %+.2f ms per update (%+.3f%%), for %d tracker calls per update\n" % (on, off, on - off, 100 * (on - off) / off, 40))


if __name__ == "__main__":
    main()
