"""What the table-driven league schedule and the pool of past policies cost, on the device.

    python tools/past_pool_bench.py [--worlds 16000] [--calls 5000] [--rounds 5] [--updates 3] [--parent-package DIR] [--out profiles/past_pool_bench.txt]
    python tools/past_pool_bench.py --fixed-only [--package DIR]       # one JSON line: hs_league_step alone, from the package in DIR

1. The step, at --worlds x (3+3) agents on the exports of a simulator stepped to its first episode end, so that after
the first call, which latches the team orders, every call books a game for every world (the most a call can do):
hs_league_step with P = 8 next to hs_league_step_scheduled with the all-pairs table for P = 8 (G = 64) and with
league.past_play_schedule(4, 4) (N = 8, G = 32).  Each variant is timed with device events around --calls
enqueued calls after warm-up; the variants alternate inside each of --rounds rounds, and the median window is reported
with the spread (max - min) of the windows.  With --parent-package (the directory that holds another checkout's
gpu_hideseek package and its built library: the parent commit's) that checkout's hs_league_step is measured as well, in a
child process per round, so that it alternates with the others; its spread is the yardstick for "no slower than the
parent".  The all-pairs table's outputs are compared with hs_league_step's once, bit for bit.
2. Training: population.Population.update_iter() with T = 4 learners and no pool next to T = 4, Q = 4, bfloat16,
steps_per_update = 40, each on a fresh simulator: one warm-up update, then --updates timed by the wall clock between two
waits for the device; the two alternate inside each round.  FPS is world steps per second, as tools/train.py prints it.
With Q = 4 half of the agent rows belong to the pool, which acts but does not learn.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--package" in sys.argv:
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--package") + 1]))
else:
    sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402
from gpu_hideseek import league  # noqa: E402

K, P_STEP, T_POOL, Q_POOL, EPISODE_STEPS = 3, 8, 4, 4, 240        # every world's first episode ends with step 240


def make_sim(n, policies=1):
    F = gpu_hideseek.SimFlags
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=int(F.RandomFlipTeams | F.UseFixedWorld | F.ZeroAgentVelocity),
        rand_seed=0, min_hiders=K, max_hiders=K, min_seekers=K, max_seekers=K, num_pbt_policies=policies)
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


def stepped_sim(worlds):
    """A simulator driven with random actions to its first episode end: the exports carry done for every world."""
    sim = make_sim(worlds)
    g = torch.Generator(device="cuda").manual_seed(3)
    action = sim.action_tensor().to_torch()
    hi = torch.tensor([5, 5, 5, 2, 2], device="cuda")
    for _ in range(EPISODE_STEPS):
        action.copy_((torch.rand(action.shape, generator=g, device="cuda") * hi).to(torch.int32).clamp_(max=hi - 1))
        sim.step()
    return sim


class StepVariant:
    """One form of the league step on `sim`'s exports, with buffers of its own."""

    def __init__(self, sim, N, fn, pairs=None):
        W, A = sim.num_worlds, sim.agents_per_world
        i32 = dict(dtype=torch.int32, device="cuda")
        self.sim, self.fn, self.pairs, self.N = sim, fn, pairs, N
        self.out = {n: torch.zeros(W * A, **i32) for n in league.ROUTING}
        self.out["bad"] = torch.zeros(1, **i32)
        self.state, self.counts = league.new_state(W, "cuda"), torch.zeros(N, N, 4, dtype=torch.int64, device="cuda")
        self.elo = torch.full((N,), 1500.0, dtype=torch.float64, device="cuda")
        kw = {} if pairs is None else {"group": len(pairs)}
        self.req = league.request(W, A, 0, N, K, self.state, self.counts, self.elo, **self.out, **kw)[1]

    def arm(self):
        if self.pairs is not None:
            self.sim.set_league_schedule(self.pairs, self.N)

    def __call__(self):
        with league.on_current_stream():
            league._run(self.sim, self.fn, self.req, None)


def bench_fixed(args):
    """hs_league_step with P = 8 alone: --rounds windows (what a child process of another checkout runs)."""
    sim = stepped_sim(args.worlds)
    v = StepVariant(sim, P_STEP, "hs_league_step")
    for _ in range(3):
        v()
    ts = [window(v, args.calls) for _ in range(args.rounds)]
    sim.close()
    return {"variant": "hs_league_step P=8", "ms_windows": ts, "games_in_table": int(v.counts.sum())}


def bench_step(args):
    sim = stepped_sim(args.worlds)
    variants = {"hs_league_step P=8": StepVariant(sim, P_STEP, "hs_league_step"),
                "scheduled, all-pairs table P=8": StepVariant(sim, P_STEP, "hs_league_step_scheduled", league.all_pairs_schedule(P_STEP)),
                "scheduled, past_play_schedule(4, 4)": StepVariant(sim, T_POOL + Q_POOL, "hs_league_step_scheduled", league.past_play_schedule(T_POOL, Q_POOL))}
    for v in variants.values():
        v.arm()
        for _ in range(3):
            v()
    a, b = variants["hs_league_step P=8"], variants["scheduled, all-pairs table P=8"]
    torch.cuda.synchronize()
    same = all(torch.equal(a.out[n], b.out[n]) for n in a.out) and torch.equal(a.counts, b.counts) and torch.equal(a.elo.view(torch.int64), b.elo.view(torch.int64))
    times = {n: [] for n in variants}
    parent = []

    def parent_windows():
        cmd = [sys.executable, os.path.abspath(__file__), "--fixed-only", "--package", args.parent_package, "--worlds", str(args.worlds), "--calls", str(args.calls),
               "--rounds", "3"]
        line = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
        return json.loads(line)["ms_windows"]
    for _ in range(args.rounds):
        if args.parent_package:
            parent += parent_windows()
        for n, v in variants.items():
            v.arm()
            times[n].append(window(v, args.calls))
    rows = sim.num_worlds * sim.agents_per_world
    res = {"rows": rows, "calls_per_window": args.calls, "all_pairs_table_equals_fixed": bool(same), "games_in_table": int(a.counts.sum()), "variants": {}}
    if parent:
        times = dict({"hs_league_step P=8 (parent commit)": parent}, **times)
    for n, ts in times.items():
        res["variants"][n] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts)}
    sim.close()
    print(json.dumps(res), flush=True)
    return res


def bench_population(args, Q):
    from gpu_hideseek import population
    sim = make_sim(args.worlds, T_POOL + Q)
    cfg = population.PopulationConfig(num_policies=T_POOL, team_size=K, steps_per_update=40, dtype=torch.bfloat16, num_past_policies=Q)
    pop = population.Population(sim, cfg)
    pop.update_iter()                      # warms up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.updates):
        out = pop.update_iter()
    torch.cuda.synchronize()
    s = (time.perf_counter() - t0) / args.updates
    sim.close()
    return {"runner": f"Population T={T_POOL} Q={Q}", "s_per_update": s, "fps_world_steps": args.worlds * cfg.steps_per_update / s, "games": out["games"], "bad": out["bad"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=16000)
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates", type=int, default=3, help="timed updates per run of a population; 0: the step alone")
    ap.add_argument("--fixed-only", action="store_true")
    ap.add_argument("--package", type=str, help="with --fixed-only: the directory that holds the gpu_hideseek package to measure")
    ap.add_argument("--parent-package", type=str, help="measure hs_league_step of this other checkout's package as well, in child processes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "past_pool_bench.txt"))
    args = ap.parse_args()
    if args.fixed_only:
        print(json.dumps(bench_fixed(args)), flush=True)
        return
    meta = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "worlds": args.worlds, "agents_per_world": 2 * K, "rounds": args.rounds}
    r = bench_step(args)
    runs = {}
    if args.updates > 0:
        for _ in range(args.rounds):          # the two alternate inside every round
            for Q in (0, Q_POOL):
                t = bench_population(args, Q)
                print(json.dumps(t), flush=True)
                runs.setdefault(t["runner"], []).append(t)
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n" + json.dumps(r) + "\n")
        for ts in runs.values():
            for t in ts:
                f.write(json.dumps(t) + "\n")
        f.write("\nthe league step, %d rows, %d calls per window, median of the windows (max - min)\n%-40s %10s %12s %8s\n" % (
            r["rows"], r["calls_per_window"], "variant", "ms", "spread ms", "windows"))
        for n, v in r["variants"].items():
            f.write("%-40s %10.4f %12.4f %8d\n" % (n, v["ms"], v["spread_ms"], len(v["ms_windows"])))
        f.write("the all-pairs table's outputs equal hs_league_step's bit for bit: %s\n" % r["all_pairs_table_equals_fixed"])
        base = r["variants"].get("hs_league_step P=8 (parent commit)")
        if base:
            d = r["variants"]["scheduled, all-pairs table P=8"]["ms"] - base["ms"]
            f.write("scheduled all-pairs - parent's hs_league_step: %+.4f ms; the parent's own spread: %.4f ms; slower by more than that: %s\n" % (
                d, base["spread_ms"], d > base["spread_ms"]))
        if runs:
            f.write("\n%d worlds x %d agents, bfloat16, steps_per_update 40, %d updates after 1 warm-up, median of %d runs that alternate\n%-28s %14s %14s %18s\n" % (
                args.worlds, 2 * K, args.updates, args.rounds, "runner", "s per update", "FPS", "FPS spread"))
            for n, ts in runs.items():
                fps = [t["fps_world_steps"] for t in ts]
                f.write("%-28s %14.3f %14.0f %18.0f\n" % (n, statistics.median(t["s_per_update"] for t in ts), statistics.median(fps), max(fps) - min(fps)))


if __name__ == "__main__":
    main()
