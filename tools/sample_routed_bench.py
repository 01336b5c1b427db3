"""Time of the routed sampler (sim.sample_actions_routed, hs_sample_actions_routed, csrc/hs_k_sample_routed.h) next to the
path it replaces and next to a plain device-to-device copy; the steps per second of league.League.run for 1, 2 and 4
policies; and, with --population, the FPS of the population trainer for P = 1, 2 and 4 next to the plain Trainer.

    python tools/sample_routed_bench.py [--worlds 16000] [--calls 200] [--rounds 3] [--run-steps 480] [--out profiles/sample_routed_bench.txt]
    python tools/sample_routed_bench.py --population [--worlds 16000] [--updates 2] [--out profiles/population_bench.txt]

The shape is tools/pack_routed_bench.py's: --worlds x (3+3) agents, 4 policies, bfloat16 logits in slot order (19 in rows of 20), routed by
hs_league_step on a simulator stepped 12 times with random actions.  Two forms are timed.  "league": the actions alone
into the action export, against a gather of the logits back to rows + sample_actions (what League.act did).  "learner":
the action export, action[t] and log_prob[t] in slot order, against the logits gather + sample_actions + a gather each of
the action and the log_prob to slots (what a population's collect() would do without it).  Each variant is timed with device
events around --calls enqueued calls after warm-up; the variants alternate inside each of --rounds rounds and the median
window is reported with the spread (max - min) of the windows.  The outputs of the two ways are compared bit for bit once.
League.run: random bfloat16 policies, mode "draw", --run-steps steps timed by the wall clock between two waits for the
device after 10 steps of warm-up, each on a fresh simulator.
--population: tools/train.py's configuration (bfloat16, T = 40, K = 8, 2 minibatches x 4 epochs) through
population.Population for P = 1, 2, 4 and through trainer.Trainer, --updates updates after one warm-up update each; FPS is
world steps per second as tools/train.py prints it.
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

K, N_KERNEL, WARM, L = 3, 4, 10, 20          # 19 logits in rows of 20 bfloat16: a gathered row is a multiple of 4 bytes


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


def bench_kernel(args):
    from gpu_hideseek import league
    from gpu_hideseek._request import on_current_stream
    N = N_KERNEL
    sim = make_sim(args.worlds, N)
    R = sim.num_worlds * sim.agents_per_world
    g = torch.Generator(device="cuda").manual_seed(3)
    export = sim.action_tensor().to_torch()
    hi = torch.tensor([5, 5, 5, 2, 2], device="cuda")
    for _ in range(12):
        export.copy_((torch.rand(export.shape, generator=g, device="cuda") * hi).to(torch.int32).clamp_(max=hi - 1))
        sim.step()
    ros, slot = (torch.zeros(R, dtype=torch.int32, device="cuda") for _ in range(2))
    sim.league_step(N, K, league.new_state(sim.num_worlds, "cuda"), torch.zeros(N, N, 4, dtype=torch.int64, device="cuda"),
                    torch.full((N,), 1500.0, dtype=torch.float64, device="cuda"), row_of_slot=ros, slot=slot)
    bf, i32 = torch.bfloat16, torch.int32
    by_slot = (3.0 * torch.randn(1, R, L, generator=g, device="cuda")).to(bf)
    by_row = torch.zeros(1, R, L, dtype=bf, device="cuda")
    act_r, act_g = (torch.zeros(R, 5, dtype=i32, device="cuda") for _ in range(2))
    lp_r, lp_g, lp_rows = (torch.zeros(R, device="cuda") for _ in range(3))
    act_rows_g = torch.zeros(R, 5, dtype=i32, device="cuda")
    seed = (5, 0)

    def league_routed():
        with on_current_stream():
            sim.sample_actions_routed(by_slot[0], ros, seed=seed, counter=7)

    def league_gathered():
        with on_current_stream():
            sim.gather_sequences(slot, [(by_slot, by_row, False)], chunks=1, chunk_steps=1, rows=R)
            sim.sample_actions(by_row[0], seed=seed, counter=7)

    def learner_routed():
        with on_current_stream():
            sim.sample_actions_routed(by_slot[0], ros, seed=seed, counter=7, action=act_r, log_prob=lp_r)

    def learner_gathered():
        with on_current_stream():
            sim.gather_sequences(slot, [(by_slot, by_row, False)], chunks=1, chunk_steps=1, rows=R)
            sim.sample_actions(by_row[0], seed=seed, counter=7, action=act_rows_g, log_prob=lp_rows)
            sim.gather_sequences(ros, [(act_rows_g.view(1, R, 5), act_g.view(1, R, 5), False)], chunks=1, chunk_steps=1, rows=R)
            sim.gather_sequences(ros, [(lp_rows.view(1, R, 1), lp_g.view(1, R, 1), False)], chunks=1, chunk_steps=1, rows=R)

    nbytes = R * L * 2 + R * 4 + R * 5 * 4 * 2 + R * 4          # what the learner's form reads and writes
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    variants = {"league_routed": league_routed, "league_gathered": league_gathered, "learner_routed": learner_routed, "learner_gathered": learner_gathered,
                "copy": lambda: dst.copy_(src)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    learner_gathered()
    rows_gathered = act_rows_g.clone()
    learner_routed()
    torch.cuda.synchronize()
    same = bool(torch.equal(act_r, act_g)) and bool(torch.equal(lp_r.view(i32), lp_g.view(i32))) and bool(torch.equal(export.reshape(R, 5), rows_gathered))
    times = {n: [] for n in variants}
    for _ in range(args.rounds):
        for n, fn in variants.items():
            times[n].append(window(fn, args.calls))
    res = {"rows": R, "policies": N, "dtype": "bfloat16", "bytes_moved_learner": nbytes, "routed_equals_gathered": same}
    for n, ts in times.items():
        res[n] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}
    res["league_gathered_over_routed"] = res["league_gathered"]["ms"] / res["league_routed"]["ms"]
    res["learner_gathered_over_routed"] = res["learner_gathered"]["ms"] / res["learner_routed"]["ms"]
    res["learner_routed_over_copy"] = res["learner_routed"]["ms"] / res["copy"]["ms"]
    sim.close()
    return res


def _policy(seed):
    from gpu_hideseek import policy
    return policy.make_policy(torch.bfloat16, generator=torch.Generator().manual_seed(seed)).cuda()


def bench_league(args, P):
    from gpu_hideseek import league
    sim = make_sim(args.worlds, P)
    lg = league.League(sim, [(_policy(1 + p), None) for p in range(P)], K, mode="draw", seed=2)
    lg.run(WARM)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lg.run(args.run_steps)
    torch.cuda.synchronize()
    sps = args.run_steps / (time.perf_counter() - t0)
    sim.close()
    return sps


def bench_population(args, P):
    """World steps per second over --updates updates after one warm-up update; P = 0 is the plain Trainer."""
    from gpu_hideseek import population, trainer
    sim = make_sim(args.worlds, max(1, P))
    if P:
        tr = population.Population(sim, population.PopulationConfig(dtype=torch.bfloat16, num_policies=P, team_size=K))
    else:
        tr = trainer.Trainer(sim, trainer.TrainConfig(dtype=torch.bfloat16))
    tr.update_iter()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.updates):
        out = tr.update_iter()
    wall = time.perf_counter() - t0
    sim.close()
    res = {"runner": f"Population P={P}" if P else "Trainer", "worlds": args.worlds, "updates": args.updates, "s_per_update": wall / args.updates,
           "fps_world_steps": args.worlds * tr.cfg.steps_per_update * args.updates / wall}
    if P:
        res.update(games=out["games"], bad=out["bad"], elo=out["elo"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=16000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--run-steps", type=int, default=480)
    ap.add_argument("--population", action="store_true")
    ap.add_argument("--updates", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_routed_bench needs a GPU")
    out = args.out or os.path.join(ROOT, "profiles", "population_bench.txt" if args.population else "sample_routed_bench.txt")
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "worlds": args.worlds, "agents": 2 * K})]

    def add(res):
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if args.population:
        for P in (0, 1, 2, 4):
            add(bench_population(args, P))
    else:
        add(bench_kernel(args))
        for P in (1, 2, 4):
            runs = [bench_league(args, P) for _ in range(args.rounds)]
            add({"runner": f"League.run P={P}", "worlds": args.worlds, "steps": args.run_steps, "steps_per_s": statistics.median(runs), "runs": runs,
                 "spread": max(runs) - min(runs)})
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
