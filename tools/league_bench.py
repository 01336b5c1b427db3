"""Time of the league's step (league.League's hs_league_step, csrc/hs_k_league.h) next to the same update written from
torch eager ops on the same device (stable argsort, bincount), and next to a plain device-to-device copy of as many
bytes as the kernel touches; and the steps per second of league.League.run for 1, 2 and 4 policies next to
evaluate.Evaluator.run on the same worlds.

    python tools/league_bench.py [--worlds 16000] [--calls 200] [--rounds 3] [--run-steps 480] [--out profiles/league_bench.txt]
    python tools/league_bench.py --evaluator-only [--package DIR]      # one JSON line: Evaluator.run alone, from the package in DIR

At --worlds x (3+3) agents and 4 policies, on the exports of a simulator stepped through its first episode end, so that
teams have flipped.  Each variant is timed with device events around --calls enqueued calls after warm-up; fused, eager
and copy alternate inside each of --rounds rounds and the median window is reported with the spread (max - min) of the
windows.  Bytes touched = done, self_type, self_mask read and policy_assignments, slot, row_of_slot, clear_slot written,
once per row, and the two world arrays read.  The eager routing, counts and ratings are compared with the fused ones
once, over the same 245 steps from the same start.
League.run and Evaluator.run: random bfloat16 policies, mode "draw", --run-steps steps timed by the wall clock between two
waits for the device, after 10 steps of warm-up, each on a fresh simulator; the runners alternate inside each of --rounds
rounds and the median is reported with the spread of the runs.  The Evaluator runs the actor and the critic
over all rows; the League runs P actors over R / P rows each, between one routed pack and one routed sampler
(tools/pack_routed_bench.py has the P packs and P gathers it made before, tools/sample_routed_bench.py the logits gather
and the plain sampler, and League.run as it stands now).  --evaluator-only with
--package measures the Evaluator of another checkout (the parent commit's) in a process of its own.
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

K, P_KERNEL, WARM = 3, 4, 10


def make_sim(n, policies=1):
    F = gpu_hideseek.SimFlags
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=int(F.RandomFlipTeams | F.UseFixedWorld | F.ZeroAgentVelocity),
        rand_seed=0, min_hiders=K, max_hiders=K, min_seekers=K, max_seekers=K, num_pbt_policies=policies)
    sim.init()
    return sim


def eager_step(st, counts, elo, P, k, done, self_type, mask, result, hider_team, k_factor):
    """hs_league_step from eager ops, in place on `st`, `counts` and `elo`; returns the routing and bad."""
    W, A = hider_team.shape[0], 2 * k
    R = W * A
    dev = done.device
    hider = self_type.view(W, A) != 0
    malformed = (hider.sum(1) != k) | (mask.view(W, A) == 0).any(1)
    side = torch.where(malformed[:, None], (torch.arange(A, device=dev) < k)[None, :], hider)
    q = torch.arange(W, device=dev) % (P * P)
    i, j = q // P, q % P
    policy = torch.where(side, i[:, None], j[:, None]).reshape(R).to(torch.int32)
    row_of_slot = torch.argsort(policy, stable=True).to(torch.int32)
    slot = torch.empty_like(row_of_slot)
    slot[row_of_slot.long()] = torch.arange(R, dtype=torch.int32, device=dev)
    clear_slot = done[row_of_slot.long()]
    ended = done.view(W, A)[:, 0] != 0
    h = st["world_hider_team"]
    known = (h == 0) | (h == 1)
    x = result.gather(1, h.clamp(0, 1).long().unsqueeze(1))[:, 0]
    o = torch.where(known & (x == 1.0), 0, torch.where(known & (x == 0.0), 1, torch.where(known & (x == 0.5), 2, 3)))
    booked = ended & (st["world_phase"] == 1)
    D = torch.bincount((q * 4 + o)[booked], minlength=P * P * 4).view(P, P, 4)
    counts += D
    latch = ended | (st["world_phase"] == 0)
    st["world_hider_team"].copy_(torch.where(latch, hider_team, h))
    st["world_phase"].copy_(torch.where(latch, torch.ones_like(h), st["world_phase"]))
    n = D[:, :, :3].sum(2).double()
    S = D[:, :, 0].double() + 0.5 * D[:, :, 2].double()
    E = 1.0 / (1.0 + 10.0 ** ((elo[None, :] - elo[:, None]) / 400.0))
    d = torch.where((n > 0) & ~torch.eye(P, dtype=torch.bool, device=dev), k_factor * (S - n * E), torch.zeros_like(E))
    elo += d.sum(1) - d.sum(0)
    return dict(policy_assignments=policy, slot=slot, row_of_slot=row_of_slot, clear_slot=clear_slot, bad=malformed.sum().to(torch.int32).reshape(1))


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
    P, k = P_KERNEL, K
    sim = make_sim(args.worlds)
    A, W = sim.agents_per_world, sim.num_worlds
    rows = W * A
    i32 = dict(dtype=torch.int32, device="cuda")
    out = {n: torch.zeros(rows, **i32) for n in league.ROUTING}
    out["bad"] = torch.zeros(1, **i32)
    st, counts, elo = league.new_state(W, "cuda"), torch.zeros(P, P, 4, dtype=torch.int64, device="cuda"), torch.full((P,), 1500.0, dtype=torch.float64, device="cuda")
    st_e, counts_e, elo_e = league.new_state(W, "cuda"), torch.zeros_like(counts), elo.clone()
    req = league.request(W, A, 0, P, k, st, counts, elo, **out)[1]

    def fused():
        with league.on_current_stream():
            league._run(sim, "hs_league_step", req, None)

    def exports():
        get = lambda n, m: getattr(sim, n + "_tensor")().to_torch().reshape(m, -1)       # noqa: E731
        x = dict(done=get("done", rows)[:, 0], self_type=get("self_type", rows)[:, 0], mask=get("self_mask", rows)[:, 0], result=get("episode_result", W))
        x["hider_team"] = (x["self_type"].view(W, A)[:, 0] == 0).to(torch.int32)
        return x

    def eager():
        return eager_step(st_e, counts_e, elo_e, P, k, x["done"], x["self_type"], x["mask"], x["result"], x["hider_team"], 32.0)
    g = torch.Generator(device="cuda").manual_seed(3)
    action = sim.action_tensor().to_torch()
    hi = torch.tensor([5, 5, 5, 2, 2], device="cuda")
    x = exports()
    fused()
    got = eager()
    same = True
    for _ in range(245):                  # through the first episode's end: flipped teams, games in the table
        action.copy_((torch.rand(action.shape, generator=g, device="cuda") * hi).to(torch.int32).clamp_(max=hi - 1))
        sim.step()
        x = exports()
        fused()
        got = eager()
        same = same and all(torch.equal(out[n], got[n]) for n in out)
    torch.cuda.synchronize()
    same_state = all(torch.equal(st[n], st_e[n]) for n in st)
    same_counts = bool(torch.equal(counts, counts_e))
    elo_diff = float((elo - elo_e).abs().max())
    nbytes = rows * 4 * 7 + W * 4 * 2
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    variants = {"fused": fused, "eager": eager, "copy": lambda: dst.copy_(src)}
    for fn in variants.values():
        for _ in range(3):
            fn()
    times = {n: [] for n in variants}
    for _ in range(args.rounds):
        for n, fn in variants.items():
            times[n].append(window(fn, args.calls))
    res = {"rows": rows, "policies": P, "bytes_touched": nbytes, "eager_routing_equals_fused": bool(same), "eager_state_equals_fused": bool(same_state),
           "eager_counts_equal_fused": same_counts, "max_elo_difference": elo_diff, "games_in_table": int(counts.sum())}
    for n, ts in times.items():
        res[n] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["fused_over_copy"] = res["fused"]["ms"] / res["copy"]["ms"]
    sim.close()
    print(json.dumps(res), flush=True)
    return res


def _policy(seed):
    from gpu_hideseek import policy
    return policy.make_policy(torch.bfloat16, generator=torch.Generator().manual_seed(seed)).cuda()


def _timed(run, steps):
    run(WARM)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def bench_evaluator(args):
    from gpu_hideseek import evaluate
    sim = make_sim(args.worlds)
    ev = evaluate.Evaluator(sim, _policy(1), None, mode="draw", seed=2)
    sps = _timed(ev.run, args.run_steps)
    sim.close()
    return {"runner": "Evaluator.run", "steps_per_s": sps, "worlds": args.worlds, "steps": args.run_steps}


def bench_league(args, P):
    from gpu_hideseek import league
    sim = make_sim(args.worlds, P)
    lg = league.League(sim, [(_policy(1 + p), None) for p in range(P)], K, mode="draw", seed=2)
    sps = _timed(lg.run, args.run_steps)
    sim.close()
    return {"runner": f"League.run P={P}", "steps_per_s": sps, "worlds": args.worlds, "steps": args.run_steps}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=16000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--run-steps", type=int, default=480)
    ap.add_argument("--evaluator-only", action="store_true")
    ap.add_argument("--package", type=str, help="with --evaluator-only: the directory that holds the gpu_hideseek package to measure")
    ap.add_argument("--parent-package", type=str, help="measure Evaluator.run of this other checkout's package as well, in a child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "league_bench.txt"))
    args = ap.parse_args()
    if args.evaluator_only:
        print(json.dumps(bench_evaluator(args)), flush=True)
        return
    meta = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "worlds": args.worlds, "agents_per_world": 2 * K, "calls_per_window": args.calls,
            "rounds": args.rounds}
    r = bench_kernel(args)
    runs = []
    if args.run_steps > 0:
        def parent():
            cmd = [sys.executable, os.path.abspath(__file__), "--evaluator-only", "--package", args.parent_package, "--worlds", str(args.worlds),
                   "--run-steps", str(args.run_steps)]
            line = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
            return dict(json.loads(line), runner="Evaluator.run (parent commit)")
        runners = ([parent] if args.parent_package else []) + [lambda: bench_evaluator(args)] + [lambda P=P: bench_league(args, P) for P in (1, 2, 4)]
        seen = {}
        for _ in range(args.rounds):          # the runners alternate inside every round
            for fn in runners:
                t = fn()
                seen.setdefault(t["runner"], []).append(t["steps_per_s"])
        for name, sps in seen.items():
            runs.append({"runner": name, "steps_per_s": statistics.median(sps), "steps_per_s_runs": sps, "spread": max(sps) - min(sps), "worlds": args.worlds,
                         "steps": args.run_steps})
            print(json.dumps(runs[-1]), flush=True)
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n" + json.dumps(r) + "\n")
        for t in runs:
            f.write(json.dumps(t) + "\n")
        f.write("\nhs_league_step, %d policies, %d rows\n%-10s %10s %12s\n" % (r["policies"], r["rows"], "variant", "ms", "spread ms"))
        for n in ("fused", "eager", "copy"):
            f.write("%-10s %10.4f %12.4f\n" % (n, r[n]["ms"], r[n]["spread_ms"]))
        f.write("eager / fused %.1f;  fused / copy of %d bytes %.2f\n" % (r["eager_over_fused"], r["bytes_touched"], r["fused_over_copy"]))
        if runs:
            base = next(t["steps_per_s"] for t in runs if t["runner"] == "Evaluator.run")
            f.write("\n%d worlds x %d agents, bfloat16, mode draw, %d steps after %d of warm-up, median of %d runs that alternate\n%-32s %12s %10s %18s\n" % (
                args.worlds, 2 * K, args.run_steps, WARM, args.rounds, "runner", "steps / s", "spread", "of Evaluator.run"))
            for t in runs:
                f.write("%-32s %12.2f %10.2f %17.1f%%\n" % (t["runner"], t["steps_per_s"], t["spread"], 100 * t["steps_per_s"] / base))

if __name__ == "__main__":
    main()
