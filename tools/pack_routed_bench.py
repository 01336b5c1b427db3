"""Time of the routed pack (sim.pack_policy_inputs_routed, hs_pack_policy_inputs_routed, csrc/hs_k_pack_routed.h) next to
what League.act() did before it existed, N x (pack_policy_inputs of all rows + a gather of the policy's block), and next
to a plain device-to-device copy of as many bytes as the routed pack writes; and the steps per second of
league.League.run for 1, 2 and 4 policies on the routed pack and on the path of the parent commit (a pack and a gather
per policy, which League keeps for policies of several dtypes: `routed = False` selects it).

    python tools/pack_routed_bench.py [--worlds 16000] [--calls 200] [--rounds 3] [--run-steps 480] [--out profiles/pack_routed_bench.txt]

The shape is tools/league_bench.py's: --worlds x (3+3) agents, 4 policies, bfloat16 actor rows, on the exports of a
simulator stepped 12 times with random actions and routed by hs_league_step, each policy with a table of its own.  Each
variant is timed with device events around --calls enqueued calls after warm-up; the variants alternate inside each of
--rounds rounds and the median window is reported with the spread (max - min) of the windows.  The rows of the two ways
are compared bit for bit once.  "with moments" is the population's call: actor and critic rows and the moments of every
policy in one launch (plus N sums), against N x (pack with moments + two gathers).
League.run: random bfloat16 policies, mode "draw", --run-steps steps timed by the wall clock between two waits for the
device after 10 steps of warm-up, each on a fresh simulator; the two paths alternate inside each round.
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

K, N_KERNEL, WARM, ROW = 3, 4, 10, 296


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
    m = R // N
    g = torch.Generator(device="cuda").manual_seed(3)
    action = sim.action_tensor().to_torch()
    hi = torch.tensor([5, 5, 5, 2, 2], device="cuda")
    for _ in range(12):
        action.copy_((torch.rand(action.shape, generator=g, device="cuda") * hi).to(torch.int32).clamp_(max=hi - 1))
        sim.step()
    ros = torch.zeros(R, dtype=torch.int32, device="cuda")
    sim.league_step(N, K, league.new_state(sim.num_worlds, "cuda"), torch.zeros(N, N, 4, dtype=torch.int64, device="cuda"),
                    torch.full((N,), 1500.0, dtype=torch.float64, device="cuda"), row_of_slot=ros)
    tables = torch.empty(N, 592, device="cuda")
    tables[:, :ROW] = torch.randn(N, ROW, generator=g, device="cuda")
    tables[:, ROW:] = torch.rand(N, ROW, generator=g, device="cuda") + 0.5
    bf = torch.bfloat16
    routed_a, routed_c = torch.zeros(R, ROW, dtype=bf, device="cuda"), torch.zeros(R, ROW, dtype=bf, device="cuda")
    packed_a, packed_c = torch.zeros(R, ROW, dtype=bf, device="cuda"), torch.zeros(R, ROW, dtype=bf, device="cuda")
    mine_a, mine_c = torch.zeros(N, 1, m, ROW, dtype=bf, device="cuda"), torch.zeros(N, 1, m, ROW, dtype=bf, device="cuda")
    mom_r, mom_p = torch.zeros(N, 593, dtype=torch.float64, device="cuda"), torch.zeros(N, 593, dtype=torch.float64, device="cuda")

    def routed():
        with on_current_stream():
            sim.pack_policy_inputs_routed(ros, N, actor=routed_a, tables=tables)

    def per_policy():
        with on_current_stream():
            for p in range(N):
                sim.pack_policy_inputs(actor=packed_a, normaliser=tables[p])
                sim.gather_sequences(ros[p * m:(p + 1) * m], [(packed_a.view(1, R, -1), mine_a[p], False)], chunks=1, chunk_steps=1, rows=R)

    def routed_moments():
        with on_current_stream():
            sim.pack_policy_inputs_routed(ros, N, actor=routed_a, critic=routed_c, moments=mom_r, tables=tables)

    def per_policy_moments():
        with on_current_stream():
            for p in range(N):
                sim.pack_policy_inputs(actor=packed_a, critic=packed_c, moments=mom_p[p], normaliser=tables[p])
                sim.gather_sequences(ros[p * m:(p + 1) * m], [(packed_a.view(1, R, -1), mine_a[p], False), (packed_c.view(1, R, -1), mine_c[p], False)],
                                     chunks=1, chunk_steps=1, rows=R)

    src = torch.empty(R * ROW * 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    variants = {"routed": routed, "per_policy": per_policy, "copy": lambda: dst.copy_(src), "routed_moments": routed_moments,
                "per_policy_moments": per_policy_moments}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(routed_a.view(torch.int16), mine_a.view(R, ROW).view(torch.int16))) and \
        bool(torch.equal(routed_c.view(torch.int16), mine_c.view(R, ROW).view(torch.int16)))
    times = {n: [] for n in variants}
    for _ in range(args.rounds):
        for n, fn in variants.items():
            times[n].append(window(fn, args.calls))
    res = {"rows": R, "policies": N, "dtype": "bfloat16", "bytes_written_actor": R * ROW * 2, "routed_rows_equal_per_policy_rows": same}
    for n, ts in times.items():
        res[n] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}
    res["per_policy_over_routed"] = res["per_policy"]["ms"] / res["routed"]["ms"]
    res["routed_over_copy"] = res["routed"]["ms"] / res["copy"]["ms"]
    res["per_policy_moments_over_routed_moments"] = res["per_policy_moments"]["ms"] / res["routed_moments"]["ms"]
    sim.close()
    print(json.dumps(res), flush=True)
    return res


def _policy(seed):
    from gpu_hideseek import policy
    return policy.make_policy(torch.bfloat16, generator=torch.Generator().manual_seed(seed)).cuda()


def bench_league(args, P, routed):
    from gpu_hideseek import league
    sim = make_sim(args.worlds, P)
    lg = league.League(sim, [(_policy(1 + p), None) for p in range(P)], K, mode="draw", seed=2)
    if not routed:                       # the parent commit's act(): a pack and a gather per policy
        lg.routed = False
        lg.gathered = {torch.bfloat16: torch.zeros(1, lg.block, ROW, dtype=torch.bfloat16, device="cuda")}
    lg.run(WARM)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lg.run(args.run_steps)
    torch.cuda.synchronize()
    sps = args.run_steps / (time.perf_counter() - t0)
    sim.close()
    return sps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=16000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--run-steps", type=int, default=480)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_routed_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pack_routed_bench needs a GPU")
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "worlds": args.worlds, "agents": 2 * K})]
    lines.append(json.dumps(bench_kernel(args)))
    for P in (1, 2, 4):
        runs = {"routed": [], "per_policy": []}
        for _ in range(args.rounds):
            for name in runs:
                runs[name].append(bench_league(args, P, name == "routed"))
        res = {"runner": f"League.run P={P}", "worlds": args.worlds, "steps": args.run_steps}
        for name, v in runs.items():
            res[name] = {"steps_per_s": statistics.median(v), "runs": v, "spread": max(v) - min(v)}
        res["routed_over_per_policy"] = res["routed"]["steps_per_s"] / res["per_policy"]["steps_per_s"]
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
