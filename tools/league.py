"""Let several trained policies play each other and rate them: gpu_hideseek.league behind the arguments of the
reference's scripts/jax_infer.py with more than one policy (eval_competitive, print_elos).

    python tools/league.py --num-worlds 1024 --num-steps 2400 --ckpt-path ckpts/run0/100 ckpts/run0/200 ckpts/run1/200 --bf16

Every --ckpt-path is a file tools/train.py saved (evaluate.load_policy: its "params" and "normaliser").  Of a population's
checkpoint (tools/train.py --pbt-ensemble-size) --member i takes that policy and --all-members every one.  With P policies the
number of worlds must be a multiple of P^2: world w plays pair w mod P^2, policy q // P as the hiders against policy
q % P as the seekers, for the whole run.  The simulator runs with num_pbt_policies = P and UseFixedWorld |
ZeroAgentVelocity, as the reference's script does; --num-hiders is the size of both teams.
It prints the Elo table before and after (four to a line, as the reference's print_elos does), the P x P matrix of the
hiders' win rate (row: the hiders' policy, column: the seekers'), and one JSON line of League.read().
--behaviour-stats also tracks what the agents do with the level, over all policies together (gpu_hideseek.behaviour), and
prints it as a JSON line before that one.
Training several policies at once is tools/train.py --pbt-ensemble-size.  Not here: drawn or rating-based matchmaking,
several GPUs.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402
from gpu_hideseek import behaviour, evaluate, league, policy  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--num-worlds", type=int, required=True)
    ap.add_argument("--num-steps", type=int, default=2400)
    ap.add_argument("--ckpt-path", type=str, nargs="+", required=True)
    ap.add_argument("--member", type=int, help="of every population checkpoint given, this policy")
    ap.add_argument("--all-members", action="store_true", help="of every population checkpoint given, all its policies")
    ap.add_argument("--record-log", type=str)
    ap.add_argument("--num-hiders", type=int, default=3, help="the size of both teams")
    ap.add_argument("--fp16", action="store_true")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--gpu-id", type=int, default=0)
    ap.add_argument("--greedy", action="store_true", help="every head's most likely action instead of a draw")
    ap.add_argument("--k-factor", type=float, default=league.DEFAULT_K_FACTOR)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--behaviour-stats", action="store_true", help="track object movement, locks, travel and grabs on the device and print them")
    ap.add_argument("--encoder", choices=policy.ENCODERS, help="every policy's network (tools/train.py --encoder); by default read from each checkpoint")
    args = ap.parse_args(argv)
    if args.fp16 and args.bf16:
        ap.error("--fp16 and --bf16 exclude each other")
    if args.member is not None and args.all_members:
        ap.error("--member and --all-members exclude each other")
    P = len(args.ckpt_path)
    if not args.all_members and (P > league.MAX_POLICIES or args.num_worlds % (P * P)):       # with --all-members: once the files are read
        ap.error(f"--num-worlds must be a multiple of {P * P} for {P} policies (at most {league.MAX_POLICIES})")
    return args


def load_policies(args, dtype, dev):
    """[(net, normaliser)] of every --ckpt-path in order, a population checkpoint giving --member or, with --all-members,
    all its members."""
    policies = []
    for path in args.ckpt_path:
        d = torch.load(path, map_location=dev, weights_only=False)
        states = evaluate.members(d)
        if "members" in d and not args.all_members:
            if args.member is None or not 0 <= args.member < len(states):
                raise SystemExit(f"{path} is a population checkpoint of {len(states)} members: give --member i or --all-members")
            states = [states[args.member]]
        policies += [evaluate.load_policy(st, dtype, dev, encoder=args.encoder) for st in states]
    P = len(policies)
    if P > league.MAX_POLICIES or args.num_worlds % (P * P):
        raise SystemExit(f"--num-worlds must be a multiple of {P * P} for {P} policies (at most {league.MAX_POLICIES})")
    return policies


def matrix(counts):
    """The lines of the hiders' win-rate matrix."""
    rates = league.hider_win_rates(counts)
    P = len(rates)
    lines = ["hider win rate (row: hiders, column: seekers)", "      " + "".join(f"{j:>8}" for j in range(P))]
    for i, row in enumerate(rates):
        lines.append(f"{i:>4}: " + "".join(f"{100 * r:>7.1f}%" for r in row))
    return lines


def main(argv=None):
    args = parse(argv)
    F = gpu_hideseek.SimFlags
    dtype = torch.float16 if args.fp16 else torch.bfloat16 if args.bf16 else torch.float32
    dev = torch.device("cuda", args.gpu_id)
    policies = load_policies(args, dtype, dev)
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=args.gpu_id, num_worlds=args.num_worlds,
        sim_flags=F.UseFixedWorld | F.ZeroAgentVelocity, rand_seed=args.seed, min_hiders=args.num_hiders, max_hiders=args.num_hiders,
        min_seekers=args.num_hiders, max_seekers=args.num_hiders, num_pbt_policies=len(policies))
    sim.init()
    lg = league.League(sim, policies, args.num_hiders, mode="greedy" if args.greedy else "draw", seed=args.seed, k_factor=args.k_factor)
    if args.behaviour_stats:
        lg.behaviour = behaviour.BehaviourStats(sim).arm(from_start=True)
    print("Elo before:")
    league.print_elos(lg.read()["elo"])
    log = open(args.record_log, "wb") if args.record_log else None
    try:
        out = lg.run(args.num_steps, record_log=log)
    finally:
        if log is not None:
            log.close()
    print(f"Elo after {out['games']} games:")
    league.print_elos(out["elo"])
    print("\n".join(matrix(out["counts"])))
    if lg.behaviour is not None:
        print("behaviour: " + json.dumps(lg.behaviour.read()))
    print(json.dumps(out))
    sim.close()
    return out


if __name__ == "__main__":
    main()
