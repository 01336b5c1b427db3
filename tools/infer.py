"""Run a trained policy on the simulator and report how the game goes: gpu_hideseek.evaluate behind the arguments of the
reference's scripts/jax_infer.py that make sense here.

    python tools/infer.py --num-worlds 1024 --num-steps 480 --ckpt-path ckpts/run0/100 --bf16 [--greedy]
    python tools/infer.py --num-worlds 16 --num-steps 250 --ckpt-path ckpts/run0/100 --record-log run.log
    python tools/render_replay.py run.log --worlds 16 --out frames              # and watch it (flags 9, seed 5: the defaults there)

--ckpt-path is a file tools/train.py saved (the trainer's state_dict): its "params" and "normaliser" are loaded, the
optimiser's state is not needed; of a population's checkpoint (tools/train.py --pbt-ensemble-size) --member i picks one
policy.  The simulator runs with UseFixedWorld | ZeroAgentVelocity, as the reference's script
does.  --record-log appends a checkpoint of every world after every step.  --print-rewards prints every step's reward
tensor.  At the end it prints the per-side table of the episodes that finished (240 steps each) and one JSON line.
--behaviour-stats also tracks what the agents do with the level (gpu_hideseek.behaviour) and prints it as a JSON line
before that one.  Several checkpoints playing each other, with Elo ratings (the reference's eval_competitive), is tools/league.py.
Training several policies at once is tools/train.py --pbt-ensemble-size.  Not here: --single-policy, --print-obs and
--print-action-probs.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402
from gpu_hideseek import behaviour, evaluate, policy  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--num-worlds", type=int, required=True)
    ap.add_argument("--num-steps", type=int, default=200)
    ap.add_argument("--ckpt-path", type=str, required=True)
    ap.add_argument("--member", type=int, help="the policy of a population checkpoint to run")
    ap.add_argument("--record-log", type=str)
    ap.add_argument("--print-rewards", action="store_true")
    ap.add_argument("--num-hiders", type=int, default=3)
    ap.add_argument("--num-seekers", type=int, default=3)
    ap.add_argument("--fp16", action="store_true")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--gpu-id", type=int, default=0)
    ap.add_argument("--greedy", action="store_true", help="every head's most likely action instead of a draw")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--behaviour-stats", action="store_true", help="track object movement, locks, travel and grabs on the device and print them")
    ap.add_argument("--encoder", choices=policy.ENCODERS, help="the policy's network (tools/train.py --encoder); by default read from the checkpoint")
    args = ap.parse_args(argv)
    if args.fp16 and args.bf16:
        ap.error("--fp16 and --bf16 exclude each other")
    return args


def table(stats):
    """The lines of the per-side table."""
    lines = ["%-8s %9s %12s %11s %16s %10s" % ("side", "episodes", "return mean", "return std", "discounted mean", "length")]
    for side in ("hiders", "seekers"):
        s = stats[side]
        lines.append("%-8s %9d %12.3f %11.3f %16.3f %10.1f" % (side, s["episodes"], s["return_mean"], s["return_std"], s["discounted_return_mean"], s["length_mean"]))
    lines.append("world episodes %d: hiders won %.1f%%, seekers won %.1f%%, draws %.1f%%" % (
        stats["world_episodes"], 100 * stats["hider_win_rate"], 100 * stats["seeker_win_rate"], 100 * stats["draw_rate"]))
    return lines


def main(argv=None):
    args = parse(argv)
    F = gpu_hideseek.SimFlags
    dtype = torch.float16 if args.fp16 else torch.bfloat16 if args.bf16 else torch.float32
    net, normaliser = evaluate.load_policy(args.ckpt_path, dtype, torch.device("cuda", args.gpu_id), member=args.member, encoder=args.encoder)
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=args.gpu_id, num_worlds=args.num_worlds,
        sim_flags=F.UseFixedWorld | F.ZeroAgentVelocity, rand_seed=args.seed, min_hiders=args.num_hiders, max_hiders=args.num_hiders,
        min_seekers=args.num_seekers, max_seekers=args.num_seekers, num_pbt_policies=1)
    sim.init()
    ev = evaluate.Evaluator(sim, net, normaliser, mode="greedy" if args.greedy else "draw", seed=args.seed)
    if args.behaviour_stats:
        ev.behaviour = behaviour.BehaviourStats(sim).arm(from_start=True)
    log = open(args.record_log, "wb") if args.record_log else None

    def on_step(i, ev):
        print(f"\nStep {i}")
        print("Rewards:", sim.reward_tensor().to_torch().reshape(args.num_worlds, -1).cpu())
    try:
        stats = ev.run(args.num_steps, record_log=log, on_step=on_step if args.print_rewards else None)
    finally:
        if log is not None:
            log.close()
    print("\n".join(table(stats)))
    if ev.behaviour is not None:
        print("behaviour: " + json.dumps(ev.behaviour.read()))
    print(json.dumps(stats))
    sim.close()
    return stats


if __name__ == "__main__":
    main()
