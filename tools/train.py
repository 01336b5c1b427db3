"""Train the policy on the simulator: the update loop of gpu_hideseek.trainer behind the arguments of the reference's
scripts/jax_train.py that make sense here, on one GPU.

    python tools/train.py --num-worlds 16000 --num-updates 100 --bf16 [--ckpt-dir ckpts --run-name run0 [--restore 50]]
    python tools/train.py --num-worlds 16000 --num-updates 10 --bf16 --phases [--out profiles/train_phases.txt]

The simulator runs with the reference's flags, RandomFlipTeams | UseFixedWorld | ZeroAgentVelocity.  Every 10 updates it
prints `Update: N` and `  FPS: ...` as the reference does: world steps per second, num_worlds * steps_per_update * updates
/ wall time since the last print (an agent-row rate is that times the agents per world).  With --ckpt-dir and --run-name
the trainer's state_dict goes to <ckpt-dir>/<run-name>/<update> at the end and every --ckpt-frequency updates, and
--restore N loads <ckpt-dir>/<run-name>/N first; the simulator's own state is not part of it.
--phases puts device events around the phases of every update (trainer.PHASES: simulator steps, pack, rollout forward, GAE
with the bootstrap, gather, update forward + backward, Adam), waits for the device once per update, and prints each
phase's time per update and share, over the updates after the first (which warms up); what the phases leave out (copies
of exports into slots, the permutation, Python between the calls) is the row "other".
--episode-stats tracks the finished episodes on the device (gpu_hideseek.episodes: one launch after every simulator step)
and prints, as a second JSON line at each `Update:` print, what has finished since the last one: per side the episodes,
the mean and standard deviation of the return, the mean discounted return and length, and the hiders' and seekers' win
rates.  On a fresh simulator the episodes are tracked from their start; after --restore the tracker waits for every row's
next episode, because the simulator's state is not restored.  tools/infer.py runs a saved policy without learning.
--behaviour-stats tracks what the agents do with the level (gpu_hideseek.behaviour: one more launch after every simulator
step) and prints it the same way, as a JSON line of its own: per episode how far the boxes and ramps were moved in the
preparation phase and after it, how many of them each side had locked when the seekers were released and at the end, and
each side's travel per agent-step and grab rate.
Saved checkpoints play each other, with Elo ratings (the reference's eval_competitive), in tools/league.py.
--pbt-ensemble-size P trains P policies at once on the one simulator (gpu_hideseek.population: the league's fixed
schedule, so --num-worlds must be a multiple of P^2 and both teams have --num-hiders agents), with live Elo ratings from the
games the rollouts play; --pbt-interval N copies the best policies over the worst and explores lr and the entropy
coefficient after every N-th update (0, the default: never).  The `Update:` print then has one metrics line per policy and
the Elo table, four ratings to a line as the reference prints it, and the checkpoint is the population's (tools/infer.py
and tools/league.py read it with --member).
--pbt-past-policies Q adds a pool of Q frozen past policies to the population (the reference's flag, which it runs with
past_play_portion = 1): the learners play the pool's members on both sides, never past against past
(league.past_play_schedule; 1 <= Q <= P, --num-worlds a multiple of P (P + Q)), and --pbt-snapshot-interval N copies the
best-rated learner into the pool's next slot after every N-th update, before that update's exploit step (0, the default:
the pool stays a copy of the first learners).  The Elo table then covers all P + Q policies, the learners first, and a
line names the update each pool slot's snapshot was taken at.
--encoder attention trains the reference's other network, EntitySelfAttentionNet (gpu_hideseek.entity_attention), in
place of SimpleNet; the checkpoint's layout says which it was, and tools/infer.py and tools/league.py read it from there.
--fp16 trains with the dynamic loss scale (gpu_hideseek.optim.LossScale: the gradients of a minibatch of about 10^6 samples
lie below float16's normal range without it): the metrics line then carries "loss_scale", the scale after the update, next
to "skipped", the steps that overflowed and halved it, and --phases prints both per update.  --loss-scale-init X sets the
start (a power of two; 2^16 by default), --no-loss-scale trains float16 with no scale.
--gpu-ids 0,1,... trains data-parallel over the shards of a ShardedSimulator, one per id (an id may repeat: two shards
on one device), through trainer.ShardedTrainer: one replica of the policy per shard, every replica stepping with the
gradient of the mean over all shards' samples (optim.reduce_gradients).  --num-worlds is the total, cut into contiguous
ranges.  --phases then needs all ids to be one device and has one more row, "reduce" (the copies between the shards and
the reduction); the trackers of --episode-stats and --behaviour-stats run per shard and print one line per shard.  Not
with --pbt-ensemble-size.  Without --gpu-ids the single-device path runs as before.
Not here: tensorboard / wandb, one process per GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402
from gpu_hideseek import behaviour, episodes, league, policy, population, trainer  # noqa: E402
from gpu_hideseek import sharded as sharded_mod  # noqa: E402

PRINT_EVERY = 10


class Trackers:
    """One tracker per shard behind a tracker's two methods: step() all of them, read() the list of their numbers."""

    def __init__(self, trackers):
        self.trackers = list(trackers)

    def step(self):
        for t in self.trackers:
            t.step()

    def read(self):
        return [t.read() for t in self.trackers]


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpu-id", type=int, default=0)
    ap.add_argument("--gpu-ids", type=str, help="comma-separated device ids, one shard each (trainer.ShardedTrainer); an id may repeat")
    ap.add_argument("--ckpt-dir", type=str)
    ap.add_argument("--run-name", type=str)
    ap.add_argument("--restore", type=int)
    ap.add_argument("--ckpt-frequency", type=int, default=500)
    ap.add_argument("--num-worlds", type=int, required=True)
    ap.add_argument("--num-updates", type=int, required=True)
    ap.add_argument("--steps-per-update", type=int, default=40)
    ap.add_argument("--num-bptt-chunks", type=int, default=8)
    ap.add_argument("--num-minibatches", type=int, default=2)
    ap.add_argument("--num-epochs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--gamma", type=float, default=0.998)
    ap.add_argument("--entropy-loss-coef", type=float, default=0.01)
    ap.add_argument("--value-loss-coef", type=float, default=1.0)
    ap.add_argument("--fp16", action="store_true")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--no-loss-scale", action="store_true", help="with --fp16: no dynamic loss scale (TrainConfig.loss_scale None); most of the gradient then underflows")
    ap.add_argument("--loss-scale-init", type=float, help="with --fp16: the loss scale's start, a power of two (default 2^16)")
    ap.add_argument("--num-hiders", type=int, default=3)
    ap.add_argument("--num-seekers", type=int, default=3)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--eager", action="store_true", help="the policy's eager pieces and the gather by torch indexing (Trainer(fused=False))")
    ap.add_argument("--encoder", choices=policy.ENCODERS, default="simple", help="the policy's network in front of the LSTM (policy.make_policy)")
    ap.add_argument("--phases", action="store_true")
    ap.add_argument("--episode-stats", action="store_true", help="track finished episodes on the device and print them with the metrics")
    ap.add_argument("--behaviour-stats", action="store_true", help="track object movement, locks, travel and grabs on the device and print them with the metrics")
    ap.add_argument("--out", type=str, help="with --phases: write the table here too")
    ap.add_argument("--pbt-ensemble-size", type=int, default=0, help="train this many policies at once (gpu_hideseek.population); 0: the plain trainer")
    ap.add_argument("--pbt-interval", type=int, default=0, help="with --pbt-ensemble-size: exploit / explore after every N-th update; 0: never")
    ap.add_argument("--pbt-past-policies", type=int, default=0, help="with --pbt-ensemble-size: a pool of this many frozen past policies; 0: none")
    ap.add_argument("--pbt-snapshot-interval", type=int, default=0, help="with --pbt-past-policies: a snapshot into the pool after every N-th update; 0: never")
    args = ap.parse_args(argv)
    if args.pbt_past_policies and not args.pbt_ensemble_size:
        ap.error("--pbt-past-policies needs --pbt-ensemble-size")
    if args.pbt_snapshot_interval and not args.pbt_past_policies:
        ap.error("--pbt-snapshot-interval needs --pbt-past-policies")
    if args.pbt_ensemble_size and args.num_hiders != args.num_seekers:
        ap.error("--pbt-ensemble-size needs equal teams: --num-hiders == --num-seekers")
    if args.pbt_interval and not args.pbt_ensemble_size:
        ap.error("--pbt-interval needs --pbt-ensemble-size")
    if args.gpu_ids is not None:
        try:
            args.gpu_ids = [int(x) for x in args.gpu_ids.split(",")]
        except ValueError:
            ap.error("--gpu-ids takes comma-separated integers")
        if args.pbt_ensemble_size:
            ap.error("--gpu-ids and --pbt-ensemble-size exclude each other: there is no population over shards")
    if args.fp16 and args.bf16:
        ap.error("--fp16 and --bf16 exclude each other")
    if (args.no_loss_scale or args.loss_scale_init is not None) and not args.fp16:
        ap.error("--no-loss-scale and --loss-scale-init need --fp16")
    if args.no_loss_scale and args.loss_scale_init is not None:
        ap.error("--no-loss-scale and --loss-scale-init exclude each other")
    if (args.ckpt_dir is None) != (args.run_name is None):
        ap.error("--ckpt-dir and --run-name go together")
    if args.restore is not None and args.ckpt_dir is None:
        ap.error("--restore needs --ckpt-dir and --run-name")
    return args


def config(args):
    dtype = torch.float16 if args.fp16 else torch.bfloat16 if args.bf16 else torch.float32
    # float16 gradients are about 1 / (samples of a minibatch) and underflow without a scale: --fp16 turns the dynamic one on
    scale = None if not args.fp16 or args.no_loss_scale else "dynamic" if args.loss_scale_init is None else {"init_scale": args.loss_scale_init}
    if args.pbt_ensemble_size:
        return population.PopulationConfig(steps_per_update=args.steps_per_update, num_bptt_chunks=args.num_bptt_chunks, num_minibatches=args.num_minibatches,
                                           num_epochs=args.num_epochs, lr=args.lr, gamma=args.gamma, entropy_coef=args.entropy_loss_coef,
                                           value_loss_coef=args.value_loss_coef, dtype=dtype, seed=args.seed, num_policies=args.pbt_ensemble_size,
                                           team_size=args.num_hiders, pbt_interval=args.pbt_interval, num_past_policies=args.pbt_past_policies,
                                           snapshot_interval=args.pbt_snapshot_interval, loss_scale=scale)
    return trainer.TrainConfig(steps_per_update=args.steps_per_update, num_bptt_chunks=args.num_bptt_chunks, num_minibatches=args.num_minibatches,
                               num_epochs=args.num_epochs, lr=args.lr, gamma=args.gamma, entropy_coef=args.entropy_loss_coef,
                               value_loss_coef=args.value_loss_coef, dtype=dtype, seed=args.seed, loss_scale=scale)


def phase_table(totals, wall_ms, updates, args, fps):
    """The lines of the --phases table: per phase the milliseconds per update and the share of the wall time."""
    lines = ["%d worlds x (%d + %d) agents, %s, T = %d, K = %d, %d minibatches x %d epochs; %d updates after 1 warm-up update" % (
        args.num_worlds, args.num_hiders, args.num_seekers, "float16" if args.fp16 else "bfloat16" if args.bf16 else "float32", args.steps_per_update,
        args.num_bptt_chunks, args.num_minibatches, args.num_epochs, updates),
        "FPS (world steps per second, as the reference prints it): %.0f;  agent rows per second: %.0f" % (fps, fps * (args.num_hiders + args.num_seekers)),
        "%-26s %14s %8s" % ("phase", "ms per update", "share")]
    rest = wall_ms
    for k in totals:
        lines.append("%-26s %14.2f %7.1f%%" % (k, totals[k] / updates, 100 * totals[k] / wall_ms))
        rest -= totals[k]
    lines.append("%-26s %14.2f %7.1f%%" % ("other", rest / updates, 100 * rest / wall_ms))
    lines.append("%-26s %14.2f %7.1f%%" % ("wall", wall_ms / updates, 100.0))
    return lines


def main(argv=None):
    args = parse(argv)
    F = gpu_hideseek.SimFlags
    kw = dict(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, num_worlds=args.num_worlds,
              sim_flags=F.RandomFlipTeams | F.UseFixedWorld | F.ZeroAgentVelocity, rand_seed=args.seed, min_hiders=args.num_hiders,
              max_hiders=args.num_hiders, min_seekers=args.num_seekers, max_seekers=args.num_seekers, num_pbt_policies=max(1, args.pbt_ensemble_size + args.pbt_past_policies))
    sharded = args.gpu_ids is not None
    sim = sharded_mod.ShardedSimulator(args.gpu_ids, **kw) if sharded else gpu_hideseek.HideAndSeekSimulator(gpu_id=args.gpu_id, **kw)
    sim.init()
    cfg = config(args)

    def fresh(index):                                                  # the trainers' own seeding, with the encoder asked for
        return policy.make_policy(cfg.dtype, generator=torch.Generator().manual_seed(cfg.seed + index), encoder=args.encoder)
    if sharded:
        tr = trainer.ShardedTrainer(sim, cfg, net=None if args.encoder == "simple" else fresh(0), fused=not args.eager)
    elif args.encoder == "simple":
        tr = (population.Population if args.pbt_ensemble_size else trainer.Trainer)(sim, cfg, fused=not args.eager)
    elif args.pbt_ensemble_size:
        tr = population.Population(sim, cfg, nets=[fresh(p) for p in range(args.pbt_ensemble_size)], fused=not args.eager)
    else:
        tr = trainer.Trainer(sim, cfg, net=fresh(0), fused=not args.eager)
    run_dir = None if args.ckpt_dir is None else os.path.join(args.ckpt_dir, args.run_name)
    if args.restore is not None:
        tr.load_state_dict(torch.load(os.path.join(run_dir, str(args.restore)), map_location=tr.device, weights_only=False))
    if args.phases:
        tr.phases = trainer.PhaseTimer(trainer.SHARDED_PHASES if sharded else trainer.PHASES)
    if args.episode_stats:
        tr.episodes = Trackers([episodes.EpisodeStats(s, gamma=args.gamma).arm(from_start=args.restore is None) for s in sim.shards]) if sharded else \
            episodes.EpisodeStats(sim, gamma=args.gamma).arm(from_start=args.restore is None)
    if args.behaviour_stats:
        tr.behaviour = Trackers([behaviour.BehaviourStats(s).arm(from_start=args.restore is None) for s in sim.shards]) if sharded else \
            behaviour.BehaviourStats(sim).arm(from_start=args.restore is None)

    def save():
        if run_dir is not None:
            os.makedirs(run_dir, exist_ok=True)
            torch.save(tr.state_dict(), os.path.join(run_dir, str(tr.update_index)))

    def show(metrics):
        """The metrics of the last update: one JSON line, or with a population one per policy and the Elo table."""
        plain = lambda m: {k: v for k, v in m.items() if not isinstance(v, list)}       # noqa: E731
        if "policies" not in metrics:
            print("  " + json.dumps(plain(metrics)))
            return
        for p, m in enumerate(metrics["policies"]):
            print(f"  policy {p}: " + json.dumps(plain(m)))
        print("  " + json.dumps({k: metrics[k] for k in ("games", "bad", "snapshot", "exploit") if k in metrics}))
        league.print_elos(metrics["elo"])
        if "past" in metrics:
            T = len(metrics["policies"])
            print("  past policies: " + ", ".join(f"{T + u} from update {n}" for u, n in enumerate(metrics["past"])))

    totals, wall_ms, timed = {k: 0.0 for k in (tr.phases.names if args.phases else trainer.PHASES)}, 0.0, 0
    last_time, last_update, metrics = 0.0, tr.update_index, {}
    for i in range(args.num_updates):
        if (tr.update_index - last_update) % PRINT_EVERY == 0 or i == 0:
            now = time.time()
            print(f"Update: {tr.update_index}")
            if last_time != 0:
                print("  FPS:", args.num_worlds * args.steps_per_update * (tr.update_index - last_update) / (now - last_time))
                show(metrics)
                if tr.episodes is not None:
                    print("  " + json.dumps(tr.episodes.read()))
                if tr.behaviour is not None:
                    print("  " + json.dumps(tr.behaviour.read()))
            last_time, last_update = now, tr.update_index
        t0 = time.perf_counter()
        metrics = tr.update_iter()
        if args.phases:
            spans = tr.phases.totals()
            scaled = "" if "loss_scale" not in metrics else ", loss scale %g, %d skipped steps" % (metrics["loss_scale"], metrics["skipped"])
            print("  update %d: %.1f ms%s" % (tr.update_index, 1e3 * (time.perf_counter() - t0), scaled), flush=True)
            if i > 0:                                                  # the first update warms up
                wall_ms += 1e3 * (time.perf_counter() - t0)
                timed += 1
                for k in totals:
                    totals[k] += spans[k]
        if args.ckpt_frequency > 0 and tr.update_index % args.ckpt_frequency == 0:
            save()
    print(f"Update: {tr.update_index}")
    show(metrics)
    if tr.episodes is not None:
        print("  " + json.dumps(tr.episodes.read()))
    if tr.behaviour is not None:
        print("  " + json.dumps(tr.behaviour.read()))
    save()
    if args.phases and timed:
        fps = args.num_worlds * args.steps_per_update * timed / (wall_ms * 1e-3)
        lines = ["encoder: " + args.encoder] + phase_table(totals, wall_ms, timed, args, fps)
        print("\n".join(lines))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "updates": timed, "wall_ms_per_update": wall_ms / timed,
                                    "fps_world_steps": fps, "phases_ms_per_update": {k: v / timed for k, v in totals.items()},
                                    "last_metrics": {k: v for k, v in metrics.items() if not isinstance(v, list) or k == "elo"}}) + "\n\n")
                f.write("\n".join(lines) + "\n")
    sim.close()


if __name__ == "__main__":
    main()
