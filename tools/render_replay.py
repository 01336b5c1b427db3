"""Replay log -> PNG frames, the headless counterpart of `viewer.cpp --replay` (src/viewer.cpp:185-215).

    python tools/render_replay.py run.log --worlds 4 --out frames/ [--camera top|agent:K|look:ex,ey,ez,tx,ty,tz]
        [--size 512x512] [--show 0,2] [--steps 0:60] [--seed 5 --flags 9 --hiders 3 --seekers 3]

The log is what scripts/jax_infer.py --record-log writes and gpu_hideseek.replay.record_step appends: per step, one
1392-byte checkpoint per world.  A load regenerates each world's level from its record, and level generation depends
on the recording simulator's arguments, so --worlds, --seed, --flags, --hiders and --seekers must be the recording's
(defaults: jax_infer.py's seed 5 and flags UseFixedWorld | ZeroAgentVelocity = 9, viewer.cpp's 3 hiders + 3 seekers).
One PNG per step; with several worlds shown, a mosaic of one camera per world.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))


def parse_size(s):
    w, h = s.lower().split("x")
    return int(w), int(h)


def parse_camera(spec):
    """-> cameras(sim, step, worlds) -> list of cameras."""
    from gpu_hideseek import spectate as S
    if spec == "top":
        return lambda sim, t, worlds: [S.top_down(w) for w in worlds]
    if spec.startswith("agent:"):
        k = int(spec.split(":", 1)[1])

        def agent(sim, t, worlds):
            bodies = sim.debug_bodies()[0]
            out = []
            for w in worlds:
                q2 = float((bodies[w, S.AGENT_SLOT0 + k, 3:7].astype(float) ** 2).sum())
                out.append(S.agent_camera(bodies, w, k) if 0.99 <= q2 <= 1.01 else S.top_down(w))   # agent k absent
            return out
        return agent
    if spec.startswith("look:"):
        v = [float(x) for x in spec.split(":", 1)[1].split(",")]
        if len(v) != 6:
            raise SystemExit("--camera look:ex,ey,ez,tx,ty,tz")
        return lambda sim, t, worlds: [S.look_at(w, v[:3], v[3:]) for w in worlds]
    raise SystemExit(f"unknown camera {spec!r}: top, agent:K or look:ex,ey,ez,tx,ty,tz")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("log")
    ap.add_argument("--worlds", type=int, required=True, help="worlds of the recording simulator")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--flags", type=int, default=9)
    ap.add_argument("--hiders", type=int, default=3)
    ap.add_argument("--seekers", type=int, default=3)
    ap.add_argument("--camera", default="top")
    ap.add_argument("--size", type=parse_size, default=(512, 512))
    ap.add_argument("--show", default=None, help="comma-separated worlds to show (default: the first 16)")
    ap.add_argument("--steps", default=None, help="first:last+1 of the steps to render (default: all)")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)

    import gpu_hideseek
    from gpu_hideseek import replay, spectate as S
    log = replay.read_log(a.log, a.worlds)
    if log.shape[0] == 0:
        raise SystemExit(f"{a.log}: no whole step of {a.worlds} worlds")
    show = [int(x) for x in a.show.split(",")] if a.show else list(range(min(a.worlds, 16)))
    steps = None
    if a.steps:
        lo, hi = (int(x) if x else None for x in a.steps.split(":"))
        steps = range(*slice(lo, hi).indices(log.shape[0]))
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=a.gpu, num_worlds=a.worlds, sim_flags=a.flags,
        rand_seed=a.seed, min_hiders=a.hiders, max_hiders=a.hiders, min_seekers=a.seekers, max_seekers=a.seekers,
        num_pbt_policies=1)
    sim.init()
    cams = parse_camera(a.camera)
    W, H = a.size
    paths = S.render_log(log, lambda s, t: cams(s, t, show), W, H, a.out, sim=sim, steps=steps)
    print(f"{len(paths)} frames of {len(show)} world(s) at {W}x{H} -> {a.out}")
    sim.close()


if __name__ == "__main__":
    main()
