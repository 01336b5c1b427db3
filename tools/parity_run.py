"""Developer tool: run the HIP simulator and the CPU oracle side by side and report the first
step/tensor where they differ (bitwise).  Usage:
    python tools/parity_run.py [--worlds 64] [--steps 50] [--flags 0] [--seed 0] [--hiders 2 --seekers 2]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import lockstep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--hiders", type=int, default=2)
    ap.add_argument("--seekers", type=int, default=2)
    ap.add_argument("--level", type=int, default=0, help="debug level for all worlds (0 = training)")
    ap.add_argument("--act", default="bench", choices=["bench", "full", "none"])
    ap.add_argument("--stop", action="store_true", help="stop at first mismatch")
    ap.add_argument("--threads", type=int, default=None, help="oracle threads (default: lockstep.oracle_threads())")
    ap.add_argument("--every", type=int, default=1, help="compare every n-th step (and the last one)")
    a = ap.parse_args()

    p = lockstep.Pair(a.worlds, flags=a.flags, seed=a.seed, hiders=(a.hiders, a.hiders), seekers=(a.seekers, a.seekers),
                      level=a.level, threads=a.threads)
    draw, cols = lockstep.stream(a.act)
    nbad = 0

    def compare(tag):
        nonlocal nbad
        bad = lockstep.diff(p.gpu, p.ref)
        if bad:
            nbad += 1
            print(f"[{tag}] MISMATCH:")
            for b in bad:
                print("   ", b)
        return not bad

    compare("init")
    for s in range(a.steps):
        p.step(None if draw is None else draw(s, p.rows), cols)
        if s % a.every == 0 or s == a.steps - 1:
            if not compare(f"step {s}") and a.stop:
                break
    print(f"done: {a.steps} steps, {a.worlds} worlds, mismatching checkpoints: {nbad}")
    return 1 if nbad else 0


if __name__ == "__main__":
    sys.exit(main())
