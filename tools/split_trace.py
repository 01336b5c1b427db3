"""The split schedule in a rocprofv3 --kernel-trace of bench.py, against a trace of the one-chain schedule:
  python tools/split_trace.py ONE_CHAIN_kernel_trace.csv SPLIT_kernel_trace.csv
A split step has a k_physics and a k_observe on each of two queues; the late chain is on the queue the one-chain steps
(the step with the deal) use.  Per split step, in microseconds: the start of the early k_physics after the late one (what the
second stream costs at the head of the step), both k_physics durations, when the early k_observe starts relative to the
end of the late k_physics (negative: it overlaps the slowest physics waves), and the span of the step's kernels."""
import csv
import sys
from collections import Counter

import numpy as np


def load(path):
    rows = [r for r in csv.DictReader(open(path)) if "k_physics" in r["Kernel_Name"] or "k_observe" in r["Kernel_Name"]]
    return sorted((int(r["Start_Timestamp"]) / 1e3, int(r["End_Timestamp"]) / 1e3, "physics" if "k_physics" in r["Kernel_Name"] else "observe",
                   r["Queue_Id"]) for r in rows)


def stat(name, x):
    x = np.asarray(x)
    print(f"  {name:58s} mean {x.mean():7.1f}  p10 {np.percentile(x, 10):7.1f}  median {np.median(x):7.1f}  p90 {np.percentile(x, 90):7.1f}")


one, split = load(sys.argv[1]), load(sys.argv[2])
print(f"one chain ({sys.argv[1]}):")
stat("k_physics", [e - s for s, e, k, _ in one if k == "physics"])
stat("k_observe", [e - s for s, e, k, _ in one if k == "observe"])
ph = [k for k in one if k[2] == "physics"]
ob = [k for k in one if k[2] == "observe"][-len(ph):]
stat("span of a step's kernels", [o[1] - p[0] for p, o in zip(ph, ob)])

main_q = Counter(q for _, _, k, q in split if k == "physics").most_common()
late_q = min(main_q, key=lambda t: (-t[1], t[0]))[0]          # the one-chain steps run there too
lp = [k for k in split if k[2] == "physics" and k[3] == late_q]
ep = [k for k in split if k[2] == "physics" and k[3] != late_q]
lo = [k for k in split if k[2] == "observe" and k[3] == late_q]
eo = [k for k in split if k[2] == "observe" and k[3] != late_q]
steps = []
for p in ep:                                               # a split step: the late k_physics that starts last before the early one
    cand = [q for q in lp if q[0] <= p[0]]
    if not cand:
        continue
    l = cand[-1]
    o2 = next(o for o in eo if o[0] >= p[1] - 1e-3)
    o1 = next(o for o in lo if o[0] >= l[1] - 1e-3)
    steps.append((l, p, o1, o2))
print(f"split ({sys.argv[2]}): {len(steps)} split steps, {len(lp) - len(steps)} one-chain steps")
stat("early k_physics starts after the late k_physics", [p[0] - l[0] for l, p, _, _ in steps])
stat("late k_physics", [l[1] - l[0] for l, _, _, _ in steps])
stat("early k_physics", [p[1] - p[0] for _, p, _, _ in steps])
stat("late k_observe", [o1[1] - o1[0] for _, _, o1, _ in steps])
stat("early k_observe", [o2[1] - o2[0] for _, _, _, o2 in steps])
stat("early k_observe starts after the end of the late k_physics", [o2[0] - l[1] for l, _, _, o2 in steps])
stat("span of a step's kernels", [max(o1[1], o2[1]) - l[0] for l, _, o1, o2 in steps])
