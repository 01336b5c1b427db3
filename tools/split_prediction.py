"""What the split schedule can gain, from recorded per-octet wave times:
  python tools/split_prediction.py oct_ticks.npy        # [steps, octets] microseconds of every physics wave
For each predictor and threshold, over the steps that run split (not the one with the deal, not the regeneration):
  T_all   = slowest wave of the step          T_early = slowest wave among the octets predicted early
  window  = T_all - T_early: how long before the end of k_physics the early group's k_observe could start
and the late fraction.  The schedule gains at most min(window, duration of the early k_observe) minus what the second
stream costs.  Predictors: the previous step's time, the mean of the last two steps' times (what k_physics computes), each
against factor x the previous step's mean wave; 'oracle' ranks by the step's own times (the bound of any predictor)."""
import sys
import numpy as np

T = np.load(sys.argv[1]).astype(np.float64)
steps, noct = T.shape
period = 32
ok = np.array([i >= 3 and (i + 1) % period != 0 and i % period != 0 and (i + 1) % period != 1 and T[i].max() < 1000 and T[i - 1].max() < 1000 and T[i - 2].max() < 1000
               for i in range(steps)])
idx = np.nonzero(ok)[0]
print(f"{len(idx)} of {steps} steps; mean wave {T[idx].mean():.1f} us, p99 {np.percentile(T[idx], 99, axis=1).mean():.1f}, slowest {T[idx].max(axis=1).mean():.1f}")
c1 = [np.corrcoef(T[i], T[i - 1])[0, 1] for i in idx]
c2 = [np.corrcoef(T[i], T[i - 2])[0, 1] for i in idx]
cm = [np.corrcoef(T[i], T[i - 1] + T[i - 2])[0, 1] for i in idx]
print(f"correlation of a wave's time with the step before {np.mean(c1):.2f}, two before {np.mean(c2):.2f}, the mean of both {np.mean(cm):.2f}")
print(f"{'predictor':12s} {'factor':>7s} {'late %':>7s} {'T_all':>7s} {'T_early':>8s} {'window':>7s} {'window p10':>10s}")


def row(name, c, late_of):
    fr, ta, te = [], [], []
    for i in idx:
        late = late_of(i)
        early = T[i][~late]
        fr.append(late.mean()); ta.append(T[i].max()); te.append(early.max() if early.size else 0.0)
    w = np.array(ta) - np.array(te)
    print(f"{name:12s} {c:7.2f} {100 * np.mean(fr):7.2f} {np.mean(ta):7.1f} {np.mean(te):8.1f} {w.mean():7.1f} {np.percentile(w, 10):10.1f}")


for c in (1.3, 1.2, 1.15, 1.1, 1.05, 1.0, 0.95, 0.9):
    row("previous", c, lambda i: T[i - 1] > c * T[i - 1].mean())
for c in (1.3, 1.2, 1.15, 1.1, 1.05, 1.0, 0.95, 0.9):
    row("mean of two", c, lambda i: T[i - 1] + T[i - 2] > 2 * c * T[i - 2].mean())
for f in (0.02, 0.05, 0.1, 0.2, 0.3):
    row("oracle", f, lambda i: T[i] >= np.quantile(T[i], 1 - f))
