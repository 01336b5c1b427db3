"""Time of the advantage kernel (sim.compute_advantages, csrc/hs_k_gae.h) next to the backwards loop over T a torch
learner writes from eager ops on the same device (the same formula), and next to a plain device-to-device copy of as many
bytes as the call moves.

    python tools/gae_bench.py [--worlds 16000] [--steps 40] [--calls 200] [--rounds 3] [--out profiles/gae_bench.txt]

At --worlds x (3+3) agents and T = --steps: values in f32 and bf16, with and without the mask and the moments.  The eager
loop is, per time step, the selects and the two to three multiply-adds of the contract on [rows] tensors, and with
moments the five reductions over the finished [T, rows] outputs.  Each variant is timed with device events around --calls
enqueued calls after warm-up; fused, eager and copy alternate inside each of --rounds rounds and the median window is
reported with the spread (max - min) of the windows.  Algorithmic bytes = reward, done, value (and mask) read once +
advantage and returns written once.  The eager loop works in f32 on widened values with the same selects, so its
advantages are compared with the fused ones once: they must be equal bit for bit (torch does not fuse the operations
either).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402

GAMMA, LAMBDA = 0.998, 0.95
VARIANTS = [(dt, mask, mom) for dt in (torch.float32, torch.bfloat16) for mask, mom in ((False, False), (True, False), (True, True))]


def make_sim(n, agents=3):
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=0, rand_seed=0, min_hiders=agents,
        max_hiders=agents, min_seekers=agents, max_seekers=agents, num_pbt_policies=1)
    sim.init()
    return sim


def eager_gae(reward, done, value, bootstrap, mask, adv, ret, moments):
    """The contract of include/hideseek.h from eager ops, backwards over T."""
    T = reward.shape[0]
    g = GAMMA
    gl = float(torch.tensor(GAMMA, dtype=torch.float32) * torch.tensor(LAMBDA, dtype=torch.float32))
    carry = torch.zeros_like(reward[0])
    vn = bootstrap.float()
    zero = torch.zeros_like(carry)
    for t in range(T - 1, -1, -1):
        v, r, ended = value[t].float(), reward[t], done[t] != 0
        delta = torch.where(ended, r - v, (r + g * vn) - v)
        run = torch.where(ended, delta, delta + gl * carry)
        if mask is not None:
            active = mask[t] != 0
            torch.where(active, run, zero, out=adv[t])
            torch.where(active, run + v, zero, out=ret[t])
        else:
            adv[t].copy_(run)
            torch.add(run, v, out=ret[t])
        carry, vn = adv[t], v
    if moments is not None:
        a, b = adv.double(), ret.double()
        n = (mask != 0).sum().double() if mask is not None else torch.tensor(float(adv.numel()), dtype=torch.float64, device=adv.device)
        moments.copy_(torch.stack([a.sum(), (a * a).sum(), b.sum(), (b * b).sum(), n]))


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls      # ms per call


def bench_variant(sim, dtype, with_mask, with_moments, args):
    R, T = sim.num_worlds * sim.agents_per_world, args.steps
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(T)
    reward = torch.randint(-1, 2, (T, R), device=dev, generator=g).float()
    done = (torch.rand(T, R, device=dev, generator=g) < 0.1).to(torch.int32)
    value = (5.0 * torch.randn(T, R, device=dev, generator=g)).to(dtype)
    bootstrap = (5.0 * torch.randn(R, device=dev, generator=g)).to(dtype)
    mask = (torch.rand(T, R, device=dev, generator=g) >= 0.25).float() if with_mask else None
    adv, ret = torch.empty(T, R, device=dev), torch.empty(T, R, device=dev)
    adv_e, ret_e = torch.empty_like(adv), torch.empty_like(ret)
    mom = torch.empty(5, dtype=torch.float64, device=dev) if with_moments else None
    mom_e = torch.empty_like(mom) if with_moments else None
    stream = torch.cuda.current_stream()

    def fused():                          # enqueue only, like the eager ops: the events see device time
        sim.compute_advantages(reward, done, value, bootstrap, gamma=GAMMA, gae_lambda=LAMBDA, mask=mask, advantages=adv,
                               returns=ret, moments=mom, stream=stream)

    def eager():
        eager_gae(reward, done, value, bootstrap, mask, adv_e, ret_e, mom_e)

    nbytes = T * R * (4 + 4 + value.element_size() + (4 if with_mask else 0) + 4 + 4) + R * value.element_size()
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    variants = {"fused": fused, "eager": eager, "copy": lambda: dst.copy_(src)}      # the copy moves nbytes: half read, half written
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(adv.view(torch.int32), adv_e.view(torch.int32)) and torch.equal(ret.view(torch.int32), ret_e.view(torch.int32)))
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    name = f"{str(dtype).replace('torch.', '')}{'/mask' if with_mask else ''}{'/moments' if with_moments else ''}"
    res = {"variant": name, "rows": R, "steps": T, "algorithmic_bytes": nbytes, "eager_equals_fused_bit_for_bit": same}
    for k, ts in times.items():
        res[k] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}
    res["fused_bytes_per_s"] = nbytes / (res["fused"]["ms"] * 1e-3)
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["fused_over_copy"] = res["fused"]["ms"] / res["copy"]["ms"]
    res["fused_faster_beyond_spread"] = bool(res["eager"]["ms"] - res["fused"]["ms"] > max(res["eager"]["spread_ms"], res["fused"]["spread_ms"]))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=16000)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gae_bench.txt"))
    args = ap.parse_args()
    sim = make_sim(args.worlds)
    results = [bench_variant(sim, dt, mask, mom, args) for dt, mask, mom in VARIANTS]
    sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "worlds": args.worlds, "agents_per_world": 6, "steps": args.steps,
            "calls_per_window": args.calls, "rounds": args.rounds}
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n")
        for r in results:
            f.write(json.dumps(r) + "\n")
        f.write("\n%-24s %10s %10s %10s %14s %13s %10s\n" % ("variant", "fused ms", "eager ms", "copy ms", "eager / fused", "fused / copy", "fused GB/s"))
        for r in results:
            f.write("%-24s %10.4f %10.4f %10.4f %14.1f %13.2f %10.0f\n" % (r["variant"], r["fused"]["ms"], r["eager"]["ms"], r["copy"]["ms"],
                                                                        r["eager_over_fused"], r["fused_over_copy"], r["fused_bytes_per_s"] / 1e9))
    if not all(r["eager"]["ms"] > r["fused"]["ms"] for r in results):
        sys.exit("the fused call is not faster than the eager loop")


if __name__ == "__main__":
    main()
