"""Time of the action sampler (sim.sample_actions, csrc/hs_k_sample.h) next to the same outputs composed from torch eager
ops on the same device, and next to a plain device-to-device copy of as many bytes.

    python tools/sample_bench.py [--worlds 16000] [--calls 200] [--rounds 3] [--out profiles/sample_bench.txt]

At --worlds x (3+3) agents: draws in place into action_tensor() with log_prob and entropy, from f32, bf16 and f16 logits,
for the buckets [5,5,5,2,2] and [11,11,11,2,2].  The eager composition is what a torch learner writes today: per head
log_softmax, an inverse-CDF draw from a supplied uniform (cumsum of the probabilities, count of the edges at or below
u), gather, entropy, the sums over the heads and the copy into action_tensor().  Each variant is timed with device events
around --calls calls after warm-up; fused, eager and copy alternate inside each of --rounds rounds and the median window
is reported with the spread (max - min) of the windows.  Algorithmic bytes = the logits read once + action, log_prob and
entropy written once.  The two draw from different uniforms, so the actions are not compared; the fused log_prob is
compared with log_softmax at the fused action once.
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

BUCKETS = ((5, 5, 5, 2, 2), (11, 11, 11, 2, 2))
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def make_sim(n, agents=3):
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=0, rand_seed=0, min_hiders=agents,
        max_hiders=agents, min_seekers=agents, max_seekers=agents, num_pbt_policies=1)
    sim.init()
    return sim


def eager_sample(logits, buckets, u, action):
    """(log_prob, entropy) of a draw from `u` [R, 5], the actions copied into `action`."""
    acts, lps, ents = [], [], []
    off = 0
    for h, K in enumerate(buckets):
        lsm = torch.log_softmax(logits[:, off:off + K].float(), dim=1)
        p = lsm.exp()
        a = (p.cumsum(1) <= u[:, h:h + 1]).sum(1).clamp(max=K - 1)
        acts.append(a)
        lps.append(lsm.gather(1, a[:, None])[:, 0])
        ents.append(-(p * lsm).sum(1))
        off += K
    action.copy_(torch.stack(acts, 1))
    return torch.stack(lps, 1).sum(1), torch.stack(ents, 1).sum(1)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls      # ms per call


def bench_variant(sim, buckets, dtype, args):
    R, L = sim.num_worlds * sim.agents_per_world, sum(buckets)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(L)
    logits = (2.0 * torch.randn(R, L, device=dev, generator=g)).to(dtype)
    u = torch.rand(R, 5, device=dev, generator=g)
    action = sim.action_tensor().to_torch()
    lp, ent = torch.empty(R, device=dev), torch.empty(R, device=dev)
    stream = torch.cuda.current_stream()
    count = [0]

    def fused():                          # enqueue only, like the eager ops: the events see device time
        count[0] += 1
        sim.sample_actions(logits, buckets=buckets, seed=(1, 2), counter=count[0], log_prob=lp, entropy=ent, stream=stream)

    def eager():
        return eager_sample(logits, buckets, u, action)

    nbytes = R * (L * logits.element_size() + 5 * 4 + 2 * 4)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    variants = {"fused": fused, "eager": eager, "copy": lambda: dst.copy_(src)}      # the copy moves nbytes: half read, half written
    for fn in variants.values():
        for _ in range(5):
            fn()
    fused()
    torch.cuda.synchronize()
    off, want = 0, torch.zeros(R, device=dev)
    for h, K in enumerate(buckets):
        want += torch.log_softmax(logits[:, off:off + K].float(), dim=1).gather(1, action[:, h:h + 1].long())[:, 0]
        off += K
    diff = float((lp - want).abs().max())
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    res = {"variant": f"k{buckets[0]}/{str(dtype).replace('torch.', '')}", "rows": R, "logits_per_row": L, "algorithmic_bytes": nbytes,
           "log_prob_max_diff_vs_log_softmax": diff}
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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.txt"))
    args = ap.parse_args()
    sim = make_sim(args.worlds)
    results = [bench_variant(sim, b, d, args) for b in BUCKETS for d in DTYPES]
    sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "worlds": args.worlds, "agents_per_world": 6, "calls_per_window": args.calls,
            "rounds": args.rounds}
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n")
        for r in results:
            f.write(json.dumps(r) + "\n")
        f.write("\n%-14s %10s %10s %10s %14s\n" % ("variant", "fused ms", "eager ms", "copy ms", "eager / fused"))
        for r in results:
            f.write("%-14s %10.4f %10.4f %10.4f %14.1f\n" % (r["variant"], r["fused"]["ms"], r["eager"]["ms"], r["copy"]["ms"], r["eager_over_fused"]))


if __name__ == "__main__":
    main()
