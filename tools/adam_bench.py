"""Time of the optimiser step (optim.Adam.step: hs_adam_step, csrc/hs_k_adam.h — the global-norm clip, the Adam update
and the zeroing of the gradients in two launches over one flat buffer) next to what a torch learner writes today on the
same 24 tensors: clip_grad_norm_ + torch.optim.Adam(foreach=True).step() + zero_grad(), the same with fused=True, and
next to a plain device-to-device copy of as many bytes as the call moves (cycling through more than 256 MB of buffers, so
that it runs at the HBM rate and not out of the last-level cache).

    python tools/adam_bench.py [--scales 1,16] [--calls 20] [--rounds 5] [--out profiles/adam_bench.txt]

At the policy's size (policy.make_policy(): 24 float32 tensors, flat length 1 532 992) and at 16 x that (the same 24
tensors with 16 x the rows each).  Each variant is timed with device events around --calls enqueued calls after warm-up;
the variants alternate inside each of --rounds rounds and the median window is reported with the spread (max - min) of the
windows.  The calls are enqueued, not waited for, so a window holds whichever is longer of the host's time to issue a call
and the device's to run it.  The torch compositions call zero_grad(set_to_none=False): the gradients have to exist for the
next call, as they do after a backward pass; with the default set_to_none=True the zeroing costs torch no kernel and the
next backward an allocation and a copy per tensor instead.  After a call the gradients are zero on every side, so every
timed call clips nothing; the kernels' work does not depend on the values.  Algorithmic bytes of the call = the gradients
read twice, parameters and both moments read once, all four written once: 36 bytes per element.
Before timing, one step of optim.Adam on random gradients is compared bit for bit with the restatement of
tests/test_optim_host.py, and one step of each torch composition with it within the tolerance derived there.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402
from gpu_hideseek import optim  # noqa: E402
from gpu_hideseek import policy as P  # noqa: E402

COPY_SET = 1 << 29        # bytes the copy baseline cycles through: twice the last-level cache
BYTES_PER_ELEMENT = 36
LR, MAX_NORM = 1e-4, 5.0


def make_sim():
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=64, sim_flags=0, rand_seed=0, min_hiders=3,
        max_hiders=3, min_seekers=3, max_seekers=3, num_pbt_policies=1)
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


def measure(variants, args):
    """{name: {ms, ms_windows, spread_ms, calls_per_window}}: the variants alternate inside each round."""
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    return {k: {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls} for k, ts in times.items()}


def tensors(scale, seed):
    """The policy's 24 parameters with `scale` x the rows each, as fresh leaves on the device: [(name, Parameter)]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for name, p in P.make_policy(fused=False, generator=g).named_parameters():
        out.append((name, torch.nn.Parameter(p.detach().repeat((scale,) + (1,) * (p.dim() - 1)).cuda())))
    return out


def torch_side(named, fused):
    params = [p for _, p in named]
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = torch.optim.Adam(params, lr=LR, **({"fused": True} if fused else {"foreach": True}))

    def call():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
        opt.step()
        opt.zero_grad(set_to_none=False)
    return params, call


def bench_scale(sim, scale, args):
    import numpy as np
    import test_optim_host as H
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    ours = tensors(scale, 1)
    opt = optim.Adam(sim, ours, lr=LR, max_grad_norm=MAX_NORM)
    n = opt.flat.params.numel()
    res = {"scale": scale, "tensors": len(ours), "elements": sum(p.numel() for _, p in ours), "flat_length": n, "algorithmic_bytes": n * BYTES_PER_ELEMENT}
    variants = {"fused_call": lambda: opt.step(stream=stream)}
    sides = {}
    for key, fused in (("torch_foreach", False), ("torch_fused", True)):
        try:
            sides[key] = torch_side(tensors(scale, 1), fused)
        except Exception as e:                                  # a torch build without the fused optimiser: said, not hidden
            res[key + "_unavailable"] = f"{type(e).__name__}: {e}"
    # one checked step on random gradients before anything is timed
    g = torch.Generator(device=dev).manual_seed(2)
    grads = torch.randn(n, device=dev, generator=g) * (20.0 / n ** 0.5)
    before = {"p": opt.flat.params, "m": opt.m, "v": opt.v}
    before = {k: t.detach().cpu().numpy().copy() for k, t in before.items()}
    lay = opt.layout()
    for lo, hi, _ in lay.values():
        opt.flat.grads[lo:hi] = grads[lo:hi]                   # the padding stays zero
    before["g"] = opt.flat.grads.cpu().numpy().copy()
    state = opt.adam_state.cpu().numpy().copy()
    for key, (params, call) in sides.items():
        for (name, _), p in zip(ours, params):
            p.data.copy_(opt.flat.view(opt.flat.params, name))
            p.grad.copy_(opt.flat.view(opt.flat.grads, name))
    stats = opt.step().clone()
    want, _, wstats = H.step(np.float32, before, state, **dict(H.HYPER, lr=LR, max_grad_norm=MAX_NORM))
    res["fused_call_is_the_restatement_bit_for_bit"] = bool(
        np.array_equal(opt.flat.params.cpu().numpy().view(np.uint32), want["p"].view(np.uint32))
        and np.array_equal(stats.cpu().numpy().view(np.uint64), wstats.view(np.uint64)))
    res["grad_norm_of_the_checked_step"] = float(wstats[0])
    for key, (params, call) in sides.items():                  # torch's first step, on the same parameters and gradients
        try:
            call()
        except Exception as e:
            res[key + "_unavailable"] = f"{type(e).__name__}: {e}"
            continue
        worst = max(float((p.detach() - opt.flat.view(opt.flat.params, name)).abs().max()) for (name, _), p in zip(ours, params))
        res[key + "_largest_difference"] = worst
        res[key + "_within_tolerance"] = worst <= H.TOL["p"]
        variants[key] = call
    esz = 4
    nbytes = n * BYTES_PER_ELEMENT
    pairs = [(torch.empty(nbytes // 2 // esz, device=dev), torch.empty(nbytes // 2 // esz, device=dev)) for _ in range(max(2, -(-COPY_SET // nbytes)))]
    turn = [0]

    def copy():
        src, dst = pairs[turn[0] % len(pairs)]
        turn[0] += 1
        dst.copy_(src)

    variants["copy"] = copy
    res["copy_buffer_pairs"] = len(pairs)
    res.update(measure(variants, args))
    res["fused_call_bytes_per_s"] = nbytes / (res["fused_call"]["ms"] * 1e-3)
    res["fused_call_over_copy"] = res["fused_call"]["ms"] / res["copy"]["ms"]
    for key in ("torch_foreach", "torch_fused"):
        if key in variants:
            res[key + "_over_fused_call"] = res[key]["ms"] / res["fused_call"]["ms"]
            res["no_longer_than_" + key] = res["fused_call"]["ms"] <= res[key]["ms"]
            res["faster_than_" + key + "_beyond_both_spreads"] = res[key]["ms"] - res["fused_call"]["ms"] > max(res[key]["spread_ms"], res["fused_call"]["spread_ms"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scales", default="1,16")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_bench.txt"))
    args = ap.parse_args()
    sim = make_sim()
    results = []
    for scale in args.scales.split(","):
        results.append(bench_scale(sim, int(scale), args))
        torch.cuda.empty_cache()
    sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "calls_per_window": args.calls, "rounds": args.rounds, "lr": LR,
            "max_grad_norm": MAX_NORM, "tolerance_p": __import__("test_optim_host").TOL["p"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    cell = lambda r, k: ("%10.4f %8.4f" % (r[k]["ms"], r[k]["spread_ms"])) if k in r else "%10s %8s" % ("-", "-")      # noqa: E731
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n")
        for r in results:
            f.write(json.dumps(r) + "\n")
        f.write("\n%-11s %10s %8s %10s %8s %10s %8s %10s %8s %15s %13s %12s %10s\n" % (
            "flat length", "call ms", "spread", "foreach ms", "spread", "fused ms", "spread", "copy ms", "spread", "foreach / call", "fused / call",
            "call / copy", "call GB/s"))
        for r in results:
            f.write("%-11d %s %s %s %s %15.1f %13.1f %12.2f %10.0f\n" % (
                r["flat_length"], cell(r, "fused_call"), cell(r, "torch_foreach"), cell(r, "torch_fused"), cell(r, "copy"),
                r.get("torch_foreach_over_fused_call", float("nan")), r.get("torch_fused_over_fused_call", float("nan")), r["fused_call_over_copy"],
                r["fused_call_bytes_per_s"] / 1e9))
    if not all(r["fused_call_is_the_restatement_bit_for_bit"] for r in results):
        sys.exit("optim.Adam.step differs from the restatement")


if __name__ == "__main__":
    main()
