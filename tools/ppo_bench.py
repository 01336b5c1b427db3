"""Time of the PPO loss kernel (sim.ppo_loss, csrc/hs_k_ppo.h) next to the eager composition a torch learner writes
today — forward from log_softmax to the masked mean, then backward() — on the same device, and next to a plain
device-to-device copy of as many bytes as the call moves (cycling through 1 GiB of buffers, so that it runs at the HBM
rate and not out of the last-level cache; the fused and the eager call read the same inputs every time, which at
n = 96 000 stay in that cache).

    python tools/ppo_bench.py [--sizes 1920000,96000] [--calls 50] [--rounds 3] [--out profiles/ppo_bench.txt]

At n = 1 920 000 (a minibatch of the training configuration: 96 000 rows x 40 steps / 2) and n = 96 000, buckets
(5, 5, 5, 2, 2): logits in bf16 and f32, with and without the value term (clipped), the mask and the statistics.  The
eager composition computes in f32 on widened logits and leaves its gradients in logits.grad / value.grad.  Each variant is
timed with device events around --calls enqueued calls after warm-up; fused, eager and copy alternate inside each of
--rounds rounds and the median window is reported with the spread (max - min) of the windows.  Algorithmic bytes =
logits, action, old_log_prob, advantage (and mask, value, returns, old_value) read once + grad_logits (and grad_value)
written once.  Before timing, the fused and the eager gradients are compared once: they must agree within the
tolerances tests/test_ppo_loss_host.py derives (plus the rounding of the narrow output type); the logits of the bench
have no -inf bucket, where eager autograd gives NaN.
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

BUCKETS = (5, 5, 5, 2, 2)
CLIP, VALUE_COEF, ENTROPY_COEF = 0.2, 0.5, 0.01
COPY_SET = 1 << 30        # bytes the copy baseline cycles through: four times the last-level cache
VARIANTS = [(dt, value, mask, stats) for dt in (torch.bfloat16, torch.float32)
            for value, mask, stats in ((False, False, False), (True, False, False), (True, True, False), (True, True, True))]


def make_sim():
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=64, sim_flags=0, rand_seed=0, min_hiders=3,
        max_hiders=3, min_seekers=3, max_seekers=3, num_pbt_policies=1)
    sim.init()
    return sim


def eager_loss(logits, value, action, old_lp, adv, mask, returns, old_value, want_stats):
    """The textbook composition; returns (loss, stats or None)."""
    lg = logits.float()
    lp, ent, off = 0.0, 0.0, 0
    for h, K in enumerate(BUCKETS):
        logp = torch.log_softmax(lg[:, off:off + K], dim=1)
        lp = lp + logp.gather(1, action[:, h:h + 1])[:, 0]
        ent = ent - (logp.exp() * logp).sum(1)
        off += K
    dlp = lp - old_lp
    ratio = torch.exp(dlp)
    s1, s2 = ratio * adv, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv
    pg = -torch.minimum(s1, s2)
    per = pg - ENTROPY_COEF * ent
    vl = None
    if value is not None:
        v = value.float()
        u1, u2 = (v - returns) ** 2, ((old_value + torch.clamp(v - old_value, -CLIP, CLIP)) - returns) ** 2
        vl = 0.5 * torch.maximum(u1, u2)
        per = per + VALUE_COEF * vl
    if mask is not None:
        loss = (per * mask).sum() / mask.sum()
    else:
        loss = per.mean()
    stats = None
    if want_stats:
        with torch.no_grad():
            m = mask if mask is not None else torch.ones_like(pg)
            stats = torch.stack([(pg * m).sum(), (vl * m).sum() if vl is not None else pg.new_zeros(()), (ent * m).sum(),
                                 (((ratio - 1) - dlp) * m).sum(), ((s2 < s1) * m).sum(),
                                 ((u2 > u1) * m).sum() if vl is not None else pg.new_zeros(()), m.sum()]).double()
    return loss, stats


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls      # ms per call


def bench_variant(sim, n, dtype, with_value, with_mask, with_stats, args):
    import test_ppo_loss_host as H
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n % 1000)
    L = sum(BUCKETS)
    logits = (2.0 * torch.randn(n, L, device=dev, generator=g)).to(dtype)
    action = torch.stack([torch.randint(0, K, (n,), device=dev, generator=g) for K in BUCKETS], 1)
    action32 = action.to(torch.int32)
    adv = torch.randn(n, device=dev, generator=g)
    lg = logits.float()
    lp, off = 0.0, 0
    for h, K in enumerate(BUCKETS):
        lp = lp + torch.log_softmax(lg[:, off:off + K], dim=1).gather(1, action[:, h:h + 1])[:, 0]
        off += K
    del lg
    old_lp = lp + 0.15 * torch.randn(n, device=dev, generator=g)
    mask = (torch.rand(n, device=dev, generator=g) < 0.8).float() if with_mask else None
    value = torch.randn(n, device=dev, generator=g).to(dtype) if with_value else None
    returns = value.float() + torch.randn(n, device=dev, generator=g) if with_value else None
    old_value = value.float() + 0.3 * torch.randn(n, device=dev, generator=g) if with_value else None
    grad_logits = torch.empty(n, L, dtype=dtype, device=dev)
    grad_value = torch.empty(n, dtype=dtype, device=dev) if with_value else None
    stats = torch.empty(7, dtype=torch.float64, device=dev) if with_stats else None
    stream = torch.cuda.current_stream()
    leaf_l = logits.clone().requires_grad_(True)
    leaf_v = value.clone().requires_grad_(True) if with_value else None

    def fused():                          # enqueue only, like the eager ops: the events see device time
        sim.ppo_loss(logits, action32, old_lp, adv, mask=mask, value=value, returns=returns, old_value=old_value, clip_coef=CLIP,
                     value_loss_coef=VALUE_COEF, entropy_coef=ENTROPY_COEF, grad_logits=grad_logits, grad_value=grad_value,
                     stats=stats, stream=stream)

    def eager():
        leaf_l.grad = None
        if leaf_v is not None:
            leaf_v.grad = None
        loss, _ = eager_loss(leaf_l, leaf_v, action, old_lp, adv, mask, returns, old_value, with_stats)
        loss.backward()

    esz = logits.element_size()
    nbytes = n * (2 * L * esz + 5 * 4 + 4 + 4 + (4 if with_mask else 0) + ((2 * esz + 8) if with_value else 0))
    # The copy moves nbytes, half read and half written, and goes round enough buffer pairs (COPY_SET bytes in all) that
    # no call finds its bytes in the 256 MB last-level cache: it is a copy at the HBM rate.
    pairs = [(torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev))
             for _ in range(-(-COPY_SET // nbytes))]
    turn = [0]

    def copy():
        src, dst = pairs[turn[0] % len(pairs)]
        turn[0] += 1
        dst.copy_(src)

    variants = {"fused": fused, "eager": eager, "copy": copy}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # the two agree within the host test's tolerances (both are f32 evaluations of the same formulas), samples within
    # the ratio tolerance of a clipping edge left out
    tol = H.tolerances()
    rel, absolute = (2 * r for r in H.ROUNDING[str(dtype).replace("torch.", "")])       # both sides round to the narrow type
    with torch.no_grad():
        ratio = torch.exp(lp - old_lp).double()
        near = ((ratio - (1 - CLIP)).abs() <= tol["ratio"]) | ((ratio - (1 + CLIP)).abs() <= tol["ratio"])
        if with_value:
            near |= ((value.double() - old_value.double()).abs() - CLIP).abs() <= tol["ratio"]
        ok = ~near
        ge = leaf_l.grad.double()
        err = ((grad_logits.double() - ge).abs() - (rel * ge.abs() + absolute))[ok].max().item()
        agree = err <= 2 * tol["grad_logits"]
        if with_value:
            gve = leaf_v.grad.double()
            errv = ((grad_value.double() - gve).abs() - (rel * gve.abs() + absolute))[ok].max().item()
            agree = agree and errv <= 2 * tol["grad_value"]
    assert agree, f"fused and eager gradients differ: {err}"
    assert int(near.sum()) <= 1e-3 * n, int(near.sum())
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    name = f"{str(dtype).replace('torch.', '')}{'/value' if with_value else ''}{'/mask' if with_mask else ''}{'/stats' if with_stats else ''}"
    res = {"variant": name, "n": n, "algorithmic_bytes": nbytes, "copy_buffer_pairs": len(pairs), "fused_agrees_with_eager": bool(agree), "near_edge_left_out": int(near.sum())}
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
    ap.add_argument("--sizes", default="1920000,96000")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_bench.txt"))
    args = ap.parse_args()
    sim = make_sim()
    results = [bench_variant(sim, int(n), dt, v, m, s, args) for n in args.sizes.split(",") for dt, v, m, s in VARIANTS]
    sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "buckets": BUCKETS, "calls_per_window": args.calls, "rounds": args.rounds}
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n")
        for r in results:
            f.write(json.dumps(r) + "\n")
        f.write("\n%-9s %-28s %10s %10s %10s %14s %13s %10s\n" % ("n", "variant", "fused ms", "eager ms", "copy ms", "eager / fused", "fused / copy", "fused GB/s"))
        for r in results:
            f.write("%-9d %-28s %10.4f %10.4f %10.4f %14.1f %13.2f %10.0f\n" % (r["n"], r["variant"], r["fused"]["ms"], r["eager"]["ms"], r["copy"]["ms"],
                                                                              r["eager_over_fused"], r["fused_over_copy"], r["fused_bytes_per_s"] / 1e9))
    if not all(r["fused_faster_beyond_spread"] for r in results):
        sys.exit("the fused call is not faster than the eager composition beyond the spread of both")


if __name__ == "__main__":
    main()
