"""Time of the attention core's kernels (sim.attend_entities / attend_entities_backward, csrc/hs_k_attend.h) next to the two
forms a torch learner writes today on the same device, entity_attention.eager (einsum, softmax, einsum) and
torch.nn.functional.scaled_dot_product_attention on the transposed views, each with backward() for the update, and next
to a plain device-to-device copy of as many bytes as the kernels touch (cycling through more than 256 MB of buffers, so
that it runs at the HBM rate and not out of the last-level cache).  The GEMMs are not part of any side: all start from
the same qkv.  key_mask is None (every key counts): the most work for the kernel and the form torch's fused paths take.

    python tools/attend_bench.py [--sizes 96000,1920000] [--embed 64,128] [--calls 5] [--rounds 3] [--out profiles/entity_attention_bench.txt]

At n = 96 000 rows (one rollout step: 16 000 worlds x 6 agents) and n = 1 920 000 (a minibatch pass of 20 steps), E = 64
and 128, qkv and out in bf16 and f32, the forward alone and the forward plus the backward.  Each variant is timed with
device events around --calls enqueued calls after warm-up; kernel, eager, sdpa and copy alternate inside each of
--rounds rounds and the median window is reported with the spread (max - min) of the windows.  A torch form that runs
out of device memory, or whose launch the runtime refuses, at a size is reported as such and left out; the fused
attention is called on 32 768 rows at a time, because its kernels put the batch in a grid dimension.  Bytes touched: forward qkv read + out written;
backward qkv and grad_out read + grad_qkv written.  Before timing, the kernel's out and grad_qkv of the first 37 rows
are compared once with eager() in float64, within 4 x |eager float32 - eager float64| plus the rounding of the dtype.
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
from gpu_hideseek import entity_attention as A  # noqa: E402

COPY_CHUNK = 1 << 30      # bytes per copy call at the most; two pairs of buffers, so the copy never reads what it just wrote
ROUNDING = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8}


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


def measure(variants, calls, rounds):
    """{name: {ms, ms_windows, spread_ms} or {"error": ...}}: the variants alternate inside each round."""
    alive, failed = {}, {}
    probe = torch.zeros(1, device="cuda")
    for k, fn in variants.items():
        try:
            fn()
            fn()
            torch.cuda.synchronize()
            probe.add_(1.0)                 # a launch of torch's own: a launch error a library kernel left pending surfaces here
            torch.cuda.synchronize()
            alive[k] = fn
        except torch.cuda.OutOfMemoryError:
            failed[k] = "out of device memory"
            torch.cuda.empty_cache()
        except RuntimeError as e:
            failed[k] = str(e).splitlines()[0]
    times = {k: [] for k in alive}
    for _ in range(rounds):
        for k, fn in alive.items():
            times[k].append(window(fn, calls))
    out = {k: {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts)} for k, ts in times.items()}
    out.update({k: {"error": msg} for k, msg in failed.items()})
    return out


SDPA_ROWS = 32768         # rows per scaled_dot_product_attention call: its fused kernels put the batch in a grid dimension (65535 at the most)


def sdpa(qkv):
    """torch's fused attention on the transposed views of qkv [n, 17, 3, 4, D]: [n, 17, E], SDPA_ROWS rows per call."""
    outs = []
    for lo in range(0, qkv.shape[0], SDPA_ROWS):
        q, k, v = (qkv[lo:lo + SDPA_ROWS, :, c].transpose(1, 2) for c in range(3))
        outs.append(torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(q.shape[0], A.TOKENS, -1))
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def check(sim, dtype, E):
    g = torch.Generator(device="cuda").manual_seed(E)
    qkv = torch.randn(37, A.TOKENS, 3, A.HEADS, E // A.HEADS, device="cuda", generator=g).to(dtype)
    gout = torch.randn(37, A.TOKENS, E, device="cuda", generator=g).to(dtype)
    got = {"out": sim.attend_entities(qkv)["out"], "grad_qkv": sim.attend_entities_backward(qkv, None, gout)["grad_qkv"]}
    ref = {}
    for ft in (torch.float32, torch.float64):
        leaf = qkv.detach().to(ft).clone().requires_grad_()
        out = A.eager(leaf)
        out.backward(gout.to(ft))
        ref[ft] = {"out": out.detach().double(), "grad_qkv": leaf.grad.double()}
    ok = True
    for k in got:
        want = ref[torch.float64][k]
        tol = 4.0 * float((ref[torch.float32][k] - want).abs().max()) + ROUNDING[dtype] * want.abs()
        ok = ok and bool(((got[k].double() - want).abs() <= tol).all())
    return ok


def bench_variant(sim, n, E, dtype, back, args):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n % 1000)
    D = E // A.HEADS
    qkv = torch.empty(n, A.TOKENS, 3, A.HEADS, D, dtype=dtype, device=dev)
    for lo in range(0, n, 1 << 16):                                       # filled in pieces: randn makes float32 first
        qkv[lo:lo + (1 << 16)] = torch.randn(min(1 << 16, n - lo), A.TOKENS, 3, A.HEADS, D, device=dev, generator=g).to(dtype)
    out = torch.empty(n, A.TOKENS, E, dtype=dtype, device=dev)
    gout = gq = None
    if back:
        gout = torch.empty(n, A.TOKENS, E, dtype=dtype, device=dev).normal_(generator=g)
        gq = torch.empty_like(qkv)
    stream = torch.cuda.current_stream()
    leaf = qkv.requires_grad_(True) if back else qkv

    def kernel():                         # enqueue only, like the eager ops: the events see device time
        sim.attend_entities(qkv.detach(), out=out, stream=stream)
        if back:
            sim.attend_entities_backward(qkv.detach(), None, gout, grad_qkv=gq, stream=stream)

    def torch_form(f):
        def fn():
            if back:
                leaf.grad = None
                f(leaf).to(dtype).backward(gout)
            else:
                with torch.no_grad():
                    f(qkv).to(dtype)
        return fn

    esz = qkv.element_size()
    nbytes = n * A.TOKENS * E * esz * (4 + (7 if back else 0))
    chunk = min(nbytes // 2, COPY_CHUNK)
    pairs = [(torch.empty(chunk, dtype=torch.uint8, device=dev), torch.empty(chunk, dtype=torch.uint8, device=dev)) for _ in range(2)]
    reps = -(-(nbytes // 2) // chunk)
    turn = [0]

    def copy():
        for _ in range(reps):
            src, dst = pairs[turn[0] % 2]
            turn[0] += 1
            dst.copy_(src)

    name = str(dtype).replace("torch.", "")
    res = {"variant": f"{name}/{'forward+backward' if back else 'forward'}", "n": n, "embed": E, "bytes_touched": nbytes, "copy_bytes_moved": 2 * chunk * reps}
    calls = args.calls if n > 500000 else 4 * args.calls
    res["calls_per_window"] = calls
    res.update(measure({"kernel": kernel, "eager": torch_form(A.eager), "sdpa": torch_form(sdpa), "copy": copy}, calls, args.rounds))
    k = res["kernel"]["ms"]
    forms = {f: res[f]["ms"] for f in ("eager", "sdpa") if "ms" in res[f]}
    res["kernel_bytes_per_s"] = nbytes / (k * 1e-3)
    res["kernel_over_copy"] = k / res["copy"]["ms"]
    if forms:
        best = min(forms, key=forms.get)
        res["faster_torch_form"], res["torch_over_kernel"] = best, forms[best] / k
        res["kernel_faster_beyond_both_spreads"] = forms[best] - k > max(res[best]["spread_ms"], res["kernel"]["spread_ms"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="96000,1920000")
    ap.add_argument("--embed", default="64,128")
    ap.add_argument("--dtypes", default="bfloat16,float32")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entity_attention_bench.txt"))
    args = ap.parse_args()
    sim = make_sim()
    dtypes = [getattr(torch, d) for d in args.dtypes.split(",")]
    agree = {f"{E}/{str(dt).replace('torch.', '')}": check(sim, dt, int(E)) for E in args.embed.split(",") for dt in dtypes}
    print(json.dumps({"kernel_agrees_with_float64": agree}), flush=True)
    results = []
    for n in args.sizes.split(","):
        for E in args.embed.split(","):
            for dt in dtypes:
                for back in (False, True):
                    results.append(bench_variant(sim, int(n), int(E), dt, back, args))
                    torch.cuda.empty_cache()
    sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds, "key_mask": None, "kernel_agrees_with_float64": agree}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def ms(r, k):
        return "%10.3f %8.3f" % (r[k]["ms"], r[k]["spread_ms"]) if "ms" in r[k] else "%10s %8s" % ("failed", "-")
    with open(args.out, "w") as f:
        f.write(json.dumps({"meta": meta}) + "\n")
        for r in results:
            f.write(json.dumps(r) + "\n")
        f.write("\n%-8s %-4s %-26s %10s %8s %10s %8s %10s %8s %10s %8s %15s %13s %11s\n" % (
            "n", "E", "variant", "kernel ms", "spread", "eager ms", "spread", "sdpa ms", "spread", "copy ms", "spread", "torch / kernel", "kernel / copy", "kernel GB/s"))
        for r in results:
            f.write("%-8d %-4d %-26s %s %s %s %s %15s %13.2f %11.0f\n" % (
                r["n"], r["embed"], r["variant"], ms(r, "kernel"), ms(r, "eager"), ms(r, "sdpa"), ms(r, "copy"),
                "%.1f (%s)" % (r["torch_over_kernel"], r["faster_torch_form"]) if "torch_over_kernel" in r else "-", r["kernel_over_copy"], r["kernel_bytes_per_s"] / 1e9))
    if not all(agree.values()):
        sys.exit("the kernel differs from eager() in float64 beyond the derived bound")


if __name__ == "__main__":
    main()
