"""What the dynamic loss scale (gpu_hideseek.optim.LossScale; csrc/hs_k_loss_scale.h) costs and what it buys.

    python tools/loss_scale_bench.py [--parent-lib PATH] [--worlds 16000] [--rounds 5] [--out profiles/loss_scale_bench.txt]

Cost.  hs_adam_step_scaled next to hs_adam_step at the policy's flat length (1 532 992 elements: the scaled step moves the
same bytes plus 64), and hs_ppo_loss_scaled / hs_twohot_value_scaled next to hs_ppo_loss / hs_twohot_value at 960 000
bfloat16 samples (one minibatch of 16 000 worlds x 6 agents x 40 steps in 2 minibatches, rounded).  With --parent-lib, a
libhideseek.so built from the parent commit, the same unscaled entry points of that library are timed beside them through
a handle of their own.  Each variant is timed with device events around a window of enqueued calls, sized after a warm-up
of every variant so that it lasts at least half a second; the variants alternate inside each of --rounds rounds, and the
median window is reported with the spread (max - min) of the windows.
Gain.  One minibatch of a rollout of --worlds worlds (T = 40, K = 8, 2 minibatches) collected by a float32 trainer whose
critic head is moved off its zero initialisation (so that the critic's backbone has a gradient); the same parameters,
buffers and index then go through forward_backward of a float16 trainer without a scale, of one with the dynamic scale
(its gradient divided by the scale; where the gradient overflows, the optimiser's skipped step halves the scale and the
minibatch is run again, as the update loop would with the next one: the scale that held is reported), and of a bfloat16
trainer.  Per parameter tensor: the relative L2 error of the flat gradient against the float32 trainer's, and the share
of entries that are exactly zero where the float32 gradient is not.  Recorded, not asserted.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-hideandseek_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import gpu_hideseek  # noqa: E402
from gpu_hideseek import _native, optim, ppo_loss, trainer, value_head  # noqa: E402

POLICY_FLAT = 1532992
SAMPLES = 960000
WINDOW_MS = 500.0


def make_sim(worlds=64):
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=worlds, sim_flags=0, rand_seed=0, min_hiders=3,
        max_hiders=3, min_seekers=3, max_seekers=3, num_pbt_policies=1)
    sim.init()
    return sim


class ParentLib:
    """The unscaled entry points of another build of the library, on a handle of its own."""

    def __init__(self, path):
        self.L = L = C.CDLL(path)
        L.hs_create.argtypes = [C.POINTER(_native.HsConfig), C.POINTER(C.c_void_p)]
        for fn in ("hs_adam_step_async", "hs_ppo_loss_async", "hs_twohot_value_async"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.hs_init.argtypes = L.hs_destroy.argtypes = [C.c_void_p]
        L.hs_destroy.restype = None
        L.hs_last_error.restype = C.c_char_p
        cfg = _native.HsConfig(exec_mode=1, gpu_id=0, num_worlds=64, sim_flags=0, rand_seed=0, min_hiders=3, max_hiders=3, min_seekers=3, max_seekers=3,
                               num_pbt_policies=1)
        cfg.exec_mode = int(gpu_hideseek.madrona.ExecMode.CUDA)
        self.h = C.c_void_p()
        self.check(L.hs_create(C.byref(cfg), C.byref(self.h)))
        self.check(L.hs_init(self.h))

    def check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.hs_last_error().decode())

    def call(self, fn, req):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return lambda: self.check(getattr(self.L, fn + "_async")(self.h, stream, C.byref(req)))

    def close(self):
        self.L.hs_destroy(self.h)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(variants, rounds):
    """{name: {us, spread_us, calls_per_window}}: a warm-up of every variant, windows of at least WINDOW_MS, the variants
    alternating inside each round."""
    for fn in variants.values():
        window(fn, 20)
    calls = {k: max(20, int(200 * WINDOW_MS / window(fn, 200)) + 1) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(1e3 * window(fn, calls[k]) / calls[k])
    return {k: {"us": statistics.median(ts), "spread_us": max(ts) - min(ts), "windows_us": ts, "calls_per_window": calls[k]} for k, ts in times.items()}


def bench_adam(sim, parent, rounds):
    dev, n = torch.device("cuda", 0), POLICY_FLAT
    stream = torch.cuda.current_stream()

    def buffers():
        g = torch.Generator(device=dev).manual_seed(1)
        return [torch.randn(n, device=dev, generator=g) for _ in range(2)] + [torch.zeros(n, device=dev), torch.zeros(n, device=dev)], optim.fresh_state(dev)
    variants = {}
    for name, scale in (("hs_adam_step", None), ("hs_adam_step_scaled", optim.LossScale(dev))):
        (p, g, m, v), state = buffers()
        stats = torch.zeros(4, dtype=torch.float64, device=dev)
        _, req = optim.request(0, p, g, m, v, state, stats=stats, loss_scale=scale)
        variants[name] = (lambda req=req, scale=scale: optim._step(sim, req, scale, stream))
        variants[name].keep = (p, g, m, v, state, stats, scale)
    if parent is not None:
        (p, g, m, v), state = buffers()
        _, req = optim.request(0, p, g, m, v, state, stats=None)
        variants["hs_adam_step (parent)"] = parent.call("hs_adam_step", req)
        variants["hs_adam_step (parent)"].keep = (p, g, m, v, state, req)
    return measure(variants, rounds)


def bench_losses(sim, parent, rounds):
    dev, n = torch.device("cuda", 0), SAMPLES
    stream = torch.cuda.current_stream()
    g = torch.Generator(device=dev).manual_seed(2)
    logits = torch.randn(n, 19, device=dev, generator=g).to(torch.bfloat16)
    action = torch.randint(0, 2, (n, 5), device=dev, generator=g, dtype=torch.int32)
    old, adv = torch.randn(n, device=dev, generator=g) * 0.1 - 5.0, torch.randn(n, device=dev, generator=g)
    mask = (torch.rand(n, device=dev, generator=g) < 0.8).float()
    critic = torch.randn(n, 255, device=dev, generator=g).to(torch.bfloat16)
    returns = torch.randn(n, device=dev, generator=g)
    state = optim.LossScale(dev).state
    variants, keep = {}, []
    for scaled in (False, True):
        ls = state if scaled else None
        res, req = ppo_loss.request(0, logits, action, old, adv, mask=mask, loss_scale=ls)
        res2, req2 = value_head.request(0, critic, returns, mask=mask, value=None, loss_scale=ls)
        keep += [res, req, res2, req2]
        extra = (C.c_void_p(state.data_ptr()),) if scaled else ()
        suffix = "_scaled" if scaled else ""
        variants["hs_ppo_loss" + suffix] = (lambda req=req, fn="hs_ppo_loss" + suffix, extra=extra: ppo_loss._run(sim, fn, req, stream, *extra))
        variants["hs_twohot_value" + suffix] = (lambda req=req2, fn="hs_twohot_value" + suffix, extra=extra: value_head._run(sim, fn, req, stream, *extra))
        if parent is not None and not scaled:
            res3, req3 = ppo_loss.request(0, logits, action, old, adv, mask=mask)
            res4, req4 = value_head.request(0, critic, returns, mask=mask, value=None)
            keep += [res3, req3, res4, req4]
            variants["hs_ppo_loss (parent)"] = parent.call("hs_ppo_loss", req3)
            variants["hs_twohot_value (parent)"] = parent.call("hs_twohot_value", req4)
    out = measure(variants, rounds)
    del keep
    return out


def gradient_fidelity(worlds):
    """Per variant and parameter tensor: (relative L2 error against the float32 trainer's gradient, share of entries that
    are exactly zero where the float32 gradient is not)."""
    sim = make_sim(worlds)
    try:
        base = trainer.Trainer(sim, trainer.TrainConfig())
        with torch.no_grad():
            base.net.critic_head.weight.copy_(0.05 * torch.randn(base.net.critic_head.weight.shape, generator=torch.Generator().manual_seed(3)))
        base.collect()
        index = next(iter(trainer.rollout.epoch_parts(base.permutation(), base.cfg.num_minibatches))).clone()
        base.forward_backward(index)
        ref = base.opt.flat.grads.double().clone()
        layout = base.opt.layout()
        out, scales = {}, {}
        for name, dtype, scale in (("float16", torch.float16, None), ("float16, dynamic", torch.float16, "dynamic"), ("bfloat16", torch.bfloat16, None)):
            tr = trainer.Trainer(sim, trainer.TrainConfig(dtype=dtype, loss_scale=scale))
            with torch.no_grad():
                tr.opt.flat.params.copy_(base.opt.flat.params)
                for k, t in vars(base.rollout).items():
                    if isinstance(t, torch.Tensor):
                        getattr(tr.rollout, k).copy_(t)
                tr.adv_moments.copy_(base.adv_moments)
                if tr.normaliser is not None:
                    tr.normaliser.load_state_dict(base.normaliser.state_dict())
            tr.forward_backward(index)
            while tr.opt.loss_scale is not None and not torch.isfinite(tr.opt.flat.grads).all().item():
                tr.opt.step()                                 # skipped: nothing moves, the gradients are zeroed, the scale is halved
                tr.forward_backward(index)
            S = 1.0 if tr.opt.loss_scale is None else tr.opt.loss_scale.state[0].item()
            scales[name] = S
            got = tr.opt.flat.grads.double() / S
            rows = {}
            for pname, (lo, hi, _) in layout.items():
                r, x = ref[lo:hi], got[lo:hi]
                live = r != 0
                rows[pname] = (((x - r).pow(2).sum().sqrt() / r.pow(2).sum().sqrt()).item(), (((x == 0) & live).sum() / live.sum().clamp(min=1)).item())
            r, x = ref, got
            rows["all"] = (((x - r).pow(2).sum().sqrt() / r.pow(2).sum().sqrt()).item(), (((x == 0) & (r != 0)).sum() / (r != 0).sum()).item())
            out[name] = rows
            del tr
            torch.cuda.empty_cache()
        return {"worlds": worlds, "samples": int(index.numel()) * base.rollout.chunk_steps, "variants": out, "scale": scales}
    finally:
        sim.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="a libhideseek.so built from the parent commit: its unscaled entry points are timed too")
    ap.add_argument("--worlds", type=int, default=16000, help="worlds of the rollout of the gradient comparison; 0 leaves it out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_scale_bench.txt"))
    args = ap.parse_args()
    sim = make_sim()
    parent = ParentLib(args.parent_lib) if args.parent_lib else None
    timed = {"optimiser step, %d elements" % POLICY_FLAT: bench_adam(sim, parent, args.rounds),
             "loss kernels, %d bfloat16 samples, masked" % SAMPLES: bench_losses(sim, parent, args.rounds)}
    if parent is not None:
        parent.close()
    sim.close()
    torch.cuda.empty_cache()
    fidelity = gradient_fidelity(args.worlds) if args.worlds else None
    meta = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds, "window_ms_at_least": WINDOW_MS,
            "parent_lib": bool(args.parent_lib)}
    lines = [json.dumps({"meta": meta}), json.dumps({"timed": timed}), json.dumps({"fidelity": fidelity}), ""]
    for title, rows in timed.items():
        lines.append(title)
        lines.append("  %-28s %10s %10s %8s" % ("entry point", "us / call", "spread", "calls"))
        for k, r in rows.items():
            lines.append("  %-28s %10.2f %10.2f %8d" % (k, r["us"], r["spread_us"], r["calls_per_window"]))
        lines.append("")
    if fidelity:
        names = list(fidelity["variants"])
        lines.append("gradient of one minibatch (%d samples of a %d-world rollout) against the float32 trainer's: relative L2 error, share flushed to 0" % (
            fidelity["samples"], fidelity["worlds"]))
        lines.append("  the scale that held: " + ", ".join("%s %g" % (n, fidelity["scale"][n]) for n in names))
        lines.append("  %-44s " % "parameter" + " ".join("%24s" % n for n in names))
        for pname in fidelity["variants"][names[0]]:
            lines.append("  %-44s " % pname + " ".join("%14.3e %8.2f%%" % (fidelity["variants"][n][pname][0], 100 * fidelity["variants"][n][pname][1]) for n in names))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
