"""Time of the policy-input pack (sim.pack_policy_inputs, csrc/hs_k_pack.h) next to the same rows composed from torch
eager ops on the exports, and next to a plain device-to-device copy of as many bytes.

    python tools/pack_bench.py [--worlds 16000] [--calls 200] [--rounds 3] [--json out.json]

At --worlds x (2+2) and x (3+3) agents, after 120 steps of the benchmark action stream: actor-bf16, critic-bf16,
actor+critic-bf16 without and with moments, actor+critic-f32, and actor+critic-bf16 normalised (normaliser=table of a real
update) without and with moments, whose eager composition is f32 rows -> (x - mu) * inv -> mask -> cast.  The time of
hs_obs_norm_update is reported once per team size, for 1 and 40 moment vectors.  Each variant is timed with device events around --calls
calls after warm-up; fused, eager and copy alternate inside each of --rounds rounds and the median window is reported
with the spread (max - min) of the windows.  The fused and the eager rows are compared bit for bit once.  Algorithmic
bytes = every input the variant needs read once + every output written once; bytes/s = that over the fused time.
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
from gpu_hideseek import policy_inputs as P  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12      # HBM3E, specification
SELF = ("prep_counter", "self_data", "self_type", "lidar")


def make_sim(n, agents, steps=120):
    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=0, rand_seed=0, min_hiders=agents,
        max_hiders=agents, min_seekers=agents, max_seekers=agents, num_pbt_policies=1)
    sim.init()
    act = sim.action_tensor().to_torch()
    g = torch.Generator(device=act.device).manual_seed(0)
    for _ in range(steps):
        act[:, 0:2] = torch.randint(-5, 5, (act.shape[0], 2), device=act.device, dtype=torch.int32, generator=g)
        sim.step()
    return sim


def exports(sim):
    names = SELF + tuple(P.MASKS) + tuple(P.MASKS.values()) + ("self_mask",)
    return {n: getattr(sim, n + "_tensor")().to_torch() for n in names}


def eager_rows(t, actor, dtype):
    """What a torch user writes today: cat, *, .to."""
    R = t["self_data"].shape[0]
    cols = [t["prep_counter"].reshape(R, 1).float() / 96.0, t["self_data"].reshape(R, -1), t["self_type"].reshape(R, 1).float(),
            t["lidar"].reshape(R, -1)]
    for d, m in P.MASKS.items():
        x = t[d].reshape(R, -1, P.LAYOUT[d][2][1])
        cols.append((x * t[m].reshape(R, -1, 1) if actor else x).reshape(R, -1))
    return torch.cat(cols, 1).to(dtype)


def eager_normalised(t, table, actor, critic, dtype):
    """The normalised rows from eager ops: the f32 critic rows, (x - mu) * inv, the actor's masks, the cast."""
    R = t["self_data"].shape[0]
    y = (eager_rows(t, False, torch.float32) - table[:P.ROW]) * table[P.ROW:]
    res = {}
    if critic:
        res["critic"] = y.to(dtype)
    if actor:
        ones = torch.ones(R, P.LAYOUT["agent_data"][0], device=y.device)
        masks = [t[m].reshape(R, -1).repeat_interleave(P.LAYOUT[d][2][1], dim=1) for d, m in P.MASKS.items()]
        res["actor"] = (y * torch.cat([ones] + masks, 1)).to(dtype)
    return res


def eager_moments(t):
    x = eager_rows(t, False, torch.float64)
    m = t["self_mask"].reshape(-1, 1).double()
    mx = m * x
    return torch.cat([mx.sum(0), (mx * x).sum(0), m.sum().reshape(1)])


def algorithmic_bytes(t, actor, critic, moments, dtype):
    R = t["self_data"].shape[0]
    read = sum(t[n].numel() * 4 for n in SELF + tuple(P.MASKS))
    if actor:
        read += sum(t[m].numel() * 4 for m in P.MASKS.values())
    if moments:
        read += t["self_mask"].numel() * 4
    size = torch.empty(0, dtype=dtype).element_size()
    return read + (int(actor) + int(critic)) * R * P.ROW * size + (P.MOMENTS * 8 if moments else 0)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls      # ms per call


def bench_variant(sim, t, name, actor, critic, moments, dtype, args, table=None):
    R = t["self_data"].shape[0]
    dev = t["self_data"].device
    out = {k: torch.empty(R, P.ROW, dtype=dtype, device=dev) for k, on in (("actor", actor), ("critic", critic)) if on}
    if moments:
        out["moments"] = torch.empty(P.MOMENTS, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream()
    norm = {} if table is None else {"normaliser": table}      # (the keyword only where it is used)

    def fused():                          # enqueue only, like the eager ops: the events see device time
        sim.pack_policy_inputs(out.get("actor"), out.get("critic"), out.get("moments"), stream=stream, **norm)

    def eager():
        res = {}
        if table is not None:
            res = eager_normalised(t, table, actor, critic, dtype)
        elif actor:
            res["actor"] = eager_rows(t, True, dtype)
        if critic and table is None:
            res["critic"] = eager_rows(t, False, dtype)
        if moments:
            res["moments"] = eager_moments(t)
        return res

    nbytes = algorithmic_bytes(t, actor, critic, moments, dtype) + (0 if table is None else table.numel() * 4)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    variants = {"fused": fused, "eager": eager, "copy": lambda: dst.copy_(src)}      # the copy moves nbytes: half read, half written
    for fn in variants.values():
        for _ in range(5):
            fn()
    ref = eager()
    fused()
    torch.cuda.synchronize()
    same = all(torch.equal(out[k].view(torch.int16 if dtype != torch.float32 else torch.int32),
                           ref[k].view(torch.int16 if dtype != torch.float32 else torch.int32)) for k in ("actor", "critic") if k in out)
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, args.calls))
    res = {"variant": name, "rows": R, "dtype": str(dtype).replace("torch.", ""), "algorithmic_bytes": nbytes,
           "fused_equals_eager_bits": bool(same)}
    if moments:
        res["moments_max_rel_diff_vs_eager"] = float(((out["moments"] - ref["moments"]).abs() / ref["moments"].abs().clamp(min=1e-300)).max())
    for k, ts in times.items():
        res[k] = {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}
    res["fused_bytes_per_s"] = nbytes / (res["fused"]["ms"] * 1e-3)
    res["fused_share_of_8TBps_peak"] = res["fused_bytes_per_s"] / PEAK_BYTES_PER_S
    res["copy_bytes_per_s"] = nbytes / (res["copy"]["ms"] * 1e-3)
    res["eager_over_fused"] = res["eager"]["ms"] / res["fused"]["ms"]
    res["fused_faster_beyond_spread"] = bool(res["eager"]["ms"] - res["fused"]["ms"] > max(res["eager"]["spread_ms"], res["fused"]["spread_ms"]))
    print(json.dumps(res), flush=True)
    return res


def bench_norm_update(sim, name, moments, args):
    """hs_obs_norm_update over `moments` [K, 593], enqueued on the current stream: ms per call."""
    norm = P.ObsNormaliser(sim.gpu_id)
    stream = torch.cuda.current_stream()

    def update():
        norm.update(sim, moments, stream=stream)
    for _ in range(5):
        update()
    ts = [window(update, args.calls) for _ in range(args.rounds)]
    res = {"variant": name, "num_moments": int(moments.shape[0]),
           "fused": {"ms": statistics.median(ts), "ms_windows": ts, "spread_ms": max(ts) - min(ts), "calls_per_window": args.calls}}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=16000)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    bf16, f32 = torch.bfloat16, torch.float32
    cases = [("actor_bf16", True, False, False, bf16), ("critic_bf16", False, True, False, bf16),
             ("actor_critic_bf16", True, True, False, bf16), ("actor_critic_bf16_moments", True, True, True, bf16),
             ("actor_critic_f32", True, True, False, f32)]
    results = []
    for agents in (2, 3):
        sim = make_sim(args.worlds, agents)
        t = exports(sim)
        for c in cases:
            r = bench_variant(sim, t, f"{agents}+{agents}/{c[0]}", *c[1:], args)
            results.append(r)
        mom = sim.pack_policy_inputs(moments=True)["moments"]
        norm = P.ObsNormaliser(0, decay=0.9)
        norm.update(sim, mom)
        for c in (("actor_critic_bf16_normalised", True, True, False, bf16), ("actor_critic_bf16_normalised_moments", True, True, True, bf16)):
            results.append(bench_variant(sim, t, f"{agents}+{agents}/{c[0]}", *c[1:], args, table=norm.table))
        for k in (1, 40):
            results.append(bench_norm_update(sim, f"{agents}+{agents}/norm_update_{k}", mom.repeat(k, 1), args))
        sim.close()
    meta = {"device": torch.cuda.get_device_name(0), "worlds": args.worlds, "calls_per_window": args.calls, "rounds": args.rounds}
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"meta": meta, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
