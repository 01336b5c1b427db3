"""Host time of the Python in front of a learner kernel launch: what request() of a module costs per call, on tensors that
are already on the device, and one DenseNormAct forward + backward through autograd as the update loop runs it
(on_current_stream(): enqueued, not waited for).

    python tools/request_host_cost.py [--package DIR] [--label head] [--calls 3000] [--repeats 5] [--rows 64]

request() validates, allocates the outputs given as True and fills the ctypes request; nothing is launched, so the time
is the host's alone (time.perf_counter around --calls calls, --repeats windows, the median window and the spread max - min
of the windows, in microseconds per call).  The last line launches: its window ends in a synchronise.  --package names
the directory that holds the gpu_hideseek package to measure (by default this tree's); with HS_LIB_PATH set to this
tree's library, another checkout's Python is measured against the same kernels.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package", default=os.path.join(ROOT, "marl-hideandseek_amd"))
    ap.add_argument("--label", default="head")
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=64)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import torch
    import gpu_hideseek
    from gpu_hideseek import entity_encoder, mlp, policy_inputs, ppo_loss, recurrent, value_head
    from gpu_hideseek._request import on_current_stream

    sim = gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=64, sim_flags=0, rand_seed=0, min_hiders=3,
        max_hiders=3, min_seekers=3, max_seekers=3, num_pbt_policies=1)
    sim.init()
    dev, bf, n, Cn, E = torch.device("cuda", 0), torch.bfloat16, args.rows, 256, 64
    z = lambda *shape, dtype=bf: torch.zeros(*shape, dtype=dtype, device=dev)      # noqa: E731
    p_mlp, p_lstm, p_enc = z(mlp.PARAM_ROWS * Cn, dtype=torch.float32), z(recurrent.PARAM_ROWS * Cn, dtype=torch.float32), z(entity_encoder.PARAM_ROWS * E, dtype=torch.float32)
    zz, gates, c_prev, clear, rows = z(n, Cn), z(n, 4 * Cn), z(n, Cn, dtype=torch.float32), z(n, dtype=torch.int32), z(n, policy_inputs.ROW)
    logits, action, f32 = z(n, 19), z(n, 5, dtype=torch.int32), z(n, dtype=torch.float32)
    critic = z(n, 255)
    layer = mlp.DenseNormAct(Cn, Cn).to(dev)
    x, g = z(n, Cn), z(n, Cn)

    def layer_step():
        layer(sim, x).backward(g)

    cases = {
        "mlp.request": lambda: mlp.request(0, zz, p_mlp),
        "mlp.request_backward": lambda: mlp.request_backward(0, zz, p_mlp, zz),
        "recurrent.request": lambda: recurrent.request(0, gates, c_prev, p_lstm, clear=clear),
        "recurrent.request_backward": lambda: recurrent.request_backward(0, gates, c_prev, p_lstm, zz, clear=clear, grad_h_next=zz, grad_c_next=c_prev),
        "entity_encoder.request": lambda: entity_encoder.request(0, rows, p_enc, argmax=True),
        "ppo_loss.request": lambda: ppo_loss.request(0, logits, action, f32, f32, mask=f32),
        "value_head.request": lambda: value_head.request(0, critic, f32, mask=f32),
        "DenseNormAct forward + backward": layer_step,
    }
    res = {"label": args.label, "device": torch.cuda.get_device_name(0), "rows": n, "calls": args.calls, "repeats": args.repeats, "us_per_call": {}}
    with on_current_stream():
        for name, fn in cases.items():
            for _ in range(200):
                fn()
            torch.cuda.synchronize()
            windows = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                windows.append(1e6 * (time.perf_counter() - t0) / args.calls)
            res["us_per_call"][name] = {"median": statistics.median(windows), "spread": max(windows) - min(windows)}
    print(json.dumps(res), flush=True)
    sim.close()


if __name__ == "__main__":
    main()
