"""Agent-view depth / RGB (Manager::depthTensor / rgbTensor, src/mgr.cpp:1241-1263): k_render through the C ABI against
the CPU restatement — BIT-EXACT for the f32 depth and the u8 colours (the ray caster is trace_ray, the shading is
IEEE +,*,min,max in a fixed order on both sides).  Parity unpinned against Madrona's renderer, which is absent from the
reference snapshot; what the image must show follows from first-party source in tests/test_oracle_render.py."""
import numpy as np
import pytest

from lockstep import EXT_RENDER, Pair

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg", [
    dict(n=24, flags=0, seed=3, hiders=(2, 2), seekers=(2, 2), W=64, H=64, mode="bench"),
    dict(n=10, flags=13, seed=5, hiders=(3, 3), seekers=(3, 3), W=32, H=16, mode="full"),
    dict(n=21, flags=0, seed=9, hiders=(1, 3), seekers=(1, 2), W=48, H=32, mode="full"),
], ids=["bench-64x64", "train-32x16", "varteams-48x32"])
def test_render_on_request_matches_oracle(oracle, cfg):
    """sim.render() after init and after driven steps (boxes pushed around, ramps, locked / grabbed bodies)."""
    W, H = cfg["W"], cfg["H"]
    p = Pair(cfg["n"], cfg["flags"], cfg["seed"], cfg["hiders"], cfg["seekers"], render=(W, H))
    sim = p.sim
    # with the reference scripts' arguments the outputs exist and stay unwritten (scripts/benchmark.py:32,47)
    assert not sim.depth_tensor().to_torch().any() and not sim.rgb_tensor().to_torch().any()
    sim.render()
    d, c = p.check_views(W, H, "init")
    assert d.any() and (c[..., 3] == 255).any()
    for chunk in range(3):
        p.drive(40, cfg["mode"], seed=chunk, every=40)
        sim.render()
        p.check_views(W, H, f"chunk {chunk}")
    if cfg["hiders"][0] != cfg["hiders"][1]:
        mask = p.ref.tensor("self_mask").reshape(-1)
        d = sim.depth_tensor().to_torch().cpu().numpy()
        assert (mask == 0).any() and not d[mask == 0].any()


def test_render_every_step_under_the_extension_flag(oracle):
    """SimFlags.ExtRender: init and every step leave the views of the new state in the tensors — across an episode end
    (level regeneration) and a host-triggered reset — also through the stream entry point."""
    W, H = 32, 32
    p = Pair(12, EXT_RENDER, 2, render=(W, H))
    sim, ref = p.sim, p.ref
    p.check_views(W, H, "init")
    rng = np.random.default_rng(0)
    for t in range(245):
        p.act(rng.integers(0, 11, size=(p.rows, 3)), cols=(0, 1, 2))
        if t == 100:
            ref.tensor("reset")[3] = 1; p.gpu.view("reset")[3] = 1
        if t % 2:
            sim.step()
        else:
            sim.step_begin(); sim.step_end()
        ref.step()
        if t % 40 == 0 or t in (100, 101, 239, 240, 241):
            p.check_views(W, H, f"step {t}")


def test_flag_needs_the_renderer_and_default_stays_dummy(oracle):
    """ExtRender without enable_batch_renderer renders nothing; the tensors can still be taken (cpu_benchmark.py:38
    asks for rgb with the renderer off) and render() fills them on request."""
    p = Pair(4, EXT_RENDER, 1)
    p.step()
    assert not p.sim.rgb_tensor().to_torch().any()
    p.sim.render()
    p.check_views(64, 64, "on request")


def test_view_culls_lose_no_hit_over_many_worlds(oracle):
    """k_render leaves out walls and hulls that cannot be in a view and skips walls beyond the depth at which a wave's
    rays leave the walls' height range; the oracle tests every ray against everything.  1 536 views of 384 different
    levels at two moments of the episode, every pixel equal."""
    W, H = 40, 24
    p = Pair(384, 0, 77, render=(W, H))
    p.sim.render()
    p.check_views(W, H, "init")
    p.drive(130, "bench", seed=5, every=130)
    p.sim.render()
    p.check_views(W, H, "step 130")
