"""Spectator cameras (hs_render_cameras / sim.spectate, csrc/hs_k_spectate.h): agent-pose equivalence with k_render,
oracle parity for pitched and rolled cameras, conservative culls, first-principles geometry, no state change, replay
frames and sharded routing."""
import math

import numpy as np
import pytest

import lockstep
from lockstep import EXT_SKIP_OBSERVATIONS, Pair, bits

pytestmark = pytest.mark.gpu

CUBE, BOX, RAMP = 2, 7, 6
BOUND_R = {CUBE: math.sqrt(3.0 * 1.02), BOX: math.sqrt(17.5625 * 1.02), RAMP: math.sqrt(6.0 * 1.02),
           4: math.sqrt(3.0 * 1.02), 5: math.sqrt(3.0 * 1.02)}


def _sim(n, seed=0, flags=0, hiders=(2, 2), seekers=(2, 2), **kw):
    import gpu_hideseek
    return gpu_hideseek.HideAndSeekSimulator(
        exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, sim_flags=flags, rand_seed=seed,
        min_hiders=hiders[0], max_hiders=hiders[1], min_seekers=seekers[0], max_seekers=seekers[1], num_pbt_policies=1,
        **kw)


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(a, b, tag):
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), (tag, k, int((bits(a[k]) != bits(b[k])).sum()))


def _agent_rows(sim):
    mask = sim.self_mask_tensor().to_torch().cpu().numpy().reshape(-1)
    return np.flatnonzero(mask > 0)


def _check_agent_views(sim, W, H, tag):
    """sim.render()'s views of every active agent == spectate with agent_camera, bit for bit; hit -1 <=> sky."""
    from gpu_hideseek.spectate import agent_camera
    sim.render()
    A = sim.agents_per_world
    d = sim.depth_tensor().to_torch().cpu().numpy().reshape(-1, H, W)
    c = sim.rgb_tensor().to_torch().cpu().numpy().reshape(-1, H, W, 4)
    bodies = sim.debug_bodies()[0]
    rows = _agent_rows(sim)
    assert rows.size > 0
    cams = [agent_camera(bodies, r // A, r % A) for r in rows]
    s = _np(sim.spectate(cams, W, H, hit=True))
    assert np.array_equal(bits(s["depth"]), bits(d[rows])), (tag, "depth", int((bits(s["depth"]) != bits(d[rows])).sum()))
    assert np.array_equal(s["rgb"], c[rows]), (tag, "rgb")
    sky = (s["rgb"][..., :3] == 0).all(-1)
    assert np.array_equal(s["hit"] == -1, sky), tag
    assert np.array_equal(s["depth"] == 0, sky), tag
    return rows.size


def test_agent_pose_cameras_reproduce_the_agent_views():
    """Every active agent's view, 256 worlds with mixed team sizes, at init, after the first load-balancing deal and
    around the episode's regeneration, at 64 x 64 and 40 x 24."""
    import torch
    n = 256
    sims = {(64, 64): _sim(n, seed=31, hiders=(1, 3), seekers=(1, 3), enable_batch_renderer=True,
                           batch_render_width=64, batch_render_height=64),
            (40, 24): _sim(n, seed=31, hiders=(1, 3), seekers=(1, 3), enable_batch_renderer=True,
                           batch_render_width=40, batch_render_height=24)}
    for s in sims.values():
        s.init()
    draw, cols = lockstep.stream("full", seed=4)
    rows = n * sims[(64, 64)].agents_per_world
    checked = 0
    for t in range(242):
        if t in (0, 20, 40, 239, 240, 241):
            for (W, H), s in sims.items():
                checked += _check_agent_views(s, W, H, f"{W}x{H} after {t} steps")
        a = torch.from_numpy(np.asarray(draw(t, rows), np.int32))
        for s in sims.values():
            s.action_tensor().to_torch()[:] = a.to("cuda")
            s.step()
    assert checked > 6 * 2 * n


def _quat(yaw, pitch, roll):
    """Rotation yaw about z, then pitch about the local x axis, then roll about the local y (forward) axis, float64."""
    def q(axis, ang):
        s = math.sin(ang / 2)
        return np.array([math.cos(ang / 2)] + [s * a for a in axis])

    def mul(a, b):
        w1, x1, y1, z1 = a; w2, x2, y2, z2 = b
        return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                         w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
    r = mul(mul(q((0, 0, 1), yaw), q((1, 0, 0), pitch)), q((0, 1, 0), roll))
    return r / np.linalg.norm(r)


AGENT_WORDS, REC_WORDS = 29, 348          # hs_ckpt_agent, hs_checkpoint in 32-bit words


@pytest.mark.parametrize("level", [0, 2, 3, 4, 5, 6, 7, 8])
def test_pitched_and_rolled_cameras_match_the_oracle(oracle, level):
    """Crafted checkpoint records put the agents anywhere in the arena or up to 40 m above it, pitched down to -90
    degrees and rolled; both sides load them (the oracle restores rot verbatim).  The oracle's agent views of those
    poses equal spectate at fov 100.  A load regenerates the training level from the record (loadCheckpointSystem),
    so a debug level's own geometry does not survive it: debug levels 5 and 6, which have agents, are also compared
    as generated, before the load."""
    import torch
    from gpu_hideseek.spectate import agent_camera
    W, H = 48, 32
    n = 12
    p = Pair(n, seed=40 + level, hiders=(1, 3), seekers=(1, 3), level=level, render=(W, H))
    sim, ref = p.sim, p.ref
    A = ref.A

    def compare(tag):
        bodies = sim.debug_bodies()[0]
        rd, rc = ref.render(W, H)
        rows = [w * A + a for w in range(n) for a in range(A) if ref.tensor("self_mask")[w * A + a, 0] > 0]
        if not rows:
            return None
        cams = [agent_camera(bodies, r // A, r % A) for r in rows]
        s = _np(sim.spectate(cams, W, H))
        assert np.array_equal(bits(s["depth"]), bits(rd[rows, ..., 0])), (tag, "depth")
        assert np.array_equal(s["rgb"], rc[rows]), (tag, "rgb")
        sim.render()
        kd = sim.depth_tensor().to_torch().cpu().numpy()
        kc = sim.rgb_tensor().to_torch().cpu().numpy()
        return bool(np.array_equal(bits(kd), bits(rd)) and np.array_equal(kc, rc))

    if level in (5, 6):
        compare(f"level {level} as generated")
    ctrl, ck = sim.ckpt_ctrl_tensor().to_torch(), sim.ckpt_tensor().to_torch()
    ctrl.view(torch.int32)[:] = 1
    ref.tensor("ckpt_ctrl")[:] = 1
    sim.save_checkpoints(); ref.save_checkpoints()
    rec = ck.cpu().numpy().view(np.float32).reshape(n, REC_WORDS).copy()
    assert np.array_equal(rec.view(np.uint8), ref.tensor("ckpt"))
    ints = rec.view(np.int32)
    rng = np.random.default_rng(100 + level)
    written = {}
    for w in range(n):
        if ints[w, 344] + ints[w, 345] == 0:                                # debug levels without agents
            ints[w, 344], ints[w, 345] = 1 + w % 3, 1 + (w // 3) % 3       # numHiders, numSeekers
        for a in range(ints[w, 344] + ints[w, 345]):
            base = 5 + AGENT_WORDS * a
            pos = np.array([rng.uniform(-15, 15), rng.uniform(-15, 15), rng.uniform(0.5, 40.0)], np.float32)
            pitch = -math.pi / 2 if a == 0 else rng.uniform(-math.pi / 2, 0)
            q = _quat(rng.uniform(-math.pi, math.pi), pitch, rng.uniform(-math.pi, math.pi)).astype(np.float32)
            rec[w, base:base + 3], rec[w, base + 3:base + 7] = pos, q
            rec[w, base + 7:base + 13] = 0                                    # at rest
            written.setdefault(w, []).append(np.concatenate([pos, q]))
    ck.copy_(torch.from_numpy(rec.view(np.uint8)).to(ck.device))
    ref.tensor("ckpt")[:] = rec.view(np.uint8)
    ctrl.view(torch.int32)[:] = 1
    ref.tensor("ckpt_ctrl")[:] = 1
    sim.load_checkpoints(); ref.load_checkpoints()
    p.check(f"level {level} loaded", names=(), bodies=True, walls=True)
    bodies = sim.debug_bodies()[0]
    for w, poses in written.items():
        have = [bits(bodies[w, 11 + a, :7]).tobytes() for a in range(6)]
        for pq in poses:
            assert bits(pq.astype(np.float32)).tobytes() in have, (w, pq)
    hs_render_matches = compare(f"level {level} crafted poses")
    print(f"level {level}: hs_render equals the oracle on the crafted poses: {hs_render_matches}")


def _random_cameras(rng, worlds, count, walls=None, bodies=None):
    from gpu_hideseek.spectate import Camera, look_at, make_camera, top_down
    cams = []
    for i in range(count):
        w = int(rng.choice(worlds))
        kind = i % 6
        fov = float(rng.uniform(20, 150))
        eye = (rng.uniform(-25, 25), rng.uniform(-25, 25), rng.choice([rng.uniform(0.2, 2.4), rng.uniform(2.6, 45)]))
        if kind == 0:                                                        # any orientation
            q = rng.normal(size=4)
            cams.append(make_camera(w, eye, q / np.linalg.norm(q), fov))
        elif kind == 1:                                                      # straight down
            cams.append(top_down(w, height=float(rng.uniform(3, 45)), fov_deg=fov,
                                 centre=(rng.uniform(-20, 20), rng.uniform(-20, 20))))
        elif kind == 2:                                                      # straight up
            cams.append(look_at(w, eye, (eye[0], eye[1], eye[2] + 5), fov_deg=fov))
        elif kind == 3:                                                      # upside-down
            c = look_at(w, eye, (rng.uniform(-10, 10), rng.uniform(-10, 10), 1.0), fov_deg=fov)
            qw, qx, qy, qz = np.asarray(c.rot, np.float64)
            # roll by 180 degrees about the local forward axis: q * (0, 0, 1, 0)
            cams.append(make_camera(w, c.pos, (-qy, -qz, qw, qx), fov))
        elif kind == 4 and bodies is not None:                               # inside a box
            b = bodies[w, int(rng.integers(0, 2))]
            cams.append(make_camera(w, b[:3] + rng.uniform(-0.3, 0.3, 3), _quat(*rng.uniform(-3, 3, 3)), fov))
        else:                                                                # along the floor, level or tilted
            cams.append(look_at(w, eye, (rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(-1, 3)), fov_deg=fov))
        assert isinstance(cams[-1], Camera)
    return cams


def test_culls_lose_no_hit():
    """300 seeded cameras over training levels and debug levels 7 and 8 (extra planes): culled == HS_SPECTATE_NO_CULL
    bit for bit, over odd and even sizes."""
    rng = np.random.default_rng(2024)
    sims = [_sim(16, seed=12, hiders=(1, 3), seekers=(1, 3))]
    for level in (7, 8):
        s = _sim(4, seed=13)
        s.reset_tensor().to_torch()[:] = level
        sims.append(s)
    for s in sims:
        s.init()
    for _ in range(30):
        sims[0].step()
    sizes = [(64, 64), (63, 17), (1, 1), (7, 129), (128, 96), (33, 34)]
    total = 0
    for k, (W, H) in enumerate(sizes):
        s = sims[0] if k % 2 == 0 else sims[1 + (k // 2) % 2]
        cams = _random_cameras(rng, range(s.num_worlds), 50, bodies=s.debug_bodies()[0])
        a = _np(s.spectate(cams, W, H, hit=True))
        b = _np(s.spectate(cams, W, H, hit=True, exact=True))
        _same(a, b, f"{W}x{H}")
        assert (a["hit"] >= 0).any()
        total += len(cams)
    assert total == 300


def test_top_down_first_principles():
    """Odd-sized top-down cameras: the centre pixel looks straight down, so its depth is the height above what lies
    under the camera (to the float32 pose's few ulps) and its hit is that object; in an overview of the arena the
    projected centres of wall tops and box tops hit those walls and boxes."""
    from gpu_hideseek.spectate import top_down
    n = 8
    sim = _sim(n, seed=21, hiders=(1, 3), seekers=(1, 3))
    sim.init()
    walls, info = sim.debug_walls()
    bodies, meta = sim.debug_bodies()
    W = H = 101
    h = 30.0

    def walls_at(w, x, y, grow=0.0):
        k = [i for i in range(info[w, 0]) if abs(x - walls[w, i, 0]) <= walls[w, i, 2] + grow
             and abs(y - walls[w, i, 1]) <= walls[w, i, 3] + grow]
        return k

    def bodies_near(w, x, y, skip=-1):
        return [b for b in range(17) if b != skip and meta[w, b, 0] in BOUND_R
                and math.hypot(x - bodies[w, b, 0], y - bodies[w, b, 1]) <= BOUND_R[meta[w, b, 0]] + 0.2]

    def centre(cams):
        r = _np(sim.spectate(cams, W, H, hit=True))
        return r["depth"][:, H // 2, W // 2], r["hit"][:, H // 2, W // 2]

    checks = {"wall": 0, "box": 0, "floor": 0}
    for w in range(n):
        cams, want = [], []
        for k in range(info[w, 0]):
            x, y = float(walls[w, k, 0]), float(walls[w, k, 1])
            if bodies_near(w, x, y):
                continue
            cams.append(top_down(w, h, 40.0, centre=(x, y)))
            want.append((100 + min(walls_at(w, x, y)), h - 2.5))
        for b in range(11):
            if meta[w, b, 0] not in (CUBE, BOX) or abs(bodies[w, b, 4]) > 1e-6 or abs(bodies[w, b, 5]) > 1e-6:
                continue
            x, y = float(bodies[w, b, 0]), float(bodies[w, b, 1])
            if bodies_near(w, x, y, skip=b) or walls_at(w, x, y):
                continue
            cams.append(top_down(w, h, 40.0, centre=(x, y)))
            want.append((b, h - float(bodies[w, b, 2]) - 1.0))
        rng = np.random.default_rng(w)
        floor = 0
        while floor < 4:
            x, y = rng.uniform(-17, 17, 2)
            if walls_at(w, x, y, 0.1) or bodies_near(w, x, y):
                continue
            cams.append(top_down(w, h, 40.0, centre=(x, y)))
            want.append((200, h))
            floor += 1
        depth, hit = centre(cams)
        for (wid, wd), d, t in zip(want, depth, hit):
            kind = "floor" if wid == 200 else ("wall" if wid >= 100 else "box")
            if kind == "floor":
                assert t >= 200, (w, t)
            else:
                assert t == wid, (w, kind, t, wid)
            tol = 1e-5 if kind != "box" else 1e-4
            assert abs(d - wd) <= tol * wd, (w, kind, d, wd)
            checks[kind] += 1
        # the overview: project wall-top and box-top centres into one 401 x 401 image from 40 m
        S = 401
        cam = top_down(w, 40.0)
        t = float(cam.tan_half_fov_y)
        r = _np(sim.spectate([cam], S, S, hit=True))["hit"][0]

        def pixel(x, y, z):
            zc = 40.0 - z
            px = ((x / zc) / t + 1) / 2 * S - 0.5
            py = (1 - (y / zc) / t) / 2 * S - 0.5
            return int(round(py)), int(round(px))
        for k in range(info[w, 0]):
            x, y = float(walls[w, k, 0]), float(walls[w, k, 1])
            if min(walls[w, k, 2], walls[w, k, 3]) < 0.2 or bodies_near(w, x, y) or walls_at(w, x, y) != [k]:
                continue
            py, px = pixel(x, y, 2.5)
            if not (0 <= py < S and 0 <= px < S):                            # outside the view
                continue
            assert r[py, px] == 100 + k, (w, k)
            checks["wall"] += 1
        for b in range(11):
            if meta[w, b, 0] not in (CUBE, BOX) or abs(bodies[w, b, 4]) > 1e-6 or abs(bodies[w, b, 5]) > 1e-6:
                continue
            x, y, z = (float(v) for v in bodies[w, b, :3])
            if bodies_near(w, x, y, skip=b) or walls_at(w, x, y, 0.4):
                continue
            py, px = pixel(x, y, z + 1.0)
            if not (0 <= py < S and 0 <= px < S):
                continue
            assert r[py, px] == b, (w, b)
            checks["box"] += 1
    assert all(v > 0 for v in checks.values()), checks


def test_spectate_changes_nothing_and_checks_its_arguments(oracle):
    """120 lock steps with spectate calls between them stay bit-exact with the oracle; every bad argument is refused
    with the outputs untouched; duplicate and unordered worlds work; no batch renderer and skipped observations do not
    matter."""
    import ctypes as C
    import torch
    from gpu_hideseek.spectate import CAMERA_DTYPE, agent_camera, camera_array, look_at, top_down
    n = 32
    p = Pair(n, seed=3, hiders=(1, 3), seekers=(1, 3))
    sim = p.sim
    draw, cols = lockstep.stream("full", seed=7)
    for s in range(120):
        p.step(draw(s, p.rows), cols)
        cams = [top_down(s % n), look_at((s * 7) % n, (3, -4, 6), (0, 0, 0)), top_down((s * 5) % n, 12.0)]
        sim.spectate(cams, 64, 48, hit=True)
        sim.spectate(cams[:1], 17, 9, rgb=False, exact=True)
        if (s + 1) % 20 == 0:
            p.check(f"step {s}")
    # duplicate and unordered worlds
    worlds = [5, 2, 5, 0, 31, 2]
    cams = [top_down(w, 25.0) for w in worlds] + [look_at(w, (1, 2, 3), (-4, 5, 0.5)) for w in worlds]
    allv = _np(sim.spectate(cams, 40, 30, hit=True))
    for i, c in enumerate(cams):
        one = _np(sim.spectate([c], 40, 30, hit=True))
        _same({k: v[i:i + 1] for k, v in allv.items()}, one, f"camera {i}")
    # bad arguments, through Python and straight through the C ABI
    good = camera_array([top_down(1)])
    dev = torch.device("cuda", 0)
    depth = torch.full((1, 8, 8), 7.0, device=dev)
    rgb = torch.full((1, 8, 8, 4), 0xAB, dtype=torch.uint8, device=dev)
    hitb = torch.full((1, 8, 8), -7, dtype=torch.int32, device=dev)
    bufs = (depth, rgb, hitb)
    before = [b.clone() for b in bufs]

    def bad_cam(**kv):
        a = good.copy()
        for k, v in kv.items():
            a[k][0] = v
        return a
    cases = [(bad_cam(world=-1), 8, 8), (bad_cam(world=n), 8, 8), (good, 0, 8), (good, 8, 0), (good, 4097, 8),
             (good, 8, 4097), (np.zeros(0, CAMERA_DTYPE), 8, 8), (bad_cam(pos=(0, np.nan, 1)), 8, 8),
             (bad_cam(pos=(np.inf, 0, 1)), 8, 8), (bad_cam(rot=(np.nan, 0, 0, 0)), 8, 8),
             (bad_cam(rot=(0.98 ** 0.5, 0, 0, 0)), 8, 8), (bad_cam(rot=(1.02 ** 0.5, 0, 0, 0)), 8, 8),
             (bad_cam(tan_half_fov_y=0.0), 8, 8), (bad_cam(tan_half_fov_y=-1.0), 8, 8),
             (bad_cam(tan_half_fov_y=np.inf), 8, 8), (bad_cam(tan_half_fov_y=np.nan), 8, 8)]
    L = sim._L
    for arr, Wd, Hd in cases:
        with pytest.raises(ValueError):
            sim.spectate(arr, Wd, Hd, out={"depth": depth, "rgb": rgb, "hit": hitb})
        rc = L.hs_render_cameras(sim._h, arr.ctypes.data if arr.size else C.c_void_p(1).value, arr.size, Wd, Hd, 0,
                                 depth.data_ptr(), rgb.data_ptr(), hitb.data_ptr())
        assert rc == 1, (arr, Wd, Hd)
    with pytest.raises(ValueError):
        sim.spectate(good, 8, 8, depth=False, rgb=False, hit=False)
    assert L.hs_render_cameras(sim._h, good.ctypes.data, 1, 8, 8, 0, None, None, None) == 1
    torch.cuda.synchronize()
    for b, b0 in zip(bufs, before):
        assert torch.equal(b, b0)
    # refused inside an open step and before init
    sim.step_begin()
    with pytest.raises(ValueError):
        sim.spectate(good, 8, 8)
    sim.step_end()
    p.ref.step()
    fresh = _sim(4, seed=3)
    with pytest.raises(ValueError):
        fresh.spectate(camera_array([top_down(0)]), 8, 8)
    # into caller-owned buffers
    got = sim.spectate(good, 8, 8, hit=True, out={"depth": depth, "rgb": rgb, "hit": hitb})
    assert got["depth"] is depth and (hitb >= 0).any()
    p.check("after the argument checks")
    # no batch renderer, observations skipped: same images as a normal handle of the same seed
    a, b = _sim(8, seed=9), _sim(8, seed=9, flags=EXT_SKIP_OBSERVATIONS)
    a.init(); b.init()
    cams = [top_down(w) for w in range(8)] + [agent_camera(a, w, 0) for w in range(8)]
    _same(_np(a.spectate(cams, 32, 32, hit=True)), _np(b.spectate(cams, 32, 32, hit=True)), "skip observations")


def test_render_log_frames_equal_live_frames(tmp_path):
    """Record 60 steps with replay.record_step and render top-down frames live; render_log in a fresh simulator writes
    PNGs whose decoded pixels are those frames."""
    import torch
    from gpu_hideseek import replay
    from gpu_hideseek.spectate import decode_png, frame, render_log, top_down
    n = 6
    kw = dict(seed=5, flags=9, hiders=(3, 3), seekers=(3, 3))
    sim = _sim(n, **kw)
    sim.init()
    cams = [top_down(w, 40.0) for w in (0, 3, 5, 1)]
    path = tmp_path / "run.log"
    rng = np.random.default_rng(1)
    live = []
    act = sim.action_tensor().to_torch()
    with open(path, "wb") as f:
        for _ in range(60):
            act[:, :3] = torch.from_numpy(rng.integers(0, 11, size=(act.shape[0], 3)).astype(np.int32)).to(act.device)
            sim.step()
            replay.record_step(sim, f)
            live.append(frame(sim.spectate(cams, 96, 64, depth=False)["rgb"].cpu().numpy()))
    player = _sim(n, **kw)
    player.init()
    paths = render_log(str(path), cams, 96, 64, str(tmp_path / "frames"), sim=player)
    assert len(paths) == 60
    for t, pth in enumerate(paths):
        with open(pth, "rb") as f:
            img = decode_png(f.read())
        assert img.shape == (128, 192, 3)
        assert np.array_equal(img, live[t]), t
    one = render_log(str(path), [cams[0]], 33, 21, str(tmp_path / "one"), sim=player, steps=[59])
    with open(one[0], "rb") as f:
        assert decode_png(f.read()).shape == (21, 33, 3)


def test_sharded_spectate_equals_the_monolithic_run():
    import torch
    import gpu_hideseek
    from gpu_hideseek.spectate import look_at, top_down
    n = 20
    kw = dict(sim_flags=0, rand_seed=8, min_hiders=1, max_hiders=3, min_seekers=1, max_seekers=3, num_pbt_policies=1)
    mono = gpu_hideseek.HideAndSeekSimulator(exec_mode=gpu_hideseek.madrona.ExecMode.CUDA, gpu_id=0, num_worlds=n, **kw)
    sh = gpu_hideseek.ShardedSimulator([0, 0, 0], n, **kw)
    mono.init(); sh.init()
    rng = np.random.default_rng(0)
    act = mono.action_tensor().to_torch()
    for _ in range(12):
        a = torch.from_numpy(rng.integers(0, 11, size=tuple(act.shape)).astype(np.int32))
        act.copy_(a.to(act.device))
        sh.action_tensor().scatter(a)
        mono.step(); sh.step()
    worlds = [19, 0, 7, 13, 6, 7, 12]
    cams = [top_down(w) for w in worlds] + [look_at(w, (5, 5, 3), (0, 0, 1)) for w in worlds]
    _same(_np(mono.spectate(cams, 80, 60, hit=True)), _np(sh.spectate(cams, 80, 60, hit=True)), "sharded")
