"""Spectator cameras, host side (no GPU): camera helpers, the PNG writer, mosaics, sharded routing, the hs_camera
layout and the argument checks made before anything touches a device."""
import ctypes as C
import math
import os
import re
import struct
import zlib

import numpy as np
import pytest

from gpu_hideseek import _native, spectate as S
from gpu_hideseek.sharded import shard_ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _axes(cam):
    q = np.asarray(cam.rot, np.float64)
    return S.qrot(q, (1, 0, 0)), S.qrot(q, (0, 1, 0)), S.qrot(q, (0, 0, 1))      # right, forward, up


def _orthonormal(r, f, u, tol=1e-6):
    m = np.stack([r, f, u])
    assert np.allclose(m @ m.T, np.eye(3), atol=tol)
    assert np.allclose(np.cross(f, u), r, atol=tol)          # right = forward x up (local x = y x z)


def test_top_down_axes_and_framing():
    c = S.top_down(3)
    r, f, u = _axes(c)
    _orthonormal(r, f, u)
    assert np.allclose(f, (0, 0, -1), atol=1e-6) and np.allclose(u, (0, 1, 0), atol=1e-6)
    assert np.allclose(r, (1, 0, 0), atol=1e-6)
    assert c.world == 3 and c.pos == (0.0, 0.0, 40.0)
    assert all(isinstance(v, float) and np.float32(v) == v for v in c.pos + c.rot)
    # the default field of view frames the +-18 m arena from 40 m
    assert 18.0 < 40.0 * float(c.tan_half_fov_y) < 20.5
    c2 = S.top_down(0, height=10.0, fov_deg=30.0, centre=(2.0, -3.0))
    assert c2.pos == (2.0, -3.0, 10.0) and c2.fov_deg == 30.0 and c2.rot == c.rot


def test_look_at_axes():
    rng = np.random.default_rng(0)
    for _ in range(200):
        eye, target = rng.uniform(-20, 20, 3), rng.uniform(-20, 20, 3)
        c = S.look_at(1, eye, target, fov_deg=70)
        r, f, u = _axes(c)
        _orthonormal(r, f, u, 1e-5)
        want = (target - eye) / np.linalg.norm(target - eye)
        assert np.allclose(f, want, atol=1e-5)
        assert abs(r[2]) < 1e-5 and u[2] >= -1e-6              # level horizon, upright
        q = np.asarray(c.rot, np.float32).astype(np.float64)
        assert abs((q ** 2).sum() - 1) < 1e-6
    down = S.look_at(0, (0, 0, 40), (0, 0, 0))
    assert np.allclose(down.rot, S.top_down(0).rot, atol=1e-7)
    up = S.look_at(0, (0, 0, 1), (0, 0, 9))
    r, f, u = _axes(up)
    _orthonormal(r, f, u)
    assert np.allclose(f, (0, 0, 1), atol=1e-6)


def test_agent_camera_copies_the_pose_in_float32():
    bodies = np.zeros((2, 17, 13), np.float32)
    bodies[1, 13, :3] = (1.1, -2.2, 0.7000001)
    q = np.array([0.9, 0.1, -0.2, 0.3], np.float64)
    bodies[1, 13, 3:7] = q / np.linalg.norm(q)
    c = S.agent_camera(bodies, 1, 2)
    assert c.world == 1
    assert np.array_equal(np.float32(c.pos), np.float32([1.1, -2.2, np.float32(0.7000001) + np.float32(0.5)]))
    assert np.array_equal(np.float32(c.rot), bodies[1, 13, 3:7])
    # fov 100: the same float32 as the agent view's tan(50 degrees) (csrc/hs_k_render.h kTanHalfFov)
    assert c.tan_half_fov_y == np.float32(1.19175359259421)


def _chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, out = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert zlib.crc32(tag + body) & 0xFFFFFFFF == crc
        out.append((tag, body))
        pos += 12 + n
    return out


@pytest.mark.parametrize("shape,colour", [((5, 7), 0), ((4, 3, 3), 2), ((1, 9, 4), 6), ((6, 1, 3), 2)])
def test_png_writer_round_trips_through_zlib(shape, colour):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    data = S.encode_png(img)
    ch = _chunks(data)
    assert [t for t, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, depth, ctype, comp, filt, inter = struct.unpack(">IIBBBBB", ch[0][1])
    assert (w, h, depth, ctype, comp, filt, inter) == (shape[1], shape[0], 8, colour, 0, 0, 0)
    c = 1 if len(shape) == 2 else shape[2]
    raw = np.frombuffer(zlib.decompress(ch[1][1]), np.uint8).reshape(h, 1 + w * c)
    assert not raw[:, 0].any()
    assert np.array_equal(raw[:, 1:].reshape(img.shape), img)
    assert np.array_equal(S.decode_png(data).reshape(img.shape), img)
    with pytest.raises(ValueError):
        S.encode_png(img.astype(np.float32))


def test_mosaic_layout():
    imgs = np.zeros((5, 2, 3, 3), np.uint8)
    for i in range(5):
        imgs[i] = i + 1
    m = S.mosaic(imgs)
    assert S.mosaic_shape(5) == (2, 3) and m.shape == (4, 9, 3)
    for i in range(5):
        r, c = divmod(i, 3)
        assert (m[r * 2:(r + 1) * 2, c * 3:(c + 1) * 3] == i + 1).all()
    assert (m[2:, 6:] == 0).all()
    assert S.mosaic_shape(4) == (2, 2) and S.mosaic_shape(1) == (1, 1) and S.mosaic_shape(7, cols=7) == (1, 7)
    one = np.arange(24, dtype=np.uint8).reshape(1, 2, 3, 4)
    assert np.array_equal(S.frame(one), one[0, ..., :3])


def test_sharded_camera_routing():
    ranges = shard_ranges(10, 3)                  # [(0, 4), (4, 3), (7, 3)]
    got = S.route(ranges, [9, 0, 4, 3, 9, 7])
    assert [g for g, _, _ in got] == [0, 1, 2]
    as_lists = {g: (idx.tolist(), loc.tolist()) for g, idx, loc in got}
    assert as_lists == {0: ([1, 3], [0, 3]), 1: ([2], [0]), 2: ([0, 4, 5], [2, 2, 0])}
    assert S.route(ranges, [5])[0][0] == 1
    with pytest.raises(ValueError):
        S.route(ranges, [10])


def test_camera_layout_matches_the_header():
    src = open(os.path.join(ROOT, "include", "hideseek.h")).read()
    body = re.search(r"typedef struct hs_camera \{(.*?)\} hs_camera;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [(t, n, int(k or 1)) for t, n, k in fields] == [("int32_t", "world", 1), ("float", "pos", 3),
                                                        ("float", "rot", 4), ("float", "tan_half_fov_y", 1)]
    cam = _native.HsCamera
    assert C.sizeof(cam) == 36 == S.CAMERA_DTYPE.itemsize
    for name, off in (("world", 0), ("pos", 4), ("rot", 16), ("tan_half_fov_y", 32)):
        assert getattr(cam, name).offset == off == S.CAMERA_DTYPE.fields[name][1]
    assert int(re.search(r"HS_SPECTATE_NO_CULL\s*=\s*(\d+)", src).group(1)) == _native.HS_SPECTATE_NO_CULL
    arr = S.camera_array([S.top_down(2), S.look_at(1, (1, 2, 3), (0, 0, 0), fov_deg=90)])
    raw = arr.tobytes()
    c = cam.from_buffer_copy(raw[36:72])
    assert c.world == 1 and abs(c.tan_half_fov_y - 1.0) < 1e-6 and c.pos[2] == 3.0


class _NoDevice:
    """A simulator stand-in whose native handle must never be touched."""
    num_worlds, gpu_id = 4, 0

    @property
    def _L(self):
        raise AssertionError("the device was touched")

    _h = None


def test_python_argument_checks_before_the_device():
    sim = _NoDevice()
    good = S.camera_array([S.top_down(1)])

    def bad(**kv):
        a = good.copy()
        for k, v in kv.items():
            a[k][0] = v
        return a
    for cams, w, h in [(bad(world=-1), 8, 8), (bad(world=4), 8, 8), (good, 0, 8), (good, 8, 4097), (good, 2.5, 8),
                       (S.camera_array([]), 8, 8), (bad(pos=(0, math.nan, 0)), 8, 8), (bad(rot=(math.inf, 0, 0, 0)), 8, 8),
                       (bad(rot=(0.5, 0, 0, 0)), 8, 8), (bad(rot=(1.2, 0, 0, 0)), 8, 8),
                       (bad(tan_half_fov_y=0.0), 8, 8), (bad(tan_half_fov_y=math.nan), 8, 8)]:
        with pytest.raises(ValueError):
            S.render(sim, cams, w, h)
    with pytest.raises(ValueError):
        S.render(sim, good, 8, 8, depth=False, rgb=False, hit=False)
    with pytest.raises(ValueError):
        S.render(sim, good, 8, 8, out={"normals": None})
    with pytest.raises(ValueError):
        S.make_camera(0, (1, 2), (1, 0, 0, 0), 60)
    assert S.check_size(4096, 1) == (4096, 1)
