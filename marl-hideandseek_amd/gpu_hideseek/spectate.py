"""Spectator cameras: images of any world from any pose, and replay logs turned into frames.

The reference's only way to look at a world is its viewer (src/viewer.cpp): a window with a free camera that starts
40 m above the arena looking down (:169-178), which plays replay logs back through loadCheckpoints() (:185-215).  This
module is that function without a window: cameras (`Camera`, `look_at`, `top_down`, `agent_camera`) rendered by
`HideAndSeekSimulator.spectate` / `ShardedSimulator.spectate` (hs_render_cameras, csrc/hs_k_spectate.h), a
dependency-free PNG writer, and `render_log`, which writes one PNG per step of a replay log (gpu_hideseek.replay).

Camera axes are the agent camera's: local +y forward, +x right, +z up; rotations are quaternions (w, x, y, z).  They
are built in float64 and stored as float32, which is what the kernel uses, as given.
"""
import math
import os
import struct
import zlib
from dataclasses import dataclass

import numpy as np

from . import replay
from ._native import HS_SPECTATE_NO_CULL

# hs_camera (include/hideseek.h)
CAMERA_DTYPE = np.dtype([("world", "<i4"), ("pos", "<f4", (3,)), ("rot", "<f4", (4,)), ("tan_half_fov_y", "<f4")])
MAX_SIZE = 4096
AGENT_FOV_DEG = 100.0          # the agent camera (src/sim.cpp:1400-1403)
AGENT_CAM_UP = np.float32(0.5)
AGENT_SLOT0 = 11               # body slot of agent 0 in debug_bodies()
ARENA_HALF = 18.0              # the arena's outer walls (geo_gen.cpp:467-505)


@dataclass(frozen=True)
class Camera:
    """One spectator camera: local world index, position, rotation (w, x, y, z) and vertical field of view."""
    world: int
    pos: tuple
    rot: tuple
    fov_deg: float

    @property
    def tan_half_fov_y(self):
        return np.float32(math.tan(math.radians(float(self.fov_deg)) / 2.0))


def _f32(v, n):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    if a.size != n:
        raise ValueError(f"expected {n} components, got {a.size}")
    return tuple(a.tolist())


def make_camera(world, pos, rot, fov_deg):
    return Camera(int(world), _f32(pos, 3), _f32(rot, 4), float(fov_deg))


def quat_from_axes(right, fwd, up):
    """The rotation (w, x, y, z), float64, that takes local +x, +y, +z to `right`, `fwd`, `up` (orthonormal)."""
    m = np.stack([np.asarray(right, np.float64), np.asarray(fwd, np.float64), np.asarray(up, np.float64)], axis=1)
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = (0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s)
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = math.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2
        q = ((m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s)
    elif m[1, 1] > m[2, 2]:
        s = math.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2
        q = ((m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s)
    else:
        s = math.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2
        q = ((m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s)
    q = np.asarray(q, np.float64)
    q /= np.linalg.norm(q)
    return q if q[0] >= 0 else -q


def qrot(q, v):
    """The kernels' quaternion rotation (csrc/hs_core.h qrot), float64: the axes a camera's quaternion gives."""
    w, p, v = float(q[0]), np.asarray(q[1:], np.float64), np.asarray(v, np.float64)
    return (2 * w * w - 1) * v + 2 * np.dot(p, v) * p + 2 * w * np.cross(p, v)


def _unit(v):
    v = np.asarray(v, np.float64)
    n = np.linalg.norm(v)
    if not n > 0:
        raise ValueError("zero-length direction")
    return v / n


def look_at(world, eye, target, up=(0.0, 0.0, 1.0), fov_deg=60.0):
    """A camera at `eye` looking at `target`, image-up as close to `up` as the view allows.  Looking along `up` (e.g.
    straight down), image-up falls back to +y, so that a straight-down camera has image-right +x as top_down's."""
    fwd = _unit(np.asarray(target, np.float64) - np.asarray(eye, np.float64))
    upv = _unit(up)
    right = np.cross(fwd, upv)
    if np.linalg.norm(right) < 1e-9:
        right = np.cross(fwd, (0.0, 1.0, 0.0))
        if np.linalg.norm(right) < 1e-9:
            right = np.cross(fwd, (1.0, 0.0, 0.0))
    right = _unit(right)
    cup = np.cross(right, fwd)
    return make_camera(world, eye, quat_from_axes(right, fwd, cup), fov_deg)


def top_down(world, height=40.0, fov_deg=None, centre=(0.0, 0.0)):
    """Straight down from `height` over `centre`: forward (0, 0, -1), image-up +y, image-right +x (the viewer's starting
    pose, viewer.cpp:169-178).  The default field of view frames the +-18 m arena with a metre to spare."""
    if fov_deg is None:
        fov_deg = 2.0 * math.degrees(math.atan2(ARENA_HALF + 1.0, float(height)))
    q = quat_from_axes((1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))
    return make_camera(world, (centre[0], centre[1], height), q, fov_deg)


def agent_camera(sim_or_bodies, world, agent):
    """Agent `agent`'s own camera in world `world`: its float32 position + 0.5 in z (float32) and its rotation, from
    debug_bodies() (a simulator, or that array), with the agent view's 100 degree field of view."""
    bodies = sim_or_bodies.debug_bodies()[0] if hasattr(sim_or_bodies, "debug_bodies") else sim_or_bodies
    b = np.asarray(bodies)[int(world), AGENT_SLOT0 + int(agent)]
    pos = b[:3].astype(np.float32).copy()
    pos[2] = np.float32(pos[2] + AGENT_CAM_UP)
    return Camera(int(world), tuple(pos.tolist()), tuple(b[3:7].astype(np.float32).tolist()), AGENT_FOV_DEG)


def camera_array(cameras):
    """Cameras (Camera objects, or an array of CAMERA_DTYPE) -> a contiguous CAMERA_DTYPE array."""
    if isinstance(cameras, np.ndarray) and cameras.dtype == CAMERA_DTYPE:
        return np.ascontiguousarray(cameras)
    if isinstance(cameras, Camera):
        cameras = [cameras]
    cameras = list(cameras)
    arr = np.zeros(len(cameras), CAMERA_DTYPE)
    for i, c in enumerate(cameras):
        arr[i]["world"] = c.world
        arr[i]["pos"] = c.pos
        arr[i]["rot"] = c.rot
        arr[i]["tan_half_fov_y"] = c.tan_half_fov_y
    return arr


def check_size(width, height):
    for name, v in (("width", width), ("height", height)):
        if int(v) != v or not 1 <= int(v) <= MAX_SIZE:
            raise ValueError(f"{name} must be an integer in [1, {MAX_SIZE}], got {v!r}")
    return int(width), int(height)


def validate(arr, num_worlds):
    """The checks hs_render_cameras makes, made before anything touches a device; raises ValueError."""
    if arr.size < 1:
        raise ValueError("need at least one camera")
    w = arr["world"]
    bad = np.flatnonzero((w < 0) | (w >= num_worlds))
    if bad.size:
        raise ValueError(f"camera {bad[0]}: world {w[bad[0]]} outside [0, {num_worlds})")
    fin = np.isfinite(arr["pos"]).all(1) & np.isfinite(arr["rot"]).all(1) & np.isfinite(arr["tan_half_fov_y"])
    if not fin.all():
        raise ValueError(f"camera {np.flatnonzero(~fin)[0]}: non-finite pose or field of view")
    q2 = (arr["rot"].astype(np.float64) ** 2).sum(1)
    bad = np.flatnonzero(~((q2 >= 0.99) & (q2 <= 1.01)))
    if bad.size:
        raise ValueError(f"camera {bad[0]}: rotation is not a unit quaternion (|q|^2 = {q2[bad[0]]})")
    bad = np.flatnonzero(~(arr["tan_half_fov_y"] > 0))
    if bad.size:
        raise ValueError(f"camera {bad[0]}: the field of view must be > 0")


_OUTPUTS = (("depth", "float32", ()), ("rgb", "uint8", (4,)), ("hit", "int32", ()))


def render(sim, cameras, width, height, depth=True, rgb=True, hit=False, out=None, exact=False):
    """HideAndSeekSimulator.spectate: {name: tensor} for the requested outputs, depth [V,H,W] f32, rgb [V,H,W,4] u8,
    hit [V,H,W] i32; `out` supplies preallocated tensors of those shapes on the simulator's device."""
    width, height = check_size(width, height)
    want = {"depth": bool(depth), "rgb": bool(rgb), "hit": bool(hit)}
    out = dict(out or {})
    for k in out:
        if k not in want:
            raise ValueError(f"unknown output {k!r}")
        want[k] = True
    if not any(want.values()):
        raise ValueError("no output requested")
    arr = camera_array(cameras)
    validate(arr, sim.num_worlds)
    import torch
    dev = torch.device("cuda", sim.gpu_id)
    V = arr.size
    res = {}
    for name, dt, tail in _OUTPUTS:
        if not want[name]:
            continue
        shape, dtype = (V, height, width) + tail, getattr(torch, dt)
        t = out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be a contiguous {dt} tensor of shape {shape} on {dev}")
        res[name] = t
    ptr = {k: (res[k].data_ptr() if k in res else None) for k in want}
    from ._native import check
    check(sim._L.hs_render_cameras(sim._h, arr.ctypes.data, V, width, height, HS_SPECTATE_NO_CULL if exact else 0,
                                   ptr["depth"], ptr["rgb"], ptr["hit"]))
    return res


def route(ranges, worlds):
    """Sharded cameras: [(shard, camera indices, local worlds)] for the shards that have any, from global world ids
    and the shards' [(start, count)] ranges (sharded.shard_ranges)."""
    from .sharded import locate
    per = {}
    for i, w in enumerate(np.asarray(worlds).tolist()):
        g, local = locate(ranges, int(w))
        per.setdefault(g, ([], []))
        per[g][0].append(i)
        per[g][1].append(local)
    return [(g, np.asarray(idx, np.int64), np.asarray(loc, np.int32)) for g, (idx, loc) in sorted(per.items())]


def render_sharded(ssim, cameras, width, height, depth=True, rgb=True, hit=False, out=None, exact=False):
    """ShardedSimulator.spectate: cameras with GLOBAL world ids, each rendered by the shard that owns its world;
    images in the caller's camera order, on the device of the first shard (or of `out`)."""
    width, height = check_size(width, height)
    arr = camera_array(cameras)
    validate(arr, ssim.num_worlds)
    import torch
    res = None
    for g, idx, local in route(ssim.ranges, arr["world"]):
        sub = arr[idx].copy()
        sub["world"] = local
        part = render(ssim.shards[g], sub, width, height, depth, rgb, hit, exact=exact)
        if res is None:
            dev0 = torch.device("cuda", ssim.shards[0].gpu_id)
            res = {}
            for k, v in part.items():
                t = (out or {}).get(k)
                if t is None:
                    t = torch.empty((arr.size,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev0)
                elif tuple(t.shape) != (arr.size,) + tuple(v.shape[1:]) or t.dtype != v.dtype:
                    raise ValueError(f"out[{k!r}] must be a {v.dtype} tensor of shape {(arr.size,) + tuple(v.shape[1:])}")
                res[k] = t
        ti = torch.from_numpy(idx)
        for k, v in part.items():
            res[k][ti.to(res[k].device)] = v.to(res[k].device)
    return res


# ---- frames ----

def encode_png(img):
    """uint8 image [H, W] (grey), [H, W, 3] (RGB) or [H, W, 4] (RGBA) -> PNG bytes (stdlib zlib / struct only)."""
    a = np.ascontiguousarray(np.asarray(img))
    if a.dtype != np.uint8:
        raise ValueError("PNG frames are uint8")
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"cannot write an image of shape {a.shape}")
    h, w, c = a.shape
    colour = {1: 0, 3: 2, 4: 6}[c]
    raw = np.zeros((h, 1 + w * c), np.uint8)         # filter byte 0 (None) per row
    raw[:, 1:] = a.reshape(h, w * c)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + chunk(b"IEND", b""))


def write_png(path, img):
    with open(path, "wb") as f:
        f.write(encode_png(img))
    return path


def decode_png(data):
    """PNG bytes as encode_png writes them (8-bit, unfiltered rows) -> uint8 array [H, W, C]."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(tag + body) & 0xFFFFFFFF != crc:
            raise ValueError(f"bad CRC in chunk {tag!r}")
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        pos += 12 + n
    w, h, depth, colour = hdr[:4]
    if depth != 8 or colour not in (0, 2, 6):
        raise ValueError("only 8-bit grey / RGB / RGBA")
    c = {0: 1, 2: 3, 6: 4}[colour]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, 1 + w * c)
    if raw[:, 0].any():
        raise ValueError("only unfiltered rows")
    return raw[:, 1:].reshape(h, w, c).copy()


def mosaic_shape(n, cols=None):
    """(rows, cols) of the mosaic of n images: ceil(sqrt(n)) columns unless given."""
    cols = int(cols) if cols else max(1, math.ceil(math.sqrt(n)))
    return (n + cols - 1) // cols, cols


def mosaic(images, cols=None):
    """Images [V, H, W, C] -> one [rows * H, cols * W, C] image; image i in row i // cols, column i % cols; black where
    no image is."""
    a = np.asarray(images)
    V, H, W = a.shape[:3]
    rows, cols = mosaic_shape(V, cols)
    outimg = np.zeros((rows * H, cols * W) + a.shape[3:], a.dtype)
    for i in range(V):
        r, c = divmod(i, cols)
        outimg[r * H:(r + 1) * H, c * W:(c + 1) * W] = a[i]
    return outimg


def frame(rgb, cols=None):
    """The RGB frame of one set of camera images (rgb [V, H, W, 4]): the image itself for one camera, else the mosaic."""
    a = np.asarray(rgb)[..., :3]
    return a[0] if a.shape[0] == 1 else mosaic(a, cols)


def render_log(log, cameras, width, height, out_dir, *, sim, steps=None, prefix="frame", cols=None):
    """Play a replay log (gpu_hideseek.replay: an array [steps, num_worlds, 1392] or a file path) back in `sim` — made
    with the recording simulator's arguments — and write one PNG per step: out_dir/{prefix}_{step:05d}.png, a mosaic
    when there are several cameras.  `cameras`: a list of cameras, or cameras(sim, step) -> list (e.g. agent_camera,
    which follows the agents).  Returns the paths written."""
    if isinstance(log, (str, os.PathLike)):
        log = replay.read_log(str(log), sim.num_worlds)
    check_size(width, height)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for t in (range(log.shape[0]) if steps is None else steps):
        replay.replay_step(sim, log, t)
        cams = cameras(sim, t) if callable(cameras) else cameras
        rgb = render(sim, cams, width, height, depth=False, rgb=True)["rgb"].cpu().numpy()
        paths.append(write_png(os.path.join(out_dir, f"{prefix}_{t:05d}.png"), frame(rgb, cols)))
    return paths
