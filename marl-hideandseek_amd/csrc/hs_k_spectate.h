// Spectator cameras: depth / RGB / hit ids of any world from any pose (hs_render_cameras) — the function of the
// reference's viewer (src/viewer.cpp: a free camera over the arena, replay logs loaded with loadCheckpoints()) without
// a window.
//
// A camera is {world, pos, rot (w,x,y,z), tan_half_fov_y} with the agent camera's axes: local +y forward, +x right,
// +z up.  A pixel is k_render's pixel, the same function (hs_k_render.h cast_pixel) with the camera's tan_half_fov_y
// in place of kTanHalfFov: ray (fwd + right u) + up v, trace_ray's hit rule (closest entry with 0 <= t <= 1000, ties to
// the lower id, no hit on a hull the ray starts inside), z-near, sky, hit_normal and render_shade.  The quaternion is
// used as given.  So a camera at an agent's pose + (0, 0, 0.5) with fov 100 degrees reproduces that agent's view bit
// for bit: its own hull drops out by the inside-start rule.
//
// One workgroup per (camera, 64 x 16 pixel tile); a wave shades one 64-pixel row segment of the tile per pass, so the
// stores run along image rows.  The workgroup stages the world's geometry in LDS (slotOfWorld: the load balancer moves
// worlds between slots) and culls per tile: a hull's bounding sphere or a wall's box (z in [0, 2.5]) that lies wholly
// outside one of the four side planes of the pyramid of the tile's pixel-centre rays, or behind the plane through the
// camera across the tile's centre ray, is left out.  The culls keep a centimetre of margin plus 1e-4 of the distance,
// so they are conservative; HS_SPECTATE_NO_CULL turns them and cast_pixel's per-ray sphere cull off (every pixel
// against everything).  The view's set-up shares k_render's vocabulary (stage_geom, PixelView); the culls, the tiling
// and the camera's source are what differs.
#pragma once
#include "hs_state.h"
#include "hs_rays.h"
#include "hs_k_render.h"

namespace hs {

constexpr int kSpectateThreads = 256;
constexpr int kSpectateTileW = 64, kSpectateTileH = 16;    // a wave per tile row, four rows per pass
constexpr unsigned kSpectateNoCull = 1u;                   // HS_SPECTATE_NO_CULL (include/hideseek.h)

// hs_camera (include/hideseek.h)
struct SpectateCam {
    int world;
    float pos[3];
    float rot[4];
    float tanHalfFovY;
};

using SpectateTile = PixelView<0>;      // what a tile's pixels share: no per-wall depth bounds

// The cull planes of one tile, through the camera origin, with unit inward normals; a degenerate plane gets n = 0 and
// keeps everything.  The tile's rays d = (f + u r) + v up, u in [u0, u1], v in [v1, v0], are convex combinations of its
// four corner rays, so every hit point p has n . (p - o) >= 0 for each plane.  A side plane holds one edge's ray family
// ((f + u0 r) + v up, ...): its normal is a cross product of two nearly orthogonal vectors, well conditioned.
struct TileCull {
    V3 n[5];
    HSD static V3 unit(V3 a) {
        const float l2 = dot(a, a);
        return l2 > 1e-30f ? a * (1.f / sqrtf(l2)) : V3{0.f, 0.f, 0.f};
    }
    HSD TileCull(V3 f, V3 r, V3 up, float u0, float u1, float v0, float v1) {
        const V3 c = (f + r * (0.5f * (u0 + u1))) + up * (0.5f * (v0 + v1));       // centre ray
        const V3 side[4] = {cross(f + r * u0, up), cross(up, f + r * u1), cross(r, f + up * v0), cross(f + up * v1, r)};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const V3 s = unit(side[i]);
            n[i] = dot(s, c) < 0.f ? V3{0.f, 0.f, 0.f} - s : s;
        }
        // the plane through the camera across the centre ray, when every corner ray lies in front of it
        const V3 cu = unit(c);
        bool front = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const V3 d = (f + r * ((k & 1) ? u1 : u0)) + up * ((k & 2) ? v1 : v0);
            front = front && dot(cu, d) > 0.f;
        }
        n[4] = front ? cu : V3{0.f, 0.f, 0.f};
    }
    // a sphere (centre - camera origin m, radius R) that may meet the tile's pyramid
    HSD bool sphere(V3 m, float R) const {
        const float tol = R + 0.01f + 1e-4f * sqrtf(dot(m, m));
        bool keep = true;
#pragma unroll
        for (int i = 0; i < 5; ++i) keep = keep && dot(n[i], m) >= -tol;
        return keep;
    }
    // an axis-aligned box (centre - camera origin m, half extents e) that may meet it
    HSD bool box(V3 m, V3 e) const {
        const float tol = 0.01f + 1e-4f * (sqrtf(dot(m, m)) + sqrtf(dot(e, e)));
        bool keep = true;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const float reach = (fabsf(n[i].x) * e.x + fabsf(n[i].y) * e.y) + fabsf(n[i].z) * e.z;
            keep = keep && dot(n[i], m) + reach >= -tol;
        }
        return keep;
    }
};

// One workgroup per (camera, tile) of cameras [cam0, cam0 + gridDim.x / tilesPerCam).  Outputs [V][H][W] (rgba packed
// r, g, b, a), each may be null.  The host has validated the cameras (world in range, finite pose).
__global__ void __launch_bounds__(kSpectateThreads) k_spectate(SimState S, const SpectateCam *cams, int cam0, int W, int H,
                                                               int tilesX, int tilesPerCam, unsigned flags, float *depth,
                                                               unsigned *rgba, int *hitOut) {
    __shared__ WorldGeom g;
    __shared__ SpectateTile tl;
    const int tid = threadIdx.x;
    const int cam = cam0 + (int)(blockIdx.x / (unsigned)tilesPerCam), tile = (int)(blockIdx.x % (unsigned)tilesPerCam);
    const int tx = tile % tilesX, ty = tile / tilesX;
    const SpectateCam &C = cams[cam];
    const int w = C.world;
    const int ps = S.slotOfWorld[w];
    stage_geom(S, ps, w, g, tid, kSpectateThreads);
    const V3 o = {C.pos[0], C.pos[1], C.pos[2]};
    const Q crot = {C.rot[0], C.rot[1], C.rot[2], C.rot[3]};
    const float tanh = C.tanHalfFovY;
    const bool exact = (flags & kSpectateNoCull) != 0;
    const int x0 = tx * kSpectateTileW, y0 = ty * kSpectateTileH;
    const int x1 = min(x0 + kSpectateTileW, W) - 1, y1 = min(y0 + kSpectateTileH, H) - 1;
    __syncthreads();
    const V3 cf = qrot(crot, {0.f, 1.f, 0.f}), cr = qrot(crot, {1.f, 0.f, 0.f}), cu = qrot(crot, {0.f, 0.f, 1.f});
    if (tid < 128) {
        const float aspect = (float)W / (float)H;
        const TileCull cull(cf, cr, cu, pixel_u(x0, W, tanh, aspect), pixel_u(x1, W, tanh, aspect),
                            pixel_v(y0, H, tanh), pixel_v(y1, H, tanh));
        if (tid < 64) {
            const int m = tid < kNumDSlots ? g.meta[tid] : 0;
            bool keep = m != 0;
            if (keep) {
                const V3 mo = tl.set_hull(g, tid, m, o);
                if (!exact) keep = cull.sphere(V3{0.f, 0.f, 0.f} - mo, sqrtf(obj_bound_r2(meta_obj(m))));
            }
            tl.set_hulls(keep, tid == 0);
        } else {
            const int q = tid - 64;
            bool keep = q < g.numWalls;
            if (keep && !exact)
                keep = cull.box(V3{g.wall[q][0] - o.x, g.wall[q][1] - o.y, 1.25f - o.z}, V3{g.wall[q][2], g.wall[q][3], 1.25f});
            tl.set_walls(keep, q, tid == 64);
        }
    } else if (tid == 128) {
        tl.set_camera(cf, cr, cu, o);
    }
    __syncthreads();
    // a wave per tile row, 64 lanes along it; lanes right of the image shade its last column and store nothing
    const int lane = tid & 63, wave = tid >> 6;
    const int px = x0 + lane;
    const bool inx = px <= x1;
    for (int py = y0 + wave; py <= y1; py += kSpectateThreads / 64) {
        float dv; unsigned cv;
        const int hv = cast_pixel(g, tl, inx ? px : x1, py, W, H, tanh, exact, &dv, &cv);
        if (inx) {
            const size_t i = ((size_t)cam * H + py) * (size_t)W + px;
            if (depth) depth[i] = dv;
            if (rgba) rgba[i] = cv;
            if (hitOut) hitOut[i] = hv;
        }
    }
}

}  // namespace hs
