// Spectator cameras: depth / RGB / hit ids of any world from any pose (hs_render_cameras) — the function of the
// reference's viewer (src/viewer.cpp: a free camera over the arena, replay logs loaded with loadCheckpoints()) without
// a window.
//
// A camera is {world, pos, rot (w,x,y,z), tan_half_fov_y} with the agent camera's axes: local +y forward, +x right,
// +z up.  A pixel is k_render's pixel (hs_k_render.h render_pixel) with the camera's tan_half_fov_y in place of
// kTanHalfFov: ray (fwd + right u) + up v, trace_ray's hit rule (closest entry with 0 <= t <= 1000, ties to the lower
// id, no hit on a hull the ray starts inside), the same z-near, sky, hit_normal and render_shade.  The quaternion is
// used as given.  So a camera at an agent's pose + (0, 0, 0.5) with fov 100 degrees reproduces that agent's view bit
// for bit: its own hull drops out by the inside-start rule.
//
// One workgroup per (camera, 64 x 16 pixel tile); a wave shades one 64-pixel row segment of the tile per pass, so the
// stores run along image rows.  The workgroup stages the world's geometry in LDS (slotOfWorld: the load balancer moves
// worlds between slots) and culls per tile: a hull's bounding sphere or a wall's box (z in [0, 2.5]) that lies wholly
// outside one of the four side planes of the pyramid of the tile's pixel-centre rays, or behind the plane through the
// camera across the tile's centre ray, is left out.  The culls keep a centimetre of margin plus 1e-4 of the distance,
// so they are conservative; HS_SPECTATE_NO_CULL turns them all off (every pixel against everything).
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

// What a tile's pixels share: the camera, the hulls that may be hit with their origin-side terms (as RenderView), and
// the walls that may be hit, ascending.
struct SpectateTile {
    float fwd[3], right[3], up[3], o[3];
    alignas(16) float rel[kNumDSlots][8];
    unsigned others;
    int nWalls;
    unsigned char wallId[kMaxWalls];
};

HSD float spectate_u(int px, int W, float tanh, float aspect) { return ((((float)px + 0.5f) / (float)W) * 2.f - 1.f) * (tanh * aspect); }
HSD float spectate_v(int py, int H, float tanh) { return (1.f - (((float)py + 0.5f) / (float)H) * 2.f) * tanh; }

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

// One pixel: render_pixel's expressions with the camera's field of view and the tile's lists; hit -1 for the sky.
HSD void spectate_pixel(const WorldGeom &g, const SpectateTile &tl, int px, int py, int W, int H, float tanh, bool exact,
                        float *depth_out, unsigned *rgba_out, int *hit_out) {
    const V3 fwd = {tl.fwd[0], tl.fwd[1], tl.fwd[2]}, right = {tl.right[0], tl.right[1], tl.right[2]}, up = {tl.up[0], tl.up[1], tl.up[2]};
    const V3 o = {tl.o[0], tl.o[1], tl.o[2]};
    const float aspect = (float)W / (float)H;
    const float u = spectate_u(px, W, tanh, aspect);
    const float v = spectate_v(py, H, tanh);
    const V3 d = (fwd + right * u) + up * v;
    const float tmax = kCamFar;
    int hit = -1; float best = tmax;
    // walls
    const V3 inv = {1.f / d.x, 1.f / d.y, 1.f / d.z};
    const WallZ wz = ray_wall_z(o.z, d.z, inv.z);
    const int nw = tl.nWalls;
    if (__ballot(d.x == 0.f || d.y == 0.f) == 0) {
        WallScan ws(tmax, wz, o.x, o.y, inv);
        for (int k = 0; k < nw; ++k) {
            const int q = tl.wallId[k];
            const f32x2 *wq = reinterpret_cast<const f32x2 *>(g.wall[q]);
            ws.wall(wq[0], wq[1], kHitWallBase + q);
        }
        ws.finish(tmax);
        best = ws.best; hit = ws.hit;
    } else {
        for (int k = 0; k < nw; ++k) {
            const int q = tl.wallId[k];
            const float t = ray_wall_xy(o.x - g.wall[q][0], o.y - g.wall[q][1], d, inv, g.wall[q][2], g.wall[q][3], wz);
            if (t >= 0.f && t <= best && (hit < 0 || t < best)) { best = t; hit = kHitWallBase + q; }
        }
    }
    // planes
    const int np = g.numPlanes;
    for (int p = 0; p < np; ++p) {
        const V3 n = {g.plane[p][0], g.plane[p][1], g.plane[p][2]};
        const float dn = dot(n, d);
        if (!(dn < 0.f)) continue;
        const float dist = dot(n, o) - g.plane[p][3];
        if (dist < 0.f) continue;
        const float t = -dist / dn;
        if (t >= 0.f && t <= best && (hit < 0 || t < best)) { best = t; hit = kHitPlaneBase + p; }
    }
    // hulls (lower ids than the static geometry: a hull wins a tie)
    const float dd2 = dot(d, d);
    const unsigned others = __builtin_amdgcn_readfirstlane(tl.others);
#pragma unroll 1
    for (int b = 0; b < kNumDSlots; ++b) {
        if (!((others >> b) & 1u)) continue;
        const float4 e = *reinterpret_cast<const float4 *>(tl.rel[b]);
        const float bb = (e.x * d.x + e.y * d.y) + e.z * d.z, cc = e.w;
        const bool culled = !exact && cc > 0.f && (bb > 0.f || bb * bb < dd2 * cc * 0.999f);
        if (__ballot(!culled) == 0ull) continue;
        if (!culled) {
            const int obj = meta_obj(g.meta[b]);
            const V3 ol = {tl.rel[b][4], tl.rel[b][5], tl.rel[b][6]};
            const V3 dl = qrot(qinv(geom_rot(g, b)), d);
            const float t = obj == OBJ_RAMP ? ray_wedge_local(ol, dl) : ray_box_local(ol, dl, obj_half_extents(obj));
            if (t >= 0.f && t <= tmax && (t < best || (t == best && b < hit) || hit < 0)) { best = t; hit = b; }
        }
    }
    if (hit < 0 || best < kCamNear) { *depth_out = 0.f; *rgba_out = 0xff000000u; *hit_out = -1; return; }
    const V3 p = o + d * best;
    const int obj = hit < kNumDSlots ? meta_obj(g.meta[hit]) : OBJ_NONE;
    *depth_out = best;
    *rgba_out = render_shade(render_base_colour(obj, hit), hit_normal(g, hit, p));
    *hit_out = hit;
}

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
    for (int i = tid; i < kNumDSlots; i += kSpectateThreads) g.meta[i] = S.bmeta(i, ps);
    for (int i = tid; i < kNumDSlots * 3; i += kSpectateThreads) g.pos[i % kNumDSlots][i / kNumDSlots] = S.bpos(i, ps);
    for (int i = tid; i < kNumDSlots * 4; i += kSpectateThreads) g.rot[i % kNumDSlots][i / kNumDSlots] = S.brot(i, ps);
    for (int i = tid; i < 4 * kMaxWalls; i += kSpectateThreads) g.wall[i % kMaxWalls][i / kMaxWalls] = S.walls(i, ps);
    for (int i = tid; i < 4 * kMaxPlanes; i += kSpectateThreads) g.plane[i % kMaxPlanes][i / kMaxPlanes] = S.planes(i, ps);
    if (tid == 0) { g.numWalls = S.numWalls[w]; g.numPlanes = S.numPlanes[w]; }
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
        const TileCull cull(cf, cr, cu, spectate_u(x0, W, tanh, aspect), spectate_u(x1, W, tanh, aspect),
                            spectate_v(y0, H, tanh), spectate_v(y1, H, tanh));
        if (tid < 64) {
            const int m = tid < kNumDSlots ? g.meta[tid] : 0;
            bool keep = m != 0;
            if (keep) {
                const V3 mo = o - geom_pos(g, tid);
                const V3 ol = qrot(qinv(geom_rot(g, tid)), mo);
                float *e = tl.rel[tid];
                const float r2 = obj_bound_r2(meta_obj(m));
                e[0] = mo.x; e[1] = mo.y; e[2] = mo.z; e[3] = dot(mo, mo) - r2;
                e[4] = ol.x; e[5] = ol.y; e[6] = ol.z; e[7] = 0.f;
                if (!exact) keep = cull.sphere(V3{0.f, 0.f, 0.f} - mo, sqrtf(r2));
            }
            const unsigned long long pm = __ballot(keep);
            if (tid == 0) tl.others = (unsigned)pm;
        } else {
            const int q = tid - 64;
            bool keep = q < g.numWalls;
            if (keep && !exact)
                keep = cull.box(V3{g.wall[q][0] - o.x, g.wall[q][1] - o.y, 1.25f - o.z}, V3{g.wall[q][2], g.wall[q][3], 1.25f});
            const unsigned long long km = __ballot(keep);
            if (keep) {
                const int k = __builtin_amdgcn_mbcnt_hi((unsigned)(km >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)km, 0u));
                tl.wallId[k] = (unsigned char)q;
            }
            if (tid == 64) tl.nWalls = __builtin_popcountll(km);
        }
    } else if (tid == 128) {
        tl.fwd[0] = cf.x; tl.fwd[1] = cf.y; tl.fwd[2] = cf.z; tl.right[0] = cr.x; tl.right[1] = cr.y; tl.right[2] = cr.z;
        tl.up[0] = cu.x; tl.up[1] = cu.y; tl.up[2] = cu.z; tl.o[0] = o.x; tl.o[1] = o.y; tl.o[2] = o.z;
    }
    __syncthreads();
    // a wave per tile row, 64 lanes along it; lanes right of the image shade its last column and store nothing
    const int lane = tid & 63, wave = tid >> 6;
    const int px = x0 + lane;
    const bool inx = px <= x1;
    for (int py = y0 + wave; py <= y1; py += kSpectateThreads / 64) {
        float dv; unsigned cv; int hv;
        spectate_pixel(g, tl, inx ? px : x1, py, W, H, tanh, exact, &dv, &cv, &hv);
        if (inx) {
            const size_t i = ((size_t)cam * H + py) * (size_t)W + px;
            if (depth) depth[i] = dv;
            if (rgba) rgba[i] = cv;
            if (hitOut) hitOut[i] = hv;
        }
    }
}

}  // namespace hs
