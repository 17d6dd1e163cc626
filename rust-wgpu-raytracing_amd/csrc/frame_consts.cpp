// Host arithmetic of a frame, in double: the culling constants, the screen rectangles of the spheres and of the whole mesh, the
// texture tables.  Pure host code: nothing here needs a device or the context.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "rwr_internal.h"

namespace rwr {

// Quad records of a w x h RGBA8 sRGB texture (rwr_internal.h QuadTex): record (px, py) of the (w + 1) x (h + 1) grid holds the
// four ClampToEdge texels of the footprint whose top-left tap is (px - 1, py - 1).
void build_tex_quads(const uint8_t *rgba8, uint32_t w, uint32_t h, uint32_t *out)
{
    auto texel = [&](int64_t x, int64_t y) {
        x = std::min<int64_t>(std::max<int64_t>(x, 0), (int64_t)w - 1);
        y = std::min<int64_t>(std::max<int64_t>(y, 0), (int64_t)h - 1);
        const uint8_t *t = rgba8 + 4u * ((size_t)y * w + (size_t)x);
        // (three bytes at bits 2-9, 12-19, 22-29: bits 0-1, 10-11, 20-21 and 30-31 are clear, which quad_texel relies on)
        return (uint32_t)t[0] << 2 | (uint32_t)t[1] << 12 | (uint32_t)t[2] << 22;
    };
    for (uint32_t py = 0; py <= h; py++)
        for (uint32_t px = 0; px <= w; px++) {
            uint32_t *r = out + 4u * ((size_t)py * (w + 1u) + px);
            r[0] = texel((int64_t)px - 1, (int64_t)py - 1);
            r[1] = texel(px, (int64_t)py - 1);
            r[2] = texel((int64_t)px - 1, py);
            r[3] = texel(px, py);
        }
}

void build_srgb_lut(float *lut)
{
    // Rgba8UnormSrgb decode (texture.rs:122): the sRGB EOTF, evaluated in double.
    for (int i = 0; i < 256; i++) {
        const double c = (double)i / 255.0;
        const double l = (c <= 0.04045) ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4);
        lut[i] = (float)l;
    }
}

namespace {

// Per-frame culling constants (rwr_internal.h CullConsts), evaluated in double.
void compute_cull_consts(const rwr_camera_inv_uniform &cam, uint32_t width, uint32_t height, CullConsts &cc)
{
    auto dir = [&](double fx, double fy, double out[3]) {
        const double xn = 2.0 * fx / (double)width - 1.0, yn = 2.0 * fy / (double)height - 1.0;
        double v[4];
        for (int r = 0; r < 4; r++)
            v[r] = cam.proj_inv[0][r] * xn + cam.proj_inv[1][r] * yn + cam.proj_inv[2][r] + cam.proj_inv[3][r];
        for (int r = 0; r < 3; r++)
            out[r] = cam.viewmodel_inv[0][r] * v[0] + cam.viewmodel_inv[1][r] * v[1] + cam.viewmodel_inv[2][r] * v[2];
    };
    auto cross = [](const double a[3], const double b[3], double o[3]) {
        o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
    };
    double A[3], Px[3], Py[3], Bx[3], By[3];
    dir(0.0, 0.0, A);
    dir((double)width, 0.0, Px);
    dir(0.0, (double)height, Py);
    for (int k = 0; k < 3; k++) { Bx[k] = (Px[k] - A[k]) / (double)width; By[k] = (Py[k] - A[k]) / (double)height; }
    double Ux[3], Vx[3], Uy[3], Vy[3];
    cross(A, By, Ux); cross(Bx, By, Vx);
    cross(A, Bx, Uy); cross(By, Bx, Vy);
    const double detx = Ux[0] * Bx[0] + Ux[1] * Bx[1] + Ux[2] * Bx[2];  // n_x . Bx
    const double dety = Uy[0] * By[0] + Uy[1] * By[1] + Uy[2] * By[2];  // n_y . By
    const double sx = detx < 0.0 ? -1.0 : 1.0, sy = dety < 0.0 ? -1.0 : 1.0;
    std::memset(&cc, 0, sizeof cc);
    double l1[4] = {0, 0, 0, 0};
    for (int k = 0; k < 3; k++) {
        cc.A[k] = (float)A[k]; cc.Bx[k] = (float)Bx[k]; cc.By[k] = (float)By[k];
        cc.Ux[k] = (float)(sx * Ux[k]); cc.Vx[k] = (float)(sx * Vx[k]);
        cc.Uy[k] = (float)(sy * Uy[k]); cc.Vy[k] = (float)(sy * Vy[k]);
        l1[0] += std::fabs(Ux[k]); l1[1] += std::fabs(Vx[k]); l1[2] += std::fabs(Uy[k]); l1[3] += std::fabs(Vy[k]);
    }
    cc.Ux[3] = (float)l1[0]; cc.Vx[3] = (float)l1[1]; cc.Uy[3] = (float)l1[2]; cc.Vy[3] = (float)l1[3];
    for (int k = 0; k < 3; k++) cc.origin[k] = cam.origin[k];
    // the largest |dir|_1 (dir is affine, so |dir|_1 peaks at a screen corner)
    double corner[4][3];
    dir(0.0, 0.0, corner[0]); dir((double)width, 0.0, corner[1]);
    dir((double)width, (double)height, corner[2]); dir(0.0, (double)height, corner[3]);
    double max_dir_l1 = 0.0;
    for (int c = 0; c < 4; c++)
        max_dir_l1 = std::fmax(max_dir_l1, std::fabs(corner[c][0]) + std::fabs(corner[c][1]) + std::fabs(corner[c][2]));
    cc.corner_margin = (float)(kCullRelHost * 1.001 * max_dir_l1);
    double vxa = 0.0, vya = 0.0;
    for (int k = 0; k < 3; k++) { vxa += sx * Vx[k] * A[k]; vya += sy * Vy[k] * A[k]; }
    cc.vxa = (float)vxa; cc.vya = (float)vya;
    // World-magnitude terms of rwr_cull.h ("World magnitude"): |O|_1; the pixel shift per unit of rho
    // anywhere on the screen, |Ux + x Vx|_1 max|dir|_1 / |vxa| with 0 <= x <= width (+1); and |Vx|_1 max|dir|_1 / |vxa|
    // (likewise for y), which bounds the shift's denominator: rho times it <= 1/2 at most doubles the shift.
    cc.origin[3] = (float)((std::fabs((double)cam.origin[0]) + std::fabs((double)cam.origin[1]) + std::fabs((double)cam.origin[2])) * 1.001);
    cc.A[3] = (float)(1.001 * (l1[0] + ((double)width + 1.0) * l1[1]) * max_dir_l1 / std::fabs(vxa));
    cc.Bx[3] = (float)(1.001 * (l1[2] + ((double)height + 1.0) * l1[3]) * max_dir_l1 / std::fabs(vya));
    cc.By[3] = (float)(1.001 * std::fmax(l1[1] / std::fabs(vxa), l1[3] / std::fabs(vya)) * max_dir_l1);
    // a pinhole camera has both determinants well away from 0; a singular or non-finite
    // uniform simply disables culling (the exact test then sees every face)
    const double bx1 = std::fabs(Bx[0]) + std::fabs(Bx[1]) + std::fabs(Bx[2]);
    const double by1 = std::fabs(By[0]) + std::fabs(By[1]) + std::fabs(By[2]);
    const bool ok = std::isfinite(detx) && std::isfinite(dety) && std::isfinite(max_dir_l1) &&
                    std::fabs(detx) > 1e-9 * l1[0] * bx1 && std::fabs(dety) > 1e-9 * l1[2] * by1;
    cc.enabled = (ok && cc.vxa != 0.0f && cc.vya != 0.0f) ? 1u : 0u;
}

// Screen rectangle {x0, y0, x1, y1} (pixel coordinates, un-clipped) of the bounding box of the whole mesh as
// this camera sees it; false when any box corner is behind (or beside) the camera plane — the camera is in or
// near the mesh — or when culling is off.  Conservative use needs the caller's margin.
bool mesh_screen_rect(const CullConsts &cc, const float lo[3], const float hi[3], double rect[4])
{
    if (!cc.enabled) return false;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int c = 0; c < 8; c++) {
        double q[3], vx = 0.0, vy = 0.0, ux = 0.0, uy = 0.0;
        for (int k = 0; k < 3; k++) {
            q[k] = (double)((c >> k & 1) ? hi[k] : lo[k]) - (double)cc.origin[k];
            vx += cc.Vx[k] * q[k]; vy += cc.Vy[k] * q[k]; ux += cc.Ux[k] * q[k]; uy += cc.Uy[k] * q[k];
        }
        // depth along the view direction of this corner (see compute_sphere_rects); must be clearly in front
        if (!(vx / cc.vxa > 1e-6) || !(vy / cc.vya > 1e-6)) return false;
        const double x = -ux / vx, y = -uy / vy;
        if (!std::isfinite(x) || !std::isfinite(y)) return false;
        x0 = std::fmin(x0, x); x1 = std::fmax(x1, x); y0 = std::fmin(y0, y); y1 = std::fmax(y1, y);
    }
    rect[0] = x0; rect[1] = y0; rect[2] = x1; rect[3] = y1;
    return true;
}

// rho (rwr_cull.h world_rho) for every face of the mesh at once: the magnitude from the box's corners, the distance
// from the box; +inf when the origin is too close to the box for the bound.
double mesh_world_rho(const CullConsts &cc, const float lo[3], const float hi[3])
{
    double mag = 0.0, dist = 0.0;
    for (int k = 0; k < 3; k++) {
        mag += std::fmax(std::fabs((double)lo[k]), std::fabs((double)hi[k]));
        dist = std::fmax(dist, std::fmax((double)lo[k] - (double)cc.origin[k], (double)cc.origin[k] - (double)hi[k]));
    }
    const double delta = kCullWorldHost * ((double)cc.origin[3] + mag);
    dist *= 0.999;
    return dist > 2.0 * delta ? delta / (dist - delta) : INFINITY;
}

// Average projected area, in pixels, of a face of the mesh: the area of that rectangle (clipped to the
// frame) over half the face count; +inf when there is no rectangle.  The frame kernel walks, per 32x4-pixel
// tile, every face that may touch the tile, one after the other; when faces are much smaller than a tile (a
// distant or finely tessellated mesh) the per-ray BVH traversal of k_primary_bvh is faster
// (tools/dense_probe.py: cube.obj, 428 faces, from 8 units away and beyond — up to 2x) and gives the same
// frame bit for bit, so the context switches to it for binned scenes (more than 256 faces; a smaller mesh
// bounds the walk by itself).
double mean_face_pixels(bool have_rect, const double rect[4], uint32_t n_tris, uint32_t width, uint32_t height)
{
    if (!have_rect || n_tris == 0) return INFINITY;
    const double x0 = std::fmax(rect[0], 0.0), y0 = std::fmax(rect[1], 0.0);
    const double x1 = std::fmin(rect[2], (double)width), y1 = std::fmin(rect[3], (double)height);
    if (!(x1 > x0) || !(y1 > y0)) return INFINITY;   // off screen: nothing to trace either way
    return (x1 - x0) * (y1 - y0) / (0.5 * (double)n_tris);
}

// Conservative pixel-space bounds of each analytic sphere's silhouette, so that
// tiles which cannot see a sphere skip its intersection test (the skipped test
// would have returned "no hit").  The sphere touches pixel column x iff its
// centre q (relative to the ray origin) is within r of the plane with normal
// n(x) = Ux + x*Vx:  (n(x).q)^2 <= r^2 |n(x)|^2, a quadratic in x.  Anything
// unusual (origin inside the sphere, sphere straddling the camera plane,
// non-finite numbers) yields "whole screen".
void compute_sphere_rects(const CullConsts &cc, const rwr_sphere_buffer_data *spheres, uint32_t n, uint32_t width,
                          uint32_t height, float (*rects)[4])
{
    const float inf = HUGE_VALF;
    for (uint32_t s = 0; s < RWR_MAX_SPHERES; s++) { rects[s][0] = -inf; rects[s][1] = -inf; rects[s][2] = inf; rects[s][3] = inf; }
    if (!cc.enabled) return;
    auto interval = [](const float *U, const float *V, const double q[3], double r, double &lo, double &hi) -> bool {
        double uq = 0, vq = 0, uu = 0, uv = 0, vv = 0;
        for (int k = 0; k < 3; k++) { uq += U[k] * q[k]; vq += V[k] * q[k]; uu += (double)U[k] * U[k]; uv += (double)U[k] * V[k]; vv += (double)V[k] * V[k]; }
        const double a = vq * vq - r * r * vv, b = uq * vq - r * r * uv, c = uq * uq - r * r * uu;  // a x^2 + 2 b x + c <= 0
        const double disc = b * b - a * c;
        if (!(a > 0.0) || !(disc >= 0.0)) return false;
        const double sq = std::sqrt(disc);
        lo = (-b - sq) / a;
        hi = (-b + sq) / a;
        return std::isfinite(lo) && std::isfinite(hi);
    };
    for (uint32_t s = 0; s < n; s++) {
        const double r = std::fabs((double)spheres[s].radius);
        double q[3], qq = 0.0, vq = 0.0, vv = 0.0;
        for (int k = 0; k < 3; k++) {
            q[k] = (double)spheres[s].center[k] - (double)cc.origin[k];
            qq += q[k] * q[k]; vq += cc.Vx[k] * q[k]; vv += (double)cc.Vx[k] * cc.Vx[k];
        }
        if (!(qq > r * r * 1.0001)) continue;  // origin inside (or on) the sphere: every ray may hit
        // depth coordinate t of a point p: (Vx.p)/vxa; over the sphere it spans t_c -+ r|Vx|/|vxa|
        const double tc = vq / cc.vxa, tr = r * std::sqrt(vv) / std::fabs((double)cc.vxa);
        if (tc + tr < 0.0) { rects[s][0] = inf; rects[s][1] = inf; rects[s][2] = -inf; rects[s][3] = -inf; continue; }  // behind
        if (!(tc - tr > 0.0)) continue;  // straddles the camera plane
        double x0, x1, y0, y1;
        if (!interval(cc.Ux, cc.Vx, q, r, x0, x1) || !interval(cc.Uy, cc.Vy, q, r, y0, y1)) continue;
        rects[s][0] = (float)(x0 - 0.5 - 1e-4 * std::fabs(x0)); rects[s][2] = (float)(x1 + 0.5 + 1e-4 * std::fabs(x1));
        rects[s][1] = (float)(y0 - 0.5 - 1e-4 * std::fabs(y0)); rects[s][3] = (float)(y1 + 0.5 + 1e-4 * std::fabs(y1));
    }
    (void)width; (void)height;
}

}  // namespace

// Everything of a frame's FrameParams and CullConsts that follows from the scene, the screen, the camera and the request.
void fill_frame_consts(const FrameScene &sc, const rwr_camera_inv_uniform &cam, const rwr_render_params &rp, bool accumulate,
                       uint32_t row_begin, uint32_t row_end, uint32_t row_pitch, FrameConsts &out)
{
    FrameParams &fp = out.fp;
    CullConsts &cc = out.cc;
    fp.cam = cam;
    fp.wave_cull_min = sc.wave_cull_min;
    fp.width = sc.width;
    fp.height = sc.height;
    fp.row_begin = row_begin;
    fp.row_end = row_end;
    fp.row_pitch = row_pitch;
    fp.n_spheres = sc.n_spheres;
    for (uint32_t i = 0; i < sc.n_spheres; i++) fp.spheres[i] = sc.spheres[i];
    fp.n_tris = sc.n_tris;
    fp.tex_w = sc.tex_w;
    fp.tex_h = sc.tex_h;
    fp.tex_wmax = sc.tex_w ? (float)(sc.tex_w - 1u) : 0.0f;
    fp.tex_hmax = sc.tex_h ? (float)(sc.tex_h - 1u) : 0.0f;
    fp.flags = rp.flags;
    for (int k = 0; k < 3; k++) {
        fp.ambient[k] = sc.material->ambient[k];
        fp.specular[k] = sc.material->specular[k];
    }
    fp.materials = sc.materials;
    fp.n_materials = sc.n_materials;
    fp.tangents = sc.tangents;
    compute_cull_consts(cam, sc.width, sc.height, cc);
    compute_sphere_rects(cc, sc.spheres, sc.n_spheres, sc.width, sc.height, fp.sphere_rect);
    // the whole mesh's screen rectangle: tiles outside it skip the mesh pass altogether (same margins as the spheres')
    double mesh_rect[4] = {0, 0, 0, 0};
    const bool have_mesh_rect = sc.n_tris != 0 && mesh_screen_rect(cc, sc.aabb_lo, sc.aabb_hi, mesh_rect);
    const float inf = std::numeric_limits<float>::infinity();
    fp.mesh_rect[0] = fp.mesh_rect[1] = -inf; fp.mesh_rect[2] = fp.mesh_rect[3] = inf;
    const double mesh_rho = have_mesh_rect ? mesh_world_rho(cc, sc.aabb_lo, sc.aabb_hi) : INFINITY;
    if (have_mesh_rect && mesh_rho * cc.By[3] <= 0.5) {
        const double wx = 2.0 * mesh_rho * cc.A[3], wy = 2.0 * mesh_rho * cc.Bx[3];   // world-magnitude stray (rwr_cull.h)
        fp.mesh_rect[0] = (float)(mesh_rect[0] - 1.0 - wx - 1e-4 * std::fabs(mesh_rect[0]));
        fp.mesh_rect[1] = (float)(mesh_rect[1] - 1.0 - wy - 1e-4 * std::fabs(mesh_rect[1]));
        fp.mesh_rect[2] = (float)(mesh_rect[2] + 1.0 + wx + 1e-4 * std::fabs(mesh_rect[2]));
        fp.mesh_rect[3] = (float)(mesh_rect[3] + 1.0 + wy + 1e-4 * std::fabs(mesh_rect[3]));
    }
    for (int k = 0; k < 4; k++) {
        const double v = k < 2 ? std::floor((double)fp.mesh_rect[k]) : std::ceil((double)fp.mesh_rect[k]);
        fp.mesh_px[k] = (int32_t)std::fmax(-1e9, std::fmin(1e9, v));   // +-inf -> +-1e9
    }
    fp.spp = rp.spp;
    fp.jitter_spp = accumulate ? std::max(rp.spp, 2u) : rp.spp;
    fp.seed = rp.seed;
    fp.bounces = rp.max_bounces;
    out.mean_face_px = mean_face_pixels(have_mesh_rect, mesh_rect, sc.n_tris, sc.width, sc.height);
}
}  // namespace rwr

using namespace rwr;

extern "C" int rwr_host_texture_quads(const uint8_t *rgba8_srgb, uint32_t tex_w, uint32_t tex_h, uint32_t *out)
{
    if (!rgba8_srgb || !out) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (tex_w == 0 || tex_h == 0 || tex_w > kMaxTextureDim || tex_h > kMaxTextureDim)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "texture %ux%u outside 1..%u", tex_w, tex_h, kMaxTextureDim);
    build_tex_quads(rgba8_srgb, tex_w, tex_h, out);
    return RWR_OK;
}
