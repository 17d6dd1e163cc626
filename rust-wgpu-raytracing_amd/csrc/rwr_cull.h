// Conservative face culling for rays that share one origin (primary rays).
//
// Nothing here decides what a pixel shows: these tests may only DROP faces that no
// ray of a tile can hit, and every comparison is written so that rounding, NaNs
// or degenerate inputs err on the side of keeping the face.  That is why this
// code, unlike the hit test, is free to use FMA and approximate constants.
//
// Once per frame k_frame_setup turns every face into a FrameTri: its conservative
// pixel-space bounding rectangle plus, per edge, the affine function
//     d_i(x, y) = dot(edge-plane normal_i, dir(x, y)) = ea_i + x*ex_i + y*ey_i ,
// signed so that a ray through pixel-space point (x, y) can reach the face at
// t >= 0 only if all three d_i >= 0 (rasteriser edge functions: the planes through
// the origin and an edge of the face).  The render kernel then rejects a face for
// a pixel rectangle with a handful of compares: rectangle overlap (good for small
// faces) and "whole rectangle outside one edge" (tight for faces much larger than
// the tile; also removes everything behind the camera — the reference camera
// sits INSIDE the mesh, lib.rs:352-360).
// Margins: 2e-5 relative on L1 norms (>100x the f32 rounding of the exact hit
// test) and 0.02 px + 1e-5 relative on the rectangle, on top of the half-pixel
// guard band between tile bounds and pixel centres.
// The exact hit test also rounds at WORLD magnitude (-dot(N, p0), dot(N, O) + d,
// t*D + O): a literal hit lies within kCullWorld * (|O|_1 + max |p_i|_1) of the
// face, so the ray passes the face by an angle up to rho = that / (distance from
// the origin to the face - that).  Both margins grow by rho ("World
// magnitude"); a face too close to its own rounding for that bound is never culled.
#pragma once

#include "rwr_device.h"

namespace rwr {

RWR_DEV float ffma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
RWR_DEV float fdot(f3 a, f3 b) { return ffma(a.z, b.z, ffma(a.y, b.y, a.x * b.x)); }
RWR_DEV float fdot(const float *a, f3 b) { return ffma(a[2], b.z, ffma(a[1], b.y, a[0] * b.x)); }
RWR_DEV f3 fcross(f3 a, f3 b)
{
    return mk3(ffma(a.y, b.z, -(a.z * b.y)), ffma(a.z, b.x, -(a.x * b.z)), ffma(a.x, b.y, -(a.y * b.x)));
}
RWR_DEV float l1norm(f3 a) { return fabsf(a.x) + fabsf(a.y) + fabsf(a.z); }

constexpr float kCullDegenerate = 1e-4f;   // (kCullRel and kCullWorld: rwr_internal.h, the host needs them too)

// rho for one face: the angle (relative to |dir|) by which a ray that the exact test lets hit the face may pass outside
// it because that test rounds at world magnitude; +inf when the bound does not hold (the face is then never culled).
// delta: that bound in world units.
RWR_DEV float world_rho(const CullConsts &cc, f3 p0, f3 p1, f3 p2, const f3 (&q)[3], float vol, float &delta)
{
    delta = kCullWorld * (cc.origin[3] + fmaxf(l1norm(p0), fmaxf(l1norm(p1), l1norm(p2))));
    // distance from the origin to the face >= max(distance to its plane, distance to its bounding box)
    const f3 a = sub3(p1, p0), b = sub3(p2, p0);
    const float nl1 = l1norm(fcross(a, b)) + 1e-6f * l1norm(a) * l1norm(b);
    float dist = fabsf(vol) * __builtin_amdgcn_rcpf(nl1);   // (v_rcp_f32: 1 ulp; the 0.999 below covers it)
    dist = fmaxf(dist, fmaxf(fminf(q[0].x, fminf(q[1].x, q[2].x)), -fmaxf(q[0].x, fmaxf(q[1].x, q[2].x))));
    dist = fmaxf(dist, fmaxf(fminf(q[0].y, fminf(q[1].y, q[2].y)), -fmaxf(q[0].y, fmaxf(q[1].y, q[2].y))));
    dist = fmaxf(dist, fmaxf(fminf(q[0].z, fminf(q[1].z, q[2].z)), -fmaxf(q[0].z, fmaxf(q[1].z, q[2].z))));
    dist *= 0.999f;
    const float rho = delta * __builtin_amdgcn_rcpf(dist - delta) * 1.0001f;
    return dist > 2.0f * delta ? rho : __builtin_inff();  // (NaN: +inf)
}

// One face -> FrameTri.  q_i = corner - ray origin.
RWR_DEV FrameTri make_frame_tri(const CullConsts &cc, const CullRec &R)
{
    const f3 O = ld3(cc.origin);
    const f3 p0 = ld3(R.p0), p1 = ld3(R.p1), p2 = ld3(R.p2);
    const f3 q[3] = {sub3(p0, O), sub3(p1, O), sub3(p2, O)};
    const f3 e[3] = {fcross(q[0], q[1]), fcross(q[1], q[2]), fcross(q[2], q[0])};
    const float vol = fdot(e[0], q[2]);
    float delta;
    const float rho = world_rho(cc, p0, p1, p2, q, vol, delta);
    const bool world_ok = rho * cc.By[3] <= 0.5f;  // (false for +inf and NaN)
    const float inf = __builtin_inff();
    FrameTri T;

    // -- pixel-space bounding rectangle ---------------------------------------
    // A corner q = t*dir(x, y) has Vx.q = t*vxa and (Ux + x*Vx).q = 0, hence
    // t = (Vx.q)/vxa and x = -(Ux.q)/(Vx.q); likewise for y.
    float xs[3], ys[3];
    bool all_front = true, all_behind = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float vx = fdot(cc.Vx, q[i]), vy = fdot(cc.Vy, q[i]);
        const float t = vx / cc.vxa;
        const float tol = 1e-5f * l1norm(q[i]) * cc.Vx[3] / fabsf(cc.vxa);
        all_front &= t > tol;
        all_behind &= t < -(tol + delta * cc.Vx[3] / fabsf(cc.vxa));   // (a literal hit lies within delta of the face)
        xs[i] = -fdot(cc.Ux, q[i]) / vx;
        ys[i] = -fdot(cc.Uy, q[i]) / vy;
    }
    // default: unbounded (also what NaNs fall into)
    T.bx0 = -inf; T.by0 = -inf; T.bx1 = inf; T.by1 = inf;
    if (all_front) {
        const float xmin = fminf(xs[0], fminf(xs[1], xs[2])), xmax = fmaxf(xs[0], fmaxf(xs[1], xs[2]));
        const float ymin = fminf(ys[0], fminf(ys[1], ys[2])), ymax = fmaxf(ys[0], fmaxf(ys[1], ys[2]));
        // + the world-magnitude stray in pixels: |dx| <= rho |dir| |Ux + x Vx| / (|vxa| - rho |dir| |Vx|) (context.cpp)
        const float px = 0.02f + 1e-5f * fmaxf(fabsf(xmin), fabsf(xmax)) + 2.0f * rho * cc.A[3];
        const float py = 0.02f + 1e-5f * fmaxf(fabsf(ymin), fabsf(ymax)) + 2.0f * rho * cc.Bx[3];
        if (world_ok && xmin <= xmax && ymin <= ymax) {  // false only with NaNs or a face too close for the world bound
            T.bx0 = xmin - px; T.bx1 = xmax + px; T.by0 = ymin - py; T.by1 = ymax + py;
        }
    } else if (all_behind && world_ok) {
        T.bx0 = inf; T.by0 = inf; T.bx1 = -inf; T.by1 = -inf;  // empty: no t >= 0 hit possible
    }

    // -- edge functions ---------------------------------------------------------
    // D reaches the face at t > 0 iff s*dot(q_i x q_j, D) >= 0 for the three edges,
    // s = sign of the signed volume (q0 x q1).q2.
    // (e and vol: above)
    const bool reliable = world_ok && fabsf(vol) > kCullDegenerate * l1norm(e[0]) * l1norm(q[2]);  // false when edge-on or NaN
    // corner_margin = kCullRel' * max |dir|_1; the world term is rho * max |dir|_1 (context.cpp: kCullRel' = 2.002e-5)
    const float mscale = 1.0f + rho * (1.0f / 2.002e-5f);
    const float s = vol > 0.0f ? 1.0f : -1.0f;
    float me[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        T.ea[i] = reliable ? s * fdot(cc.A, e[i]) : inf;  // +inf: this edge never rejects
        T.ex[i] = reliable ? s * fdot(cc.Bx, e[i]) : 0.0f;
        T.ey[i] = reliable ? s * fdot(cc.By, e[i]) : 0.0f;
        me[i] = cc.corner_margin * mscale * l1norm(e[i]);
        if (!(T.ea[i] == T.ea[i]) || !(T.ex[i] == T.ex[i]) || !(T.ey[i] == T.ey[i]) || !(me[i] == me[i])) {
            T.ea[i] = inf; T.ex[i] = 0.0f; T.ey[i] = 0.0f; me[i] = 0.0f;
        }
    }
    T.me0 = me[0]; T.me1 = me[1]; T.me2 = me[2];
    return T;
}

// Pixel rectangle of a tile, in pixel units (uniform across the wave / block).
struct TileRect { float x0, y0, x1, y1; };

// True = no ray through the rectangle can reach the face at t >= 0.
RWR_DEV bool rect_culls(const FrameTri &T, const TileRect &r)
{
    bool c = (T.bx1 < r.x0) || (T.bx0 > r.x1) || (T.by1 < r.y0) || (T.by0 > r.y1);
    const float me[3] = {T.me0, T.me1, T.me2};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        // d_i is affine, so its maximum over the rectangle is at the corner its gradient points to
        // (a NaN anywhere makes the comparison false: the face is kept)
        const float xs = T.ex[i] >= 0.0f ? r.x1 : r.x0, ys = T.ey[i] >= 0.0f ? r.y1 : r.y0;
        const float dmax = ffma(xs, T.ex[i], ffma(ys, T.ey[i], T.ea[i]));
        c |= dmax < -me[i];
    }
    return c;
}

}  // namespace rwr
