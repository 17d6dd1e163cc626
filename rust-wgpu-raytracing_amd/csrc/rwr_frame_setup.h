// Per-frame records and tables (FrameParams::ray_colp / ray_row / tnum, FrameTri): the work of one 256-thread block, shared
// by k_frame_setup (kernels_primary.hip: its own launch ahead of every render kernel) and by the frame kernel's fused form
// (kernels_primary_p2.hip: the first workgroups of the frame's ONE launch make the records, the others wait for them).
// Blocks [0, nb_tris) make one face each per thread (the culling record of rwr_cull.h and the ray-independent numerator of
// the plane distance), the blocks after them fill the ray tables, one column pair or one row per thread.
#pragma once

#include "rwr_cull.h"
#include "rwr_device.h"

namespace rwr {

// A face's FrameTri; a degenerate camera (cc.enabled == 0) gets one that no rectangle culls
RWR_DEV FrameTri frame_tri(const CullConsts &cc, const CullRec &R)
{
    if (cc.enabled) return make_frame_tri(cc, R);
    const float inf = __builtin_inff();
    FrameTri T;
    T.bx0 = -inf; T.by0 = -inf; T.bx1 = inf; T.by1 = inf;
    T.ea[0] = T.ea[1] = T.ea[2] = inf;
    T.ex[0] = T.ex[1] = T.ex[2] = 0.0f;
    T.ey[0] = T.ey[1] = T.ey[2] = 0.0f;
    T.me0 = T.me1 = T.me2 = 0.0f;
    return T;
}

RWR_DEV void frame_setup_block(uint32_t block, uint32_t n_blocks, const CullConsts &cc, const rwr_camera_inv_uniform &cam, uint32_t width,
                               uint32_t height, const CullRec *__restrict__ cull, const TriRecord *__restrict__ tris, uint32_t n_tris,
                               uint32_t nb_tris, const FrameSetupOut &out)
{
    {   // what the frame wants zeroed: all blocks together
        const uint32_t t = block * 256u + threadIdx.x, stride = n_blocks * 256u;
        for (uint32_t i = t; i < out.n_zero_a; i += stride) out.zero_a[i] = 0u;
        for (uint32_t i = t; i < out.n_zero_b; i += stride) out.zero_b[i] = 0u;
    }
    if (block >= nb_tris) {
        const uint32_t e = (block - nb_tris) * 256u + threadIdx.x;
        const float(&p)[4][4] = cam.proj_inv;
        if (e < out.ray_pairs) {
            // compute.wgsl:151-152 for columns 2e and 2e + 1 (pixel centre: + 0.5), then the first term of :155
            const float xa = 2.0f * ((float)(2u * e) + 0.5f) / (float)width - 1.0f;
            const float xb = 2.0f * ((float)(2u * e + 1u) + 0.5f) / (float)width - 1.0f;
            out.ray_colp[2u * e] = make_float4(p[0][0] * xa, p[0][0] * xb, p[0][1] * xa, p[0][1] * xb);
            out.ray_colp[2u * e + 1u] = make_float4(p[0][2] * xa, p[0][2] * xb, xa, xb);
        } else if (e - out.ray_pairs < out.ray_rows) {
            const uint32_t y = e - out.ray_pairs;
            const float ya = 2.0f * ((float)y + 0.5f) / (float)height - 1.0f;
            out.ray_row[y] = make_float4(p[1][0] * ya, p[1][1] * ya, p[1][2] * ya, ya);
        }
        return;
    }
    const uint32_t i = block * 256u + threadIdx.x;
    if (i >= n_tris) return;
    out.tnum[i] = -(dot3(ld3(tris[i].N), ld3(cam.origin)) + tris[i].d);  // compute.wgsl:99-102
    out.ftris[i] = frame_tri(cc, cull[i]);
}

// Per-tile face sets of the two-pixel frame kernel (FrameParams::tile_lists), made by list_blocks extra blocks of k_frame_setup
// for scenes of at most kTileListMaxFaces faces: bit f of a tile's set <=> !rect_culls(face f, the tile's 32x4 rectangle), the
// test the kernel would otherwise run itself, so the kernel walks the same faces (and its debug counts count the same ones).
// The blocks do not wait for the face records of the launch's other blocks: each makes the <= 256 FrameTris it needs into LDS
// (same function, same inputs, same bits).  A wave then covers regions of 4x4 frame-kernel workgroups (64 tiles, one per lane):
// it culls every face against the region's rectangle (one face per lane), then tests only the region's survivors against each
// tile (one face at a time, one tile per lane).  This two-level build gives the same sets as testing every face per tile because
// rect_culls is monotone in the rectangle: for a sub-rectangle r' of r the bounding-box compares only get easier to satisfy, and
// each edge's dmax = fma(xs, ex, fma(ys, ey, ea)) takes corner coordinates no larger in xs * ex and ys * ey, so its exact value
// is no larger and, rounding being monotone, neither is the rounded one (a NaN at r' needs an infinite term that r has too, and
// then r's compare fails as well).  A face culled for the region is culled for each of its tiles.
//
// With tc.classes each lane also leaves its tile's class word (rwr_internal.h kTileFaces*): everything the frame kernel would find
// out about the tile before it looks at a ray — how many faces the set holds (and which, when it is one), whether the tile lies
// in the mesh's pixel rectangle (the kernel's `live`: the same integer compares on the same integers), and which spheres'
// rectangles it touches (the kernel's float compares on the same floats: tx0 / ty0 are formed here as the kernel forms them,
// and the rectangles are the frame's own).
RWR_DEV void frame_tile_lists_block(uint32_t block, const CullConsts &cc, const CullRec *__restrict__ cull, uint32_t n_tris,
                                    const FrameSetupOut &out, const TileClassIn &tc)
{
    __shared__ float4 s_ft[4][kTileListMaxFaces];   // the faces' FrameTris, one plane per 16 B
    for (uint32_t i = threadIdx.x; i < n_tris; i += 256u) {
        const FrameTri T = frame_tri(cc, cull[i]);
        s_ft[0][i] = make_float4(T.bx0, T.by0, T.bx1, T.by1);
        s_ft[1][i] = make_float4(T.ea[0], T.ea[1], T.ea[2], T.me0);
        s_ft[2][i] = make_float4(T.ex[0], T.ex[1], T.ex[2], T.me1);
        s_ft[3][i] = make_float4(T.ey[0], T.ey[1], T.ey[2], T.me2);
    }
    __syncthreads();
    auto face = [&](uint32_t f) {
        const float4 q0 = s_ft[0][f], q1 = s_ft[1][f], q2 = s_ft[2][f], q3 = s_ft[3][f];
        return FrameTri{q0.x, q0.y, q0.z, q0.w, {q1.x, q1.y, q1.z}, q1.w, {q2.x, q2.y, q2.z}, q2.w, {q3.x, q3.y, q3.z}, q3.w};
    };
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t rx_n = (out.list_gx + kListRegionWgs - 1u) / kListRegionWgs, ry_n = (out.list_gy + kListRegionWgs - 1u) / kListRegionWgs;
    for (uint32_t r = block * 4u + wave; r < rx_n * ry_n; r += out.list_blocks * 4u) {   // (wave-uniform)
        const uint32_t rx = r % rx_n, ry = r / rx_n;
        const float rx0 = (float)(rx * kListRegionWgs * 64u), ry0 = (float)(out.list_row_begin + ry * kListRegionWgs * out.list_row_pitch);
        const float ry1 = (float)(out.list_row_begin + (ry * kListRegionWgs + kListRegionWgs - 1u) * out.list_row_pitch) + 8.0f;
        const TileRect region = {rx0, ry0, rx0 + (float)(kListRegionWgs * 64u), ry1};
        // lane: tile (lane & 3) (the frame kernel's wave) of workgroup (bx, by); its rectangle as the kernel forms it
        const uint32_t bx = rx * kListRegionWgs + ((lane >> 2) & 3u), by = ry * kListRegionWgs + (lane >> 4), w = lane & 3u;
        const float tx0 = (float)(bx * 64u + (w & 1u) * 32u), ty0 = (float)(out.list_row_begin + by * out.list_row_pitch + (w >> 1) * 4u);
        const TileRect tile = {tx0, ty0, tx0 + 32.0f, ty0 + 4.0f};
        uint32_t set[kTileListWords];
#pragma unroll
        for (uint32_t k = 0; k < kTileListMaxFaces / 64u; k++) {
            uint64_t acc = 0;
            if (64u * k < n_tris) {
                const uint32_t f = 64u * k + lane;
                unsigned long long m = __ballot(f < n_tris && !rect_culls(face(min(f, n_tris - 1u)), region));
                while (m) {   // the region's survivors among faces [64 k, 64 k + 64), each against every lane's tile, two at a
                              // time (two independent LDS read -> test chains; an odd last one is tested twice)
                    const uint32_t b0 = (uint32_t)__builtin_ctzll(m);
                    m &= m - 1ull;
                    const uint32_t b1 = m ? (uint32_t)__builtin_ctzll(m) : b0;
                    m &= m - 1ull;
                    const bool keep0 = !rect_culls(face(64u * k + b0), tile), keep1 = !rect_culls(face(64u * k + b1), tile);
                    acc |= (keep0 ? 1ull << b0 : 0ull) | (keep1 ? 1ull << b1 : 0ull);
                }
            }
            set[2u * k] = (uint32_t)acc;
            set[2u * k + 1u] = (uint32_t)(acc >> 32);
        }
        if (bx < out.list_gx && by < out.list_gy) {
            uint4 *dst = reinterpret_cast<uint4 *>(out.tile_lists + ((size_t)(by * out.list_gx + bx) * 4u + w) * kTileListWords);
            dst[0] = make_uint4(set[0], set[1], set[2], set[3]);
            dst[1] = make_uint4(set[4], set[5], set[6], set[7]);
            if (tc.classes) {
                uint32_t n = 0, one = 0;
#pragma unroll
                for (uint32_t k = 0; k < kTileListWords; k++) {
                    n += (uint32_t)__popc(set[k]);
                    if (set[k]) one = 32u * k + (uint32_t)__builtin_ctz(set[k]);   // (the face, when n == 1)
                }
                const int32_t sx0 = (int32_t)(bx * 64u + (w & 1u) * 32u), sy0 = (int32_t)(out.list_row_begin + by * out.list_row_pitch + (w >> 1) * 4u);
                const bool live = !(sx0 + 32 < tc.mesh_px[0] || sx0 > tc.mesh_px[2] || sy0 + 4 < tc.mesh_px[1] || sy0 > tc.mesh_px[3]);
                uint32_t cls = !live || n == 0u ? kTileFacesNone : n == 1u ? (kTileFacesOne | one << kTileFaceShift) : kTileFacesMore;
                for (uint32_t s = 0; s < tc.n_spheres; s++) {   // (uniform; launch_frame_setup: at most RWR_MAX_SPHERES)
                    const bool off = (tx0 + 32.0f < tc.sphere_rect[s][0]) || (tx0 > tc.sphere_rect[s][2]) ||
                                     (ty0 + 4.0f < tc.sphere_rect[s][1]) || (ty0 > tc.sphere_rect[s][3]);
                    if (!off) cls |= 1u << (kTileSphereShift + s);
                }
                tc.classes[(size_t)(by * out.list_gx + bx) * 4u + w] = cls;
                tc.cover[(size_t)(by * out.list_gx + bx) * 4u + w] = 0u;   // what a frame kernel learnt about the tile (kTileCovered) goes with the records it learnt it from
            }
        }
    }
}

}  // namespace rwr
