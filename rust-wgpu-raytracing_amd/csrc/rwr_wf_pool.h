// What the kernels that add to a tile's pixels share (kernels_wf_bounce.hip, kernels_wf_shadow.hip): the workgroup's per-pixel
// fixed-point sums in LDS, the slot -> pixel map, the flush into the frame's planes, and the surface point a hit's next rays
// start from.
#pragma once

#include "rwr_device.h"

namespace rwr {

// What a trace workgroup keeps in LDS: fixed-point sums of albedo * E(h1) per pixel of the tile.
struct TraceShared {
    unsigned long long acc[kWfTilePixels * 3u];
    uint32_t oct_begin[9], pk_begin[9];   // packet kernel: where each octant's rays / packets begin
    uint32_t next_packet;
    uint32_t item;                        // the work item the workgroup pulled
};

// the sums of pool slot e's pixel
RWR_DEV unsigned long long *slot_sums(TraceShared &sh, uint32_t e)
{
    const uint32_t r = e & (kWfTilePixels - 1u), w = r >> 7, k = (r >> 6) & 1u, l = r & 63u;
    const uint32_t lx = (w & 1u) * 32u + 2u * (l & 15u) + k, ly = (w >> 1) * 4u + (l >> 4);
    return &sh.acc[(ly * kWfTileW + lx) * 3u];
}

// Adds one ray's contribution albedo(h0) * E(h1) to its pixel's fixed-point sums.  e: the ray's pool slot.
RWR_DEV void add_contribution(TraceShared &sh, uint32_t e, float cr, float cg, float cb)
{
    unsigned long long *dst = slot_sums(sh, e);
    // float -> u32 conversion saturates and sends NaN / negatives to 0
    atomicAdd(dst + 0, (unsigned long long)(uint32_t)(cr * kWfFixedScale));
    atomicAdd(dst + 1, (unsigned long long)(uint32_t)(cg * kWfFixedScale));
    atomicAdd(dst + 2, (unsigned long long)(uint32_t)(cb * kWfFixedScale));
}

// The same for values that are fixed point already (RWR_FLAG_SHADOWS: a term's ambient part at the hit, and later — wrapping, as
// two's complement — what the light adds to it when the shadow ray gets through).
RWR_DEV void add_fixed(TraceShared &sh, uint32_t e, unsigned long long r, unsigned long long g, unsigned long long b)
{
    unsigned long long *dst = slot_sums(sh, e);
    if (r) atomicAdd(dst + 0, r);
    if (g) atomicAdd(dst + 1, g);
    if (b) atomicAdd(dst + 2, b);
}

// Step 4: the workgroup's sums -> the frame's fixed-point bounce planes (integer atomics: whichever workgroups
// share the pool, in whatever order, the sums are the same bits).  Call after a barrier.
RWR_DEV void flush_pool(TraceShared &sh, const FrameParams &p, const WfBuffers &wf, uint32_t tile)
{
    const uint32_t tile_x0 = (tile % wf.tiles_x) * kWfTileW, tile_y0 = p.row_begin + (tile / wf.tiles_x) * p.row_pitch;
    const size_t plane = (size_t)p.width * p.height;   // (planes 0..2: red, green, blue; plane 3 is the primary stage's alpha)
    for (uint32_t q = threadIdx.x; q < kWfTilePixels; q += blockDim.x) {
        const uint32_t px = tile_x0 + (q & (kWfTileW - 1u)), py = tile_y0 + q / kWfTileW;
        const unsigned long long sr = sh.acc[q * 3u], sg = sh.acc[q * 3u + 1u], sb = sh.acc[q * 3u + 2u];
        if ((sr | sg | sb) != 0ull && px < p.width && py < p.row_end) {
            const size_t pixel = (size_t)py * p.width + px;
            if (sr) atomicAdd(&wf.fix[pixel], sr);
            if (sg) atomicAdd(&wf.fix[plane + pixel], sg);
            if (sb) atomicAdd(&wf.fix[2u * plane + pixel], sb);
        }
    }
}

// Where the rays that leave a hit start: P + 1e-4 n, P = O + t D, n = the face's normal flipped towards the ray or the sphere's
// outward normal (the reference's HitRecord normal) — the next bounce ray's origin and the shadow ray's, the same operations.
RWR_DEV f3 hit_exit_point(const FrameParams &p, const TriRecord *__restrict__ tris, f3 O, f3 D, int32_t obj, float t, float ndotd, f3 &n)
{
    const f3 P = along(O, t, D);
    if (obj >= 0) {
        n = ld3(tris[obj].nhat);
        if (ndotd > 0.0f) n = neg3(n);   // compute.wgsl:140-142
    } else {
        n = normalize3(sub3(P, ld3(p.spheres[-2 - obj].center)));
    }
    return mk3(P.x + n.x * 1e-4f, P.y + n.y * 1e-4f, P.z + n.z * 1e-4f);
}

// RWR_FLAG_SHADOWS: the ambient part of a hit's local shading — what E(h) is without its light terms: the part's
// MaterialData.ambient for a face, 0.1 * mat_color for a sphere (sphere/compute.wgsl:137-152).
RWR_DEV f3 hit_ambient(const FrameParams &p, const ShadeRec *__restrict__ shade, int32_t obj)
{
    if (obj < 0) return mk3(0.1f, 0.0f, 0.0f);
    if (p.n_materials > 1u) return ld3(p.materials[shade[obj].material].ambient);
    return mk3(p.ambient[0], p.ambient[1], p.ambient[2]);
}

// RWR_FLAG_SHADOWS: a hit's shadow record into pool slot `slot` (global: pool base + e) and its bit in the shadow ballots.
// fa / ff: the term's fixed-point values with the ambient part alone and with the light (each below 2^32).
RWR_DEV void write_shadow_record(const WfShadow &sw, size_t slot, size_t mask_word, uint32_t bit, f3 O1, bool sphere_light,
                                 const uint32_t fa[3], const uint32_t ff[3])
{
    uint32_t flags = sphere_light ? 1u : 0u;
#pragma unroll
    for (int c = 0; c < 3; c++) flags |= (ff[c] < fa[c]) ? (2u << c) : 0u;
    uint4 *dst = reinterpret_cast<uint4 *>(sw.recs + slot);
    dst[0] = make_uint4(__float_as_uint(O1.x), __float_as_uint(O1.y), __float_as_uint(O1.z), flags);
    dst[1] = make_uint4(ff[0] - fa[0], ff[1] - fa[1], ff[2] - fa[2], 0u);
    atomicOr(&sw.masks[mask_word], 1ull << bit);
}

}  // namespace rwr
