// Wavefront integrator, light stage (RWR_FLAG_LIGHT_SAMPLING; definition: include/rwr_hip.h).
//
// Every hit that sends on a DIFFUSE ray — the primary stage's h0, a trace kernel's h_k in a generation that emits — has left its
// normal at its fixed queue slot (rwr_surface.h LightRec) and its bit in the light ballots; the ray it sent on sits in the same
// slot of the ray queue, marked, with the origin O and the throughput T the light sample shares with it.
//   k_wf_light   runs once behind the primary stage and once behind every generation's trace kernels but the last, on the launch
//                group's stream, ahead of the next generation's sort: per record it chooses one emitting sphere, draws a direction
//                uniformly over the solid angle the sphere subtends from O, and — when the ray reaches that sphere — adds
//                clamp(T * Le * g) to the tile's sums (LDS, then the frame's planes: rwr_wf_pool.h), g = 2 M kc (n . w).
// Work item = (tile, share of its ballot words); a wave takes one ballot word — 64 slots, one record per lane — at a time and
// skips empty words, as k_wf_shadow does.  Every lane has its own direction, so it builds its own slab constants (make_slab_ray).
// "Reaches" is the integrator's nearest-hit rule decided without a nearest-hit walk: the ray must hit its sphere s at t_s; a sphere
// before s in the order occludes at t <= t_s, one behind it at t < t_s (strict '<' keeps the earlier candidate), a face at
// t < t_s (rwr_bvh.h bvh_occluded_before).  The emitting spheres' indices and radiances arrive as a kernel argument (WfLights:
// scalar registers), centre and radius are the frame's (FrameParams::spheres); with one emitter nothing is selected per lane.
// Arithmetic: f32, operation for operation the header's rule and tests/light_ref.c; no contraction.
// PARTS forms (RWR_FLAG_LIGHT_PARTS; rwr_part_lights.h): the lights are the M emitting spheres and, last, the mesh light — the list
// of the faces of emitting parts (WfPartLights, a kernel argument behind WfLights).  The choice is per lane; a lane that takes the
// mesh light finds its face by binary search over the list's cdf (global memory, 16-byte records, at most ceil(log2 n) + 1 dependent
// loads), gathers the face's TriRecord, draws a point on it and aims there.  It reaches when it hits its face at t_f, no sphere at
// t <= t_f and no face g at t_g < t_f or at t_g == t_f with g < f (bvh_occluded_before<true>).  Lanes of either kind share the
// sphere tests and the one walk: a sphere lane passes self = 0, a face lane compares every sphere with '<='.  The forms without
// PARTS hold the instructions they held before there were any.  tests/part_light_ref.c is the rule's literal evaluation.
// RWR_FLAG_LIGHT_MIS (WfGlow::light & 4): the term is T Le m(g), m = mis_weight (rwr_surface.h), behind a wave-uniform switch at
// both add sites — a scalar branch around two divisions in each of the eight forms, not eight forms more (resources:
// profiles/mis_kernel_resources.txt).  tests/mis_ref.c is that rule's literal evaluation.
// SKY forms (RWR_FLAG_LIGHT_SKY; rwr_sky_light.h, rwr_device.h sky_light_draw / sky_light_g): the sky's image is the last of the L lights
// (L = gl.light >> 8).  A lane that takes it draws a texel from the image's table (two binary searches in global memory), a point in
// the texel's cell and the direction there; it is "a light at infinity" in the same walk — s = n_spheres and ts = +inf, so that any
// sphere hit and any face hit occludes (bvh_occluded_before<true> with a face index no face has) — and its radiance is S_img of the
// direction it drew.  sk is the kernel's last argument; the forms without SKY hold the instructions they held before there were any
// (profiles/sky_light_asm_identity.txt).  tests/sky_light_ref.c is the rule's literal evaluation.
#include <algorithm>
#include <type_traits>

#include "rwr_bvh.h"
#include "rwr_wf_forms.h"
#include "rwr_wf_pool.h"

namespace rwr {

// (the SKY forms are bound to the five waves per SIMD their twins run at: unbound they take 97 to 102 VGPRs, one to six more than five
// waves allow; bound they hold 96 with no scratch.  The second argument 1 is no bound: the other forms' text is the parent's.)
template <bool NODES_IN_LDS, bool STACK16, bool PARTS, bool SKY = false>
__global__ void __launch_bounds__(256, SKY ? 5 : 1)
k_wf_light(const FrameParams p, const TriRecord *__restrict__ tris, const BvhDevice bvh, const WfBuffers wf, const WfGlow gl,
           uint32_t n_tiles, uint32_t sample_count, uint32_t n_shares, uint32_t dim0, uint32_t sample_base, const WfLights lights,
           const WfPartLights parts, const WfSkyImage sk)
{
    __shared__ TraceShared sh;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    BvhNode4 *s_nodes = reinterpret_cast<BvhNode4 *>(s_dyn);
    const uint32_t node_bytes = NODES_IN_LDS ? bvh.n_nodes * (uint32_t)sizeof(BvhNode4) : 0u;
    typedef typename std::conditional<STACK16, uint16_t, uint32_t>::type StackT;
    StackT *s_stack = reinterpret_cast<StackT *>(s_dyn + node_bytes);
    // the tiles anything can be seen through, when the frame listed them (the others hold no record: their ballots are cleared)
    const uint32_t n_live = wf.live_list ? (uint32_t)__builtin_amdgcn_readfirstlane((int)*wf.live_count) : n_tiles;
    const uint32_t n_items = n_live * n_shares, n_words = sample_count * 8u;
    const uint32_t M = lights.m;
    const uint32_t Lc = SKY ? (gl.light >> 8) : (PARTS ? parts.l : M);   // the lights the lanes choose among
    const float Mf = (float)Lc;   // (PARTS: L = M + 1 takes M's place in the choice and in g; SKY: L = M + P + 1)
    uint32_t n_rays = 0, n_reached = 0;   // this wave's (wave-uniform)
    uint32_t n_part_rays = 0, n_part_reached = 0;   // PARTS: the mesh light's share of them
    uint32_t n_sky_rays = 0, n_sky_reached = 0;     // SKY: the sky's share of them
    bool staged = false;
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const uint32_t t = item / n_shares, share = item - t * n_shares;
        const uint32_t tile = wf.live_list ? (uint32_t)__builtin_amdgcn_readfirstlane((int)wf.live_list[t]) : t;
        __syncthreads();   // everybody is done with the previous item's sums
        if (NODES_IN_LDS && !staged) {
            const float4 *src = reinterpret_cast<const float4 *>(bvh.nodes);
            float4 *dst = reinterpret_cast<float4 *>(s_nodes);
            for (uint32_t i = tid; i < bvh.n_nodes * 8u; i += 256u) dst[i] = src[i];
            staged = true;
        }
        for (uint32_t i = tid; i < kWfTilePixels * 3u; i += 256u) sh.acc[i] = 0ull;
        if (tid == 0u) sh.next_packet = 0u;
        __syncthreads();
        const size_t pool_base = (size_t)tile * wf.group * kWfTilePixels;
        const unsigned long long *__restrict__ masks = gl.light_masks + (size_t)tile * wf.group * 8u;
        for (;;) {   // the item's ballot words share, share + n_shares, ...: whichever wave is free takes the next
            uint32_t j = 0u;
            if (lane == 0u) j = atomicAdd(&sh.next_packet, 1u);
            j = (uint32_t)__builtin_amdgcn_readfirstlane((int)j);
            const uint32_t w = share + j * n_shares;
            if (w >= n_words) break;
            const unsigned long long m = masks[w];   // wave-uniform
            if (m == 0ull) continue;
            const bool live = (m >> lane) & 1ull;
            const uint32_t e = w * 64u + lane;
            float4 ra = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb = ra, rn = ra;
            if (live) {
                ra = wf.rays[2u * (pool_base + e)];
                rb = wf.rays[2u * (pool_base + e) + 1u];
                rn = *reinterpret_cast<const float4 *>(gl.light_recs + pool_base + e);
            }
            const f3 O = mk3(ra.x, ra.y, ra.z), n = mk3(rn.x, rn.y, rn.z);
            const f3 thr = mk3(wf_unorm16_lo(ra.w), wf_unorm16_hi(ra.w), wf_unorm16_lo(rb.w));
            // the slot's pixel (as add_contribution maps it) and sample, as emit_next_ray finds them
            const uint32_t r = e & (kWfTilePixels - 1u), wv = r >> 7, k = (r >> 6) & 1u, l = r & 63u;
            const uint32_t px = (tile % wf.tiles_x) * kWfTileW + (wv & 1u) * 32u + 2u * (l & 15u) + k;
            const uint32_t py = p.row_begin + (tile / wf.tiles_x) * p.row_pitch + (wv >> 1) * 4u + (l >> 4);
            const uint32_t pixel = py * p.width + px, sample = sample_base + e / kWfTilePixels;
            const bool sob = (p.flags & RWR_FLAG_SOBOL) != 0u;   // (uniform) the light stage's numbers are the sequence's: RWR_FLAG_SOBOL
            // which sphere: one emitter needs no random number's value and no select
            uint32_t s = lights.index[0];
            f3 Le = mk3(lights.le[0][0], lights.le[0][1], lights.le[0][2]);
            bool mesh = PARTS && live && M == 0u;   // PARTS: this lane's light is the mesh light (the only one there is when M is 0)
            bool skyl = SKY && live && Lc == 1u;    // SKY: this lane's light is the sky's image (the only one there is when L is 1)
            if (SKY && Lc > 1u) mesh = false;       // (the choice below decides)
            if (Lc > 1u) {   // uniform
                const float u = rng_uniform(pixel, sample, dim0, p.seed, sob);
                const uint32_t i = min((uint32_t)(u * Mf), Lc - 1u);
#pragma unroll
                for (uint32_t q = 1; q < RWR_MAX_SPHERES; q++)
                    if (q < M && i == q) { s = lights.index[q]; Le = mk3(lights.le[q][0], lights.le[q][1], lights.le[q][2]); }
                if (PARTS) mesh = live && i == M;
                if (SKY) skyl = live && i == Lc - 1u;
            }
            f3 C = ld3(p.spheres[0].center);
            float R = p.spheres[0].radius;
            if (M > 1u || s != 0u) {   // uniform
#pragma unroll
                for (uint32_t q = 1; q < RWR_MAX_SPHERES; q++)
                    if (q < p.n_spheres && s == q) { C = ld3(p.spheres[q].center); R = p.spheres[q].radius; }
            }
            // the cone towards the sphere
            f3 wd = sub3(C, O);
            const float d2 = dot3(wd, wd);
            bool go = live && d2 > R * R;   // (an origin inside or on the sphere takes no sample)
            const float dl = sqrtf(d2);
            wd = mk3(wd.x / dl, wd.y / dl, wd.z / dl);
            const float s2 = R * R / d2;
            const float cmax = sqrtf(fmaxf(0.0f, 1.0f - s2));
            const float kc = s2 / (1.0f + cmax);
            float da = 0.0f, db = 0.0f;
            rng_disk_point(pixel, sample, dim0 + 1u, p.seed, sob, da, db);   // bounce_direction's rejection loop, operation for operation
            const float qq = da * da + db * db;
            const float c = 1.0f - qq * kc;
            const float rr = qq > 0.0f ? sqrtf(fmaxf(0.0f, 1.0f - c * c) / qq) : 0.0f;
            // bounce_direction's basis about wd
            const float sign = copysignf(1.0f, wd.z);
            const float aa = -1.0f / (sign + wd.z);
            const float bb = wd.x * wd.y * aa;
            const f3 b1 = mk3(1.0f + sign * wd.x * wd.x * aa, sign * bb, -sign * wd.x);
            const f3 b2 = mk3(bb, sign + wd.y * wd.y * aa, -wd.y);
            const f3 L = mk3(rr * (da * b1.x + db * b2.x) + c * wd.x, rr * (da * b1.y + db * b2.y) + c * wd.y, rr * (da * b1.z + db * b2.z) + c * wd.z);
            if constexpr (SKY) {
            // a sphere lane's sample, as in the PARTS forms below (garbage in a mesh or sky lane, which replaces every value)
            float ndw = dot3(n, L);
            go = go && !mesh && !skyl && ndw > 0.0f;
            float g = 2.0f * Mf * kc * ndw;
            f3 Ld = L;
            uint32_t self = 0u;
            bool face_ok = false;
            float ts = 0.0f;
            if constexpr (PARTS) {
            if (__any(mesh)) {   // the PARTS forms' face sample, operation for operation
                const float uf = rng_uniform(pixel, sample, dim0 + 1u, p.seed, sob);
                uint32_t lo = 0u, hi = mesh ? parts.n - 1u : 0u;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (uf < parts.list[mid].cdf) hi = mid; else lo = mid + 1u;
                }
                float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (mesh) rec = *reinterpret_cast<const float4 *>(parts.list + lo);
                const uint32_t f = __float_as_uint(rec.y);
                const bool listed = mesh && f < p.n_tris;
                const float inv_pdf = rec.z;
                float u1 = rng_uniform(pixel, sample, dim0 + 2u, p.seed, sob), u2 = rng_uniform(pixel, sample, dim0 + 3u, p.seed, sob);
                if (u1 + u2 > 1.0f) { u1 = 1.0f - u1; u2 = 1.0f - u2; }
                const TriRecord &T = tris[listed ? f : 0u];
                f3 p0 = mk3(0.0f, 0.0f, 0.0f), p1 = p0, p2 = p0, nh = p0, Lf = p0;
                if (listed) {
                    p0 = ld3(T.p0); p1 = ld3(T.p1); p2 = ld3(T.p2); nh = ld3(T.nhat);
                    const float4 lr = glow_record(gl, true, parts.shade, (int32_t)f);
                    Lf = mk3(lr.x, lr.y, lr.z);
                }
                const f3 P = mk3((p0.x + u1 * (p1.x - p0.x)) + u2 * (p2.x - p0.x), (p0.y + u1 * (p1.y - p0.y)) + u2 * (p2.y - p0.y),
                                 (p0.z + u1 * (p1.z - p0.z)) + u2 * (p2.z - p0.z));
                const f3 v = sub3(P, O);
                const float v2 = dot3(v, v);
                const float vl = sqrtf(v2);
                const f3 w = mk3(v.x / vl, v.y / vl, v.z / vl);
                const float nw = dot3(n, w);
                const float cf = fabsf(dot3(nh, w));
                if (mesh) {
                    Ld = w; ndw = nw; Le = Lf; self = f;
                    go = listed && v2 > 0.0f && nw > 0.0f;
                    g = Mf * inv_pdf * nw * cf * 0.318309886f / v2;
                    s = p.n_spheres;
                }
                face_ok = face_hit_t(T, O, Ld, mesh && go, ts);
            }
            }
            if (__any(skyl)) {   // the sky lanes: texel, point, direction; the factor from the direction drawn, as a bounce ray would make it
                const float u0 = rng_uniform(pixel, sample, dim0 + 1u, p.seed, sob), u1 = rng_uniform(pixel, sample, dim0 + 2u, p.seed, sob);
                const float u2 = rng_uniform(pixel, sample, dim0 + 3u, p.seed, sob), u3 = rng_uniform(pixel, sample, dim0 + 4u, p.seed, sob);
                uint32_t ti, tj;
                const f3 w = sky_light_draw(sk.table, sk.n, u0, u1, u2, u3, skyl, ti, tj);
                if (skyl) {
                    const float nw = dot3(n, w);
                    float P = 0.0f;
                    const float gs = sky_light_g(sk.table, sk.n, w, nw, Mf, ti, tj, P);
                    Ld = w; ndw = nw; g = gs;
                    go = P > 0.0f && nw > 0.0f;
                    Le = go ? sky_image_radiance(sk.image, sk.n, w) : mk3(0.0f, 0.0f, 0.0f);
                    s = p.n_spheres;              // (every sphere occludes, at any t)
                    ts = __builtin_inff();
                    self = 0xffffffffu;           // (and every face)
                }
            }
            float tsph = 0.0f;
            const bool sph_ok = !mesh && !skyl && go && sphere_ray_intersect_t(C, R, O, Ld, tsph);
            if (!mesh && !skyl) ts = tsph;
            bool reach = skyl ? go : mesh ? face_ok : sph_ok;
            for (uint32_t q = 0; q < p.n_spheres; q++) {
                float tq;
                if (reach && q != s && sphere_ray_intersect_t(ld3(p.spheres[q].center), p.spheres[q].radius, O, Ld, tq))
                    if (q < s ? tq <= ts : tq < ts) reach = false;
            }
            if (p.n_tris) {
                const SlabRay sr = make_slab_ray(O, Ld);
                bool occ;
                if (NODES_IN_LDS) occ = bvh_occluded_before<true>(s_nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, Ld, sr, ts, reach, self);
                else occ = bvh_occluded_before<true>(bvh.nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, Ld, sr, ts, reach, self);
                reach = reach && !occ;
            }
            if (gl.light & 4u) g = mis_weight(g);   // (uniform) RWR_FLAG_LIGHT_MIS item 4
            if (reach) add_contribution(sh, e, thr.x * (Le.x * g), thr.y * (Le.y * g), thr.z * (Le.z * g));
            n_rays += (uint32_t)__popcll(__ballot(go));
            n_reached += (uint32_t)__popcll(__ballot(reach));
            if (PARTS) {
                n_part_rays += (uint32_t)__popcll(__ballot(mesh && go));
                n_part_reached += (uint32_t)__popcll(__ballot(mesh && reach));
            }
            n_sky_rays += (uint32_t)__popcll(__ballot(skyl && go));
            n_sky_reached += (uint32_t)__popcll(__ballot(skyl && reach));
            } else if constexpr (!PARTS) {
            const float ndw = dot3(n, L);
            go = go && ndw > 0.0f;
            // visibility: the ray's own sphere, then the others by the nearest-hit rule's ties, then the mesh
            float ts = 0.0f;
            bool reach = go && sphere_ray_intersect_t(C, R, O, L, ts);
            for (uint32_t q = 0; q < p.n_spheres; q++) {
                float tq;
                if (reach && q != s && sphere_ray_intersect_t(ld3(p.spheres[q].center), p.spheres[q].radius, O, L, tq))
                    if (q < s ? tq <= ts : tq < ts) reach = false;
            }
            if (p.n_tris) {
                const SlabRay sr = make_slab_ray(O, L);
                bool occ;
                if (NODES_IN_LDS) occ = bvh_occluded_before(s_nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, L, sr, ts, reach);
                else occ = bvh_occluded_before(bvh.nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, L, sr, ts, reach);
                reach = reach && !occ;
            }
            if (reach) {
                float g = 2.0f * Mf * kc * ndw;
                if (gl.light & 4u) g = mis_weight(g);   // (uniform) RWR_FLAG_LIGHT_MIS item 4
                add_contribution(sh, e, thr.x * (Le.x * g), thr.y * (Le.y * g), thr.z * (Le.z * g));
            }
            n_rays += (uint32_t)__popcll(__ballot(go));
            n_reached += (uint32_t)__popcll(__ballot(reach));
            } else {
            // a sphere lane's sample, as above (garbage in a mesh lane, which replaces every value below)
            float ndw = dot3(n, L);
            go = go && !mesh && ndw > 0.0f;
            float g = 2.0f * Mf * kc * ndw;
            f3 Ld = L;             // the light ray's direction: the cone's, or towards the face's point
            uint32_t self = 0u;    // a mesh lane's face
            bool face_ok = false;  // the mesh lane's ray hits its face, at ts
            float ts = 0.0f;
            if (__any(mesh)) {
                // the face: the first list entry j with uf < cdf_j (the last cdf is 1 > uf: the search ends inside the list)
                const float uf = rng_uniform(pixel, sample, dim0 + 1u, p.seed, sob);
                uint32_t lo = 0u, hi = mesh ? parts.n - 1u : 0u;
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (uf < parts.list[mid].cdf) hi = mid; else lo = mid + 1u;
                }
                float4 rec = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (mesh) rec = *reinterpret_cast<const float4 *>(parts.list + lo);
                const uint32_t f = __float_as_uint(rec.y);
                const bool listed = mesh && f < p.n_tris;   // (a well-formed list names faces of the scene: nothing is read past them)
                const float inv_pdf = rec.z;
                float u1 = rng_uniform(pixel, sample, dim0 + 2u, p.seed, sob), u2 = rng_uniform(pixel, sample, dim0 + 3u, p.seed, sob);
                if (u1 + u2 > 1.0f) { u1 = 1.0f - u1; u2 = 1.0f - u2; }
                const TriRecord &T = tris[listed ? f : 0u];
                f3 p0 = mk3(0.0f, 0.0f, 0.0f), p1 = p0, p2 = p0, nh = p0, Lf = p0;
                if (listed) {
                    p0 = ld3(T.p0); p1 = ld3(T.p1); p2 = ld3(T.p2); nh = ld3(T.nhat);
                    const float4 lr = glow_record(gl, true, parts.shade, (int32_t)f);
                    Lf = mk3(lr.x, lr.y, lr.z);
                }
                const f3 P = mk3((p0.x + u1 * (p1.x - p0.x)) + u2 * (p2.x - p0.x), (p0.y + u1 * (p1.y - p0.y)) + u2 * (p2.y - p0.y),
                                 (p0.z + u1 * (p1.z - p0.z)) + u2 * (p2.z - p0.z));
                const f3 v = sub3(P, O);
                const float v2 = dot3(v, v);
                const float vl = sqrtf(v2);
                const f3 w = mk3(v.x / vl, v.y / vl, v.z / vl);
                const float nw = dot3(n, w);
                const float cf = fabsf(dot3(nh, w));
                if (mesh) {
                    Ld = w; ndw = nw; Le = Lf; self = f;
                    go = listed && v2 > 0.0f && nw > 0.0f;
                    g = Mf * inv_pdf * nw * cf * 0.318309886f / v2;
                    s = p.n_spheres;   // (every sphere is ahead of the mesh in the order: each occludes at t <= t_f)
                }
                face_ok = face_hit_t(T, O, Ld, mesh && go, ts);
            }
            // visibility: the ray's own sphere or face, then the others by the nearest-hit rule's ties, then the mesh
            float tsph = 0.0f;
            const bool sph_ok = !mesh && go && sphere_ray_intersect_t(C, R, O, Ld, tsph);
            if (!mesh) ts = tsph;
            bool reach = mesh ? face_ok : sph_ok;
            for (uint32_t q = 0; q < p.n_spheres; q++) {
                float tq;
                if (reach && q != s && sphere_ray_intersect_t(ld3(p.spheres[q].center), p.spheres[q].radius, O, Ld, tq))
                    if (q < s ? tq <= ts : tq < ts) reach = false;
            }
            if (p.n_tris) {
                const SlabRay sr = make_slab_ray(O, Ld);
                bool occ;
                if (NODES_IN_LDS) occ = bvh_occluded_before<true>(s_nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, Ld, sr, ts, reach, self);
                else occ = bvh_occluded_before<true>(bvh.nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, Ld, sr, ts, reach, self);
                reach = reach && !occ;
            }
            if (gl.light & 4u) g = mis_weight(g);   // (uniform) RWR_FLAG_LIGHT_MIS item 4
            if (reach) add_contribution(sh, e, thr.x * (Le.x * g), thr.y * (Le.y * g), thr.z * (Le.z * g));
            n_rays += (uint32_t)__popcll(__ballot(go));
            n_reached += (uint32_t)__popcll(__ballot(reach));
            n_part_rays += (uint32_t)__popcll(__ballot(mesh && go));
            n_part_reached += (uint32_t)__popcll(__ballot(mesh && reach));
            }
        }
        __syncthreads();
        flush_pool(sh, p, wf, tile);
    }
    if (lane == 0u && n_rays) {
        atomicAdd(&gl.light_counts[0], (unsigned long long)n_rays);
        if (n_reached) atomicAdd(&gl.light_counts[1], (unsigned long long)n_reached);
        if (PARTS && n_part_rays) atomicAdd(&gl.light_counts[3], (unsigned long long)n_part_rays);
        if (PARTS && n_part_reached) atomicAdd(&gl.light_counts[4], (unsigned long long)n_part_reached);
        if (SKY && n_sky_rays) atomicAdd(&gl.light_counts[6], (unsigned long long)n_sky_rays);
        if (SKY && n_sky_reached) atomicAdd(&gl.light_counts[7], (unsigned long long)n_sky_reached);
    }
}

struct LightForms {   // rwr_wf_forms.h
    struct Form { bool nodes_in_lds, stack16, parts, sky; };
    static constexpr uint32_t kRange = 16u;
    static constexpr uint32_t encode(Form f) { return f.nodes_in_lds + 2u * f.stack16 + 4u * f.parts + 8u * f.sky; }
    static constexpr Form decode(uint32_t i) { return Form{(i & 1u) != 0, (i & 2u) != 0, (i & 4u) != 0, (i & 8u) != 0}; }
    static constexpr bool valid(Form) { return true; }
    using Kernel = decltype(&k_wf_light<false, false, false>);
    template <uint32_t I> static constexpr Kernel kernel() { return &k_wf_light<decode(I).nodes_in_lds, decode(I).stack16, decode(I).parts, decode(I).sky>; }
};
static constexpr auto kLightForms = form_table<LightForms>();
static_assert(check_forms<LightForms>(16), "nodelets in LDS or not, 16-bit stacks or not, the mesh light or not, the sky's image or not");

// gen: the generation whose hits' light samples these are (0: h0's, behind the primary stage) — RNG block 274 + 17 gen, behind
// soft shadows' last (130 + 16 * 8 + 15 = 273).  expected_tiles: as launch_wf_shadow.
hipError_t launch_wf_light(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const BvhDevice &bvh, const WfBuffers &wf,
                           const WfGlow &glow, const WfLights &lights, const WfPartLights &parts, const WfSkyImage &sky, uint32_t n_tiles,
                           uint32_t expected_tiles, uint32_t sample_count, uint32_t gen, uint32_t sample_base)
{
    if (n_tiles == 0 || sample_count == 0 || (lights.m == 0 && parts.n == 0 && sky.table == nullptr)) return hipSuccess;
    const uint32_t work_tiles = std::max(1u, std::min(expected_tiles, n_tiles));
    const uint32_t n_shares = std::max(1u, std::min(std::min(32u, sample_count * 8u), 4096u / work_tiles));
    const dim3 grid((uint32_t)std::min<uint64_t>(2048u, (uint64_t)n_tiles * n_shares));
    const LaneLdsPlan l = lane_lds_plan(bvh, fp, false);   // (no 1 024-thread form here)
    hipLaunchKernelGGL(kLightForms[LightForms::encode({l.nodes_in_lds, l.stack16, parts.n != 0u, sky.table != nullptr})], grid, dim3(256), l.bytes, s, fp, tris, bvh, wf, glow,
                       n_tiles, sample_count, n_shares, 274u + 17u * gen, sample_base, lights, parts, sky);
    return hipGetLastError();
}

hipError_t preload_kernels_wf_light()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>((&k_wf_light<true, true, false>)));
}

}  // namespace rwr
