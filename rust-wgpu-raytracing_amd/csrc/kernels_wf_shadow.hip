// Wavefront integrator, shadow stage (RWR_FLAG_SHADOWS; definition: include/rwr_hip.h).
//
// Every hit the integrator shades — the primary stage's h0, a trace kernel's h_k — has added the AMBIENT part of its term to the
// sums and left a shadow record at its fixed queue slot (rwr_internal.h ShadowRec), with its bit in the shadow ballots.
//   k_wf_shadow   runs once behind the primary stage and once behind every generation's trace kernels, on the launch group's
//                 stream: traces the records any-hit (spheres, then the BVH: rwr_bvh.h bvh_occluded) towards the light of the
//                 shader that shaded the hit and adds, for every ray that got through, the record's fixed-point difference
//                 fix(lit term) - fix(ambient term) to the tile's sums (LDS, then the frame's planes: rwr_wf_pool.h).  Wrapping
//                 integer sums: ambient + (lit - ambient) is the lit term's bits, whoever adds what when.
// Work item = (tile, share of its ballot words); a wave takes one ballot word — 64 slots, one record per lane — at a time and
// skips empty words.  All rays towards one light are PARALLEL: the direction, the slab test's reciprocals and its near-plane choice
// are made on the host and arrive as kernel arguments (wave-uniform scalars; rwr_bvh.h SlabDir); everything else of the walk —
// origin terms, node, stack, face records — is per lane, as in k_wf_trace_lane.  A word whose records want both lights (a sphere
// hit among mesh hits) is traced once per light.
// The origin and the two hit tests are written operation for operation like the oracle; boxes only skip what cannot be hit.
// SOFT forms (RWR_FLAG_SOFT_SHADOWS; definition: include/rwr_hip.h): the lights have an angular size, and a ray runs towards a
// point of its light's disk, S = L + r (a b1 + b b2).  A lane finds its global pixel and sample from (tile, slot) the way
// emit_next_ray does and draws (a, b) by bounce_direction's rejection loop ONCE, ahead of the two-light loop (two registers
// across it; the basis and the radius of a light are wave-uniform scalars, WfSoft); per light it forms S and its own slab
// constants (make_slab_ray) and walks the same any-hit traversal with a per-lane direction.  The hard forms keep their code: what
// the SOFT forms need arrives in a kernel argument of its own behind the others.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "rwr_bvh.h"
#include "rwr_wf_forms.h"
#include "rwr_wf_pool.h"

namespace rwr {

struct ShadowLights { float dir[2][3]; SlabDir slab[2]; };   // [0] the mesh shader's light, [1] the sphere shader's

template <bool NODES_IN_LDS, bool STACK16, bool SOFT>
__global__ void __launch_bounds__(256)
k_wf_shadow(const FrameParams p, const TriRecord *__restrict__ tris, const BvhDevice bvh, const WfBuffers wf, const WfShadow sw,
            uint32_t n_tiles, uint32_t sample_count, uint32_t n_shares, const ShadowLights lights, const WfSoft soft)
{
    __shared__ TraceShared sh;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    BvhNode4 *s_nodes = reinterpret_cast<BvhNode4 *>(s_dyn);
    const uint32_t node_bytes = NODES_IN_LDS ? bvh.n_nodes * (uint32_t)sizeof(BvhNode4) : 0u;
    typedef typename std::conditional<STACK16, uint16_t, uint32_t>::type StackT;
    StackT *s_stack = reinterpret_cast<StackT *>(s_dyn + node_bytes);
    // the tiles anything can be seen through, when the frame listed them (the others hold no record — and, behind the primary
    // stage, ballots nobody wrote)
    const uint32_t n_live = wf.live_list ? (uint32_t)__builtin_amdgcn_readfirstlane((int)*wf.live_count) : n_tiles;
    const uint32_t n_items = n_live * n_shares, n_words = sample_count * 8u;
    uint32_t n_rays = 0, n_occluded = 0;   // this wave's (wave-uniform)
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
        const unsigned long long *__restrict__ masks = sw.masks + (size_t)tile * wf.group * 8u;
        const ShadowRec *__restrict__ recs = sw.recs + (size_t)tile * wf.group * kWfTilePixels;
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
            uint4 ra = make_uint4(0u, 0u, 0u, 0u), rb = ra;
            if (live) {
                const uint4 *src = reinterpret_cast<const uint4 *>(recs + e);
                ra = src[0]; rb = src[1];
            }
            const f3 O = mk3(__uint_as_float(ra.x), __uint_as_float(ra.y), __uint_as_float(ra.z));
            float da = 0.0f, db = 0.0f;   // SOFT: the lane's point on the unit disk
            if (SOFT) {
                // the slot's pixel (as add_contribution maps it) and sample, as emit_next_ray finds them
                const uint32_t r = e & (kWfTilePixels - 1u), wv = r >> 7, k = (r >> 6) & 1u, l = r & 63u;
                const uint32_t px = (tile % wf.tiles_x) * kWfTileW + (wv & 1u) * 32u + 2u * (l & 15u) + k;
                const uint32_t py = p.row_begin + (tile / wf.tiles_x) * p.row_pitch + (wv >> 1) * 4u + (l >> 4);
                const uint32_t pixel = py * p.width + px, sample = soft.sample_base + e / kWfTilePixels;
                // bounce_direction's rejection loop, operation for operation (dim0 is even: a try is one pair of RWR_FLAG_SOBOL's sequence)
                rng_disk_point(pixel, sample, soft.dim0, p.seed, (p.flags & RWR_FLAG_SOBOL) != 0u, da, db);
            }
            bool occluded = false;
#pragma unroll
            for (uint32_t kind = 0; kind < 2u; kind++) {
                const bool mine = live && (ra.w & 1u) == kind;
                if (!__any(mine)) continue;   // uniform
                f3 L = mk3(lights.dir[kind][0], lights.dir[kind][1], lights.dir[kind][2]);
                if (SOFT) {   // S = L + r (a b1 + b b2): two products and a sum inside, one product, one sum; not re-normalised
                    const float rl = soft.radius[kind];
                    L = mk3(L.x + rl * (da * soft.b1[kind][0] + db * soft.b2[kind][0]), L.y + rl * (da * soft.b1[kind][1] + db * soft.b2[kind][1]),
                            L.z + rl * (da * soft.b1[kind][2] + db * soft.b2[kind][2]));
                }
                bool occ = false;
                for (uint32_t s = 0; s < p.n_spheres; s++) {   // spheres first, literal sphereRayIntersect
                    float ts;
                    if (mine && sphere_ray_intersect_t(ld3(p.spheres[s].center), p.spheres[s].radius, O, L, ts)) occ = true;
                }
                if (p.n_tris) {
                    const bool go = mine && !occ;
                    bool o2;
                    if (SOFT) {   // a direction per lane: its own reciprocals and near planes
                        const SlabRay sr = make_slab_ray(O, L);
                        if (NODES_IN_LDS) o2 = bvh_occluded(s_nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, L, sr, go);
                        else o2 = bvh_occluded(bvh.nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, L, sr, go);
                    } else if (NODES_IN_LDS) o2 = bvh_occluded(s_nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, L, lights.slab[kind], go);
                    else o2 = bvh_occluded(bvh.nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, L, lights.slab[kind], go);
                    occ = occ || (go && o2);
                }
                occluded = occluded || (mine && occ);
            }
            if (live && !occluded) {   // the light reaches the hit: ambient part -> lit term
                const unsigned long long hi = 0xffffffff00000000ull;
                add_fixed(sh, e, (unsigned long long)rb.x | ((ra.w & 2u) ? hi : 0ull), (unsigned long long)rb.y | ((ra.w & 4u) ? hi : 0ull),
                          (unsigned long long)rb.z | ((ra.w & 8u) ? hi : 0ull));
            }
            n_rays += (uint32_t)__popcll(m);
            n_occluded += (uint32_t)__popcll(__ballot(live && occluded));
        }
        __syncthreads();
        flush_pool(sh, p, wf, tile);
    }
    if (lane == 0u && n_rays) {
        atomicAdd(&sw.counts[0], (unsigned long long)n_rays);
        if (n_occluded) atomicAdd(&sw.counts[1], (unsigned long long)n_occluded);
    }
}

struct ShadowForms {   // rwr_wf_forms.h
    struct Form { bool nodes_in_lds, stack16, soft; };
    static constexpr uint32_t kRange = 8u;
    static constexpr uint32_t encode(Form f) { return f.nodes_in_lds + 2u * f.stack16 + 4u * f.soft; }
    static constexpr Form decode(uint32_t i) { return Form{(i & 1u) != 0, (i & 2u) != 0, (i & 4u) != 0}; }
    static constexpr bool valid(Form) { return true; }
    using Kernel = decltype(&k_wf_shadow<false, false, false>);
    template <uint32_t I> static constexpr Kernel kernel() { return &k_wf_shadow<decode(I).nodes_in_lds, decode(I).stack16, decode(I).soft>; }
};
static constexpr auto kShadowForms = form_table<ShadowForms>();
static_assert(check_forms<ShadowForms>(8), "nodelets in LDS or not, 16-bit stacks or not, lights of a size or not");

hipError_t launch_wf_shadow(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const BvhDevice &bvh, const WfBuffers &wf,
                            const WfShadow &shadow, uint32_t n_tiles, uint32_t expected_tiles, uint32_t sample_count, const float light_mesh[3],
                            const float light_sphere[3], uint32_t gen, uint32_t sample_base, const rwr_shadow_params *soft,
                            LanePlanRecord *plan)
{
    if (n_tiles == 0 || sample_count == 0) return hipSuccess;
    ShadowLights lights;
    for (int k = 0; k < 3; k++) { lights.dir[0][k] = light_mesh[k]; lights.dir[1][k] = light_sphere[k]; }
    for (int l = 0; l < 2; l++) {   // make_slab_ray's direction terms (rwr_bvh.h), the same IEEE divisions
        const float *d = lights.dir[l];
        const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
        uint32_t sign[3];
        for (int k = 0; k < 3; k++) { uint32_t u; std::memcpy(&u, &inv[k], 4); sign[k] = u >> 31; }
        lights.slab[l] = SlabDir{inv[0], inv[1], inv[2], 3u * sign[0], 3u * sign[1] + 1u, 3u * sign[2] + 2u};
    }
    WfSoft sf{};
    if (soft) {   // bounce_direction's basis about each light (rwr_device.h), the same f32 operations (this unit is built without contraction)
        for (int l = 0; l < 2; l++) {
            const float *n = lights.dir[l];
            const float sign = std::copysign(1.0f, n[2]);
            const float aa = -1.0f / (sign + n[2]);
            const float bb = n[0] * n[1] * aa;
            sf.b1[l][0] = 1.0f + sign * n[0] * n[0] * aa; sf.b1[l][1] = sign * bb; sf.b1[l][2] = -sign * n[0];
            sf.b2[l][0] = bb; sf.b2[l][1] = sign + n[1] * n[1] * aa; sf.b2[l][2] = -n[1];
        }
        sf.radius[0] = soft->mesh_light_radius; sf.radius[1] = soft->sphere_light_radius;
        sf.dim0 = 2u + 16u * RWR_MAX_BOUNCES + 16u * gen;
        sf.sample_base = sample_base;
    }
    // enough work items to fill the chip a few times over when the tiles with work are few — expected_tiles: the live tiles of
    // the frame before when this frame walks a live list, else all of them (a share zeroes and flushes 12 KiB of sums; any
    // split gives the same frame)
    const uint32_t work_tiles = std::max(1u, std::min(expected_tiles, n_tiles));
    const uint32_t n_shares = std::max(1u, std::min(std::min(32u, sample_count * 8u), 4096u / work_tiles));
    const dim3 grid((uint32_t)std::min<uint64_t>(2048u, (uint64_t)n_tiles * n_shares));
    const LaneLdsPlan l = lane_lds_plan(bvh, fp, false);   // (no 1 024-thread form here)
    if (plan) *plan = LanePlanRecord{plan->launches + 1u, l.nodes_in_lds, l.stack16, l.wide};
    hipLaunchKernelGGL(kShadowForms[ShadowForms::encode({l.nodes_in_lds, l.stack16, soft != nullptr})], grid, dim3(256), l.bytes, s, fp, tris, bvh, wf, shadow,
                       n_tiles, sample_count, n_shares, lights, sf);
    return hipGetLastError();
}

hipError_t preload_kernels_wf_shadow()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>((&k_wf_shadow<true, true, false>)));
}

}  // namespace rwr
