// Wavefront integrator, second stage: the bounce rays of one launch group (kernels_wf_primary.hip).
//
// The unit of work is a POOL: everything the 64x8 pixels of one tile of the primary stage emitted in the group's
// samples (up to 32 x 512 rays: origins within one small patch of surface, directions all over the hemisphere).
// Three kernels per launch group:
//   k_wf_sort          (one workgroup per pool) steps 1 below + how the pool is traced;
//   k_wf_trace_packet  well-filled compact pools: 128 rays per wave walk the BVH together (see there);
//   k_wf_trace_lane    the other pools: one ray per lane, rwr_bvh.h.
// The trace kernels are persistent (2048 workgroups pulling work items from a device counter); into how many work
// items a pool is cut is decided ON THE DEVICE from the number of live pools the sort counted (pool_split): one
// when the frame fills the chip by itself, up to 32 when only a few tiles see the mesh — otherwise four waves
// would chew through thousands of rays while 250 CUs idle.
//                  1. compaction + sort, in one: the ballots the primary stage published say which fixed queue
//                     slots hold a ray; every ray's direction is binned (octant x 16x16 cells of the octahedral map,
//                     Morton order inside an octant), a histogram / prefix sum / scatter through LDS atomics
//                     leaves the pool's live slots in direction order (wf.sorted, 2 B per ray).
//                     Rays of one wave then start from almost the same point in almost the same direction:
//                     they walk the BVH together (measured on the simulator, tools/sim: 62 -> 36 wave
//                     instructions per ray at cfg3 — neighbouring queue entries share an origin, not a direction).
//                  2. traversal: per-lane, 4-wide BVH with nodelets staged in LDS (rwr_bvh.h), the reference's
//                     exact hit test with ties broken by face index — the winner equals the brute-force
//                     winner (oracle) for any visiting order.
//                  3. shading of the second hit; the contribution albedo(h0) * E(h1) is added to the pool's
//                     per-pixel sums in LDS as 64-bit FIXED-POINT atomics: integer sums do not depend on the
//                     order in which rays retire, so the frame is bit-reproducible whatever the sort did.
//                  4. the work item's sums go to the frame's fixed-point planes (WfBuffers::fix) by integer atomics:
//                     another share of the pool, the primary stage of the other launch group in flight or nobody may
//                     be adding to the same pixels at the same time — the sums are the same bits.
// On frames that show little the sort strides over the live tiles k_wf_classify listed instead of visiting every pool.
//
// Deeper paths (RWR_FLAG_MULTI_BOUNCE, max_bounces B >= 2): the host runs the sort and the trace kernels once per GENERATION
// of rays, B times per launch group.  Every generation but the last uses the trace kernels' EMIT forms: besides adding the
// term T * E(h) a hit writes the path's next ray back into ITS OWN fixed slot (a slot's pixel never changes, so the sums and
// their flush stay as they are), with its direction bin, and sets the slot's bit in the next generation's ballots
// (WfEmit::masks_out, cleared before, swapped with WfBuffers::masks after the generation).  The last generation runs the plain forms.
// Nothing here decides what the first hit shows; bounce rays are the oracle's rays bit for bit (first stage) and
// their nearest hits are exact, so the stage's output differs from the oracle's only by the fixed-point rounding
// of the terms and of the throughput (tolerance 1e-4).
#include <atomic>
#include <algorithm>
#include <type_traits>

#include "rwr_bvh.h"
#include "rwr_primary.h"
#include "rwr_shade_p2.h"
#include "rwr_wf_forms.h"
#include "rwr_wf_pool.h"

namespace rwr {

// Per pool, written by k_wf_sort and read by the two trace kernels.
struct PoolInfo {
    uint32_t n_rays;         // 0: nothing to trace
    uint32_t packets;        // 1: packet traversal, 0: per-lane traversal
    uint32_t oct_begin[9];   // sorted position where each octant's rays begin; [8] = n_rays
    uint32_t pad;
};
static_assert(sizeof(PoolInfo) == 48, "PoolInfo is 48 B");

constexpr uint32_t kWfMaxSplit = 32;       // at most this many work items share one pool
constexpr uint32_t kWfWholePools = 1024;   // this many live pools keep the chip busy by themselves
constexpr uint32_t kWfTargetItemsDense = 4096;
constexpr uint32_t kWfTraceGroups = 2048;  // workgroups of a trace launch (persistent: they pull work items)
// Fewer packet pools than `min_packet_pools` (default 64, BvhDevice) in a launch group: the per-lane kernel takes them
// (a packet is one long chain of dependent scalar loads; a handful of them on an otherwise idle chip take longer
// than everything else in the frame).
// device counters of one launch group (one set per ray queue, WfBuffers::counters): pools of each class, work items handed out
enum { kLivePackets = 0, kLiveLane = 1, kWorkPackets = 2, kWorkLane = 3, kCountersPerQueue = 4 };

// float -> uint32 key whose unsigned order is the float order
RWR_DEV uint32_t float_key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
RWR_DEV float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// Into how many work items a pool of a class with `live` pools in this launch group is cut: one when the frame
// keeps the chip busy by itself, up to kWfMaxSplit when only a few tiles see anything (a small mesh on an empty
// screen: otherwise four waves would walk through a pool of thousands of rays one after the other while 250 CUs idle).
RWR_DEV uint32_t pool_split(uint32_t live, bool packets, uint32_t lane_items)
{
    if (live == 0u) return 1u;
    // just enough pieces that every workgroup gets a few items and the last round is short: every share zeroes and flushes
    // 12 KiB of sums (measured at configs[2], 4 050 packet pools: two shares beat one by 8 % and five by 6 %; a 135-row band
    // of the same frame, 510 packet pools: 8 shares, not 32 — 2.9 -> 1.9 ms).  Few pools of the per-lane class (a small mesh on
    // an empty screen: their rays are few, the traversals long): one 256-ray chunk per item.
    const uint32_t target = (packets || live >= kWfWholePools) ? kWfTargetItemsDense : lane_items;
    return min(kWfMaxSplit, max(1u, (target + live - 1u) / live));
}

struct SortShared {
    unsigned long long masks[kWfMaxGroup * 8u];
    uint32_t hist[kWfDirBins];   // rays per direction bin, then (in place) where the bin's next ray goes in the sorted list
    uint32_t lo[3], hi[3];   // bounds of the ray origins of the group's first samples (order-preserving keys)
    uint32_t wave_sum[4];
    uint32_t total;
};

// Steps 0 and 1 for one pool: the published ballots -> live slot count; how it will be traced; direction sort ->
// wf.sorted[pool] holds the live slots octant by octant, fine bins in Morton order inside; the pool is appended to
// its class's list.  Queue reads are issued eight at a time per thread (the kernel is all memory latency).
// A pool is traced as PACKETS when it is well filled (min_fill rays) and its rays start close together compared
// with the geometry (origins within bvh.packet_extent): then the rays of one direction bin really travel
// together.  A tile that spans many small faces (a distant instance) is not such a pool.
template <uint32_t NT>
RWR_DEV void sort_pool(SortShared &sh, uint16_t *s_bins, const uint32_t tile, const WfBuffers &wf, PoolInfo *__restrict__ info,
                       uint32_t *__restrict__ counters, uint32_t *__restrict__ pool_list, uint32_t n_tiles,
                       uint32_t sample_count, uint32_t min_fill, float packet_extent, uint32_t dense_rays)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t n_masks = sample_count * 8u, n_slots = sample_count * kWfTilePixels;
    if (tid == 0u) sh.total = 0u;
    if (tid < 3u) { sh.lo[tid] = 0xffffffffu; sh.hi[tid] = 0u; }
    __syncthreads();
    if (tid < n_masks) {
        const unsigned long long m = wf.masks[(size_t)tile * wf.group * 8u + tid];
        sh.masks[tid] = m;
        if (m) atomicAdd(&sh.total, (uint32_t)__popcll(m));
    }
    for (uint32_t i = tid; i < kWfDirBins; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    const uint32_t n_rays = sh.total;
    if (n_rays == 0u) {  // uniform
        if (tid == 0u) info[tile].n_rays = 0u;
        return;
    }
    const size_t pool_base = (size_t)tile * wf.group * kWfTilePixels;
    // (a pool of very many rays sorts into packets that are tight in DIRECTION whatever patch of surface they start from: a
    // packet covers 128 / n_rays of the sphere)
    const bool dense = dense_rays != 0u && n_rays >= dense_rays;
    bool packets = dense || n_rays >= min_fill;
    if (packets && !dense) {   // uniform: how far apart do the rays start?  (the first two samples' slots)
        constexpr int kPerThread = 1024 / (int)NT;
        float4 o[kPerThread];
        bool live_slot[kPerThread];
#pragma unroll
        for (int u = 0; u < kPerThread; u++) {
            const uint32_t e = tid + NT * (uint32_t)u;
            live_slot[u] = e < n_slots && ((sh.masks[e >> 6] >> (e & 63u)) & 1ull);
            o[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (live_slot[u]) o[u] = wf.rays[2u * (pool_base + e)];
        }
        uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
#pragma unroll
        for (int u = 0; u < kPerThread; u++)
            if (live_slot[u]) {
                const uint32_t k[3] = {float_key(o[u].x), float_key(o[u].y), float_key(o[u].z)};
#pragma unroll
                for (int c = 0; c < 3; c++) { lo[c] = min(lo[c], k[c]); hi[c] = max(hi[c], k[c]); }
            }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                lo[c] = min(lo[c], (uint32_t)__shfl_xor((int)lo[c], d));
                hi[c] = max(hi[c], (uint32_t)__shfl_xor((int)hi[c], d));
            }
        if ((tid & 63u) == 0u)
            for (int c = 0; c < 3; c++) { atomicMin(&sh.lo[c], lo[c]); atomicMax(&sh.hi[c], hi[c]); }
        __syncthreads();
        float ext = 0.0f;
        if (sh.hi[0] >= sh.lo[0])
            ext = fmaxf(fmaxf(key_float(sh.hi[0]) - key_float(sh.lo[0]), key_float(sh.hi[1]) - key_float(sh.lo[1])),
                        key_float(sh.hi[2]) - key_float(sh.lo[2]));
        packets = ext <= packet_extent;   // a NaN extent: no packets
    }
    // histogram of the direction bins; e = sample * 512 + wave * 128 + k * 64 + lane
    for (uint32_t e0 = tid; e0 < n_slots; e0 += NT * 8u) {
        uint32_t bin[8];   // the primary stage stored every ray's bin beside it: 2 B to read instead of the 32-byte record
        bool live_slot[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t e = e0 + NT * (uint32_t)u;
            live_slot[u] = e < n_slots && ((sh.masks[e >> 6] >> (e & 63u)) & 1ull);
            bin[u] = 0xffffu;
            if (live_slot[u]) bin[u] = min((uint32_t)wf.bins[pool_base + e], kWfDirBins - 1u);
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t e = e0 + NT * (uint32_t)u;
            if (e < n_slots) {
                s_bins[e] = (uint16_t)bin[u];
                if (live_slot[u]) atomicAdd(&sh.hist[bin[u]], 1u);
            }
        }
    }
    __syncthreads();
    {   // exclusive prefix over the bins by the first 256 threads: kPer consecutive bins each, shuffle scan inside a wave, four
        // wave totals through LDS
        constexpr uint32_t kPer = kWfDirBins / 256u;
        static_assert(kWfDirBins % 2048u == 0u || kWfDirBins == 512u, "whole bins per thread, an octant starts at a thread's first bin");
        const bool scan = tid < 256u;   // (whole waves)
        uint32_t c[kPer], sum = 0, incl = 0;
        if (scan) {
#pragma unroll
            for (uint32_t k = 0; k < kPer; k++) { c[k] = sh.hist[kPer * tid + k]; sum += c[k]; }
            incl = sum;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
                if ((int)(tid & 63u) >= d) incl += up;
            }
            if ((tid & 63u) == 63u) sh.wave_sum[tid >> 6] = incl;
        }
        __syncthreads();
        if (scan) {
            uint32_t before = incl - sum;
            for (uint32_t w = 0; w < (tid >> 6); w++) before += sh.wave_sum[w];
            if ((tid & 31u) == 0u) info[tile].oct_begin[tid >> 5] = before;   // octant o begins at bin (kWfDirBins / 8) o = kPer * (32 o)
#pragma unroll
            for (uint32_t k = 0; k < kPer; k++) { sh.hist[kPer * tid + k] = before; before += c[k]; }   // (its own bins: in place)
        }
    }
    if (tid == 0u) {
        info[tile].oct_begin[8] = n_rays;
        info[tile].n_rays = n_rays;
        info[tile].packets = packets ? 1u : 0u;
        // append to the class's pool list (order of arrival: any order gives the same frame)
        const uint32_t pos = atomicAdd(&counters[(packets ? kLivePackets : kLiveLane)], 1u);
        pool_list[(packets ? 0u : n_tiles) + pos] = tile;
        if (wf.dbg) {
            atomicAdd(&wf.dbg[packets ? 0 : 2], 1ull);
            atomicAdd(&wf.dbg[packets ? 1 : 3], (unsigned long long)n_rays);
        }
    }
    __syncthreads();
    // scatter inside LDS (64 two-byte stores to 64 different places would cost the memory pipe a cycle each), then the
    // sorted list goes out in whole 16-byte pieces
    uint16_t *s_sorted = s_bins + n_slots;
    for (uint32_t e = tid; e < n_slots; e += NT) {
        const uint32_t bin = s_bins[e];
        if (bin != 0xffffu) s_sorted[atomicAdd(&sh.hist[bin], 1u)] = (uint16_t)e;
    }
    __syncthreads();
    uint4 *__restrict__ out = reinterpret_cast<uint4 *>(wf.sorted + pool_base);   // pool_base is a multiple of 512
    const uint4 *src = reinterpret_cast<const uint4 *>(s_sorted);
    for (uint32_t i = tid; i < (n_rays + 7u) / 8u; i += NT) out[i] = src[i];
}

// One workgroup per pool — or, on a frame that shows little, workgroups striding over the live tiles of k_wf_classify's list
// (the other tiles emitted nothing and nobody looks at their pools).
#ifndef RWR_SORT_THREADS
#define RWR_SORT_THREADS 1024
#endif
constexpr uint32_t kWfSortThreads = RWR_SORT_THREADS;   // (a pool's sort is all latency; on whole frames 256 and 1024 measure the same — the
                                                        // sort hides behind the other queue — on a band of 510 pools 1024 is 3x faster)
static_assert(kWfSortThreads >= kWfMaxGroup * 8u && kWfSortThreads >= 256u, "one thread per ballot word of a pool; the prefix sum needs four waves");
template <bool LIST>
__global__ void __launch_bounds__(kWfSortThreads)
k_wf_sort(const WfBuffers wf, PoolInfo *__restrict__ info, uint32_t *__restrict__ counters, uint32_t *__restrict__ pool_list,
          uint32_t n_tiles, uint32_t sample_count, uint32_t min_fill, float packet_extent, uint32_t dense_rays)
{
    __shared__ SortShared sh;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    uint16_t *s_bins = reinterpret_cast<uint16_t *>(s_dyn);   // direction bin of every slot (0xffff: no ray), then the sorted list: 2 x 2 B x sample_count x 512
    if (!LIST) {
        sort_pool<kWfSortThreads>(sh, s_bins, blockIdx.x, wf, info, counters, pool_list, n_tiles, sample_count, min_fill, packet_extent, dense_rays);
        return;
    }
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)*wf.live_count);
    for (uint32_t t = blockIdx.x; t < n; t += gridDim.x) {
        const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)wf.live_list[t]);
        sort_pool<kWfSortThreads>(sh, s_bins, tile, wf, info, counters, pool_list, n_tiles, sample_count, min_fill, packet_extent, dense_rays);
        __syncthreads();   // (the next pool reuses the LDS)
    }
}

// emit_next_ray's view of its WfGlow argument: the mark of the ray a hit sends on — 1 (0xffff as unorm16) for a diffuse ray of a frame
// that samples its lights, else the 0 the records always held
RWR_DEV float light_mark(const WfGlow &gl, bool mirror, float eta, float rho) { return (gl.light && !mirror && eta == 0.0f && rho == 0.0f) ? 1.0f : 0.0f; }
RWR_DEV LightRec *light_recs_of(const WfGlow &gl) { return gl.light_recs; }
RWR_DEV unsigned long long *light_masks_of(const WfGlow &gl) { return gl.light_masks; }

// EMIT forms: the next ray of the path whose ray hit (obj, t) — from P + 1e-4 n (P = O + t D, n = the face's normal flipped
// towards the ray or the sphere's outward normal, as the first stage builds the first bounce ray), in the cosine-distributed
// direction of RNG dimensions em.next_dim ... keyed by the slot's global pixel and sample, throughput thr — goes back into slot
// e of the tile's pool; the slot's bit is set in the next generation's ballots.
// MIRROR forms (RWR_FLAG_MIRRORS; SURF != kSurfNone), a hit on a mirror surface (`mirror`): the direction is the reflection of D
// about n instead (reflect_direction: no random number is read, the generation's RNG dimensions are left unused), thr is T * R.
// Glass forms (RWR_FLAG_GLASS; SURF == kSurfGlass), a hit on glass (`eta` != 0, its index): direction and side by
// refract_or_reflect with the generation's first random number, origin P + 1e-4 m, thr is T * C — computed here, where the
// traversal's registers are dead.  Returns the hit's SurfaceEvent (rwr_surface.h): refract_or_reflect's, kEventNone for no counted hit.
// Glossy forms (RWR_FLAG_GLOSSY; SURF == kSurfGloss), a hit on a glossy surface (`rho` != 0, its roughness): the diffuse direction
// of the same dimensions goes through gloss_direction — computed for every lane that draws a diffuse direction and selected, so
// that the lanes stay together — thr is T * R.  Returns kEventGlossy for such a hit.
// GLOW forms pass their WfGlow behind the other arguments (gl: one argument or none — the other forms' calls, arguments and code are
// what they were).  With light sampling on (WfGlow::light; rwr_surface.h) a hit that sends on a DIFFUSE ray — no mirror, glass or
// glossy one — marks the ray's record, leaves its normal at the slot and sets the slot's bit in the light ballots, for k_wf_light.
template <int SURF = kSurfNone, typename... Glow>
RWR_DEV uint32_t emit_next_ray(const FrameParams &p, const WfBuffers &wf, const WfEmit &em, const TriRecord *__restrict__ tris, uint32_t tile,
                               uint32_t e, f3 O, f3 D, int32_t obj, float t, float ndotd, f3 thr, bool mirror = false, float eta = 0.0f,
                               float rho = 0.0f, const Glow &...gl)
{
    static_assert(sizeof...(Glow) <= 1u, "the kernel's WfGlow, or nothing");
    f3 n;
    f3 O1 = hit_exit_point(p, tris, O, D, obj, t, ndotd, n);
    f3 D1;
    uint32_t event = kEventNone;
    if constexpr (sizeof...(Glow) != 0u) {   // (here, while n is live anyway)
        if (light_mark(gl..., SURF != kSurfNone && mirror, eta, rho) != 0.0f) {
            *reinterpret_cast<float4 *>(light_recs_of(gl...) + (size_t)tile * wf.group * kWfTilePixels + e) = make_float4(n.x, n.y, n.z, 0.0f);
            atomicOr(&light_masks_of(gl...)[(size_t)tile * wf.group * 8u + (e >> 6)], 1ull << (e & 63u));
        }
    }
    // glossy forms: a ray that starts at P + 1e-4 n (every one but a glass hit's) has its origin and the first two channels of its
    // throughput stored ahead of the direction's arithmetic — five registers fewer across the disk loop and the rule, which these
    // forms hold live together
    if (SURF == kSurfGloss && eta == 0.0f)
        wf.rays[2u * ((size_t)tile * wf.group * kWfTilePixels + e)] = make_float4(O1.x, O1.y, O1.z, wf_pack_unorm16x2(thr.x, thr.y));
    if (SURF != kSurfNone && mirror) {
        D1 = reflect_direction(n, D);
    } else {
        // the slot's pixel (as add_contribution maps it) and sample
        const uint32_t r = e & (kWfTilePixels - 1u), w = r >> 7, k = (r >> 6) & 1u, l = r & 63u;
        const uint32_t px = (tile % wf.tiles_x) * kWfTileW + (w & 1u) * 32u + 2u * (l & 15u) + k;
        const uint32_t py = p.row_begin + (tile / wf.tiles_x) * p.row_pitch + (w >> 1) * 4u + (l >> 4);
        const bool sob = (p.flags & RWR_FLAG_SOBOL) != 0u;   // (uniform) RWR_FLAG_SOBOL: the sequence's numbers in place of the hash's
        if ((SURF == kSurfGlass || SURF == kSurfGloss) && eta != 0.0f) {
            const float u = rng_uniform(py * p.width + px, em.sample_base + e / kWfTilePixels, em.next_dim, p.seed, sob);
            f3 m;
            event = refract_or_reflect(n, D, obj >= 0, ndotd, eta, u, D1, m);
            const f3 P = along(O, t, D);
            O1 = mk3(P.x + m.x * 1e-4f, P.y + m.y * 1e-4f, P.z + m.z * 1e-4f);
        } else {
            f3 Rf = D;
            if (SURF == kSurfGloss) Rf = gloss_reflection(n, D);   // (gloss_direction's first half, ahead of the disk loop: fewer registers across it)
            D1 = bounce_direction(n, py * p.width + px, em.sample_base + e / kWfTilePixels, p.seed, sob, em.next_dim);
            if (SURF == kSurfGloss) {
                const bool glossy = rho != 0.0f;
                const f3 S = gloss_blend(Rf, D1, rho);
                D1 = mk3(glossy ? S.x : D1.x, glossy ? S.y : D1.y, glossy ? S.z : D1.z);
                event = glossy ? kEventGlossy : event;
            }
        }
    }
    const size_t slot = (size_t)tile * wf.group * kWfTilePixels + e;
    if (SURF != kSurfGloss || eta != 0.0f) wf.rays[2u * slot] = make_float4(O1.x, O1.y, O1.z, wf_pack_unorm16x2(thr.x, thr.y));
    if constexpr (sizeof...(Glow) != 0u)   // (the record's spare half: 0xffff on a diffuse ray of a frame that samples its lights)
        wf.rays[2u * slot + 1u] = make_float4(D1.x, D1.y, D1.z, wf_pack_unorm16x2(thr.z, light_mark(gl..., SURF != kSurfNone && mirror, eta, rho)));
    else
    wf.rays[2u * slot + 1u] = make_float4(D1.x, D1.y, D1.z, wf_pack_unorm16x2(thr.z, 0.0f));
    wf.bins[slot] = (uint16_t)wf_direction_bin(D1);
    atomicOr(&em.masks_out[(size_t)tile * wf.group * 8u + (e >> 6)], 1ull << (e & 63u));
    return event;
}

// The surface forms' emit step for the hit (obj, t): the hit's record (rwr_surface.h surface_record), decoded; a surface with a
// model sends on T * its record's colour, a diffuse one T * albedo; emit_next_ray does the rest.  Returns its event.
template <int SURF, typename... Glow>
RWR_DEV uint32_t emit_from_surface(const FrameParams &p, const WfBuffers &wf, const WfEmit &em, const WfSurfaces &sf, const TriRecord *__restrict__ tris,
                                   const ShadeRec *__restrict__ shade, uint32_t tile, uint32_t e, f3 O, f3 D, int32_t obj, float t, float ndotd,
                                   f3 thr, f3 albedo, const Glow &...gl)
{
    const float4 m = surface_record(sf.table, sf.n_parts, p.n_materials > 1u, shade, obj);
    const SurfaceDecode s = decode_surface<SURF>(m.w);
    const f3 next = (s.mirror || s.glass || s.gloss) ? mk3(m.x, m.y, m.z) : albedo;
    return emit_next_ray<SURF>(p, wf, em, tris, tile, e, O, D, obj, t, ndotd, mk3(thr.x * next.x, thr.y * next.y, thr.z * next.z), s.mirror, s.eta, s.rho, gl...);
}

// SHADOW forms: the term T * E(h) of the hit (obj, t) of the ray in slot e is a select between clamp(T * ambient part) and
// clamp(T * E(h)), decided by the hit's shadow ray.  The ambient value goes into the sums here, the record for k_wf_shadow
// (origin = the next bounce ray's, the light of the shader that shades h, the difference of the two fixed-point values) into
// the hit's slot, its bit into the shadow ballots (cleared before the generation).
// GLOW forms: e1 comes with the surface's radiance added, and `le` — that radiance — is added to the ambient part here: ambient(h) + Le(h).
template <bool GLOW = false>
RWR_DEV void shadow_hit(TraceShared &sh, const FrameParams &p, const WfBuffers &wf, const WfShadow &sw, const TriRecord *__restrict__ tris,
                        const ShadeRec *__restrict__ shade, uint32_t tile, uint32_t e, f3 O, f3 D, int32_t obj, float t, float ndotd, f3 thr, f3 e1,
                        f3 le = f3{})
{
    f3 amb = hit_ambient(p, shade, obj);
    if (GLOW) amb = mk3(amb.x + le.x, amb.y + le.y, amb.z + le.z);
    const float cf[3] = {thr.x * e1.x, thr.y * e1.y, thr.z * e1.z}, ca[3] = {thr.x * amb.x, thr.y * amb.y, thr.z * amb.z};
    uint32_t ff[3], fa[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { ff[c] = (uint32_t)(cf[c] * kWfFixedScale); fa[c] = (uint32_t)(ca[c] * kWfFixedScale); }   // (as add_contribution)
    add_fixed(sh, e, fa[0], fa[1], fa[2]);
    f3 n;
    const f3 O1 = hit_exit_point(p, tris, O, D, obj, t, ndotd, n);
    write_shadow_record(sw, (size_t)tile * wf.group * kWfTilePixels + e, (size_t)tile * wf.group * 8u + (e >> 6), e & 63u, O1, obj < 0, fa, ff);
}

// SKY forms (RWR_FLAG_SKY): the ray in slot e, direction D with D.y = dy, throughput thr, found no hit.  Its path ends as ever, and
// its term is clamp(thr * S(D)): S = horizon + (zenith - horizon) * u per channel, u = clamp(0.5 dy + 0.5, 0, 1) (+y is up) — f32
// operations in this order, no contraction (the build's -ffp-contract=off), converted like a hit's term (add_contribution) and added
// to the same sums.  sky is a kernel argument: its six floats sit in scalar registers.
RWR_DEV void add_sky(TraceShared &sh, const WfSky &sky, uint32_t e, float dy, f3 thr)
{
    const float u = fminf(fmaxf(0.5f * dy + 0.5f, 0.0f), 1.0f);
    const float s0 = sky.hr + (sky.zr - sky.hr) * u;
    const float s1 = sky.hg + (sky.zg - sky.hg) * u;
    const float s2 = sky.hb + (sky.zb - sky.hb) * u;
    // (a black sky adds nothing at all: add_fixed skips zeros)
    add_fixed(sh, e, (uint32_t)(thr.x * s0 * kWfFixedScale), (uint32_t)(thr.y * s1 * kWfFixedScale), (uint32_t)(thr.z * s2 * kWfFixedScale));
}
// IMG forms (RWR_FLAG_SKY_IMAGE; SKY forms of their own): S = S_img(D) of the whole direction, four 16-byte taps of the context's
// octahedral map (rwr_device.h sky_image_radiance), on the lanes whose ray missed alone; the term is formed and added as add_sky's.
// si is the kernels' last argument (its pointer and side sit in scalar registers); no other form reads it.
RWR_DEV void add_sky_image(TraceShared &sh, const WfSkyImage &si, uint32_t e, f3 D, f3 thr)
{
    const f3 s = sky_image_radiance(si.image, si.n, D);
    add_fixed(sh, e, (uint32_t)(thr.x * s.x * kWfFixedScale), (uint32_t)(thr.y * s.y * kWfFixedScale), (uint32_t)(thr.z * s.z * kWfFixedScale));
}

// whether a ray record's last word carries emit_next_ray's mark
RWR_DEV bool wf_ray_marked(float w) { return (__float_as_uint(w) >> 16) != 0u; }
// LSKY forms (RWR_FLAG_LIGHT_SKY item 6; forms of their own of the IMG x GLOW forms): the miss of a
// MARKED ray — w is its record's last word — adds no sky term, the light sample of the ray's origin may have aimed at the image
// already; under RWR_FLAG_LIGHT_MIS (gl.light & 4) it adds T * S_img(D) m(g') instead, g' = sky_light_g of D and the normal the
// ray's origin left at its queue slot — and all of S where the sampler cannot go (!(P > 0)).  Such misses, silenced or weighted, are
// counted in light_counts[2] and [8], one atomic per wave each.  Unmarked rays add what add_sky_image adds.
RWR_DEV void add_sky_image_lit(TraceShared &sh, const WfSkyImage &si, const WfGlow &gl, uint32_t e, f3 D, f3 thr, float w, size_t pool_base, bool &suppressed)
{
    f3 s = sky_image_radiance(si.image, si.n, D);
    if (wf_ray_marked(w)) {
        float m = 0.0f;
        suppressed = true;
        if (gl.light & 4u) {   // (uniform)
            const float4 rn = *reinterpret_cast<const float4 *>(gl.light_recs + pool_base + e);
            uint32_t ti, tj;
            float P;
            const float gp = sky_light_g(si.table, si.n, D, dot3(mk3(rn.x, rn.y, rn.z), D), (float)(gl.light >> 8), ti, tj, P);
            m = mis_weight(gp);
            if (!(P > 0.0f)) { m = 1.0f; suppressed = false; }
        }
        s = mk3(s.x * m, s.y * m, s.z * m);
    }
    add_fixed(sh, e, (uint32_t)(thr.x * s.x * kWfFixedScale), (uint32_t)(thr.y * s.y * kWfFixedScale), (uint32_t)(thr.z * s.z * kWfFixedScale));
}
// a wave's suppressed misses (two per lane) into the frame's total of suppressed hits and the sky's share of it; call where the
// wave's lanes have come together again
RWR_DEV void count_sky_suppressed(const WfGlow &gl, bool s0, bool s1 = false)
{
    const unsigned long long active = __ballot(true);
    const uint32_t n = (uint32_t)__popcll(__ballot(s0)) + (uint32_t)__popcll(__ballot(s1));
    if (n && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(active)) {
        atomicAdd(&gl.light_counts[2], (unsigned long long)n);
        atomicAdd(&gl.light_counts[8], (unsigned long long)n);
    }
}

// GLOW forms (RWR_FLAG_EMISSIVE): the local shading of the hit `obj` becomes E'(h) = E(h) + Le(h), Le the radiance of the hit's
// surface (rwr_surface.h glow_record) — one f32 add per channel to the shader's value, ahead of the product with the throughput.
// le: that radiance, for shadow_hit's ambient part.  Returns whether the surface emits (count_glow_hits).
// Light sampling on (gl.light, RWR_FLAG_LIGHT_SAMPLING item 4): O is the origin of the ray that found the hit and `marked` whether
// its record says a diffuse hit sent it.  Such a ray's hit on an emitting sphere that O lies outside of — dot3(C - O, C - O) > R R,
// the light stage's own test on the same origin — takes Le as 0: O's light sample has that light already; such hits are counted.
// gl.light & 4 (RWR_FLAG_LIGHT_MIS item 5; uniform, a scalar branch): a silenced hit takes Le m(gp) instead, gp the g' that
// mis_bounce_g made of the ray and its hit before the hit was shaded.
RWR_DEV bool add_glow(const FrameParams &p, const WfGlow &gl, const ShadeRec *__restrict__ shade, int32_t obj, f3 &e1, f3 &le, f3 O, bool marked,
                      float gp)
{
    float4 g = glow_record(gl, p.n_materials > 1u, shade, obj);
    bool silenced = false;
    if (gl.light) {   // (uniform)
        if ((gl.light & 1u) && marked && obj < -1 && glows(g)) {
            const f3 w = sub3(ld3(p.spheres[-2 - obj].center), O);
            const float R = p.spheres[-2 - obj].radius;
            silenced = dot3(w, w) > R * R;
        }
        // bit 2 (RWR_FLAG_LIGHT_PARTS item 8): such a ray's hit on a face of an emitting part — O's light sample may have aimed there
        const bool face = (gl.light & 2u) && marked && obj >= 0 && glows(g);
        silenced = silenced || face;
        if (silenced) {
            const float m = (gl.light & 4u) ? mis_weight(gp) : 0.0f;   // (0 * Le: Le is finite and not negative, the product +0)
            g = make_float4(g.x * m, g.y * m, g.z * m, 0.0f);
        }
        count_glow_hits(gl.light_counts + 2, silenced);   // (the lanes that shade a hit here: the ballots take whoever is active)
        if (gl.light & 2u) count_glow_hits(gl.light_counts + 5, face);   // (uniform) the mesh light's share
    }
    le = mk3(g.x, g.y, g.z);
    e1 = mk3(e1.x + g.x, e1.y + g.y, e1.z + g.z);
    return glows(g);
}
// RWR_FLAG_LIGHT_MIS item 5: g' — the light sampler's g for the direction the ray (O, D) did take — of the hit (obj, t) of a marked
// ray, in the rule's operations: one float, made where the ray and its hit are at hand anyway, ahead of the shading (the registers of
// D, t and the normals are free again by then).  n is the normal the ray's origin left at its queue slot (pool_base + e): read here, ahead of
// the emit step of the hit, which overwrites it.  The value means something only for a hit add_glow silences (a face whose part
// is not listed has inv_pdf 0, a sphere seen from inside a kc without meaning: neither is silenced).
RWR_DEV float mis_bounce_g(const FrameParams &p, const WfGlow &gl, const ShadeRec *__restrict__ shade, const TriRecord *__restrict__ tris, int32_t obj,
                           f3 O, f3 D, float t, size_t pool_base, uint32_t e)
{
    // (the slot's address is made here, from a copy of e the compiler cannot tie to the ray record's address of long before: that
    // one would stay in registers across the whole traversal)
    asm volatile("" : "+v"(e));
    const float4 rn = *reinterpret_cast<const float4 *>(gl.light_recs + pool_base + e);
    const float nd = dot3(mk3(rn.x, rn.y, rn.z), D);
    // (L and 1 / pi are made here, per call: as loop invariants they would be converted and moved into vector registers ahead of the
    // kernel's item loop and stay there across the traversal, three to four registers that cost the per-lane forms a wave per SIMD)
    uint32_t l = gl.light >> 8;
    float inv_pi = 0.318309886f;
    asm volatile("" : "+s"(l), "+v"(inv_pi));
    const float Lf = (float)l;
    if (obj >= 0) {
        const float inv_pdf = glow_record(gl, p.n_materials > 1u, shade, obj).w;
        const float cf = fabsf(dot3(ld3(tris[obj].nhat), D));
        return Lf * inv_pdf * nd * cf * inv_pi / (t * t);
    }
    const f3 w = sub3(ld3(p.spheres[-2 - obj].center), O);
    const float R = p.spheres[-2 - obj].radius;
    const float s2 = R * R / dot3(w, w);
    const float cmax = sqrtf(fmaxf(0.0f, 1.0f - s2));
    const float kc = s2 / (1.0f + cmax);
    return 2.0f * Lf * kc * nd;
}

// The trace kernels are PERSISTENT: kWfTraceGroups workgroups pull work items — (pool of the class, share of it)
// — from a device counter until the class's live x split items are handed out.  Returns false when none are left.
// Contains barriers; uniform over the workgroup.
RWR_DEV bool next_item(TraceShared &sh, const PoolInfo *__restrict__ info, uint32_t *__restrict__ counters, const uint32_t *__restrict__ pool_list,
                       uint32_t n_tiles, uint32_t want_packets, uint32_t min_packet_pools, uint32_t lane_items, uint32_t &tile, uint32_t &share,
                       uint32_t &n_shares, PoolInfo &pi)
{
    const uint32_t live_p = counters[kLivePackets], live_l = counters[kLiveLane];
    const bool demote = live_p < min_packet_pools;
    if (want_packets && demote) return false;
    const uint32_t live = want_packets ? live_p : live_l + (demote ? live_p : 0u);
    n_shares = pool_split(live, want_packets != 0u, lane_items);
    __syncthreads();   // everybody is done with the previous item (sh.item, sh.acc)
    if (threadIdx.x == 0u) sh.item = atomicAdd(&counters[(want_packets ? kWorkPackets : kWorkLane)], 1u);
    __syncthreads();
    // (values read back from LDS are uniform, but only we know that: readfirstlane keeps everything derived from
    // them — and with it the traversal's node and face loads — on the scalar unit)
    const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.item);
    if (item >= live * n_shares) return false;
    // item -> (share, pool): consecutive items are DIFFERENT pools, so that early items spread over the pools
    share = item / live;
    const uint32_t k = item % live;
    const uint32_t list_pos = want_packets ? k : (k < live_l ? n_tiles + k : k - live_l);
    tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)pool_list[list_pos]);
    pi.n_rays = (uint32_t)__builtin_amdgcn_readfirstlane((int)info[tile].n_rays);
#pragma unroll
    for (int o = 0; o < 9; o++) pi.oct_begin[o] = (uint32_t)__builtin_amdgcn_readfirstlane((int)info[tile].oct_begin[o]);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// Pools that are sparse or spread out (silhouette tiles, distant instances): one ray per lane, per-lane BVH
// traversal with the nodelets and the traversal stacks in LDS (rwr_bvh.h).
// STACK16: 16-bit traversal stack entries (rwr_bvh.h) for scenes of at most 4 095 faces and 32 767 nodes.
#ifdef RWR_LANE_OCC   // (6 waves per SIMD: 80 VGPRs + 92 B of scratch, measured below)
#define RWR_LANE_BOUNDS __launch_bounds__(256, RWR_LANE_OCC)
#else
#define RWR_LANE_BOUNDS __launch_bounds__(256)
#endif
// WIDE: a workgroup of 1 024 threads that shares ONE copy of the nodelets in LDS (a BVH too large for four 256-thread
// workgroups per CU to hold a copy each — 508 nodes = 65 KB at configs[3] — but small enough for one per CU): every node fetch
// of the traversal then comes from LDS instead of through the vector memory pipe, 64 different 16-byte pieces per load.
// EMIT: a generation of a deeper path that is not its last (emit_next_ray).
// SHADOW: RWR_FLAG_SHADOWS — a hit adds its term's ambient part and leaves a shadow record (shadow_hit); separate instantiations,
// so that frames without the flag keep their kernels.
// SKY: RWR_FLAG_SKY — a ray that hits nothing adds the sky's term (add_sky); separate instantiations for the same reason.
// LSKY: RWR_FLAG_LIGHT_SKY — of the IMG x GLOW forms alone: the miss of a marked ray is silenced or weighted (add_sky_image_lit);
// separate instantiations, so that the IMG forms without the flag keep their instructions and registers: behind a run-time switch
// thirteen packet forms spilled vector registers their parents did not (profiles/sky_light_kernel_resources.txt).
// IMG: RWR_FLAG_SKY_IMAGE — of the SKY forms alone: the sky's term comes from the context's image (add_sky_image); separate
// instantiations for the same reason, and so that the SKY forms under the gradient keep their registers (profiles/sky_image_kernel_resources.txt).
// MIRROR: RWR_FLAG_MIRRORS — of the EMIT forms alone: a hit on a mirror surface sends the reflected ray on, with T * R
// (emit_next_ray); separate instantiations for the same reason.
// SURF: which surface models the EMIT form knows — kSurfNone, kSurfMirrors (RWR_FLAG_MIRRORS alone: the MIRROR forms), kSurfGlass
// (RWR_FLAG_GLASS, with or without mirrors: a hit on glass sends on a reflected or a refracted ray with T * C and is counted) or
// kSurfGloss (RWR_FLAG_GLOSSY, with or without the other two: a glossy hit sends on gloss_direction's ray with T * R and is counted).
// GLOW: RWR_FLAG_EMISSIVE — a hit's local shading gets the radiance of its surface added (add_glow) and the emitting hits are
// counted; of the forms that end a path as of the EMIT forms; separate instantiations for the same reason.
// Which combinations exist, and how launch_wf_bounce picks one: LaneForms and PacketForms below, behind the kernels.
template <bool NODES_IN_LDS, bool NMAP, bool STACK16, bool WIDE = false, bool EMIT = false, bool SHADOW = false, bool SKY = false,
          int SURF = kSurfNone, bool GLOW = false, bool IMG = false, bool LSKY = false>
__global__ void __launch_bounds__(WIDE ? 1024 : 256)
k_wf_trace_lane(const FrameParams p, const TriRecord *__restrict__ tris, const ShadeRec *__restrict__ shade,
                const BvhDevice bvh, const float4 *__restrict__ tex, const WfBuffers wf, const PoolInfo *__restrict__ info,
                uint32_t *__restrict__ counters, const uint32_t *__restrict__ pool_list, uint32_t n_tiles, const WfEmit em, const WfShadow sw,
                const WfSky sky, const WfSurfaces sf, const WfGlow gl, const WfSkyImage si)
{
    static_assert(EMIT || SURF == kSurfNone, "only a kernel that emits rays has a MIRROR or a glass form");
    static_assert(SKY || !IMG, "the sky's image is a form of the SKY forms");
    static_assert(!LSKY || (IMG && GLOW), "light rays towards the sky's image: a form of the IMG x GLOW forms");
    constexpr bool MIRROR = SURF != kSurfNone;
    __shared__ TraceShared sh;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
    const uint32_t tid = threadIdx.x;
    // LDS carve of the dynamic part: [nodelets][traversal stack]
    BvhNode4 *s_nodes = reinterpret_cast<BvhNode4 *>(s_dyn);
    const uint32_t node_bytes = NODES_IN_LDS ? bvh.n_nodes * (uint32_t)sizeof(BvhNode4) : 0u;
    typedef typename std::conditional<STACK16, uint16_t, uint32_t>::type StackT;
    StackT *s_stack = reinterpret_cast<StackT *>(s_dyn + node_bytes);
    bool staged = false;
    uint32_t tile, share, n_shares;
    PoolInfo pi;
    while (next_item(sh, info, counters, pool_list, n_tiles, 0u, bvh.min_packet_pools, bvh.lane_items, tile, share, n_shares, pi)) {
        const uint32_t n_rays = pi.n_rays;
        if (share * 256u >= n_rays) continue;   // uniform
        if (NODES_IN_LDS && !staged) {
            const float4 *src = reinterpret_cast<const float4 *>(bvh.nodes);
            float4 *dst = reinterpret_cast<float4 *>(s_nodes);
            for (uint32_t i = tid; i < bvh.n_nodes * 8u; i += blockDim.x) dst[i] = src[i];
            staged = true;
        }
        for (uint32_t i = tid; i < kWfTilePixels * 3u; i += blockDim.x) sh.acc[i] = 0ull;
        if (tid == 0u) sh.next_packet = 0u;
        __syncthreads();
        const size_t pool_base = (size_t)tile * wf.group * kWfTilePixels;
        const uint16_t *__restrict__ sorted = wf.sorted + pool_base;
        // The item's rays: chunks share, share + n_shares, ... of 256 sorted rays.  Its waves take them 64 rays at a time from a
        // counter in LDS: a wave whose rays had short traversals goes on with the next 64 instead of waiting for the others at
        // a barrier (traversal lengths differ several-fold between waves of sparse pools).
        const uint32_t n_chunks = (n_rays + 255u) / 256u;
        const uint32_t n_sub = share < n_chunks ? 4u * ((n_chunks - share + n_shares - 1u) / n_shares) : 0u;
        for (;;) {
            uint32_t j = 0u;
            if ((tid & 63u) == 0u) j = atomicAdd(&sh.next_packet, 1u);
            j = (uint32_t)__builtin_amdgcn_readfirstlane((int)j);
            if (j >= n_sub) break;
            const uint32_t i = (share + (j >> 2) * n_shares) * 256u + (j & 3u) * 64u + (tid & 63u);
            if (i >= n_rays) continue;
            const uint32_t e = sorted[i];
            const float4 a = wf.rays[2u * (pool_base + e)], b = wf.rays[2u * (pool_base + e) + 1u];   // one 32-byte record
            const f3 O = mk3(a.x, a.y, a.z), D = mk3(b.x, b.y, b.z);
            const f3 thr = mk3(wf_unorm16_lo(a.w), wf_unorm16_hi(a.w), wf_unorm16_lo(b.w));

            // nearest over spheres (in order), then the mesh; strict '<' keeps the earlier candidate on ties
            bool have = false;
            float best_t = 0.0f;
            int32_t obj = -1;
            for (uint32_t s = 0; s < p.n_spheres; s++) {
                float t;
                if (sphere_ray_intersect_t(ld3(p.spheres[s].center), p.spheres[s].radius, O, D, t)) {
                    if (!have || t < best_t) { have = true; best_t = t; obj = -2 - (int32_t)s; }
                }
            }
            MeshHit mh;
            mh.have = false; mh.t = 0.0f; mh.u = 0.0f; mh.v = 0.0f; mh.ndotd = 0.0f; mh.idx = 0u;
            if (p.n_tris) {
                if (NODES_IN_LDS) bvh_nearest(s_nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, D, mh);
                else bvh_nearest(bvh.nodes, bvh.leaf_faces, tris, p.n_tris, s_stack, O, D, mh);
                if (mh.have && (!have || mh.t < best_t)) { have = true; best_t = mh.t; obj = (int32_t)mh.idx; }
            }
            uint32_t event = kEventNone;   // glass and glossy forms: what a counted hit did
            bool lit = false;              // GLOW forms: the hit's surface emits
            bool quiet = false;            // LSKY forms: a marked ray's miss, silenced or weighted (RWR_FLAG_LIGHT_SKY)
            if (have) {
                float gp = 0.0f;   // GLOW forms under RWR_FLAG_LIGHT_MIS: a marked ray's g'
                if constexpr (GLOW)
                    if ((gl.light & 4u) && wf_ray_marked(b.w)) gp = mis_bounce_g(p, gl, shade, tris, obj, O, D, best_t, pool_base, e);
                const Shaded s1 = shade_winner<NMAP>(p, obj, best_t, mh.u, mh.v, mh.ndotd, shade, tex, O, D);
                f3 e1 = s1.colour, le = f3{};
                if (GLOW) lit = add_glow(p, gl, shade, obj, e1, le, O, wf_ray_marked(b.w), gp);
                if (SHADOW) shadow_hit<GLOW>(sh, p, wf, sw, tris, shade, tile, e, O, D, obj, best_t, mh.ndotd, thr, e1, le);
                else add_contribution(sh, e, thr.x * e1.x, thr.y * e1.y, thr.z * e1.z);
                if constexpr (GLOW) {   // (the same calls, with the kernel's WfGlow behind the other arguments)
                    if (EMIT && !MIRROR)
                        emit_next_ray(p, wf, em, tris, tile, e, O, D, obj, best_t, mh.ndotd,
                                      mk3(thr.x * s1.albedo.x, thr.y * s1.albedo.y, thr.z * s1.albedo.z), false, 0.0f, 0.0f, gl);
                    if (EMIT && MIRROR) event = emit_from_surface<SURF>(p, wf, em, sf, tris, shade, tile, e, O, D, obj, best_t, mh.ndotd, thr, s1.albedo, gl);
                } else {
                if (EMIT && !MIRROR)
                    emit_next_ray(p, wf, em, tris, tile, e, O, D, obj, best_t, mh.ndotd,
                                  mk3(thr.x * s1.albedo.x, thr.y * s1.albedo.y, thr.z * s1.albedo.z));
                if (EMIT && MIRROR) event = emit_from_surface<SURF>(p, wf, em, sf, tris, shade, tile, e, O, D, obj, best_t, mh.ndotd, thr, s1.albedo);
                }
            } else if (SKY) {
                if constexpr (LSKY) add_sky_image_lit(sh, si, gl, e, D, thr, b.w, pool_base, quiet);
                else if constexpr (IMG) add_sky_image(sh, si, e, D, thr);
                else add_sky(sh, sky, e, D.y, thr);
            }
            if (SURF == kSurfGlass || SURF == kSurfGloss) count_surface_events<SURF == kSurfGloss>(sf.events, event);
            if (GLOW) count_glow_hits(gl.hits, lit);
            if constexpr (LSKY) count_sky_suppressed(gl, quiet);
            if (EMIT) {   // rays written for the next generation (lanes past the pool's end have left the iteration)
                const unsigned long long em = __ballot(have);
                if (em && (tid & 63u) == (uint32_t)__builtin_ctzll(em)) atomicAdd(&wf.wave_total[tile * 4u], (uint32_t)__popcll(em));
            }
        }
        __syncthreads();
        flush_pool(sh, p, wf, tile);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Dense pools: PACKET traversal.  A wave takes 128 consecutive rays of one octant of the sorted pool, two per
// lane (v_pk_* arithmetic), and walks the BVH ONCE for all of them: the node index is wave-uniform, so the
// nodelet's planes and child links arrive by scalar loads and sit in SGPRs, the one traversal stack is a VGPR
// addressed by lane (entry i in lane i, popped with v_readlane), children are ordered by the entry distance of the first ray that
// hits them, and a leaf's faces are tested like the frame kernel tests them — record in scalar registers, all rays
// in lock-step, branch-free.  No LDS in the loop, no per-lane gathers.  A child is entered when ANY ray of the
// packet can reach it; rays the box test excluded still run the exact test (it can only find true hits).
// Same conservative slab test, same exact hit test and (t, face index) selection as the per-lane traversal, so the
// winner of every ray is the brute-force winner.
// Scene data the packet kernel reads at wave-uniform addresses, through the CONSTANT address space: the kernel is a
// persistent loop with global atomics in it, and behind those the compiler would no longer dare to use scalar
// loads for plain global pointers (it cannot see that nobody writes the scene) — node and face records would come
// in through the vector memory pipe, 64 identical addresses per load.
struct PairRays {
    v3 O, D;             // the two rays of a lane
    f2 ix, iy, iz, ox, oy, oz;   // slab constants (rwr_bvh.h make_slab_ray)
    i2 valid;
};

RWR_DEV f2 max2(f2 a, f2 b) { return f2{fmaxf(a.x, b.x), fmaxf(a.y, b.y)}; }
RWR_DEV f2 min2(f2 a, f2 b) { return f2{fminf(a.x, b.x), fminf(a.y, b.y)}; }

// triangleRayIntersect + selection with the explicit lowest-index tie break, for a ray pair with separate origins
// against a wave-uniform record (cf. rwr_bvh.h intersect_and_select_any_order, rwr_device_p2.h intersect_and_select).
RWR_DEV void intersect_pair_any_order(const TriRecord &T, uint32_t idx, const PairRays &R, MeshHit2 &best)
{
    const v3 N = splat3(ld3(T.N));
    const f2 ndotd = dot3(N, R.D);
    i2 hit = R.valid & ~(abs2(ndotd) < kEpsilon);             // :94
    const f2 t = -(dot3(N, R.O) + T.d) / ndotd;               // :99-102
    hit &= ~(t < 0.0f);                                       // :105
    // a hit farther than the ray's best can never be selected (ties need t == best.t); when no ray of the packet is
    // left after a stage, the rest of the test is skipped for the whole wave (lanes that stay compute what the
    // branch-free form computes)
    hit &= ~(best.have & (t > best.t));
    if (!__any(any2(hit))) return;
    const v3 P = along(R.O, t, R.D);                          // :110
    v3 C = cross3(splat3(ld3(T.e0)), sub3(P, splat3(ld3(T.p0))));
    hit &= ~(dot3(N, C) < 0.0f);                              // :118
    if (!__any(any2(hit))) return;
    C = cross3(splat3(ld3(T.e1)), sub3(P, splat3(ld3(T.p1))));
    const f2 u = dot3(N, C);
    hit &= ~(u < 0.0f);                                       // :127
    if (!__any(any2(hit))) return;
    C = cross3(splat3(ld3(T.e2)), sub3(P, splat3(ld3(T.p2))));
    const f2 v = dot3(N, C);
    hit &= ~(v < 0.0f);                                       // :136
    const i2 lower = i2{idx < best.idx.x ? -1 : 0, idx < best.idx.y ? -1 : 0};
    const i2 take = hit & (~best.have | (t < best.t) | ((t == best.t) & lower));
    best.have |= take;
    best.t = take ? t : best.t;
    best.u = take ? u : best.u;
    best.v = take ? v : best.v;
    best.ndotd = take ? ndotd : best.ndotd;
    best.idx = take ? u2{idx, idx} : best.idx;
}

// sphereRayIntersect (sphere/compute.wgsl:63-85) for a ray pair with separate origins.
RWR_DEV i2 sphere_pair_intersect_t(f3 center, float radius, v3 O, v3 D, f2 &t_out)
{
    const v3 oc = sub3(O, splat3(center));
    const f2 a = dot3(D, D);
    const f2 b = 2.0f * dot3(oc, D);
    const f2 c = dot3(oc, oc) - (radius * radius);
    const f2 discriminant = b * b - 4.0f * a * c;
    const i2 miss = discriminant < 0.0f;
    if (!any2(~miss)) return i2{0, 0};
    const f2 sq = sqrt2(discriminant);
    const f2 t1 = (-b - sq) / (2.0f * a);
    const f2 t2 = (-b + sq) / (2.0f * a);
    const i2 use1 = t1 >= 0.0f, use2 = t2 >= 0.0f;
    t_out = use1 ? t1 : t2;
    return ~miss & (use1 | use2);
}

#ifndef RWR_PACKET_OCC
#define RWR_PACKET_OCC 4
#endif
// The glossy EMIT + SKY forms without shadow rays need close to 140 VGPRs: held to four waves (128) they spill, as their mirror and glass
// twins do, so these two forms alone are bound to three waves and spill nothing (measured: profiles/gloss_probe.txt, section 4).
#ifndef RWR_GLOSS_SKY_PACKET_OCC
#define RWR_GLOSS_SKY_PACKET_OCC 3
#endif
template <bool NMAP, bool EMIT = false, bool SHADOW = false, bool SKY = false, int SURF = kSurfNone, bool GLOW = false, bool IMG = false, bool LSKY = false>   // EMIT, SHADOW, SKY, SURF, GLOW, IMG, LSKY: see k_wf_trace_lane
__global__ void __launch_bounds__(256, (SURF == kSurfGloss && SKY && !SHADOW) ? RWR_GLOSS_SKY_PACKET_OCC : RWR_PACKET_OCC)
k_wf_trace_packet(const FrameParams p, const TriRecord *__restrict__ tris, const ShadeRec *__restrict__ shade,
                  const BvhDevice bvh, const float4 *__restrict__ tex, const WfBuffers wf, const PoolInfo *__restrict__ info,
                  uint32_t *__restrict__ counters, const uint32_t *__restrict__ pool_list, uint32_t n_tiles, const WfEmit em, const WfShadow sw,
                  const WfSky sky, const WfSurfaces sf, const WfGlow gl, const WfSkyImage si)
{
    static_assert(EMIT || SURF == kSurfNone, "only a kernel that emits rays has a MIRROR or a glass form");
    static_assert(SKY || !IMG, "the sky's image is a form of the SKY forms");
    static_assert(!LSKY || (IMG && GLOW), "light rays towards the sky's image: a form of the IMG x GLOW forms");
    constexpr bool MIRROR = SURF != kSurfNone;
    __shared__ TraceShared sh;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const const_ptr<BvhNode4> nodes = to_const_space(bvh.nodes);
    const const_ptr<uint32_t> leaf_faces = to_const_space(bvh.leaf_faces);
    const const_ptr<TriRecord> tris_c = to_const_space(tris);
    uint32_t tile, share, n_shares;
    PoolInfo pi;
    while (next_item(sh, info, counters, pool_list, n_tiles, 1u, bvh.min_packet_pools, bvh.lane_items, tile, share, n_shares, pi)) {
    // packets never straddle an octant: packet q of octant o covers sorted[oct_begin[o] + 128 q ...)
    uint32_t n_packets = 0;
#pragma unroll
    for (int o = 0; o < 8; o++) {
        if (tid == 0u) { sh.oct_begin[o] = pi.oct_begin[o]; sh.pk_begin[o] = n_packets; }
        n_packets += (pi.oct_begin[o + 1] - pi.oct_begin[o] + 127u) / 128u;
    }
    if (share >= n_packets) continue;   // uniform
    if (tid == 0u) { sh.oct_begin[8] = pi.oct_begin[8]; sh.pk_begin[8] = n_packets; sh.next_packet = 0u; }
    for (uint32_t i = tid; i < kWfTilePixels * 3u; i += 256u) sh.acc[i] = 0ull;
    __syncthreads();
    const size_t pool_base = (size_t)tile * wf.group * kWfTilePixels;
    const uint16_t *__restrict__ sorted = wf.sorted + pool_base;

    // A wave always holds its NEXT packet too: which one it is, and the slots of its rays — requested while the current packet
    // is traversed, so that a packet begins with one memory round trip (the ray records), not three in a row.
    struct Packet { uint32_t pk, oct, first, last, e0, e1; };
    auto grab = [&]() {
        Packet q;
        uint32_t pk = 0;
        if (lane == 0u) pk = atomicAdd(&sh.next_packet, 1u);
        q.pk = (uint32_t)__builtin_amdgcn_readfirstlane((int)pk) * n_shares + share;   // this workgroup's share of the packets
        q.oct = 0; q.first = 0; q.last = 0; q.e0 = 0; q.e1 = 0;
        if (q.pk < n_packets) {   // uniform
            uint32_t oct = 0;
#pragma unroll
            for (int o = 1; o < 8; o++) oct += (q.pk >= sh.pk_begin[o]) ? 1u : 0u;
            q.oct = (uint32_t)__builtin_amdgcn_readfirstlane((int)oct);
            q.first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(sh.oct_begin[q.oct] + (q.pk - sh.pk_begin[q.oct]) * 128u));
            q.last = (uint32_t)__builtin_amdgcn_readfirstlane((int)sh.oct_begin[q.oct + 1]);
            const uint32_t i0 = q.first + lane, i1 = q.first + 64u + lane;
            q.e0 = sorted[i0 < q.last ? i0 : q.first];
            q.e1 = sorted[i1 < q.last ? i1 : q.first];
        }
        return q;
    };
    Packet next = grab();
    for (;;) {
        const Packet cur_pk = next;
        if (cur_pk.pk >= n_packets) break;
        const uint32_t oct = cur_pk.oct, first = cur_pk.first, last = cur_pk.last;
        // Gray-coded octant -> sign bits (rwr_device.h wf_direction_bin): sz = bit 2, sy = bit 1 ^ sz, sx = bit 0 ^ sy
        const uint32_t sz = oct >> 2, sy = ((oct >> 1) & 1u) ^ sz, sx = (oct & 1u) ^ sy;

        // -- the lane's two rays ---------------------------------------------------------------------------------
        const uint32_t i0 = first + lane, i1 = first + 64u + lane;
        PairRays R;
        R.valid = i2{i0 < last ? -1 : 0, i1 < last ? -1 : 0};
        const uint32_t e0 = cur_pk.e0, e1 = cur_pk.e1;
        const float4 a0 = wf.rays[2u * (pool_base + e0)], b0 = wf.rays[2u * (pool_base + e0) + 1u];   // one 32-byte record per ray
        const float4 a1 = wf.rays[2u * (pool_base + e1)], b1 = wf.rays[2u * (pool_base + e1) + 1u];
        next = grab();
        R.O = v3{f2{a0.x, a1.x}, f2{a0.y, a1.y}, f2{a0.z, a1.z}};
        R.D = v3{f2{b0.x, b1.x}, f2{b0.y, b1.y}, f2{b0.z, b1.z}};
        const v3 thr = v3{f2{wf_unorm16_lo(a0.w), wf_unorm16_lo(a1.w)}, f2{wf_unorm16_hi(a0.w), wf_unorm16_hi(a1.w)},
                          f2{wf_unorm16_lo(b0.w), wf_unorm16_lo(b1.w)}};
        // slab constants by v_rcp_f32 (1 ulp): the box test is conservative by 4e-5 relative on either side
        R.ix = f2{__builtin_amdgcn_rcpf(R.D.x.x), __builtin_amdgcn_rcpf(R.D.x.y)};
        R.iy = f2{__builtin_amdgcn_rcpf(R.D.y.x), __builtin_amdgcn_rcpf(R.D.y.y)};
        R.iz = f2{__builtin_amdgcn_rcpf(R.D.z.x), __builtin_amdgcn_rcpf(R.D.z.y)};
        R.ox = -R.O.x * R.ix; R.oy = -R.O.y * R.iy; R.oz = -R.O.z * R.iz;

        // -- nearest mesh hit: packet traversal ----------------------------------------------------------------------
        MeshHit2 best;
        best.have = i2{0, 0};
        best.t = best.u = best.v = best.ndotd = splat(0.0f);
        best.idx = u2{0u, 0u};
        if (p.n_tris) {
            uint32_t stk = 0;   // the packet's traversal stack: lane i holds entry i
            uint32_t sp = 0;    // wave-uniform
            uint32_t cur = 0;   // the root is always an inner node
            for (;;) {
                if (!(cur & kBvhLeafBit)) {
                    const const_ptr<BvhNode4> nd = nodes + cur;   // wave-uniform index: scalar loads
                    const const_ptr<float> nearx = sx ? nd->bmax_x : nd->bmin_x, farx = sx ? nd->bmin_x : nd->bmax_x;
                    const const_ptr<float> neary = sy ? nd->bmax_y : nd->bmin_y, fary = sy ? nd->bmin_y : nd->bmax_y;
                    const const_ptr<float> nearz = sz ? nd->bmax_z : nd->bmin_z, farz = sz ? nd->bmin_z : nd->bmax_z;
                    // rays that are out of the running: invalid ones, and no distance beyond a ray's best hit matters
                    const f2 tb = f2{R.valid.x ? (best.have.x ? best.t.x : __builtin_inff()) : -1.0f,
                                     R.valid.y ? (best.have.y ? best.t.y : __builtin_inff()) : -1.0f};
                    // per child slot: entry-distance key (0xffffffff: nobody reaches it) and link — wave-uniform values
                    uint32_t k0 = 0xffffffffu, k1 = 0xffffffffu, k2 = 0xffffffffu, k3 = 0xffffffffu;
                    uint32_t c0 = nd->child[0], c1 = nd->child[1], c2 = nd->child[2], c3 = nd->child[3];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t child = i == 0 ? c0 : i == 1 ? c1 : i == 2 ? c2 : c3;
                        if (child == kBvhEmpty) continue;   // uniform
                        const f2 x0 = fma2(splat(nearx[i]), R.ix, R.ox), x1 = fma2(splat(farx[i]), R.ix, R.ox);
                        const f2 y0 = fma2(splat(neary[i]), R.iy, R.oy), y1 = fma2(splat(fary[i]), R.iy, R.oy);
                        const f2 z0 = fma2(splat(nearz[i]), R.iz, R.oz), z1 = fma2(splat(farz[i]), R.iz, R.oz);
                        const f2 tnear = max2(max2(x0, y0), z0), tfar = min2(min2(x1, y1), z1);
                        // conservative like rwr_bvh.h bvh_inner_step (relative slack on both distances, <=), in fewer
                        // instructions: entry distances below 0 clamp to 0 whatever their slack, and a box whose exit
                        // distance is negative lies behind the ray with or without slack — so the slack is a scale
                        const f2 lo = max2(tnear * 0.99996f, splat(0.0f));
                        const f2 hi = min2(fma2(tfar, splat(1.00004f), splat(1e-30f)), tb);
                        const i2 in = lo <= hi;
                        const unsigned long long m = __ballot(any2(in));
                        if (m) {   // uniform: some ray of the packet can reach this child
                            // order key: entry distance of the first lane that reaches it (lo >= 0: bits order like floats)
                            const float lo1 = in.x ? lo.x : lo.y;
                            const uint32_t kk = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(lo1), (int)__builtin_ctzll(m)) & ~3u;
                            if (i == 0) k0 = kk; else if (i == 1) k1 = kk | 1u; else if (i == 2) k2 = kk | 2u; else k3 = kk | 3u;
                        }
                    }
                    // sort the four (key, link) pairs ascending by key: a network of five compare-exchanges on scalars
#define RWR_CE(ka, ca, kb, cb) { const bool sw = kb < ka; const uint32_t tk = sw ? kb : ka, tc = sw ? cb : ca; kb = sw ? ka : kb; cb = sw ? ca : cb; ka = tk; ca = tc; }
                    RWR_CE(k0, c0, k1, c1) RWR_CE(k2, c2, k3, c3) RWR_CE(k0, c0, k2, c2) RWR_CE(k1, c1, k3, c3) RWR_CE(k1, c1, k2, c2)
#undef RWR_CE
                    if (k0 == 0xffffffffu) {   // nobody reaches any child: pop
                        if (sp == 0u) break;
                        sp--;
                        cur = (uint32_t)__builtin_amdgcn_readlane((int)stk, (int)sp);
                        continue;
                    }
                    // nearest child next; the others go on the stack, farthest first (entry sp lives in lane sp)
                    if (k3 != 0xffffffffu) { stk = (lane == sp) ? c3 : stk; sp++; }
                    if (k2 != 0xffffffffu) { stk = (lane == sp) ? c2 : stk; sp++; }
                    if (k1 != 0xffffffffu) { stk = (lane == sp) ? c1 : stk; sp++; }
                    cur = c0;
                } else {
                    const uint32_t lf = (cur & ~kBvhLeafBit) >> 3, count = (cur & 7u) + 1u;
                    for (uint32_t k = 0; k < count; k++) {
                        const uint32_t idx = leaf_faces[lf + k];   // uniform: scalar load
                        if (idx < p.n_tris) {
                            const TriRecord T = load_tri_record(tris_c + idx);   // into scalar registers
                            intersect_pair_any_order(T, idx, R, best);
                        }
                    }
                    if (sp == 0u) break;
                    sp--;
                    cur = (uint32_t)__builtin_amdgcn_readlane((int)stk, (int)sp);
                }
            }
        }

        // -- spheres (in order), then the mesh; strict '<' keeps the earlier candidate on ties -----------------------
        i2 have = i2{0, 0}, obj = i2{-1, -1};
        f2 best_t = splat(0.0f);
        for (uint32_t s = 0; s < p.n_spheres; s++) {
            f2 t = splat(0.0f);
            const i2 hit = sphere_pair_intersect_t(ld3(p.spheres[s].center), p.spheres[s].radius, R.O, R.D, t);
            const i2 take = hit & R.valid & (~have | (t < best_t));
            have |= take;
            best_t = take ? t : best_t;
            obj = take ? i2{-2 - (int)s, -2 - (int)s} : obj;
        }
        {
            const i2 take = best.have & (~have | (best.t < best_t));
            have |= take;
            best_t = take ? best.t : best_t;
            obj = take ? i2{(int)best.idx.x, (int)best.idx.y} : obj;
        }

        // (glossy forms: the sky's terms first — integer sums, any order gives the same bytes — so that the packet's ray numbers and a
        // missed ray's throughput are dead while the hits' next rays are made: the registers the disk loop and the rule need)
        if (SKY && SURF == kSurfGloss) {
            if constexpr (LSKY) {
                bool q0 = false, q1 = false;
                if (i0 < last && !have.x) add_sky_image_lit(sh, si, gl, e0, lane3(R.D, 0), mk3(thr.x.x, thr.y.x, thr.z.x), b0.w, pool_base, q0);
                if (i1 < last && !have.y) add_sky_image_lit(sh, si, gl, e1, lane3(R.D, 1), mk3(thr.x.y, thr.y.y, thr.z.y), b1.w, pool_base, q1);
                count_sky_suppressed(gl, q0, q1);
            } else if constexpr (IMG) {
                if (i0 < last && !have.x) add_sky_image(sh, si, e0, lane3(R.D, 0), mk3(thr.x.x, thr.y.x, thr.z.x));
                if (i1 < last && !have.y) add_sky_image(sh, si, e1, lane3(R.D, 1), mk3(thr.x.y, thr.y.y, thr.z.y));
            } else {
            if (i0 < last && !have.x) add_sky(sh, sky, e0, R.D.y.x, mk3(thr.x.x, thr.y.x, thr.z.x));
            if (i1 < last && !have.y) add_sky(sh, sky, e1, R.D.y.y, mk3(thr.x.y, thr.y.y, thr.z.y));
            }
        }
        // -- shade the second hit, add albedo(h0) * E(h1) to the pixel's sums --------------------------------------
        if (__any(any2(have))) {
            f2 er = splat(0.0f), eg = splat(0.0f), eb = splat(0.0f);
            f2 ar = splat(0.0f), ag = splat(0.0f), ab = splat(0.0f);   // albedo (EMIT)
            const i2 is_mesh = have & (obj >= 0);
            if (__any(any2(is_mesh))) {   // mesh winners: both rays of a lane at once (packed arithmetic, rwr_shade_p2.h)
                const ShadeRec none = {};
                if (EMIT) {
                    if (NMAP) shade_mesh_pair<true, false, true>(p, shade, tex, obj, none, best, R.D, er, eg, eb, ar, ag, ab);
                    else if (p.n_materials > 1u) shade_mesh_pair<true, false>(p, shade, tex, obj, none, best, R.D, er, eg, eb, ar, ag, ab);
                    else shade_mesh_pair<false, false>(p, shade, tex, obj, none, best, R.D, er, eg, eb, ar, ag, ab);
                } else {
                    if (NMAP) shade_mesh_pair<true, false, true>(p, shade, tex, obj, none, best, R.D, er, eg, eb);
                    else if (p.n_materials > 1u) shade_mesh_pair<true, false>(p, shade, tex, obj, none, best, R.D, er, eg, eb);
                    else shade_mesh_pair<false, false>(p, shade, tex, obj, none, best, R.D, er, eg, eb);
                }
            }
            if (__any(any2(have & (obj < -1)))) {   // sphere winners (rare): one ray at a time
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int o = k ? obj.y : obj.x;
                    if ((k ? have.y : have.x) && o < -1) {
                        const f3 Ok = lane3(R.O, k), Dk = lane3(R.D, k);
                        const f3 ek = shade_winner<false>(p, o, k ? best_t.y : best_t.x, 0.0f, 0.0f, 0.0f, shade, tex, Ok, Dk).colour;
                        if (k) { er.y = ek.x; eg.y = ek.y; eb.y = ek.z; } else { er.x = ek.x; eg.x = ek.y; eb.x = ek.z; }
                        if (EMIT) { if (k) { ar.y = 1.0f; ag.y = 0.0f; ab.y = 0.0f; } else { ar.x = 1.0f; ag.x = 0.0f; ab.x = 0.0f; } }
                    }
                }
            }
            f2 lr = splat(0.0f), lg = splat(0.0f), lb = splat(0.0f);   // GLOW: Le of each ray's hit
            if (GLOW) {   // here, where the wave's lanes are together: each ray's record, the add, the count
                bool lit[2] = {false, false};
#pragma unroll
                for (int k = 0; k < 2; k++)
                    if (k ? have.y : have.x) {
                        f3 ek = k ? mk3(er.y, eg.y, eb.y) : mk3(er.x, eg.x, eb.x), le;
                        // (RWR_FLAG_LIGHT_MIS: g' is made here, behind the shading — the packet forms sit at their register bound, and a value
                        // carried across the shading is a spilled one; the ray, its hit and the slot's normal are still at hand)
                        float gpk = 0.0f;
                        if ((gl.light & 4u) && wf_ray_marked(k ? b1.w : b0.w))
                            gpk = mis_bounce_g(p, gl, shade, tris, k ? obj.y : obj.x, lane3(R.O, k), lane3(R.D, k), k ? best_t.y : best_t.x,
                                               (size_t)tile * wf.group * kWfTilePixels, k ? e1 : e0);
                        lit[k] = add_glow(p, gl, shade, k ? obj.y : obj.x, ek, le, lane3(R.O, k), wf_ray_marked(k ? b1.w : b0.w), gpk);
                        if (k) { er.y = ek.x; eg.y = ek.y; eb.y = ek.z; lr.y = le.x; lg.y = le.y; lb.y = le.z; }
                        else { er.x = ek.x; eg.x = ek.y; eb.x = ek.z; lr.x = le.x; lg.x = le.y; lb.x = le.z; }
                    }
                count_glow_hits(gl.hits, lit[0], lit[1]);
            }
            if (SHADOW) {   // one ray of the lane after the other
#pragma unroll
                for (int k = 0; k < 2; k++)
                    if (k ? have.y : have.x)
                        shadow_hit<GLOW>(sh, p, wf, sw, tris, shade, tile, k ? e1 : e0, lane3(R.O, k), lane3(R.D, k), k ? obj.y : obj.x, k ? best_t.y : best_t.x,
                                         k ? best.ndotd.y : best.ndotd.x, k ? mk3(thr.x.y, thr.y.y, thr.z.y) : mk3(thr.x.x, thr.y.x, thr.z.x),
                                         k ? mk3(er.y, eg.y, eb.y) : mk3(er.x, eg.x, eb.x), k ? mk3(lr.y, lg.y, lb.y) : mk3(lr.x, lg.x, lb.x));
            } else {
            const f2 cr = thr.x * er, cg = thr.y * eg, cb = thr.z * eb;
            if (have.x) add_contribution(sh, e0, cr.x, cg.x, cb.x);
            if (have.y) add_contribution(sh, e1, cr.y, cg.y, cb.y);
            }
            if (EMIT && !MIRROR) {   // every hit's next ray, one ray of the lane after the other
                const f2 nr = thr.x * ar, ng = thr.y * ag, nb = thr.z * ab;
#pragma unroll
                for (int k = 0; k < 2; k++)
                    if (k ? have.y : have.x) {
                        if constexpr (GLOW)
                            emit_next_ray(p, wf, em, tris, tile, k ? e1 : e0, lane3(R.O, k), lane3(R.D, k), k ? obj.y : obj.x, k ? best_t.y : best_t.x,
                                          k ? best.ndotd.y : best.ndotd.x, k ? mk3(nr.y, ng.y, nb.y) : mk3(nr.x, ng.x, nb.x), false, 0.0f, 0.0f, gl);
                        else
                        emit_next_ray(p, wf, em, tris, tile, k ? e1 : e0, lane3(R.O, k), lane3(R.D, k), k ? obj.y : obj.x, k ? best_t.y : best_t.x,
                                      k ? best.ndotd.y : best.ndotd.x, k ? mk3(nr.y, ng.y, nb.y) : mk3(nr.x, ng.x, nb.x));
                    }
            }
            if (EMIT && MIRROR) {   // the same, but a hit on a mirror sends T * R on, not T * albedo, in the reflected direction
                uint32_t event[2] = {kEventNone, kEventNone};   // glass and glossy forms: what each ray's counted hit did
#pragma unroll
                for (int k = 0; k < 2; k++)
                    if (k ? have.y : have.x) {
                        if constexpr (GLOW)
                            event[k] = emit_from_surface<SURF>(p, wf, em, sf, tris, shade, tile, k ? e1 : e0, lane3(R.O, k), lane3(R.D, k), k ? obj.y : obj.x,
                                                               k ? best_t.y : best_t.x, k ? best.ndotd.y : best.ndotd.x,
                                                               k ? mk3(thr.x.y, thr.y.y, thr.z.y) : mk3(thr.x.x, thr.y.x, thr.z.x),
                                                               k ? mk3(ar.y, ag.y, ab.y) : mk3(ar.x, ag.x, ab.x), gl);
                        else
                        event[k] = emit_from_surface<SURF>(p, wf, em, sf, tris, shade, tile, k ? e1 : e0, lane3(R.O, k), lane3(R.D, k), k ? obj.y : obj.x,
                                                           k ? best_t.y : best_t.x, k ? best.ndotd.y : best.ndotd.x,
                                                           k ? mk3(thr.x.y, thr.y.y, thr.z.y) : mk3(thr.x.x, thr.y.x, thr.z.x),
                                                           k ? mk3(ar.y, ag.y, ab.y) : mk3(ar.x, ag.x, ab.x));
                    }
                if (SURF == kSurfGlass || SURF == kSurfGloss) count_surface_events<SURF == kSurfGloss>(sf.events, event[0], event[1]);
            }
            if (EMIT) {
                const uint32_t n_emit = (uint32_t)__popcll(__ballot(have.x != 0)) + (uint32_t)__popcll(__ballot(have.y != 0));
                if (lane == 0u) atomicAdd(&wf.wave_total[tile * 4u], n_emit);
            }
        }
        if (SKY && SURF != kSurfGloss) {   // per ray, not per wave: every ray of the packet (not the padding of its last lanes: i0, i1 < last) that found nothing
            if constexpr (LSKY) {
                bool q0 = false, q1 = false;
                if (i0 < last && !have.x) add_sky_image_lit(sh, si, gl, e0, lane3(R.D, 0), mk3(thr.x.x, thr.y.x, thr.z.x), b0.w, pool_base, q0);
                if (i1 < last && !have.y) add_sky_image_lit(sh, si, gl, e1, lane3(R.D, 1), mk3(thr.x.y, thr.y.y, thr.z.y), b1.w, pool_base, q1);
                count_sky_suppressed(gl, q0, q1);
            } else if constexpr (IMG) {
                if (i0 < last && !have.x) add_sky_image(sh, si, e0, lane3(R.D, 0), mk3(thr.x.x, thr.y.x, thr.z.x));
                if (i1 < last && !have.y) add_sky_image(sh, si, e1, lane3(R.D, 1), mk3(thr.x.y, thr.y.y, thr.z.y));
            } else {
            if (i0 < last && !have.x) add_sky(sh, sky, e0, R.D.y.x, mk3(thr.x.x, thr.y.x, thr.z.x));
            if (i1 < last && !have.y) add_sky(sh, sky, e1, R.D.y.y, mk3(thr.x.y, thr.y.y, thr.z.y));
            }
        }
    }
    __syncthreads();
    flush_pool(sh, p, wf, tile);
    }   // next work item
}

// The three templates' forms (rwr_wf_forms.h).  Only a kernel that emits rays has a surface form: SURF != kSurfNone only with EMIT.
struct SortForms {
    struct Form { bool list; };
    static constexpr uint32_t kRange = 2u;
    static constexpr uint32_t encode(Form f) { return f.list; }
    static constexpr Form decode(uint32_t i) { return Form{i != 0u}; }
    static constexpr bool valid(Form) { return true; }
    using Kernel = decltype(&k_wf_sort<false>);
    template <uint32_t I> static constexpr Kernel kernel() { return &k_wf_sort<decode(I).list>; }
};
struct PacketForms {
    struct Form { bool nmap, emit, shadow, sky; int surf; bool glow, img, lsky; };
    static constexpr uint32_t kRange = 16u * 4u * 2u * 2u * 2u;
    static constexpr uint32_t encode(Form f) { return f.nmap + 2u * f.emit + 4u * f.shadow + 8u * f.sky + 16u * (uint32_t)f.surf + 64u * f.glow + 128u * f.img + 256u * f.lsky; }
    static constexpr Form decode(uint32_t i)
    {
        return Form{(i & 1u) != 0, (i & 2u) != 0, (i & 4u) != 0, (i & 8u) != 0, (int)((i >> 4) & 3u), (i & 64u) != 0, (i & 128u) != 0, (i & 256u) != 0};
    }
    static constexpr bool valid(Form f) { return (f.emit || f.surf == kSurfNone) && (f.sky || !f.img) && (!f.lsky || (f.img && f.glow)); }
    using Kernel = decltype(&k_wf_trace_packet<false>);
    template <uint32_t I> static constexpr Kernel kernel()
    {
        constexpr Form f = decode(I);
        return &k_wf_trace_packet<f.nmap, f.emit, f.shadow, f.sky, f.surf, f.glow, f.img, f.lsky>;
    }
};
// WIDE — 1 024 threads around one copy of the nodelets — only with the nodelets in LDS, 16-bit stacks and no normal map (LaneLdsPlan)
struct LaneForms {
    struct Form { bool nodes_in_lds, nmap, stack16, wide, emit, shadow, sky; int surf; bool glow, img, lsky; };
    static constexpr uint32_t kRange = 128u * 4u * 2u * 2u * 2u;
    static constexpr uint32_t encode(Form f)
    {
        return f.nodes_in_lds + 2u * f.nmap + 4u * f.stack16 + 8u * f.wide + 16u * f.emit + 32u * f.shadow + 64u * f.sky + 128u * (uint32_t)f.surf +
               512u * f.glow + 1024u * f.img + 2048u * f.lsky;
    }
    static constexpr Form decode(uint32_t i)
    {
        return Form{(i & 1u) != 0, (i & 2u) != 0, (i & 4u) != 0, (i & 8u) != 0, (i & 16u) != 0, (i & 32u) != 0, (i & 64u) != 0, (int)((i >> 7) & 3u),
                    (i & 512u) != 0, (i & 1024u) != 0, (i & 2048u) != 0};
    }
    static constexpr bool valid(Form f)
    {
        return (f.emit || f.surf == kSurfNone) && (f.sky || !f.img) && (!f.lsky || (f.img && f.glow)) && (!f.wide || (f.nodes_in_lds && !f.nmap && f.stack16));
    }
    static constexpr bool is_wide(Form f) { return f.wide; }
    using Kernel = decltype(&k_wf_trace_lane<false, false, false>);
    template <uint32_t I> static constexpr Kernel kernel()
    {
        constexpr Form f = decode(I);
        return &k_wf_trace_lane<f.nodes_in_lds, f.nmap, f.stack16, f.wide, f.emit, f.shadow, f.sky, f.surf, f.glow, f.img, f.lsky>;
    }
};
static constexpr auto kSortForms = form_table<SortForms>();
static constexpr auto kPacketForms = form_table<PacketForms>();
static constexpr auto kLaneForms = form_table<LaneForms>();
// (GLOW goes with every form and adds no condition to valid(): the rule is stated beside PrimaryForms, kernels_wf_primary.hip)
static_assert(check_forms<SortForms>(2) && check_forms<PacketForms>(140),
              "packets: NMAP x (4 path-ending + 16 EMIT forms), with and without GLOW; the SKY half again with IMG; the IMG x GLOW forms again with LSKY");
static_assert(check_forms<LaneForms>(630) && count_forms<LaneForms>(LaneForms::is_wide) == 70,
              "per lane: 8 x 20 with 256 threads, 20 wide, with and without GLOW; the SKY half again with IMG; the IMG x GLOW forms again with LSKY");

// RWR_WF_STATS=1 (wf.dbg set): launches of the packet kernel, the per-lane kernel and its WIDE form, by this process
static std::atomic<uint64_t> g_trace_launches[3];

hipError_t launch_wf_bounce(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const ShadeRec *shade,
                            const BvhDevice &bvh, const float4 *tex, const WfBuffers &wf, uint32_t n_tiles,
                            uint32_t sample_count, uint32_t packet_min_rays, void *pool_info, uint32_t *pool_list, const WfFeatures &ft,
                            LanePlanRecord *plan)
{
    if (n_tiles == 0 || sample_count == 0) return hipSuccess;
    uint32_t *counters = wf.counters;   // this queue's set, zeroed by the primary stage that filled the queue
    PoolInfo *info = static_cast<PoolInfo *>(pool_info);
    // well-filled, compact pools: packet traversal (its one stack is a VGPR of 64 entries)
    const bool packets = bvh.stack_depth <= 64u && packet_min_rays <= sample_count * kWfTilePixels && bvh.packet_extent > 0.0f;
    const size_t sort_lds = 2u * (size_t)sample_count * kWfTilePixels * sizeof(uint16_t);
    if (sort_lds > 64u * 1024u) {   // beyond the default limit of dynamic LDS (groups of more than 32 samples)
        static std::atomic<uint64_t> raised_on{0};
        const hipError_t e = raise_dynamic_lds_once(raised_on, 144 * 1024, {kSortForms[0], kSortForms[1]});
        if (e != hipSuccess) return e;
    }
    const bool list = wf.live_list != nullptr;   // striding over the live tiles instead of one workgroup per pool
    hipLaunchKernelGGL(kSortForms[SortForms::encode({list})], dim3(list ? std::min(n_tiles, 2048u) : n_tiles), dim3(kWfSortThreads), sort_lds, s,
                       wf, info, counters, pool_list, n_tiles, sample_count, packets ? packet_min_rays : 0xffffffffu, bvh.packet_extent, bvh.packet_dense_rays);
    const bool nmap = (fp.flags & RWR_FLAG_NORMAL_MAP) != 0;
    const int surf = ft.trace_surf();
    const bool img = ft.sky_on && ft.sky_image.image != nullptr;   // RWR_FLAG_SKY_IMAGE in effect: the IMG forms
    const bool lsky = img && ft.glows && (ft.glow.light & 8u) != 0u;   // RWR_FLAG_LIGHT_SKY in effect: their LSKY forms
    if (packets) {
        if (wf.dbg) g_trace_launches[0].fetch_add(1u, std::memory_order_relaxed);
        hipLaunchKernelGGL(kPacketForms[PacketForms::encode({nmap, ft.emits, ft.shadows, ft.sky_on, surf, ft.glows, img, lsky})], dim3(std::min(kWfTraceGroups, n_tiles * kWfMaxSplit)),
                           dim3(256), 0, s, fp, tris, shade, bvh, tex, wf, info, counters, pool_list, n_tiles, ft.emit, ft.shadow, ft.sky, ft.surfaces, ft.glow, ft.sky_image);
    }
    const LaneLdsPlan l = lane_lds_plan(bvh, fp, bvh.wide_lane && !nmap);
    const uint32_t form = LaneForms::encode({l.nodes_in_lds, nmap, l.stack16, l.wide, ft.emits, ft.shadows, ft.sky_on, surf, ft.glows, img, lsky});
    if (wf.dbg) g_trace_launches[l.wide ? 2 : 1].fetch_add(1u, std::memory_order_relaxed);
    if (plan) *plan = LanePlanRecord{plan->launches + 1u, l.nodes_in_lds, l.stack16, l.wide};
    if (l.wide) {   // (at most 146 KiB: beyond the default limit, raised per form)
        static std::atomic<uint64_t> wide_raised_on[LaneForms::kRange];
        const hipError_t e = raise_dynamic_lds_once(wide_raised_on[form], 146 * 1024, {kLaneForms[form]});
        if (e != hipSuccess) return e;
    }
    const dim3 grid(std::min(l.wide ? 512u : kWfTraceGroups, n_tiles * kWfMaxSplit));
    hipLaunchKernelGGL(kLaneForms[form], grid, dim3(l.wide ? 1024 : 256), l.bytes, s, fp, tris, shade, bvh, tex, wf, info, counters, pool_list, n_tiles,
                       ft.emit, ft.shadow, ft.sky, ft.surfaces, ft.glow, ft.sky_image);
    return hipGetLastError();
}

size_t wf_pool_info_bytes() { return sizeof(PoolInfo); }

void wf_trace_launch_counts(uint64_t out[3])
{
    for (int i = 0; i < 3; i++) out[i] = g_trace_launches[i].load(std::memory_order_relaxed);
}

hipError_t preload_kernels_wf_bounce()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>((&k_wf_trace_packet<false>)));
}

}  // namespace rwr
