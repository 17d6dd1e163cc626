// A frame of the wavefront integrator on the slot's stream: enqueue_wavefront and its steps, in the order they run.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rwr_frame.h"

namespace rwr {

namespace {

// One frame of the integrator: what its steps share, and the steps — each puts its commands on the frame's streams, in the
// order enqueue_wavefront calls them.
struct WfFrame {
    rwr_context *ctx;
    FrameSlot &sl;
    const FrameRequest &rq;
    const rwr_render_params &rp;
    const FrameParams &fp;
    const Targets &tg;
    WfState &W;                // this slot's accumulators and queues
    hipStream_t stream;        // the slot's
    size_t n;                  // pixels of the screen
    uint32_t tiles_x, n_tiles, group;
    size_t n_queues, slots;    // launch groups in flight, each with its part (`slots` slots) of the ray queue
    bool overlap;
    // the schedule (any choice gives the same frame: all sums are integers), each queue's buffers, what the kernels know
    uint32_t z_split = 1u, shadow_tiles = 0u;
    BvhDevice bvh{};
    WfBuffers wfq[kWfMaxQueues];
    WfFeatures ft;
    const uint32_t *last_counters = nullptr;   // the last group's live-pool counts, for the next frame's split
    LanePlanRecord trace_plan, shadow_plan;    // what the frame's two stages launched per lane (rwr_last_traversal_plan)

    WfFrame(rwr_context *c, FrameSlot &s, const FrameRequest &r, const FrameParams &p, const Targets &t)
        : ctx(c), sl(s), rq(r), rp(r.rp), fp(p), tg(t), W(c->wf_state[c->n_slots > 1u ? c->cur : 0u]), stream(s.stream), n((size_t)p.width * p.height)
    {
        tiles_x = (fp.width + kWfTileW - 1u) / kWfTileW;
        n_tiles = tiles_x * band_strips(fp);
        group = std::min(rp.spp, ctx->wf_group ? ctx->wf_group : (ctx->n_slots > 1u ? 64u : 32u));
        // two launch groups in flight (each on its own stream, with its own half of the queue) when the frame has several
        n_queues = rp.max_bounces ? std::min<size_t>(ctx->wf_queues, (rp.spp + group - 1u) / group) : 1u;
        overlap = n_queues > 1u;
        slots = (size_t)n_tiles * group * kWfTilePixels;
    }
    int reserve();
    int schedule();
    int surface_table();
    int glow_table();
    int trace_groups(const AccumPlan &ap);
    int resolve(AccumPlan &ap);
    int reproject_stage(ReprojectPlan &pp);
    int denoise_stage();
    int tonemap_stage();
};

// The frame's sums, queues, streams, events and pinned words; the refusal of a frame whose queues cannot be held.
int WfFrame::reserve()
{
    if (W.d_fix.count < 4u * n) W.fix_clean = false;
    RWR_HIP_CHECK(W.d_fix.ensure(4u * n));
    if (!W.fix_clean)   // first use, a new size, or a frame that did not reach its resolve
        RWR_HIP_CHECK(hipMemsetAsync(W.d_fix.ptr, 0, 4u * n * sizeof(unsigned long long), stream));
    W.fix_clean = false;
    // The ray queues are fixed-slot (space instead of atomics: 36 B per slot of every tile of the launch), the one large
    // allocation of the library — 19 GB for a 4K frame at 64 samples per group — and a frame with shadow rays holds a 32-byte
    // record per slot on top (or alone, without a bounce).  A frame whose queues cannot be held is refused with its size, not
    // left to a failed hipMalloc half-way through.
    const size_t ray_slots = rp.max_bounces ? n_queues * slots : 0u, shadow_slots = rq.shadows ? n_queues * slots : 0u;
    if (W.d_rays.count < 2u * ray_slots || W.d_shadow_recs.count < shadow_slots) {
        const size_t slot_bytes = (rp.max_bounces ? 2u * sizeof(float4) + 2u * sizeof(uint16_t) : 0u) + (rq.shadows ? sizeof(ShadowRec) : 0u);
        const size_t need = n_queues * slots * slot_bytes;
        const size_t held = (rp.max_bounces ? W.d_rays.count * sizeof(float4) + (W.d_sorted.count + W.d_bins.count) * sizeof(uint16_t) : 0u) +
                            (rq.shadows ? W.d_shadow_recs.count * sizeof(ShadowRec) : 0u);
        size_t free_b = 0, total_b = 0;
        RWR_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b + held)
            return set_error(RWR_ERR_UNSUPPORTED, "the frame's ray queues need %.1f GB (%zu tiles x %u samples per launch group x 512 slots x %zu B x %zu queues), "
                             "%.1f GB are free: fewer frames in flight (each slot holds its own queues) or RWR_WF_GROUP < %u",
                             need * 1e-9, (size_t)n_tiles, group, slot_bytes, n_queues, (free_b + held) * 1e-9, group);
    }
    const size_t mask_words = n_queues * n_tiles * group * 8u;
    if (rp.max_bounces) {
        RWR_HIP_CHECK(W.d_rays.ensure(n_queues * 2u * slots));
        RWR_HIP_CHECK(W.d_sorted.ensure(n_queues * slots));
        RWR_HIP_CHECK(W.d_bins.ensure(n_queues * slots));
        RWR_HIP_CHECK(W.d_masks.ensure(mask_words));
        if (rp.max_bounces > 1u) RWR_HIP_CHECK(W.d_masks_next.ensure(mask_words));
        RWR_HIP_CHECK(W.d_pool_info.ensure(n_queues * n_tiles * wf_pool_info_bytes()));
        RWR_HIP_CHECK(W.d_pool_list.ensure(n_queues * 2u * (size_t)n_tiles));
        if (overlap && !W.fork) RWR_HIP_CHECK(hipEventCreateWithFlags(&W.fork.h, hipEventDisableTiming));
        for (size_t q = 0; q < n_queues; q++) {
            if (q && !W.streams[q]) RWR_HIP_CHECK(hipStreamCreateWithFlags(&W.streams[q].h, hipStreamNonBlocking));
            if (q && !W.join[q]) RWR_HIP_CHECK(hipEventCreateWithFlags(&W.join[q].h, hipEventDisableTiming));
        }
        if (!W.d_live.ptr) {
            RWR_HIP_CHECK(W.d_live.ensure(4u * kWfMaxQueues));
            RWR_HIP_CHECK(hipMemsetAsync(W.d_live.ptr, 0, 4u * kWfMaxQueues * sizeof(uint32_t), stream));
        }
        if (!ctx->h_wf_live) {
            RWR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_wf_live.h), 2 * sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped));   // fine-grained: kernels store to it, the host reads it without a synchronisation
            ctx->h_wf_live[0] = ctx->h_wf_live[1] = 0u;
        }
    }
    // Shadow rays (RWR_FLAG_SHADOWS): a record per queue slot and their ballots, per queue like the rays (and kept like them: until
    // the slot is given up or the context destroyed); the slot's two counters start the frame from zero
    if (rq.shadows) {
        RWR_HIP_CHECK(W.d_shadow_recs.ensure(n_queues * slots));
        RWR_HIP_CHECK(W.d_shadow_masks.ensure(mask_words));
        RWR_HIP_CHECK(W.d_shadow_counts.ensure(2));
        RWR_HIP_CHECK(hipMemsetAsync(W.d_shadow_counts.ptr, 0, 2 * sizeof(unsigned long long), stream));
    }
    return RWR_OK;
}

// The split of a tile's samples, the live list, each queue's buffers, and the trace kernels' BvhDevice.
int WfFrame::schedule()
{
    // Did the frame before show LITTLE — fewer than 1 024 live tiles, and at most half of this frame's tiles (a small mesh
    // on an empty screen; not a small frame full of geometry, such as a row band of a multi-GPU frame: measured, that one
    // is best left alone)?  Its count arrives through pinned memory, a frame late, never waited for.  Then several
    // workgroups share a tile's samples in the primary stage (enough of them to fill the chip twice, up to one per
    // sample), and the tiles anything can be seen through are listed first (below).
    const uint32_t prev_packets = ctx->h_wf_live ? ctx->h_wf_live[0] : 0u, prev_lane = ctx->h_wf_live ? ctx->h_wf_live[1] : 0u;
    const uint32_t live = prev_packets + prev_lane;
    const bool shows_little = live != 0u && live < 1024u && 2u * live <= n_tiles;
    z_split = ctx->wf_z_split;
    if (z_split == 0u) {
        z_split = 1u;
        if (shows_little)
            while (z_split < kWfMaxGroup && z_split * live < 2048u) z_split *= 2u;
    }
    // queue q: its half of every per-group buffer and its set of four counters (the primary stage zeroes the set it
    // is about to fill).  With one queue the frame's sums are read-modify-written by the tile's only workgroup; with
    // two, a group's primary stage runs beside the other group's trace kernels and everybody adds atomically.
    // A frame expected to show little (z_split > 1: the previous frame did) first lists the tiles anything can be seen
    // through; the primary stage, the sort and the resolve then touch those alone.  Same frame either way.
    uint32_t *live_list = nullptr, *live_count = nullptr, *tile_live = nullptr;
    if (z_split > 1u && (shows_little || ctx->wf_z_split != 0u) && !(rp.flags & RWR_FLAG_NO_CULL)) {   // (a forced split: the tests' way in)
        live_list = W.d_tiles.ptr; tile_live = live_list + n_tiles; live_count = tile_live + n_tiles;   // (zeroed by k_frame_setup)
        RWR_HIP_CHECK(launch_wf_classify(stream, fp, sl.d_ftris.ptr, tg, tiles_x, live_list, live_count, tile_live));
    }
    // tiles expected to hold shadow records (sizes k_wf_shadow's work items): the live pools of the frame before when this one
    // walks a live list, else every tile
    shadow_tiles = live_list ? std::max(1u, live) : n_tiles;
    for (size_t q = 0; q < n_queues; q++) {
        wfq[q] = WfBuffers{W.d_fix.ptr,
                           W.d_rays.ptr ? W.d_rays.ptr + q * 2u * slots : nullptr,
                           W.d_masks.ptr ? W.d_masks.ptr + q * n_tiles * group * 8u : nullptr,
                           W.d_bins.ptr ? W.d_bins.ptr + q * slots : nullptr,
                           W.d_sorted.ptr ? W.d_sorted.ptr + q * slots : nullptr,
                           W.d_wave_total.ptr, group, tiles_x, ctx->d_wf_dbg.ptr,
                           rp.max_bounces ? W.d_live.ptr + q * 4u : nullptr, overlap ? 1u : 0u, live_list, live_count, tile_live};
    }
    // The per-lane trace kernel as 1 024-thread workgroups that share ONE copy of the nodelets in LDS (kernels_wf_bounce.hip,
    // WIDE; only for a BVH too large for a copy per 256-thread workgroup and small enough for one per CU), one work item per
    // pool: when frames overlap and the frame before traced most of its pools per lane (a small mesh on an empty screen at few
    // samples: configs[3] 0.604 -> 0.54 ms; one frame at a time it loses, 0.73 -> 0.81, and configs[4]'s frame, whose large
    // pools are packets, loses 2 %: both keep the 256-thread kernel).  Same frame either way.
    const bool wide_lane = ctx->wf_wide_lane >= 0 ? ctx->wf_wide_lane != 0
                                                   : (ctx->n_slots > 1u && prev_lane >= 128u && prev_lane >= 4u * prev_packets);
    bvh = BvhDevice{ctx->d_bvh_nodes.ptr, ctx->d_bvh_leaf_faces.ptr, ctx->bvh_n_nodes, 3u * ctx->bvh_depth + 2u,
                        ctx->wf_packet_extent * ctx->bvh_leaf_extent, ctx->wf_min_packet_pools,
                        // work items of the per-lane trace kernel when pools are few: one 256-ray chunk each for a context that
                        // renders one frame at a time (the chip has nothing else to do: as many items as possible), about four
                        // chunks each when frames overlap (a pool's rays grow with the group's samples; measured at configs[3],
                        // 16 samples: 0.625 -> 0.607 ms with 4 096 items, but 0.74 -> 0.79 ms one frame at a time; configs[4]'s
                        // frame, 64 samples: 16 384 is best either way)
                        ctx->wf_lane_items ? ctx->wf_lane_items : (wide_lane ? 256u : ctx->n_slots > 1u ? std::min(16384u, 256u * group) : 16384u),
                        ctx->wf_packet_dense_rays, wide_lane ? 1u : 0u, ctx->wf_stack16 ? 0u : 1u};
    return RWR_OK;
}

// RWR_FLAG_MIRRORS, _GLASS, _GLOSSY: this slot's copy of the surface table — a record per part, then one per sphere index —
// refreshed on the frame's stream (ahead of the fork: every queue's kernels read it) when the context's attributes have changed
// since the slot's last copy; and the frame's event counters, from zero.
int WfFrame::surface_table()
{
    ft.surf = rq.gloss ? kSurfGloss : rq.glass ? kSurfGlass : rq.mirrors ? kSurfMirrors : kSurfNone;
    // whose records the frame's copy holds (surface_mode bits): a flag switches its own surfaces on
    const uint32_t modes = (rq.mirrors ? surface_mode(SurfaceModel::kMirror) : 0u) | (rq.glass ? surface_mode(SurfaceModel::kGlass) : 0u) |
                           (rq.gloss ? surface_mode(SurfaceModel::kGloss) : 0u);
    if (!modes) return RWR_OK;
    const size_t n_parts = ctx->part_surfaces.size(), n_recs = n_parts + RWR_MAX_SPHERES;
    if (W.surface_version != ctx->surface_version || W.surface_modes != modes || W.d_surface.count < n_recs) {
        if (W.surface_version != 0u) RWR_HIP_CHECK(hipEventSynchronize(W.surface_copied));   // the image's last copy has been read
        if (W.h_surface_count < n_recs) {
            W.h_surface = PinnedSurface();
            RWR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&W.h_surface.h), n_recs * sizeof(SurfaceRec), hipHostMallocDefault));
            W.h_surface_count = n_recs;
        }
        RWR_HIP_CHECK(W.d_surface.ensure(n_recs));
        if (!W.surface_copied) RWR_HIP_CHECK(hipEventCreateWithFlags(&W.surface_copied.h, hipEventDisableTiming));
        for (size_t i = 0; i < n_parts; i++) W.h_surface.h[i] = visible_record(ctx->part_surfaces[i], modes);
        for (size_t i = 0; i < RWR_MAX_SPHERES; i++) W.h_surface.h[n_parts + i] = visible_record(ctx->sphere_surfaces[i], modes);
        RWR_HIP_CHECK(hipMemcpyAsync(W.d_surface.ptr, W.h_surface.h, n_recs * sizeof(SurfaceRec), hipMemcpyHostToDevice, stream));
        RWR_HIP_CHECK(hipEventRecord(W.surface_copied, stream));
        W.surface_version = ctx->surface_version;
        W.surface_modes = modes;
    }
    ft.surfaces = WfSurfaces{W.d_surface.ptr, (uint32_t)n_parts, 0u, nullptr};
    // (intended: a frame with RWR_FLAG_GLASS alone also holds and zeroes the glossy counter, 8 bytes more than its three — one
    // buffer of one size for either flag, so that a context alternating between them never reallocates; no launch is added)
    if (rq.glass || rq.gloss) {   // the frame's event counters (SurfaceEvent) start from zero
        RWR_HIP_CHECK(W.d_surface_events.ensure(kEventNone));
        RWR_HIP_CHECK(hipMemsetAsync(W.d_surface_events.ptr, 0, kEventNone * sizeof(unsigned long long), stream));
        ft.surfaces.events = W.d_surface_events.ptr;
    }
    return RWR_OK;
}

// RWR_FLAG_EMISSIVE: this slot's copy of the emission table — the radiance of every part, then of every sphere index — kept as
// the surface table's copy is (refreshed on the frame's stream when the context's attributes have changed since), and the frame's
// count of emitting hits, from zero.
int WfFrame::glow_table()
{
    // (RWR_FLAG_LIGHT_SKY without RWR_FLAG_EMISSIVE in effect: the GLOW forms — they carry the marks, the normals and the ballots —
    // over a table that emits nothing)
    ft.glows = rq.glow || rq.light_sky;
    if (!ft.glows) return RWR_OK;
    const bool dark = !rq.glow;
    const size_t n_parts = ctx->part_glow.size(), n_recs = n_parts + RWR_MAX_SPHERES;
    if (W.glow_version != ctx->glow_version || W.glow_dark != dark || W.d_glow.count < n_recs) {
        if (W.glow_version != 0u) RWR_HIP_CHECK(hipEventSynchronize(W.glow_copied));   // the image's last copy has been read
        if (W.h_glow_count < n_recs) {
            W.h_glow = PinnedSurface();
            RWR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&W.h_glow.h), n_recs * sizeof(SurfaceRec), hipHostMallocDefault));
            W.h_glow_count = n_recs;
        }
        RWR_HIP_CHECK(W.d_glow.ensure(n_recs));
        if (!W.glow_copied) RWR_HIP_CHECK(hipEventCreateWithFlags(&W.glow_copied.h, hipEventDisableTiming));
        for (size_t i = 0; i < n_parts; i++) {
            W.h_glow.h[i] = ctx->part_glow[i];
            // (the spare component: the part's inv_pdf in the mesh light built last — read by mis_bounce_g under RWR_FLAG_LIGHT_MIS
            // alone, in frames whose validation made that list current; a rebuild that changes one changes glow_version)
            if (i < ctx->part_inv_pdf.size()) W.h_glow.h[i].on = ctx->part_inv_pdf[i];
        }
        for (size_t i = 0; i < RWR_MAX_SPHERES; i++) W.h_glow.h[n_parts + i] = ctx->sphere_glow[i];
        if (dark)
            for (size_t i = 0; i < n_recs; i++) W.h_glow.h[i] = SurfaceRec{0.0f, 0.0f, 0.0f, 0.0f};
        RWR_HIP_CHECK(hipMemcpyAsync(W.d_glow.ptr, W.h_glow.h, n_recs * sizeof(SurfaceRec), hipMemcpyHostToDevice, stream));
        RWR_HIP_CHECK(hipEventRecord(W.glow_copied, stream));
        W.glow_version = ctx->glow_version;
        W.glow_dark = dark;
    }
    RWR_HIP_CHECK(W.d_glow_hits.ensure(1));
    RWR_HIP_CHECK(hipMemsetAsync(W.d_glow_hits.ptr, 0, sizeof(unsigned long long), stream));
    ft.glow = WfGlow{W.d_glow.ptr, (uint32_t)n_parts, 0u, W.d_glow_hits.ptr, nullptr, nullptr, nullptr};
    // RWR_FLAG_LIGHT_SAMPLING, RWR_FLAG_LIGHT_PARTS: a normal per queue slot and the light ballots, per queue like the rays and kept like
    // them (allocated by the first frame that needs them); the frame's nine counts start from zero.  trace_groups points ft.glow at a
    // queue's share.  glow.light: 1 the spheres, 2 the mesh light (validate made its list and device copy current), 4
    // RWR_FLAG_LIGHT_MIS, 8 RWR_FLAG_LIGHT_SKY (mask values, as rwr_surface.h states them), bits 8-15 L, the lights the stage chooses among.
    ft.lights_on = rq.light || rq.light_parts || rq.light_sky;
    if (ft.lights_on) {
        if (rq.light) ft.lights = scene_lights(ctx);
        if (rq.light_parts)
            ft.part_lights = WfPartLights{ctx->d_part_lights.ptr, ctx->d_shade.ptr, (uint32_t)ctx->part_lights.size(), ft.lights.m + 1u};
        RWR_HIP_CHECK(W.d_light_recs.ensure(n_queues * slots));
        RWR_HIP_CHECK(W.d_light_masks.ensure(n_queues * n_tiles * group * 8u));
        RWR_HIP_CHECK(W.d_light_counts.ensure(9));
        RWR_HIP_CHECK(hipMemsetAsync(W.d_light_counts.ptr, 0, 9 * sizeof(unsigned long long), stream));
        ft.glow.light = (rq.light ? 1u : 0u) | (rq.light_parts ? 2u : 0u) | (rq.light_mis ? 4u : 0u) | (rq.light_sky ? 8u : 0u) |
                        ((ft.lights.m + (rq.light_parts ? 1u : 0u) + (rq.light_sky ? 1u : 0u)) << 8);
        ft.glow.light_counts = W.d_light_counts.ptr;
    }
    return RWR_OK;
}

// The samples, in launch groups that alternate between the queues: per group the primary stage, then per bounce one generation
// of the bounce stage; the other queues' streams fork off the slot's ahead of the first group and join it behind the last.
// ft: what the frame's kernels know (WfFeatures) — the surfaces come filled in, the sky here, a queue's shadow records per launch
// group, emit per generation.
int WfFrame::trace_groups(const AccumPlan &ap)
{
    const size_t mask_words = (size_t)n_tiles * group * 8u;
    const float4 *tex0 = tex0_of(ctx);
    // the unit vectors towards the reference's two lights, -normalize(kLightDir) in the oracle's f32 operations
    // (triangle_list/compute.wgsl:55, sphere/compute.wgsl:41)
    float light_mesh[3], light_sphere[3];
    {
        const float km[3] = {1.0f, -1.0f, -5.0f}, ks[3] = {1.0f, -5.0f, 1.0f};
        const float lm = std::sqrt(km[0] * km[0] + km[1] * km[1] + km[2] * km[2]), ls = std::sqrt(ks[0] * ks[0] + ks[1] * ks[1] + ks[2] * ks[2]);
        for (int k = 0; k < 3; k++) { light_mesh[k] = -(km[k] / lm); light_sphere[k] = -(ks[k] / ls); }
    }
    if (overlap) {   // the other streams start behind this frame's setup (and so behind the previous frame's resolve)
        RWR_HIP_CHECK(hipEventRecord(W.fork, stream));
        for (size_t q = 1; q < n_queues; q++) RWR_HIP_CHECK(hipStreamWaitEvent(W.streams[q], W.fork, 0));
    }
    if (rq.sky) std::memcpy(&ft.sky, &ctx->sky, sizeof ft.sky);
    ft.sky_on = rq.sky;
    // (the slot lets go of the image of its last frame, whose kernels ran ahead of this frame's on the slot's stream, and holds on to this one's)
    W.sky_image = rq.sky_image ? ctx->sky_image : nullptr;
    W.sky_light = rq.light_sky ? ctx->sky_light : nullptr;   // (validate made it current; held as the image is)
    ft.sky_image = rq.sky_image ? WfSkyImage{W.sky_image->ptr, ctx->sky_image_n, 0u, W.sky_light ? W.sky_light->ptr : nullptr} : WfSkyImage{nullptr, 0u, 0u, nullptr};
    ft.soft = rq.soft;
    const rwr_shadow_params *soft = ft.soft ? &ctx->shadow : nullptr;
    // (global sample indices: an accumulating frame traces [accum_before, accum_before + spp), keyed like one frame of them all)
    for (uint32_t s0 = 0, g = 0; s0 < ap.trace_spp; s0 += group, g++) {
        const uint32_t cnt = std::min(group, rp.spp - s0);
        const size_t q = g % n_queues;
        hipStream_t gs = q ? W.streams[q].h : stream;
        if (rq.shadows) ft.shadow = WfShadow{W.d_shadow_recs.ptr + q * slots, W.d_shadow_masks.ptr + q * mask_words, W.d_shadow_counts.ptr};
        ft.shadows = ft.shadow.recs != nullptr;
        if (ft.lights_on) {   // this queue's light records; the primary stage stores whole ballot words where it emits, the rest stay clear
            ft.glow.light_recs = W.d_light_recs.ptr + q * slots;
            ft.glow.light_masks = W.d_light_masks.ptr + q * mask_words;
            RWR_HIP_CHECK(hipMemsetAsync(ft.glow.light_masks, 0, mask_words * sizeof(unsigned long long), gs));
        }
        RWR_HIP_CHECK(launch_wf_primary(gs, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, sl.d_ftris.ptr, tex0, tg, wfq[q],
                                        (uint32_t)ap.before + s0, cnt, z_split, ft));
        if (rq.shadows)   // h0's shadow rays
            RWR_HIP_CHECK(launch_wf_shadow(gs, fp, ctx->d_tris.ptr, bvh, wfq[q], ft.shadow, n_tiles, shadow_tiles, cnt, light_mesh, light_sphere, 0u,
                                           (uint32_t)ap.before + s0, soft, &shadow_plan));
        if (ft.lights_on)   // h0's light samples: ray 1 sits in the queue, the first sort has not run
            RWR_HIP_CHECK(launch_wf_light(gs, fp, ctx->d_tris.ptr, bvh, wfq[q], ft.glow, ft.lights, ft.part_lights, ft.sky_image, n_tiles, shadow_tiles, cnt, 0u, (uint32_t)ap.before + s0));
        // the bounce stage: one generation of rays per bounce (RWR_FLAG_MULTI_BOUNCE: up to RWR_MAX_BOUNCES).  Generation k traces
        // ray k of every path that is still alive — the sort and trace kernels run again over the same fixed slots — and, unless
        // it is the last, writes ray k + 1 back into the slot of every hit, with its bit in the other ballot array.
        WfBuffers wg = wfq[q];
        unsigned long long *masks_next = W.d_masks_next.ptr ? W.d_masks_next.ptr + q * mask_words : nullptr;
        for (uint32_t gen = 1; gen <= rp.max_bounces; gen++) {
            if (gen > 1u)   // the sort counts this generation's live pools from zero (the primary stage zeroed the set of four for the first)
                RWR_HIP_CHECK(hipMemsetAsync(wg.counters, 0, 4u * sizeof(uint32_t), gs));
            const bool emit = gen < rp.max_bounces;
            ft.emits = emit;
            ft.emit = emit ? WfEmit{masks_next, 2u + 16u * gen, (uint32_t)ap.before + s0} : WfEmit{nullptr, 0u, 0u};
            if (emit) RWR_HIP_CHECK(hipMemsetAsync(masks_next, 0, mask_words * sizeof(unsigned long long), gs));
            if (rq.shadows) RWR_HIP_CHECK(hipMemsetAsync(ft.shadow.masks, 0, mask_words * sizeof(unsigned long long), gs));   // the trace kernels set bits
            if (ft.lights_on && emit) RWR_HIP_CHECK(hipMemsetAsync(ft.glow.light_masks, 0, mask_words * sizeof(unsigned long long), gs));   // likewise
            RWR_HIP_CHECK(launch_wf_bounce(gs, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, bvh, tex0, wg, n_tiles, cnt,
                                           (uint32_t)std::fmax(1.0f, std::ceil(ctx->wf_packet_fill * (float)(cnt * kWfTilePixels))),
                                           W.d_pool_info.ptr + q * n_tiles * wf_pool_info_bytes(), W.d_pool_list.ptr + q * 2u * (size_t)n_tiles, ft, &trace_plan));
            if (rq.shadows)   // this generation's hits
                RWR_HIP_CHECK(launch_wf_shadow(gs, fp, ctx->d_tris.ptr, bvh, wg, ft.shadow, n_tiles, shadow_tiles, cnt, light_mesh, light_sphere, gen,
                                               (uint32_t)ap.before + s0, soft, &shadow_plan));
            if (ft.lights_on && emit)   // the light samples of this generation's hits, from the rays it just wrote, ahead of the next sort
                RWR_HIP_CHECK(launch_wf_light(gs, fp, ctx->d_tris.ptr, bvh, wg, ft.glow, ft.lights, ft.part_lights, ft.sky_image, n_tiles, shadow_tiles, cnt, gen, (uint32_t)ap.before + s0));
            if (emit) std::swap(wg.masks, masks_next);
        }
        if (rp.max_bounces && s0 + group >= rp.spp) last_counters = wfq[q].counters;
    }
    for (size_t q = 1; q < n_queues; q++) {
        RWR_HIP_CHECK(hipEventRecord(W.join[q], W.streams[q]));
        RWR_HIP_CHECK(hipStreamWaitEvent(stream, W.join[q], 0));
    }
    return RWR_OK;
}

// Either resolve, and an accumulating frame's commit to the context's history.
// (The resolve also hands the last group's live pool counts to the host: a store to pinned memory, no copy command.  The
// same store at the top of the per-lane trace kernel made THAT kernel twice as slow, 453 -> 840 us at configs[3], with the
// pointer null and the instruction mix unchanged; here it costs nothing measurable.)
int WfFrame::resolve(AccumPlan &ap)
{
    uint32_t *live_out = last_counters ? ctx->h_wf_live.h : nullptr;
    if (!rq.accumulate) {
        RWR_HIP_CHECK(launch_wf_resolve(stream, fp, tg, wfq[0], last_counters, live_out));
    } else {
        // The history is the context's, not the slot's: frames in flight trace side by side, their resolves run in frame order
        Accum &A = ctx->accum;
        if (ap.mode == AccumMode::kFirst) {
            RWR_HIP_CHECK(A.d_hist.ensure(4u * n));
            RWR_HIP_CHECK(A.d_depth.ensure(n));
            if (rq.aux) { RWR_HIP_CHECK(A.d_obj_id.ensure(n)); RWR_HIP_CHECK(A.d_hit_t.ensure(n)); }
        }
        if (!A.done) RWR_HIP_CHECK(hipEventCreateWithFlags(&A.done.h, hipEventDisableTiming));
        if (A.done_recorded) RWR_HIP_CHECK(hipStreamWaitEvent(stream, A.done, 0));
        const AccumBuffers ab{A.d_hist.ptr, A.d_depth.ptr, rq.aux ? A.d_obj_id.ptr : nullptr, rq.aux ? A.d_hit_t.ptr : nullptr};
        const uint64_t total = ap.mode == AccumMode::kShow ? ap.before : ap.before + rp.spp;
        RWR_HIP_CHECK(launch_wf_resolve_accum(stream, fp, tg, wfq[0], ab, ap.mode, (uint32_t)total, last_counters, live_out));
        RWR_HIP_CHECK(hipEventRecord(A.done, stream));
        A.done_recorded = true;
        A.key.swap(ap.key);
        A.samples = total;
        ctx->last_accum_samples = total;
    }
    W.fix_clean = true;   // (the resolve zeroes what it reads; rows outside the band were never touched)
    return RWR_OK;
}

// RWR_FLAG_REPROJECT: the stage, behind the resolve on the slot's stream.  The history is the context's, not the slot's: frames
// in flight trace side by side, their stages run in frame order behind an event.  Frame k gathers from set (k - 1) & 1 and
// writes set k & 1 — the set frame k - 1 read from, which that frame's stage (the event) has finished with.
int WfFrame::reproject_stage(ReprojectPlan &pp)
{
    Reproject &R = ctx->reproj;
    const uint32_t set = (uint32_t)(pp.k & 1u);
    for (uint32_t i = 0; i < 2u; i++) {
        RWR_HIP_CHECK(R.d_colour[i].ensure(n));
        RWR_HIP_CHECK(R.d_guide[i].ensure(n));
        RWR_HIP_CHECK(R.d_id[i].ensure(n));
    }
    RWR_HIP_CHECK(R.d_counts.ensure(6));
    if (!R.done) RWR_HIP_CHECK(hipEventCreateWithFlags(&R.done.h, hipEventDisableTiming));
    if (R.done_recorded) RWR_HIP_CHECK(hipStreamWaitEvent(stream, R.done, 0));
    RWR_HIP_CHECK(hipMemsetAsync(R.d_counts.ptr + 3u * set, 0, 3 * sizeof(unsigned long long), stream));
    const RpHistory from{R.d_colour[set ^ 1u].ptr, R.d_guide[set ^ 1u].ptr, R.d_id[set ^ 1u].ptr};
    const RpHistory to{R.d_colour[set].ptr, R.d_guide[set].ptr, R.d_id[set].ptr};
    RWR_HIP_CHECK(launch_wf_reproject(stream, fp.width, fp.height, ctx->d_tris.ptr, tg, fp.cam, pp.k ? &R.camera : nullptr, ctx->reproject,
                                      from, to, R.d_counts.ptr + 3u * set));
    RWR_HIP_CHECK(hipEventRecord(R.done, stream));
    R.done_recorded = true;
    R.camera = reproject_camera(fp.cam);
    R.key.swap(pp.key);
    R.frames = pp.k + 1u;
    ctx->last_reproject_frames = R.frames;
    ctx->last_reproject_set = set;
    return RWR_OK;
}

// RWR_FLAG_DENOISE: the filter, behind either resolve (and the reprojection stage: it filters `out`, and runs behind the event
// the next stage waits for — the history never sees the filter) on the slot's stream.  (An accumulating frame: behind the event the next
// accumulating resolve waits for — the history never sees the filter, and no other slot waits for it.)
int WfFrame::denoise_stage()
{
    RWR_HIP_CHECK(sl.d_dn_guide.ensure(n));
    RWR_HIP_CHECK(sl.d_dn_a.ensure(n));
    RWR_HIP_CHECK(sl.d_dn_b.ensure(n));
    RWR_HIP_CHECK(launch_wf_denoise(stream, fp.width, fp.height, ctx->d_tris.ptr, tg, ctx->denoise, sl.d_dn_guide.ptr, sl.d_dn_a.ptr, sl.d_dn_b.ptr));
    return RWR_OK;
}

// RWR_FLAG_TONEMAP: the last stage on the slot's stream, behind either resolve, the reprojection stage and the filter (and behind the
// events the next accumulating resolve and the next reprojection stage wait for: the histories never see it).  It rewrites the
// frame's rgba8 plane from its colour_f32 plane; the record is the slot's, zeroed on the stream — the host waits for nothing.
int WfFrame::tonemap_stage()
{
    RWR_HIP_CHECK(sl.d_tm_record.ensure(1));
    RWR_HIP_CHECK(launch_wf_tonemap(stream, fp.width, fp.height, tg, ctx->tonemap, sl.d_tm_record.ptr));
    return RWR_OK;
}

}  // namespace

// A frame of the wavefront integrator: the samples are traced in launch groups; per group the primary stage (all of the
// group's samples of every pixel, rays into the fixed-slot queue) then the bounce stage (one workgroup per
// 64x8-pixel tile and its ray pool)
int enqueue_wavefront(rwr_context *ctx, FrameSlot &sl, const FrameRequest &rq, AccumPlan &ap, ReprojectPlan &pp, FrameConsts &fc,
                      const Targets &tg, FrameTiming &timing)
{
    WfFrame F(ctx, sl, rq, fc.fp, tg);
    FrameSetupOut so{};
    int rc = frame_tables(ctx, sl, fc.fp, so);
    if (rc != RWR_OK) return rc;
    // the per-tile ray counts and the live-tile count start every frame from zero: k_frame_setup zeroes them
    RWR_HIP_CHECK(F.W.d_wave_total.ensure((size_t)F.n_tiles * 4u));
    RWR_HIP_CHECK(F.W.d_tiles.ensure(2u * (size_t)F.n_tiles + 1u));
    so.zero_a = F.W.d_wave_total.ptr; so.n_zero_a = F.n_tiles * 4u;
    so.zero_b = F.W.d_tiles.ptr + 2u * (size_t)F.n_tiles; so.n_zero_b = 1u;   // live_count (WfFrame::schedule)
    if ((rc = enqueue_records(ctx, sl, FrameKernel::kWavefront, fc, so, timing)) != RWR_OK) return rc;
    if ((rc = F.reserve()) != RWR_OK || (rc = F.schedule()) != RWR_OK || (rc = F.surface_table()) != RWR_OK || (rc = F.glow_table()) != RWR_OK) return rc;
    if ((rc = F.trace_groups(ap)) != RWR_OK || (rc = F.resolve(ap)) != RWR_OK) return rc;
    if (rq.reproject && (rc = F.reproject_stage(pp)) != RWR_OK) return rc;
    if (rq.denoise && (rc = F.denoise_stage()) != RWR_OK) return rc;
    if (rq.tonemap && (rc = F.tonemap_stage()) != RWR_OK) return rc;
    ctx->last_segments = F.n_tiles;
    ctx->last_trace_plan = F.trace_plan;
    ctx->last_shadow_plan = F.shadow_plan;
    ctx->last_wf_state = ctx->n_slots > 1u ? ctx->cur : 0u;
    return RWR_OK;
}

}  // namespace rwr
