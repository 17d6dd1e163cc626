// C-ABI implementation: the context's life cycle, targets, timers and statistics.
// Replaces the wgpu plumbing of State (the reference's src/lib.rs:260-1231) with
// one HIP stream and a handful of device buffers.  The scene, the frame, the self-tests and the
// multi-GPU gather have their own units (scene.cpp, the frame units of rwr_frame.h, diagnostics.cpp, dist.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <vector>

#include "rwr_context.h"
#include "rwr_sky_light.h"
#include "rwr_tonemap.h"

namespace rwr {

static thread_local std::string g_last_error;

int set_error(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// Per-frame buffers of every active slot for the current scene and screen, so that the first frame
// does not pay for allocations (the render path re-checks: both calls are no-ops once sized).
hipError_t ensure_frame_buffers(rwr_context *ctx)
{
    const uint32_t total = (uint32_t)instanced_faces(ctx->n_faces, ctx->n_instances);
    for (uint32_t i = 0; i < ctx->n_slots; i++) {
        FrameSlot &sl = ctx->slots[i];
        const void *const before[4] = {sl.d_ftris.ptr, sl.d_tnum.ptr, sl.d_ray_colp.ptr, sl.d_ray_row.ptr};
        hipError_t e = hipSuccess;
        if (total && (e = sl.d_ftris.ensure(total)) == hipSuccess) e = sl.d_tnum.ensure(total);
        if (e == hipSuccess && ctx->screen.width) {
            e = sl.d_ray_colp.ensure(2u * (size_t)(((ctx->screen.width + 63u) / 64u) * 32u));
            if (e == hipSuccess) e = sl.d_ray_row.ensure(ctx->screen.height + 8u);
        }
        // a buffer that moves here moves outside any frame: a later frame's key could name the old address again (the
        // allocator may hand it back) over memory nobody has written, so the slot's records no longer stand
        if (before[0] != sl.d_ftris.ptr || before[1] != sl.d_tnum.ptr || before[2] != sl.d_ray_colp.ptr || before[3] != sl.d_ray_row.ptr)
            sl.records_key.clear();
        if (before[2] != sl.d_ray_colp.ptr || before[3] != sl.d_ray_row.ptr) sl.forget_ray_plane();   // (its key names the tables' addresses)
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace rwr

using namespace rwr;

namespace {

// Targets of slot `i` for the current screen (the reference's textures start zeroed and are cleared every frame).
hipError_t ensure_slot_targets(rwr_context *ctx, uint32_t i)
{
    FrameSlot &sl = ctx->slots[i];
    const size_t n = (size_t)ctx->screen.width * ctx->screen.height;
    if (n == 0) return hipSuccess;
    hipError_t e;
    if ((e = sl.d_color.ensure(n * 4)) != hipSuccess || (e = sl.d_depth.ensure(n)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(sl.d_color.ptr, 0, n * 4, sl.stream)) != hipSuccess) return e;
    return hipMemsetAsync(sl.d_depth.ptr, 0, n * sizeof(float), sl.stream);
}

// The tunables: an unset variable leaves the default, and the helpers say whether it was set.  Parsed as ever: strtoull base
// 10 (cut to 32 bits where the field has 32), atof, atoi != 0.
bool env_u64(const char *name, uint64_t *v) { const char *e = std::getenv(name); if (e) *v = std::strtoull(e, nullptr, 10); return e != nullptr; }
bool env_u32(const char *name, uint32_t *v) { uint64_t w = 0; const bool set = env_u64(name, &w); if (set) *v = (uint32_t)w; return set; }
bool env_f32(const char *name, float *v) { const char *e = std::getenv(name); if (e) *v = (float)std::atof(e); return e != nullptr; }
bool env_flag(const char *name, bool *v) { const char *e = std::getenv(name); if (e) *v = std::atoi(e) != 0; return e != nullptr; }

void read_tunables(rwr_context *ctx)
{
    env_u32("RWR_WAVE_CULL_MIN", &ctx->wave_cull_min);
    env_flag("RWR_ONE_PIXEL_PER_LANE", &ctx->force_one_pixel);
    env_flag("RWR_FRAME_GRAPH", &ctx->frame_graph);
    if (env_flag("RWR_FUSED_SETUP", &ctx->fused_setup)) ctx->fused_setup_force = ctx->fused_setup;
    env_flag("RWR_TILE_LISTS", &ctx->tile_lists);
    env_flag("RWR_SETUP_CACHE", &ctx->setup_cache);
    env_flag("RWR_RAY_PLANE", &ctx->ray_plane);
    env_flag("RWR_TILE_CLASS", &ctx->tile_class);
    env_flag("RWR_TILE_COVER", &ctx->tile_cover);
    env_flag("RWR_LEAN_REST", &ctx->lean_rest);
    env_f32("RWR_AUTO_BVH_FACE_PX", &ctx->auto_bvh_face_px);
    if (env_u32("RWR_WF_GROUP", &ctx->wf_group)) ctx->wf_group = std::min(kWfMaxGroup, std::max(1u, ctx->wf_group));
    bool stats = false, wide = false;
    if (env_flag("RWR_WF_STATS", &stats) && stats && ctx->d_wf_dbg.ensure(4) == hipSuccess) {
        (void)hipMemset(ctx->d_wf_dbg.ptr, 0, 32);
        wf_trace_launch_counts(ctx->wf_launches_before);
    }
    if (env_u32("RWR_WF_OVERLAP", &ctx->wf_queues)) ctx->wf_queues = std::min(kWfMaxQueues, std::max(1u, ctx->wf_queues));
    env_u32("RWR_WF_ZSPLIT", &ctx->wf_z_split);
    env_u32("RWR_WF_PACKET_RAYS", &ctx->wf_packet_dense_rays);
    if (env_flag("RWR_WF_WIDE_LANE", &wide)) ctx->wf_wide_lane = wide ? 1 : 0;
    if (const char *e = std::getenv("RWR_WF_STACK16")) {   // a number that is 0 switches the 16-bit entries off; nothing switches them on
        char *end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end != e && *end == '\0' && v == 0) ctx->wf_stack16 = false;
    }
    if (env_u32("RWR_WF_LANE_ITEMS", &ctx->wf_lane_items)) ctx->wf_lane_items = std::max(1u, ctx->wf_lane_items);
    env_u32("RWR_WF_MIN_PACKET_POOLS", &ctx->wf_min_packet_pools);
    env_f32("RWR_WF_PACKET_EXTENT", &ctx->wf_packet_extent);
    env_f32("RWR_WF_PACKET_FILL", &ctx->wf_packet_fill);
    env_u32("RWR_BIN_CAPACITY", &ctx->bin_min_capacity);
    env_u32("RWR_BIN_MIN_FACES", &ctx->bin_min_faces);
    if (env_u64("RWR_ACCUM_MAX_SAMPLES", &ctx->accum_max)) ctx->accum_max = std::min<uint64_t>(1u << 24, std::max<uint64_t>(1u, ctx->accum_max));
}
}  // namespace

// RWR_FLAG_LIGHT_SKY item 1: the table of the context's image, built on the host by the first frame that asks for the flag after the image
// changed, into a buffer of its own, filled before anything can read it (as the image is: the buffer before stays with the frame
// slots whose frames read it, WfState::sky_light).  No image, or an image without weight: no table, and the flag is not effective.
int rwr::scene_sky_light(rwr_context *ctx, bool &have)
{
    if (ctx->sky_light_generation != ctx->sky_image_generation) {
        ctx->sky_light.reset();
        if (ctx->sky_image && !ctx->sky_image_host.empty()) {
            const std::vector<float> table = build_sky_light(&ctx->sky_image_host[0].x, ctx->sky_image_n, 4u);
            if (!table.empty()) {
                DeviceGuard g(ctx->device);
                auto buf = std::make_shared<DeviceBuffer<float>>();
                RWR_HIP_CHECK(buf->ensure(table.size()));
                RWR_HIP_CHECK(hipMemcpy(buf->ptr, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
                ctx->sky_light = std::move(buf);
            }
        }
        ctx->sky_light_generation = ctx->sky_image_generation;
    }
    have = ctx->sky_light != nullptr;
    return RWR_OK;
}

extern "C" {

const char *rwr_last_error_string(void) { return g_last_error.c_str(); }

int rwr_device_count(int *out_count)
{
    if (!out_count) return set_error(RWR_ERR_INVALID_ARGUMENT, "out_count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out_count = 0;
        return set_error(RWR_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    }
    *out_count = n;
    return RWR_OK;
}

int rwr_ctx_create(int device_id, rwr_context **out_ctx)
{
    if (!out_ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return set_error(RWR_ERR_HIP, "no HIP device available (%s)", e == hipSuccess ? "count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "device_id %d out of range [0,%d)", device_id, n);
    rwr_context *ctx = new (std::nothrow) rwr_context();
    if (!ctx) return set_error(RWR_ERR_HIP, "out of host memory");
    ctx->device = device_id;
    DeviceGuard g(device_id);
    if (!g.ok) {
        delete ctx;
        return set_error(RWR_ERR_HIP, "hipSetDevice(%d) failed", device_id);
    }
    if ((e = hipStreamCreateWithFlags(&ctx->own_stream.h, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&ctx->ev_begin.h)) != hipSuccess || (e = hipEventCreate(&ctx->ev_end.h)) != hipSuccess) {
        rwr_ctx_destroy(ctx);
        return set_error(RWR_ERR_HIP, "stream/event creation failed: %s", hipGetErrorString(e));
    }
    {   // the sRGB decode table of the frame kernel's quad texels (every frame kernel reads it, with or without a mesh)
        float lut[256];
        build_srgb_lut(lut);
        if ((e = ctx->d_srgb_lut.ensure(256)) != hipSuccess || (e = hipMemcpy(ctx->d_srgb_lut.ptr, lut, sizeof lut, hipMemcpyHostToDevice)) != hipSuccess) {
            rwr_ctx_destroy(ctx);
            return set_error(RWR_ERR_HIP, "sRGB table upload failed: %s", hipGetErrorString(e));
        }
    }
    ctx->stream = ctx->own_stream;
    ctx->slots[0].stream = ctx->stream;
    (void)preload_kernels();   // have the code objects on the device before the first frame asks for them
    read_tunables(ctx);
    *out_ctx = ctx;
    return RWR_OK;
}

void rwr_ctx_destroy(rwr_context *ctx)
{
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    (void)sync_all(ctx);
    for (WfState &w : ctx->wf_state)   // the side streams, which sync_all does not cover
        for (hipStream_t q : w.streams)
            if (q) (void)hipStreamSynchronize(q);
    if (ctx->probe_stream) (void)hipStreamSynchronize(ctx->probe_stream);
    if (ctx->d_wf_dbg.ptr) {
        unsigned long long h[4] = {0, 0, 0, 0};
        (void)hipMemcpy(h, ctx->d_wf_dbg.ptr, sizeof h, hipMemcpyDeviceToHost);
        std::fprintf(stderr, "rwr wavefront pools: packets %llu pools / %llu rays, per-lane %llu pools / %llu rays (leaf extent %g)\n",
                     h[0], h[1], h[2], h[3], (double)ctx->bvh_leaf_extent);
        uint64_t n[3];
        wf_trace_launch_counts(n);   // (of the process: exact while one context renders at a time)
        std::fprintf(stderr, "rwr wavefront launches: packet %llu, per-lane %llu, per-lane wide %llu\n",
                     (unsigned long long)(n[0] - ctx->wf_launches_before[0]), (unsigned long long)(n[1] - ctx->wf_launches_before[1]),
                     (unsigned long long)(n[2] - ctx->wf_launches_before[2]));
    }
    (void)rwr_dist_destroy(ctx);
    delete ctx;   // (inside the scope of the guard: the members free themselves with the right device current)
}

int rwr_ctx_device_info(rwr_context *ctx, char *name, size_t name_cap, int *cu_count, int *wave_size)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    hipDeviceProp_t prop;
    RWR_HIP_CHECK(hipGetDeviceProperties(&prop, ctx->device));
    if (name && name_cap) {
        std::snprintf(name, name_cap, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (wave_size) *wave_size = prop.warpSize;
    return RWR_OK;
}

int rwr_ctx_set_stream(rwr_context *ctx, void *hip_stream)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(sync_all(ctx));
    ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    ctx->slots[0].stream = ctx->stream;
    return RWR_OK;
}

void *rwr_ctx_get_stream(rwr_context *ctx) { return ctx ? reinterpret_cast<void *>(ctx->stream) : nullptr; }

int rwr_resize(rwr_context *ctx, const rwr_screen *screen)
{
    if (!ctx || !screen) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    // resize ignores zero sizes (lib.rs:773); here that is an explicit error.
    if (screen->width == 0 || screen->height == 0) return set_error(RWR_ERR_INVALID_ARGUMENT, "zero-sized screen");
    if ((uint64_t)screen->width * screen->height > (1ull << 30)) return set_error(RWR_ERR_INVALID_ARGUMENT, "screen too large");
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(sync_all(ctx));
    ctx->screen = *screen;
    ctx->accum.reset();   // (the key holds the screen size too)
    ctx->reproj.reset();  // (likewise; a resize to the same size starts a new history too)
    ctx->last_reproject_frames = 0;
    for (uint32_t i = 0; i < ctx->n_slots; i++) {
        RWR_HIP_CHECK(ensure_slot_targets(ctx, i));
        ctx->slots[i].aux_valid = false;
        ctx->slots[i].forget_ray_plane();   // (the key holds the screen size too; the buffer stays for the next build)
    }
    for (GatherSet &gs : ctx->gather) gs.valid = false;   // a frame gathered at the old size is gone
    RWR_HIP_CHECK(ensure_frame_buffers(ctx));
    return RWR_OK;
}

int rwr_synchronize(rwr_context *ctx)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(sync_all(ctx));
    for (uint32_t i = 0; i < ctx->n_slots; i++) {
        const int rc = check_fused_frame(ctx, i);
        if (rc != RWR_OK) return rc;
    }
    return RWR_OK;
}

int rwr_readback(rwr_context *ctx, uint8_t *rgba8, float *depth, float *rgba_f32, int32_t *obj_id, float *hit_t)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ctx->screen.width == 0) return set_error(RWR_ERR_NOT_READY, "rwr_resize has not been called");
    if ((rgba_f32 || obj_id || hit_t) && !ctx->slots[ctx->cur].aux_valid)
        return set_error(RWR_ERR_NOT_READY, "aux planes requested but the last render did not set RWR_FLAG_AUX_OUTPUTS");
    DeviceGuard g(ctx->device);
    const size_t n = (size_t)ctx->screen.width * ctx->screen.height;
    RWR_HIP_CHECK(hipStreamSynchronize(ctx->slots[ctx->cur].stream));
    {
        const int rc = check_fused_frame(ctx, ctx->cur);
        if (rc != RWR_OK) return rc;
    }
    if (rgba8) RWR_HIP_CHECK(hipMemcpy(rgba8, ctx->slots[ctx->cur].d_color.ptr, n * 4, hipMemcpyDeviceToHost));
    if (depth) RWR_HIP_CHECK(hipMemcpy(depth, ctx->slots[ctx->cur].d_depth.ptr, n * sizeof(float), hipMemcpyDeviceToHost));
    if (rgba_f32) RWR_HIP_CHECK(hipMemcpy(rgba_f32, ctx->slots[ctx->cur].d_color_f32.ptr, n * 4 * sizeof(float), hipMemcpyDeviceToHost));
    if (obj_id) RWR_HIP_CHECK(hipMemcpy(obj_id, ctx->slots[ctx->cur].d_obj_id.ptr, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (hit_t) RWR_HIP_CHECK(hipMemcpy(hit_t, ctx->slots[ctx->cur].d_hit_t.ptr, n * sizeof(float), hipMemcpyDeviceToHost));
    return RWR_OK;
}

int rwr_get_device_targets(rwr_context *ctx, void **d_rgba8, void **d_depth)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ctx->screen.width == 0) return set_error(RWR_ERR_NOT_READY, "rwr_resize has not been called");
    if (ctx->cur != 0u) {
        // the frame rendered last ran on an internal stream: order the context's stream (rwr_ctx_get_stream) after it,
        // so that whatever the caller enqueues there next sees the finished targets
        DeviceGuard g(ctx->device);
        FrameSlot &sl = ctx->slots[ctx->cur];
        RWR_HIP_CHECK(hipEventRecord(sl.done, sl.stream));
        RWR_HIP_CHECK(hipStreamWaitEvent(ctx->stream, sl.done, 0));
    }
    if (d_rgba8) *d_rgba8 = ctx->slots[ctx->cur].d_color.ptr;
    if (d_depth) *d_depth = ctx->slots[ctx->cur].d_depth.ptr;
    return RWR_OK;
}

int rwr_ctx_set_frames_in_flight(rwr_context *ctx, uint32_t n)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (n < 1u || n > kMaxFramesInFlight)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "frames in flight must be 1..%u", kMaxFramesInFlight);
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(sync_all(ctx));
    for (uint32_t i = 1; i < n; i++) {
        FrameSlot &sl = ctx->slots[i];
        if (!sl.owned) RWR_HIP_CHECK(hipStreamCreateWithFlags(&sl.owned.h, hipStreamNonBlocking));
        if (!sl.done) RWR_HIP_CHECK(hipEventCreateWithFlags(&sl.done.h, hipEventDisableTiming));
        sl.stream = sl.owned;
    }
    for (uint32_t i = n; i < kMaxFramesInFlight; i++) {  // slots no longer used give their memory back
        ctx->slots[i].reset();
        ctx->wf_state[i] = WfState{};   // (gigabytes of ray queue when the slot rendered path-traced frames)
        ctx->gather[i] = GatherSet{};
    }
    if (ctx->last_gather >= n) ctx->last_gather = 0;
    if (ctx->last_wf_state >= n) { ctx->last_wf_state = 0; ctx->last_segments = 0; ctx->last_spp = 0; }
    // the most recent frame stays where it is if its slot survives, otherwise it is gone
    ctx->n_slots = n;
    if (ctx->cur >= n) ctx->cur = 0;
    for (uint32_t i = 0; i < n; i++)
        if (!ctx->slots[i].d_color.ptr) RWR_HIP_CHECK(ensure_slot_targets(ctx, i));
    RWR_HIP_CHECK(ensure_frame_buffers(ctx));
    RWR_HIP_CHECK(sync_all(ctx));
    return RWR_OK;
}

int rwr_timer_begin(rwr_context *ctx)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    DeviceGuard g(ctx->device);
    if (ctx->n_slots > 1u) RWR_HIP_CHECK(sync_all(ctx));  // the interval starts with nothing in flight
    RWR_HIP_CHECK(hipEventRecord(ctx->ev_begin, ctx->stream));
    return RWR_OK;
}

int rwr_timer_end(rwr_context *ctx, float *elapsed_ms)
{
    if (!ctx || !elapsed_ms) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard g(ctx->device);
    const int rc = rwr_timer_stop(ctx);
    return rc == RWR_OK ? rwr_timer_elapsed(ctx, elapsed_ms) : rc;
}

int rwr_timer_stop(rwr_context *ctx)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    DeviceGuard g(ctx->device);
    for (uint32_t i = 1; i < ctx->n_slots; i++) {  // the interval ends when every frame in flight has ended
        RWR_HIP_CHECK(hipEventRecord(ctx->slots[i].done, ctx->slots[i].stream));
        RWR_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->slots[i].done, 0));
    }
    RWR_HIP_CHECK(hipEventRecord(ctx->ev_end, ctx->stream));
    return RWR_OK;
}

int rwr_timer_elapsed(rwr_context *ctx, float *elapsed_ms)
{
    if (!ctx || !elapsed_ms) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(hipEventSynchronize(ctx->ev_end));
    RWR_HIP_CHECK(hipEventElapsedTime(elapsed_ms, ctx->ev_begin, ctx->ev_end));
    return RWR_OK;
}

int rwr_ctx_set_kernel_timing(rwr_context *ctx, uint32_t every_n)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ctx->timing_every = every_n;
    ctx->timing_calls = 0;
    ctx->timing_pairs = 0;
    return RWR_OK;
}

int rwr_kernel_timing_stats(rwr_context *ctx, double *mean_us, uint32_t *count)
{
    if (!ctx || !mean_us || !count) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(sync_all(ctx));
    double sum = 0.0;
    for (uint32_t i = 0; i < ctx->timing_pairs; i++) {
        float ms = 0.0f;
        RWR_HIP_CHECK(hipEventElapsedTime(&ms, ctx->timing_events[2 * i], ctx->timing_events[2 * i + 1]));
        sum += ms * 1e3;
    }
    *count = ctx->timing_pairs;
    *mean_us = ctx->timing_pairs ? sum / ctx->timing_pairs : 0.0;
    return RWR_OK;
}

int rwr_last_render_stats(rwr_context *ctx, uint64_t *primary_rays, uint64_t *bounce_rays)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ctx->last_spp && ctx->last_had_bounce) {
        DeviceGuard g(ctx->device);
        std::vector<uint32_t> counts((size_t)ctx->last_segments * 4u);   // per tile and wave of the primary stage
        RWR_HIP_CHECK(hipStreamSynchronize(ctx->slots[ctx->cur].stream));
        RWR_HIP_CHECK(hipMemcpy(counts.data(), ctx->wf_state[ctx->last_wf_state].d_wave_total.ptr, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        ctx->last_bounce = 0;
        for (uint32_t c : counts) ctx->last_bounce += c;
    }
    if (primary_rays) *primary_rays = ctx->last_primary;
    if (bounce_rays) *bounce_rays = ctx->last_bounce;
    return RWR_OK;
}

int rwr_frame_setup_launches(rwr_context *ctx, uint64_t *launches)
{
    if (!ctx || !launches) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *launches = ctx->setup_launches;
    return RWR_OK;
}

int rwr_ray_plane_stats(rwr_context *ctx, uint64_t *builds, uint64_t *frames)
{
    if (!ctx || !builds || !frames) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *builds = ctx->ray_plane_builds;
    *frames = ctx->ray_plane_frames;
    return RWR_OK;
}

int rwr_last_shadow_stats(rwr_context *ctx, uint64_t *shadow_rays, uint64_t *occluded)
{
    if (!ctx || !shadow_rays || !occluded) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    unsigned long long counts[2] = {0ull, 0ull};
    if (ctx->last_shadows && ctx->wf_state[ctx->last_wf_state].d_shadow_counts.ptr) {
        DeviceGuard g(ctx->device);
        RWR_HIP_CHECK(hipStreamSynchronize(ctx->slots[ctx->cur].stream));
        RWR_HIP_CHECK(hipMemcpy(counts, ctx->wf_state[ctx->last_wf_state].d_shadow_counts.ptr, sizeof counts, hipMemcpyDeviceToHost));
    }
    *shadow_rays = counts[0];
    *occluded = counts[1];
    return RWR_OK;
}

int rwr_last_glass_stats(rwr_context *ctx, uint64_t *reflected, uint64_t *transmitted, uint64_t *tir)
{
    if (!ctx || !reflected || !transmitted || !tir) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    unsigned long long counts[kEventGlossy] = {0ull, 0ull, 0ull};   // the glass events come first
    if (ctx->last_glass && ctx->wf_state[ctx->last_wf_state].d_surface_events.ptr) {
        DeviceGuard g(ctx->device);
        RWR_HIP_CHECK(hipStreamSynchronize(ctx->slots[ctx->cur].stream));
        RWR_HIP_CHECK(hipMemcpy(counts, ctx->wf_state[ctx->last_wf_state].d_surface_events.ptr, sizeof counts, hipMemcpyDeviceToHost));
    }
    *reflected = counts[kEventReflected];
    *transmitted = counts[kEventTransmitted];
    *tir = counts[kEventTotalReflection];
    return RWR_OK;
}

int rwr_last_gloss_stats(rwr_context *ctx, uint64_t *glossy_rays)
{
    if (!ctx || !glossy_rays) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    unsigned long long count = 0ull;
    if (ctx->last_gloss && ctx->wf_state[ctx->last_wf_state].d_surface_events.ptr) {
        DeviceGuard g(ctx->device);
        RWR_HIP_CHECK(hipStreamSynchronize(ctx->slots[ctx->cur].stream));
        RWR_HIP_CHECK(hipMemcpy(&count, ctx->wf_state[ctx->last_wf_state].d_surface_events.ptr + kEventGlossy, sizeof count, hipMemcpyDeviceToHost));
    }
    *glossy_rays = count;
    return RWR_OK;
}

int rwr_last_emission_stats(rwr_context *ctx, uint64_t *emissive_hits)
{
    if (!ctx || !emissive_hits) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    unsigned long long count = 0ull;
    if (ctx->last_glow && ctx->wf_state[ctx->last_wf_state].d_glow_hits.ptr) {
        DeviceGuard g(ctx->device);
        RWR_HIP_CHECK(hipStreamSynchronize(ctx->slots[ctx->cur].stream));
        RWR_HIP_CHECK(hipMemcpy(&count, ctx->wf_state[ctx->last_wf_state].d_glow_hits.ptr, sizeof count, hipMemcpyDeviceToHost));
    }
    *emissive_hits = count;
    return RWR_OK;
}

// the last frame's nine light counts (WfGlow::light_counts): the stage's totals, then the mesh light's share, then the sky's; zeros for a frame without the stage
static int last_light_counts(rwr_context *ctx, unsigned long long counts[9])
{
    for (int i = 0; i < 9; i++) counts[i] = 0ull;
    if (ctx->last_light && ctx->wf_state[ctx->last_wf_state].d_light_counts.ptr) {
        DeviceGuard g(ctx->device);
        RWR_HIP_CHECK(hipStreamSynchronize(ctx->slots[ctx->cur].stream));
        RWR_HIP_CHECK(hipMemcpy(counts, ctx->wf_state[ctx->last_wf_state].d_light_counts.ptr, 9 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    return RWR_OK;
}

int rwr_last_light_stats(rwr_context *ctx, uint64_t *light_rays, uint64_t *reached, uint64_t *suppressed_hits)
{
    if (!ctx || !light_rays || !reached || !suppressed_hits) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    unsigned long long counts[9];
    const int rc = last_light_counts(ctx, counts);
    if (rc != RWR_OK) return rc;
    *light_rays = counts[0]; *reached = counts[1]; *suppressed_hits = counts[2];
    return RWR_OK;
}

int rwr_last_part_light_stats(rwr_context *ctx, uint64_t *light_rays, uint64_t *reached, uint64_t *suppressed_hits)
{
    if (!ctx || !light_rays || !reached || !suppressed_hits) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    unsigned long long counts[9];
    const int rc = last_light_counts(ctx, counts);
    if (rc != RWR_OK) return rc;
    *light_rays = counts[3]; *reached = counts[4]; *suppressed_hits = counts[5];
    return RWR_OK;
}

int rwr_last_sky_light_stats(rwr_context *ctx, uint64_t *light_rays, uint64_t *reached, uint64_t *suppressed_misses)
{
    if (!ctx || !light_rays || !reached || !suppressed_misses) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    unsigned long long counts[9];
    const int rc = last_light_counts(ctx, counts);
    if (rc != RWR_OK) return rc;
    *light_rays = counts[6]; *reached = counts[7]; *suppressed_misses = counts[8];
    return RWR_OK;
}

int rwr_denoise_set_params(rwr_context *ctx, const rwr_denoise_params *params)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!params) {
        ctx->denoise = kDenoiseDefaults;
        return RWR_OK;
    }
    const rwr_denoise_params p = *params;
    if (p.iterations < 1u || p.iterations > 5u) return set_error(RWR_ERR_INVALID_ARGUMENT, "denoise iterations %u: 1 ... 5", p.iterations);
    // inv_0 = 1 / (sigma * sigma) and its multiples up to 4^4 must be finite f32 numbers, sigma * sigma non-zero
    const float s2 = p.sigma_color * p.sigma_color, inv4 = 1.0f / s2 * 256.0f;
    if (!(p.sigma_color > 0.0f) || !std::isfinite(p.sigma_color) || !(s2 > 0.0f) || !std::isfinite(inv4))
        return set_error(RWR_ERR_INVALID_ARGUMENT, "denoise sigma_color %g: positive, finite, 256 / sigma^2 finite", (double)p.sigma_color);
    if (std::isnan(p.normal_cos_min)) return set_error(RWR_ERR_INVALID_ARGUMENT, "denoise normal_cos_min is NaN");
    if (!(p.depth_rel >= 0.0f)) return set_error(RWR_ERR_INVALID_ARGUMENT, "denoise depth_rel %g: >= 0", (double)p.depth_rel);
    ctx->denoise = p;
    return RWR_OK;
}

int rwr_denoise_get_params(rwr_context *ctx, rwr_denoise_params *out)
{
    if (!ctx || !out) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = ctx->denoise;
    return RWR_OK;
}

// RWR_FLAG_TONEMAP: no history holds these — an accumulation and a reprojection history go on across a call
int rwr_tonemap_set_params(rwr_context *ctx, const rwr_tonemap_params *params)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!params) {
        ctx->tonemap = kTonemapDefaults;
        return RWR_OK;
    }
    const rwr_tonemap_params p = *params;
    const float lo = 1.0f / 65536.0f, hi = 65536.0f;
    auto within = [](float v, float a, float b) { return v >= a && v <= b; };   // (false for NaN)
    if (p.curve > (uint32_t)RWR_TONEMAP_ACES) return set_error(RWR_ERR_INVALID_ARGUMENT, "tonemap curve %u: 0 (clamp), 1 (Reinhard), 2 (ACES)", p.curve);
    if (p.auto_exposure > 1u) return set_error(RWR_ERR_INVALID_ARGUMENT, "tonemap auto_exposure %u: 0 or 1", p.auto_exposure);
    if (!within(p.exposure, lo, hi)) return set_error(RWR_ERR_INVALID_ARGUMENT, "tonemap exposure %g: finite, 2^-16 ... 2^16", (double)p.exposure);
    if (!within(p.key, lo, hi)) return set_error(RWR_ERR_INVALID_ARGUMENT, "tonemap key %g: finite, 2^-16 ... 2^16", (double)p.key);
    if (!within(p.white, 1.0f / 256.0f, hi)) return set_error(RWR_ERR_INVALID_ARGUMENT, "tonemap white %g: finite, 2^-8 ... 2^16", (double)p.white);
    ctx->tonemap = p;
    return RWR_OK;
}

int rwr_tonemap_get_params(rwr_context *ctx, rwr_tonemap_params *out)
{
    if (!ctx || !out) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = ctx->tonemap;
    return RWR_OK;
}

// the last frame's sums from its slot's record; E on the host, by the function k_tm_exposure calls
int rwr_last_tonemap_stats(rwr_context *ctx, int64_t *log_sum, uint32_t *count, float *exposure)
{
    if (!ctx || !log_sum || !count || !exposure) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    TonemapRecord rec{0, 0u, 0.0f};
    const rwr_tonemap_params &tp = ctx->last_tonemap_params;
    if (ctx->last_tonemap && tp.auto_exposure && ctx->slots[ctx->cur].d_tm_record.ptr) {
        DeviceGuard g(ctx->device);
        RWR_HIP_CHECK(hipStreamSynchronize(ctx->slots[ctx->cur].stream));
        RWR_HIP_CHECK(hipMemcpy(&rec, ctx->slots[ctx->cur].d_tm_record.ptr, sizeof rec, hipMemcpyDeviceToHost));
    }
    *log_sum = rec.log_sum;
    *count = rec.count;
    *exposure = ctx->last_tonemap ? tonemap_exposure(rec.log_sum, rec.count, tp.auto_exposure, tp.key, tp.exposure) : 0.0f;
    return RWR_OK;
}

// every accepted call starts a new history, also one that sets the values the context has (as the mirror setters change the scene)
int rwr_reproject_set_params(rwr_context *ctx, const rwr_reproject_params *params)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    rwr_reproject_params p = kReprojectDefaults;
    if (params) p = *params;
    if (p.max_history < 1u || p.max_history > 1024u) return set_error(RWR_ERR_INVALID_ARGUMENT, "reproject max_history %u: 1 ... 1024", p.max_history);
    if (!(p.normal_cos_min >= -1.0f && p.normal_cos_min <= 1.0f))   // (false for NaN)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "reproject normal_cos_min %g: finite, -1 ... 1", (double)p.normal_cos_min);
    if (!(p.depth_rel >= 0.0f) || !std::isfinite(p.depth_rel))
        return set_error(RWR_ERR_INVALID_ARGUMENT, "reproject depth_rel %g: finite, >= 0", (double)p.depth_rel);
    ctx->reproject = p;
    ctx->reproj.key.clear();
    return RWR_OK;
}

int rwr_reproject_get_params(rwr_context *ctx, rwr_reproject_params *out)
{
    if (!ctx || !out) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = ctx->reproject;
    return RWR_OK;
}

int rwr_reproject_reset(rwr_context *ctx)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ctx->reproj.key.clear();
    return RWR_OK;
}

int rwr_reproject_frames(rwr_context *ctx, uint64_t *frames)
{
    if (!ctx || !frames) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *frames = ctx->last_reproject_frames;
    return RWR_OK;
}

int rwr_last_reproject_stats(rwr_context *ctx, uint64_t *reused, uint64_t *fresh, uint64_t *background)
{
    if (!ctx || !reused || !fresh || !background) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    unsigned long long counts[3] = {0ull, 0ull, 0ull};
    if (ctx->last_reproject_frames != 0 && ctx->reproj.d_counts.ptr) {
        DeviceGuard g(ctx->device);
        RWR_HIP_CHECK(hipStreamSynchronize(ctx->slots[ctx->cur].stream));
        RWR_HIP_CHECK(hipMemcpy(counts, ctx->reproj.d_counts.ptr + 3u * ctx->last_reproject_set, sizeof counts, hipMemcpyDeviceToHost));
    }
    *reused = counts[0];
    *fresh = counts[1];
    *background = counts[2];
    return RWR_OK;
}

int rwr_reproject_readback(rwr_context *ctx, float *history_len)
{
    if (!ctx || !history_len) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    const DeviceBuffer<float4> &plane = ctx->reproj.d_colour[ctx->last_reproject_set];
    const size_t n = (size_t)ctx->screen.width * ctx->screen.height;
    if (ctx->last_reproject_frames == 0 || !plane.ptr || plane.count < n)
        return set_error(RWR_ERR_NOT_READY, "the last render did not set RWR_FLAG_REPROJECT");
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(hipStreamSynchronize(ctx->slots[ctx->cur].stream));
    std::vector<float4> records(n);   // n' is the fourth float of the history's colour records
    RWR_HIP_CHECK(hipMemcpy(records.data(), plane.ptr, n * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) history_len[i] = records[i].w;
    return RWR_OK;
}

int rwr_sky_set_params(rwr_context *ctx, const rwr_sky_params *params)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!params) {
        ctx->sky = kSkyDefaults;
        return RWR_OK;
    }
    const rwr_sky_params p = *params;
    for (int c = 0; c < 3; c++) {
        if (!(p.zenith[c] >= 0.0f && p.zenith[c] <= RWR_SKY_COMPONENT_MAX))   // (false for NaN)
            return set_error(RWR_ERR_INVALID_ARGUMENT, "sky zenith[%d] %g: finite, 0 ... 16", c, (double)p.zenith[c]);
        if (!(p.horizon[c] >= 0.0f && p.horizon[c] <= RWR_SKY_COMPONENT_MAX))
            return set_error(RWR_ERR_INVALID_ARGUMENT, "sky horizon[%d] %g: finite, 0 ... 16", c, (double)p.horizon[c]);
    }
    ctx->sky = p;
    return RWR_OK;
}

int rwr_sky_get_params(rwr_context *ctx, rwr_sky_params *out)
{
    if (!ctx || !out) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = ctx->sky;
    return RWR_OK;
}

// The image goes into a buffer of its own, filled before anything can read it; the context then points at it.  The buffer before
// stays with the frame slots whose frames read it (WfState::sky_image) and goes when the last of them lets go (hipFree waits for the device).
int rwr_sky_set_image(rwr_context *ctx, const float *rgb, uint32_t n)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!rgb || n == 0u) {
        ctx->sky_image.reset();
        ctx->sky_image_n = 0u;
        ctx->sky_image_generation++;
        ctx->sky_image_host = std::vector<float4>();
        return RWR_OK;
    }
    if (n < 2u || n > RWR_SKY_IMAGE_SIZE_MAX)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "sky image size %u: 2 ... %u", n, RWR_SKY_IMAGE_SIZE_MAX);
    const size_t texels = (size_t)n * n;
    std::vector<float4> host(texels);
    for (size_t i = 0; i < texels * 3u; i++) {
        if (!(rgb[i] >= 0.0f && rgb[i] <= RWR_SKY_IMAGE_COMPONENT_MAX))   // (false for NaN)
            return set_error(RWR_ERR_INVALID_ARGUMENT, "sky image component [%zu] %g: finite, 0 ... 64", i, (double)rgb[i]);
    }
    for (size_t i = 0; i < texels; i++) host[i] = make_float4(rgb[3u * i], rgb[3u * i + 1u], rgb[3u * i + 2u], 0.0f);
    DeviceGuard g(ctx->device);
    auto buf = std::make_shared<DeviceBuffer<float4>>();
    RWR_HIP_CHECK(buf->ensure(texels));
    RWR_HIP_CHECK(hipMemcpy(buf->ptr, host.data(), texels * sizeof(float4), hipMemcpyHostToDevice));
    ctx->sky_image = std::move(buf);
    ctx->sky_image_n = n;
    ctx->sky_image_generation++;
    ctx->sky_image_host = std::move(host);   // (RWR_FLAG_LIGHT_SKY builds its table from these texels, when a frame first asks)
    return RWR_OK;
}

int rwr_sky_get_light_info(rwr_context *ctx, uint32_t *n, uint64_t *generation)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    bool have = false;
    const int rc = rwr::scene_sky_light(ctx, have);
    if (rc != RWR_OK) return rc;
    if (n) *n = have ? ctx->sky_image_n : 0u;
    if (generation) *generation = ctx->sky_light_generation;
    return RWR_OK;
}

int rwr_sky_get_image_info(rwr_context *ctx, uint32_t *n, uint64_t *generation)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (n) *n = ctx->sky_image ? ctx->sky_image_n : 0u;
    if (generation) *generation = ctx->sky_image_generation;
    return RWR_OK;
}

int rwr_shadow_set_params(rwr_context *ctx, const rwr_shadow_params *params)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (!params) {
        ctx->shadow = kShadowDefaults;
        return RWR_OK;
    }
    const rwr_shadow_params p = *params;
    if (!(p.mesh_light_radius >= 0.0f && p.mesh_light_radius <= RWR_SHADOW_RADIUS_MAX))   // (false for NaN)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "shadow mesh_light_radius %g: finite, 0 ... 1", (double)p.mesh_light_radius);
    if (!(p.sphere_light_radius >= 0.0f && p.sphere_light_radius <= RWR_SHADOW_RADIUS_MAX))
        return set_error(RWR_ERR_INVALID_ARGUMENT, "shadow sphere_light_radius %g: finite, 0 ... 1", (double)p.sphere_light_radius);
    ctx->shadow = p;
    return RWR_OK;
}

int rwr_shadow_get_params(rwr_context *ctx, rwr_shadow_params *out)
{
    if (!ctx || !out) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *out = ctx->shadow;
    return RWR_OK;
}

int rwr_accum_reset(rwr_context *ctx)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ctx->accum.key.clear();
    ctx->accum.samples = 0;
    return RWR_OK;
}

int rwr_accum_samples(rwr_context *ctx, uint64_t *samples)
{
    if (!ctx || !samples) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *samples = ctx->last_accum_samples;
    return RWR_OK;
}

}  // extern "C"
