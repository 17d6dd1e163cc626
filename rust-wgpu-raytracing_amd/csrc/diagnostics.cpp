// Self-tests and clock measurements behind the C ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "rwr_context.h"

using namespace rwr;

// out4 += what one of the self-test kernels counted (kernels_selftest.hip)
template <typename Launch>
static int run_selftest(rwr_context *ctx, uint64_t out4[4], Launch launch)
{
    if (!ctx || !out4) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard g(ctx->device);
    DeviceBuffer<unsigned long long> d_out;
    RWR_HIP_CHECK(d_out.ensure(4));
    RWR_HIP_CHECK(hipMemsetAsync(d_out.ptr, 0, 4 * sizeof(unsigned long long), ctx->stream));
    RWR_HIP_CHECK(launch(d_out.ptr));
    unsigned long long h[4];
    RWR_HIP_CHECK(hipMemcpyAsync(h, d_out.ptr, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    RWR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; k++) out4[k] = h[k];
    return RWR_OK;
}

extern "C" {

int rwr_selftest_exact_math(rwr_context *ctx, uint32_t normalize_count, uint32_t seed, uint64_t out4[4])
{
    return run_selftest(ctx, out4, [&](unsigned long long *d) { return launch_selftest_exact_math(ctx->stream, d, normalize_count, seed); });
}

int rwr_selftest_exact_div(rwr_context *ctx, uint32_t count, uint32_t seed, uint64_t out4[4])
{
    return run_selftest(ctx, out4, [&](unsigned long long *d) { return launch_selftest_exact_div(ctx->stream, d, count, seed); });
}

int rwr_selftest_sobol(rwr_context *ctx, const uint32_t *pixel, const uint32_t *sample, const uint32_t *dim, const uint32_t *seed, size_t n,
                       uint32_t *out)
{
    if (!ctx || !pixel || !sample || !dim || !seed || !out) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > (size_t)1 << 24) return set_error(RWR_ERR_INVALID_ARGUMENT, "at most 2^24 tuples a call, not %zu", n);
    if (n == 0) return RWR_OK;
    DeviceGuard g(ctx->device);
    DeviceBuffer<uint32_t> d;   // the four columns, then the words
    RWR_HIP_CHECK(d.ensure(5 * n));
    const uint32_t *cols[4] = {pixel, sample, dim, seed};
    for (size_t k = 0; k < 4; k++)
        RWR_HIP_CHECK(hipMemcpyAsync(d.ptr + k * n, cols[k], n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    RWR_HIP_CHECK(launch_selftest_sobol(ctx->stream, d.ptr, (uint32_t)n, d.ptr + 4 * n));
    RWR_HIP_CHECK(hipMemcpyAsync(out, d.ptr + 4 * n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    RWR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RWR_OK;
}

int rwr_selftest_sky_image(rwr_context *ctx, const float *dirs, size_t count, float *out_rgb)
{
    if (!ctx || !dirs || !out_rgb) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (count > (size_t)1 << 24) return set_error(RWR_ERR_INVALID_ARGUMENT, "at most 2^24 directions a call, not %zu", count);
    if (!ctx->sky_image) return set_error(RWR_ERR_NOT_READY, "the context holds no sky image (rwr_sky_set_image)");
    if (count == 0) return RWR_OK;
    DeviceGuard g(ctx->device);
    const std::shared_ptr<DeviceBuffer<float4>> image = ctx->sky_image;
    DeviceBuffer<float> d;   // the directions, then the values
    RWR_HIP_CHECK(d.ensure(6 * count));
    RWR_HIP_CHECK(hipMemcpyAsync(d.ptr, dirs, 3 * count * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    RWR_HIP_CHECK(launch_selftest_sky_image(ctx->stream, WfSkyImage{image->ptr, ctx->sky_image_n, 0u, nullptr}, d.ptr, (uint32_t)count, d.ptr + 3 * count));
    RWR_HIP_CHECK(hipMemcpyAsync(out_rgb, d.ptr + 3 * count, 3 * count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    RWR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RWR_OK;
}

int rwr_selftest_sky_light(rwr_context *ctx, const float *u4, size_t count, const float normal[3], uint32_t n_lights, float *out)
{
    if (!ctx || !u4 || !normal || !out) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (count > (size_t)1 << 24) return set_error(RWR_ERR_INVALID_ARGUMENT, "at most 2^24 tuples a call, not %zu", count);
    if (!ctx->sky_image) return set_error(RWR_ERR_NOT_READY, "the context holds no sky image (rwr_sky_set_image)");
    bool have = false;
    const int rc = scene_sky_light(ctx, have);
    if (rc != RWR_OK) return rc;
    if (!have) return set_error(RWR_ERR_NOT_READY, "the sky image has no weight (every texel is black): there is no table to draw from");
    if (count == 0) return RWR_OK;
    DeviceGuard g(ctx->device);
    const std::shared_ptr<DeviceBuffer<float4>> image = ctx->sky_image;
    const std::shared_ptr<DeviceBuffer<float>> table = ctx->sky_light;
    DeviceBuffer<float> d;   // the uniforms, then the records
    RWR_HIP_CHECK(d.ensure(12 * count));
    RWR_HIP_CHECK(hipMemcpyAsync(d.ptr, u4, 4 * count * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    RWR_HIP_CHECK(launch_selftest_sky_light(ctx->stream, WfSkyImage{image->ptr, ctx->sky_image_n, 0u, table->ptr}, d.ptr, (uint32_t)count, normal, n_lights,
                                            d.ptr + 4 * count));
    RWR_HIP_CHECK(hipMemcpyAsync(out, d.ptr + 4 * count, 8 * count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    RWR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return RWR_OK;
}

int rwr_debug_tile_classes(rwr_context *ctx, uint32_t *classes, size_t capacity, uint32_t *grid_x, uint32_t *grid_y)
{
    if (!ctx || !grid_x || !grid_y) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    const rwr_context::LastClasses lc = ctx->last_classes;
    const size_t n = (size_t)lc.gx * lc.gy * 4u;
    if (n == 0 || lc.slot >= ctx->n_slots || ctx->slots[lc.slot].d_tile_lists.count < tile_list_words(lc.gx, lc.gy))
        return set_error(RWR_ERR_NOT_READY, "the frame rendered last has no tile classes (they come with the per-tile face sets of the "
                         "two-pixel frame kernel's two-launch form: a scene of at most %u faces, culled)", kTileListMaxFaces);
    *grid_x = lc.gx;
    *grid_y = lc.gy;
    if (!classes) return RWR_OK;
    if (capacity < n) return set_error(RWR_ERR_INVALID_ARGUMENT, "room for %zu class words, the frame has %zu", capacity, n);
    DeviceGuard g(ctx->device);
    FrameSlot &sl = ctx->slots[lc.slot];
    RWR_HIP_CHECK(hipMemcpyAsync(classes, sl.d_tile_lists.ptr + n * kTileListWords, n * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
    RWR_HIP_CHECK(hipStreamSynchronize(sl.stream));   // that frame's stream alone
    return RWR_OK;
}

int rwr_debug_tile_cover(rwr_context *ctx, uint32_t *cover, size_t capacity, uint32_t *grid_x, uint32_t *grid_y)
{
    if (!ctx || !grid_x || !grid_y) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    const rwr_context::LastClasses lc = ctx->last_classes;
    const size_t n = (size_t)lc.gx * lc.gy * 4u;
    if (n == 0 || lc.slot >= ctx->n_slots || ctx->slots[lc.slot].d_tile_lists.count < tile_list_words(lc.gx, lc.gy))
        return set_error(RWR_ERR_NOT_READY, "the frame rendered last has no cover words (they lie beside the tile classes: rwr_debug_tile_classes)");
    *grid_x = lc.gx;
    *grid_y = lc.gy;
    if (!cover) return RWR_OK;
    if (capacity < n) return set_error(RWR_ERR_INVALID_ARGUMENT, "room for %zu cover words, the frame has %zu", capacity, n);
    DeviceGuard g(ctx->device);
    FrameSlot &sl = ctx->slots[lc.slot];
    RWR_HIP_CHECK(hipMemcpyAsync(cover, sl.d_tile_lists.ptr + n * (kTileListWords + 1u), n * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.stream));
    RWR_HIP_CHECK(hipStreamSynchronize(sl.stream));   // that frame's stream alone
    return RWR_OK;
}

int rwr_tile_cover_stats(rwr_context *ctx, uint64_t *frames, uint64_t *tiles_last)
{
    if (!ctx || !frames || !tiles_last) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *frames = ctx->tile_cover_frames;
    *tiles_last = 0;
    // The last frame took covered exactly the tiles whose words were set before it: none when it was its slot's first frame with
    // the flag since a setup (it learnt them), else the words as they stand (what a tile's tests say does not change while the
    // records stand, so every frame after the first finds and leaves the same words) — counted here, not by the kernel.
    if (ctx->last_cover_frames < 2u) return RWR_OK;
    uint32_t gx = 0, gy = 0;
    int rc = rwr_debug_tile_cover(ctx, nullptr, 0, &gx, &gy);
    if (rc != RWR_OK) return rc;
    std::vector<uint32_t> words((size_t)gx * gy * 4u);
    if ((rc = rwr_debug_tile_cover(ctx, words.data(), words.size(), &gx, &gy)) != RWR_OK) return rc;
    for (uint32_t w : words) *tiles_last += w == kTileCovered ? 1u : 0u;
    return RWR_OK;
}

int rwr_lean_rest_stats(rwr_context *ctx, uint64_t *frames)
{
    if (!ctx || !frames) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *frames = ctx->lean_rest_frames;
    return RWR_OK;
}

int rwr_last_traversal_plan(rwr_context *ctx, uint32_t trace[4], uint32_t shadow[4])
{
    if (!ctx || !trace || !shadow) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    const LanePlanRecord *from[2] = {&ctx->last_trace_plan, &ctx->last_shadow_plan};
    uint32_t *to[2] = {trace, shadow};
    for (int k = 0; k < 2; k++) {
        to[k][0] = from[k]->launches; to[k][1] = from[k]->nodes_in_lds; to[k][2] = from[k]->stack16; to[k][3] = from[k]->wide;
    }
    return RWR_OK;
}

int rwr_measure_valu_clock(rwr_context *ctx, uint32_t waves_per_simd, double out4[4])
{
    if (!ctx || !out4) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (waves_per_simd < 1u || waves_per_simd > 8u) return set_error(RWR_ERR_INVALID_ARGUMENT, "waves_per_simd must be 1..8");
    DeviceGuard g(ctx->device);
    hipDeviceProp_t prop;
    RWR_HIP_CHECK(hipGetDeviceProperties(&prop, ctx->device));
    const uint32_t n_wg = (uint32_t)prop.multiProcessorCount * waves_per_simd, n_waves = n_wg * 4u, iters = 1u << 15;
    DeviceBuffer<ulonglong2> d_out;
    OwnedEvent e0, e1;
    RWR_HIP_CHECK(d_out.ensure(n_waves));
    RWR_HIP_CHECK(hipEventCreate(&e0.h));
    RWR_HIP_CHECK(hipEventCreate(&e1.h));
    std::vector<ulonglong2> h(n_waves);
    RWR_HIP_CHECK(sync_all(ctx));
    for (int mode = 0; mode < 2; mode++) {
        // an untimed launch first: the stamped one then starts on a busy, clocked-up chip
        RWR_HIP_CHECK(launch_measure_valu(ctx->stream, mode, d_out.ptr, n_wg, iters));
        RWR_HIP_CHECK(hipEventRecord(e0, ctx->stream));
        RWR_HIP_CHECK(launch_measure_valu(ctx->stream, mode, d_out.ptr, n_wg, iters));
        RWR_HIP_CHECK(hipEventRecord(e1, ctx->stream));
        RWR_HIP_CHECK(hipMemcpyAsync(h.data(), d_out.ptr, n_waves * sizeof(ulonglong2), hipMemcpyDeviceToHost, ctx->stream));
        RWR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        float ms = 0.0f;
        RWR_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        std::vector<double> mhz(n_waves);
        for (uint32_t i = 0; i < n_waves; i++) mhz[i] = h[i].y ? (double)h[i].x / (double)h[i].y * 100.0 : 0.0;
        std::nth_element(mhz.begin(), mhz.begin() + n_waves / 2, mhz.end());
        const double clock_mhz = mhz[n_waves / 2];
        // every SIMD issued (waves on it) * iters * 8 wave instructions during the launch (HIP events around it);
        // cycles = elapsed time x the in-kernel clock
        const double instr_per_simd = (double)n_waves / (4.0 * prop.multiProcessorCount) * iters * 8.0;
        const double per_instr = (double)ms * 1e-3 * clock_mhz * 1e6 / instr_per_simd;
        if (mode == 0) { out4[0] = clock_mhz; out4[1] = per_instr; }
        else { out4[2] = per_instr; out4[3] = clock_mhz; }
    }
    return RWR_OK;
}

int rwr_clock_probe_start(rwr_context *ctx, uint32_t micros)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (micros == 0u || micros > 100000u) return set_error(RWR_ERR_INVALID_ARGUMENT, "probe duration must be 1..100000 us");
    DeviceGuard g(ctx->device);
    if (!ctx->probe_stream) RWR_HIP_CHECK(hipStreamCreateWithFlags(&ctx->probe_stream.h, hipStreamNonBlocking));
    RWR_HIP_CHECK(ctx->d_probe.ensure(1));
    RWR_HIP_CHECK(hipStreamSynchronize(ctx->probe_stream));
    RWR_HIP_CHECK(launch_clock_probe(ctx->probe_stream, ctx->d_probe.ptr, micros * 100u));
    return RWR_OK;
}

int rwr_clock_probe_read(rwr_context *ctx, double *shader_mhz)
{
    if (!ctx || !shader_mhz) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!ctx->probe_stream) return set_error(RWR_ERR_NOT_READY, "rwr_clock_probe_start has not been called");
    DeviceGuard g(ctx->device);
    ulonglong2 h{0, 0};
    RWR_HIP_CHECK(hipMemcpyAsync(&h, ctx->d_probe.ptr, sizeof h, hipMemcpyDeviceToHost, ctx->probe_stream));
    RWR_HIP_CHECK(hipStreamSynchronize(ctx->probe_stream));
    *shader_mhz = h.y ? (double)h.x / (double)h.y * 100.0 : 0.0;
    return RWR_OK;
}

}  // extern "C"
