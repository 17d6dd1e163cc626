// One frame behind the C ABI: the request, its slot, the kernel that renders it, and what the context remembers of it.
#include <algorithm>

#include "rwr_frame.h"

using namespace rwr;

namespace {

// rows a launch renders: its strips' rows inside [row_begin, row_end) — band_strips with the last strip clipped
uint64_t band_rows(const FrameParams &fp)
{
    const uint32_t strips = band_strips(fp);
    if (strips == 0u) return 0u;
    const uint32_t last = fp.row_begin + (strips - 1u) * fp.row_pitch;
    return (uint64_t)(strips - 1u) * kStripRows + std::min(kStripRows, fp.row_end - last);
}

// One frame — rows [row_begin, row_end) in strips of 8 rows, strip k starting at row_begin + k * row_pitch (row_pitch 8: the
// whole band; 8 N: every N-th strip).
int render_frame(rwr_context *ctx, const rwr_camera_inv_uniform *camera, const rwr_render_params *params,
                 uint32_t row_begin, uint32_t row_end, uint32_t row_pitch)
{
    FrameRequest rq;
    int rc = validate(ctx, camera, params, row_begin, row_end, row_pitch, rq);
    if (rc != RWR_OK) return rc;
    AccumPlan ap;
    if ((rc = plan_accumulation(ctx, *camera, rq, ap)) != RWR_OK) return rc;
    ReprojectPlan pp;
    plan_reprojection(ctx, rq, pp);

    DeviceGuard g(ctx->device);
    if ((rc = rebuild_tris(ctx)) != RWR_OK) return rc;
    // Frame slot: the next one in turn.  A slot owns everything a frame writes — targets, per-frame records, and for the
    // wavefront integrator a whole set of accumulators and ray queues (WfState) — so frames in different slots share
    // nothing and a slot is reused in stream order.
    ctx->cur = (ctx->cur + 1u) % ctx->n_slots;
    FrameSlot &sl = ctx->slots[ctx->cur];
    if (rq.aux) {
        // a band render leaves the rest of the planes untouched: they start zeroed, like the targets
        const size_t n = (size_t)ctx->screen.width * ctx->screen.height;
        const bool fresh = sl.d_color_f32.count < n * 4 || sl.d_obj_id.count < n || sl.d_hit_t.count < n;
        RWR_HIP_CHECK(sl.d_color_f32.ensure(n * 4));
        RWR_HIP_CHECK(sl.d_obj_id.ensure(n));
        RWR_HIP_CHECK(sl.d_hit_t.ensure(n));
        if (fresh) {
            RWR_HIP_CHECK(hipMemsetAsync(sl.d_color_f32.ptr, 0, n * 4 * sizeof(float), sl.stream));
            RWR_HIP_CHECK(hipMemsetAsync(sl.d_obj_id.ptr, 0, n * sizeof(int32_t), sl.stream));
            RWR_HIP_CHECK(hipMemsetAsync(sl.d_hit_t.ptr, 0, n * sizeof(float), sl.stream));
        }
    }
    RWR_HIP_CHECK(sl.d_ftris.ensure(ctx->n_tris));
    RWR_HIP_CHECK(sl.d_tnum.ensure(ctx->n_tris));
    const Targets tg{sl.d_color.ptr, sl.d_depth.ptr, rq.aux ? sl.d_color_f32.ptr : nullptr,
                     rq.aux ? sl.d_obj_id.ptr : nullptr, rq.aux ? sl.d_hit_t.ptr : nullptr};

    const FrameScene scene{ctx->screen.width, ctx->screen.height, ctx->spheres, ctx->n_spheres, ctx->n_tris, ctx->tex_w, ctx->tex_h,
                           ctx->aabb_lo, ctx->aabb_hi, &ctx->material, ctx->d_materials.ptr, (uint32_t)ctx->st_materials.size(),
                           ctx->d_tangent.ptr, ctx->wave_cull_min};
    FrameConsts fc{};
    fill_frame_consts(scene, *camera, rq.rp, rq.accumulate, row_begin, row_end, row_pitch, fc);
    const FrameKernel kernel = choose_kernel(ctx, rq, fc);

    FrameTiming timing;
    ctx->last_classes = rwr_context::LastClasses{};   // (enqueue_reference: a frame whose setup makes class words)
    ctx->last_cover_frames = 0;
    rc = kernel == FrameKernel::kWavefront ? enqueue_wavefront(ctx, sl, rq, ap, pp, fc, tg, timing)
                                           : enqueue_reference(ctx, sl, rq, kernel, fc, tg, timing);
    if (rc != RWR_OK) return rc;

    // the frame is on its stream: what the context remembers of it
    if (timing.on) {
        if (!timing.dispatch) RWR_HIP_CHECK(hipEventRecord(ctx->timing_events[2 * ctx->timing_pairs + 1], sl.stream));
        ctx->timing_pairs++;
    }
    sl.aux_valid = rq.aux;
    ctx->last_spp = rq.wavefront ? rq.rp.spp : 0u;
    ctx->last_had_bounce = rq.wavefront && rq.rp.max_bounces != 0;
    ctx->last_primary = (uint64_t)ctx->screen.width * band_rows(fc.fp) * ap.trace_spp;
    ctx->last_shadows = rq.shadows;
    ctx->last_glass = rq.wavefront && rq.glass && ap.trace_spp != 0u;
    ctx->last_gloss = rq.wavefront && rq.gloss && ap.trace_spp != 0u;
    ctx->last_glow = rq.wavefront && rq.glow && ap.trace_spp != 0u;
    ctx->last_light = rq.wavefront && (rq.light || rq.light_parts || rq.light_sky) && ap.trace_spp != 0u;
    ctx->last_tonemap = rq.tonemap;
    if (rq.tonemap) ctx->last_tonemap_params = ctx->tonemap;
    ctx->last_bounce = 0;  // filled in lazily by rwr_last_render_stats from the pass counters
    return RWR_OK;
}

}  // namespace

extern "C" {

int rwr_render(rwr_context *ctx, const rwr_camera_inv_uniform *camera, const rwr_render_params *params)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    return render_frame(ctx, camera, params, 0, ctx->screen.height, kStripRows);
}

int rwr_render_rows(rwr_context *ctx, const rwr_camera_inv_uniform *camera, const rwr_render_params *params,
                    uint32_t row_begin, uint32_t row_end)
{
    return render_frame(ctx, camera, params, row_begin, row_end, kStripRows);
}

int rwr_render_strips(rwr_context *ctx, const rwr_camera_inv_uniform *camera, const rwr_render_params *params,
                      uint32_t first_strip, uint32_t strip_stride)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (strip_stride == 0u || first_strip >= strip_stride || strip_stride > 0x0fffffffu)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "strips %u, %u + %u, ...: the first strip must be below the stride", first_strip, first_strip, strip_stride);
    const uint32_t h = ctx->screen.height, first_row = first_strip * kStripRows;
    return render_frame(ctx, camera, params, std::min(first_row, h), h, strip_stride * kStripRows);
}

}  // extern "C"
