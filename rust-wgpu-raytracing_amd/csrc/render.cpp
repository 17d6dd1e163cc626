// One frame behind the C ABI: what was asked, which kernel renders it, and the commands it puts on the slot's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "rwr_context.h"

using namespace rwr;

namespace {

// A render call, validated.
struct FrameRequest {
    rwr_render_params rp;
    uint32_t row_begin, row_end, row_pitch;
    bool aux, accumulate, shadows;
    bool denoise;     // RWR_FLAG_DENOISE: the filter runs behind the resolve (rp.flags holds the effective flags: AUX implied, this bit cleared)
    bool reproject;   // RWR_FLAG_REPROJECT: the reprojection stage runs behind the resolve, ahead of the filter (AUX implied, this bit cleared)
    bool mirrors;     // RWR_FLAG_MIRRORS with at least one bounce and one mirror surface: the MIRROR forms (else the bit is cleared from rp.flags)
    bool glass;       // RWR_FLAG_GLASS with at least one bounce and one glass surface: the glass forms (else the bit is cleared from rp.flags)
    bool gloss;       // RWR_FLAG_GLOSSY with at least one bounce and one glossy surface: the glossy forms (else the bit is cleared from rp.flags)
    bool sky;         // RWR_FLAG_SKY with at least one bounce: the trace kernels' SKY forms (without a bounce the bit is cleared from rp.flags)
    bool wavefront;   // the wavefront integrator renders it (several samples, a bounce, or an accumulation)
    bool dormant;     // the reference's dormant parts (single-triangle passes, orthographic rays) have their own plain kernel
};

// Progressive accumulation: what this frame does with the context's history.
struct AccumPlan {
    std::vector<unsigned char> key;
    AccumMode mode = AccumMode::kFirst;
    uint64_t before = 0;      // samples the history holds before this frame
    uint32_t trace_spp = 0;   // samples this frame traces
};

// Temporal reprojection: what this frame does with the context's history.
struct ReprojectPlan {
    std::vector<unsigned char> key;
    uint64_t k = 0;           // the frame's number in the history: 0 starts a new one
};

// The kernel that renders a frame.  Decided once (choose_kernel); every other question about the frame's form is asked of it.
enum class FrameKernel { kDormant, kBvh, kOnePixel, kTwoPixel, kWavefront };

// The frame's timing pair (rwr_ctx_set_kernel_timing): the two-pixel frame kernel is timed by its own dispatch timestamps,
// everything else by stream events around it.
struct FrameTiming {
    bool on = false, dispatch = false;
};

int validate(rwr_context *ctx, const rwr_camera_inv_uniform *camera, const rwr_render_params *params, uint32_t row_begin,
             uint32_t row_end, uint32_t row_pitch, FrameRequest &rq)
{
    if (!ctx || !camera) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    if (ctx->screen.width == 0) return set_error(RWR_ERR_NOT_READY, "rwr_resize has not been called");
    if (!ctx->have_mesh) return set_error(RWR_ERR_NOT_READY, "rwr_scene_upload_mesh has not been called");
    if (row_begin > row_end || row_end > ctx->screen.height)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "row band [%u,%u) outside the %u-row frame", row_begin, row_end,
                         ctx->screen.height);
    rwr_render_params rp = {1, 0, 0, 0};
    if (params) rp = *params;
    if (rp.spp == 0) return set_error(RWR_ERR_INVALID_ARGUMENT, "spp must be >= 1");
    if ((rp.flags & RWR_FLAG_MULTI_BOUNCE) && rp.max_bounces > RWR_MAX_BOUNCES)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "max_bounces %u is more than RWR_MAX_BOUNCES (%u)", rp.max_bounces, RWR_MAX_BOUNCES);
    if (rp.max_bounces > 1 && !(rp.flags & RWR_FLAG_MULTI_BOUNCE))
        return set_error(RWR_ERR_UNSUPPORTED, "max_bounces > 1 is not supported without RWR_FLAG_MULTI_BOUNCE");
    if ((rp.flags & RWR_FLAG_USE_BVH) && (rp.spp != 1 || rp.max_bounces != 0))
        return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_USE_BVH applies to the reference frame (spp 1, no bounce); bounce rays always use the BVH");
    if (rp.spp > 4096) return set_error(RWR_ERR_INVALID_ARGUMENT, "spp must be <= 4096");
    const bool accumulate = (rp.flags & RWR_FLAG_ACCUMULATE) != 0;
    if (accumulate && ((rp.flags & (RWR_FLAG_ORTHO_RAYS | RWR_FLAG_USE_BVH)) || ctx->n_triangles != 0))
        return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_ACCUMULATE: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only");
    const bool shadows = (rp.flags & RWR_FLAG_SHADOWS) != 0;
    if (shadows && ((rp.flags & (RWR_FLAG_ORTHO_RAYS | RWR_FLAG_USE_BVH)) || ctx->n_triangles != 0))
        return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_SHADOWS: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only");
    // the filter works on the whole frame's planes: the colour and the id / t planes it is guided by (so RWR_FLAG_AUX_OUTPUTS is
    // implied).  From here on rp.flags is what the frame is rendered with; the filter's own bit is not part of it (nor of the
    // accumulation's key).
    const bool denoise = (rp.flags & RWR_FLAG_DENOISE) != 0;
    if (denoise) {
        if ((rp.flags & (RWR_FLAG_ORTHO_RAYS | RWR_FLAG_USE_BVH)) || ctx->n_triangles != 0)
            return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_DENOISE: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only");
        if (row_begin != 0u || row_end != ctx->screen.height || row_pitch != kStripRows)
            return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_DENOISE: the filter needs the whole frame (its taps reach 62 pixels); rows [%u,%u) "
                             "every %u-th strip is a part of it", row_begin, row_end, row_pitch / kStripRows);
        rp.flags = (rp.flags & ~(uint32_t)RWR_FLAG_DENOISE) | RWR_FLAG_AUX_OUTPUTS;
    }
    // the reprojection stage gathers from the whole previous frame and blends over the whole of this one, behind the integrator's
    // resolve: the filter's rules (rwr_hip.h, RWR_FLAG_REPROJECT item 7).  Its bit is not part of the flags the frame is traced with.
    const bool reproject = (rp.flags & RWR_FLAG_REPROJECT) != 0;
    if (reproject) {
        if (accumulate) return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_REPROJECT with RWR_FLAG_ACCUMULATE: a context blends one history, not two");
        if ((rp.flags & (RWR_FLAG_ORTHO_RAYS | RWR_FLAG_USE_BVH)) || ctx->n_triangles != 0)
            return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_REPROJECT: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only");
        if (row_begin != 0u || row_end != ctx->screen.height || row_pitch != kStripRows)
            return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_REPROJECT: the stage needs the whole frame (its taps land anywhere in the previous one); rows [%u,%u) "
                             "every %u-th strip is a part of it", row_begin, row_end, row_pitch / kStripRows);
        rp.flags = (rp.flags & ~(uint32_t)RWR_FLAG_REPROJECT) | RWR_FLAG_AUX_OUTPUTS;
    }
    // the refusal first: it holds whatever max_bounces is (rwr_hip.h, RWR_FLAG_SKY item 7)
    if ((rp.flags & RWR_FLAG_SKY) && ((rp.flags & (RWR_FLAG_ORTHO_RAYS | RWR_FLAG_USE_BVH)) || ctx->n_triangles != 0))
        return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_SKY: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only");
    // the sky lights bounce rays alone: a frame without a bounce is the frame without the flag
    if (rp.max_bounces == 0u) rp.flags &= ~(uint32_t)RWR_FLAG_SKY;
    const bool sky = (rp.flags & RWR_FLAG_SKY) != 0;
    // mirror surfaces: the refusal first, as the sky's (rwr_hip.h, RWR_FLAG_MIRRORS item 8); then a frame whose paths end at h0, or
    // whose scene has no mirror, is the frame without the flag, in the same kernels (item 6)
    if ((rp.flags & RWR_FLAG_MIRRORS) && ((rp.flags & (RWR_FLAG_ORTHO_RAYS | RWR_FLAG_USE_BVH)) || ctx->n_triangles != 0))
        return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_MIRRORS: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only");
    if (rp.flags & RWR_FLAG_MIRRORS) {
        bool any = false;
        for (const MirrorRec &m : ctx->part_mirrors) any = any || m.on == 1.0f;
        for (uint32_t i = 0; i < ctx->n_spheres; i++) any = any || ctx->sphere_mirrors[i].on == 1.0f;
        if (rp.max_bounces == 0u || !any) rp.flags &= ~(uint32_t)RWR_FLAG_MIRRORS;
    }
    const bool mirrors = (rp.flags & RWR_FLAG_MIRRORS) != 0;
    // glass surfaces: the same two rules (rwr_hip.h, RWR_FLAG_GLASS items 10 and 8); a glass record is one with on < 0
    if ((rp.flags & RWR_FLAG_GLASS) && ((rp.flags & (RWR_FLAG_ORTHO_RAYS | RWR_FLAG_USE_BVH)) || ctx->n_triangles != 0))
        return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_GLASS: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only");
    if (rp.flags & RWR_FLAG_GLASS) {
        bool any = false;
        for (const MirrorRec &m : ctx->part_mirrors) any = any || m.on < 0.0f;
        for (uint32_t i = 0; i < ctx->n_spheres; i++) any = any || ctx->sphere_mirrors[i].on < 0.0f;
        if (rp.max_bounces == 0u || !any) rp.flags &= ~(uint32_t)RWR_FLAG_GLASS;
    }
    const bool glass = (rp.flags & RWR_FLAG_GLASS) != 0;
    // glossy surfaces: the same two rules (rwr_hip.h, RWR_FLAG_GLOSSY items 8 and 7); a glossy record is one with on > 1
    if ((rp.flags & RWR_FLAG_GLOSSY) && ((rp.flags & (RWR_FLAG_ORTHO_RAYS | RWR_FLAG_USE_BVH)) || ctx->n_triangles != 0))
        return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_GLOSSY: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only");
    if (rp.flags & RWR_FLAG_GLOSSY) {
        bool any = false;
        for (const MirrorRec &m : ctx->part_mirrors) any = any || m.on > 1.0f;
        for (uint32_t i = 0; i < ctx->n_spheres; i++) any = any || ctx->sphere_mirrors[i].on > 1.0f;
        if (rp.max_bounces == 0u || !any) rp.flags &= ~(uint32_t)RWR_FLAG_GLOSSY;
    }
    const bool gloss = (rp.flags & RWR_FLAG_GLOSSY) != 0;
    // an accumulating frame always takes the wavefront integrator (its samples are jittered even at spp 1), and so does a frame
    // with shadow rays (the integrator's stages trace them) or one the filter follows (it runs behind the integrator's resolve)
    const bool wavefront = rp.spp != 1 || rp.max_bounces != 0 || accumulate || shadows || denoise || reproject;
    const bool dormant = ctx->n_triangles != 0 || (rp.flags & RWR_FLAG_ORTHO_RAYS) != 0;
    if (dormant && (wavefront || (rp.flags & RWR_FLAG_USE_BVH)))
        return set_error(RWR_ERR_UNSUPPORTED, "single-triangle passes and RWR_FLAG_ORTHO_RAYS apply to the reference frame (spp 1, no bounce, no RWR_FLAG_USE_BVH)");
    rq = FrameRequest{rp, row_begin, row_end, row_pitch, (rp.flags & RWR_FLAG_AUX_OUTPUTS) != 0, accumulate, shadows, denoise, reproject, mirrors, glass, gloss, sky, wavefront, dormant};
    return RWR_OK;
}

// What an accumulating frame must share with the frame before for the accumulation to go on (rwr_hip.h RWR_FLAG_ACCUMULATE): the
// camera uniform's bytes, the screen, the rows, bounces, seed, flags but the ACCUMULATE bit, frames in flight and the scene — and, while
// the frame is lit by the sky (RWR_FLAG_SKY), the sky's parameters.  (Mirror surfaces, RWR_FLAG_MIRRORS: the flag is one of the
// flags, and every call of their setters changes the scene's generation; glass surfaces, RWR_FLAG_GLASS, and glossy ones, RWR_FLAG_GLOSSY, likewise.)
std::vector<unsigned char> accum_key_of(const rwr_context *ctx, const rwr_camera_inv_uniform &cam, const FrameRequest &rq)
{
    const uint32_t words[9] = {ctx->screen.width, ctx->screen.height, rq.row_begin, rq.row_end, rq.row_pitch, rq.rp.max_bounces, rq.rp.seed,
                               rq.rp.flags & ~(uint32_t)RWR_FLAG_ACCUMULATE, ctx->n_slots};
    std::vector<unsigned char> key(sizeof cam + sizeof words + sizeof ctx->scene_generation + (rq.sky ? sizeof ctx->sky : 0u));
    std::memcpy(key.data(), &cam, sizeof cam);
    std::memcpy(key.data() + sizeof cam, words, sizeof words);
    std::memcpy(key.data() + sizeof cam + sizeof words, &ctx->scene_generation, sizeof ctx->scene_generation);
    if (rq.sky) std::memcpy(key.data() + sizeof cam + sizeof words + sizeof ctx->scene_generation, &ctx->sky, sizeof ctx->sky);
    return key;
}

// Progressive accumulation: does this frame go on with the context's accumulation (same key, room below the cap), start a
// new one, or only show it (past the cap)?  A frame without the flag ends it.  Committed once the frame is enqueued.
int plan_accumulation(rwr_context *ctx, const rwr_camera_inv_uniform &cam, const FrameRequest &rq, AccumPlan &ap)
{
    if (rq.accumulate) {
        ap.key = accum_key_of(ctx, cam, rq);
        if (ap.key == ctx->accum.key && ctx->accum.samples != 0) {
            ap.before = ctx->accum.samples;
            ap.mode = ap.before + rq.rp.spp > ctx->accum_max ? AccumMode::kShow : AccumMode::kAdd;
        } else if (rq.rp.spp > ctx->accum_max) {
            return set_error(RWR_ERR_INVALID_ARGUMENT, "spp %u is more than the %llu samples an accumulation may hold (RWR_ACCUM_MAX_SAMPLES)",
                             rq.rp.spp, (unsigned long long)ctx->accum_max);
        }
    } else {
        ctx->accum.key.clear();
        ctx->accum.samples = 0;
        ctx->last_accum_samples = 0;
    }
    ap.trace_spp = ap.mode == AccumMode::kShow ? 0u : rq.rp.spp;
    return RWR_OK;
}

// What a reprojecting frame must share with the one before for the history to go on (rwr_hip.h RWR_FLAG_REPROJECT item 2): the
// screen, spp, bounces, seed, the effective flags (the DENOISE and REPROJECT bits are not among them), frames in flight, the scene,
// the stage's parameters and, while the sky lights the frame, the sky's.  NOT the camera.
std::vector<unsigned char> reproject_key_of(const rwr_context *ctx, const FrameRequest &rq)
{
    const uint32_t words[7] = {ctx->screen.width, ctx->screen.height, rq.rp.spp, rq.rp.max_bounces, rq.rp.seed, rq.rp.flags, ctx->n_slots};
    std::vector<unsigned char> key(sizeof words + sizeof ctx->scene_generation + sizeof ctx->reproject + (rq.sky ? sizeof ctx->sky : 0u));
    unsigned char *at = key.data();
    std::memcpy(at, words, sizeof words); at += sizeof words;
    std::memcpy(at, &ctx->scene_generation, sizeof ctx->scene_generation); at += sizeof ctx->scene_generation;
    std::memcpy(at, &ctx->reproject, sizeof ctx->reproject); at += sizeof ctx->reproject;
    if (rq.sky) std::memcpy(at, &ctx->sky, sizeof ctx->sky);
    return key;
}

// Temporal reprojection: does this frame go on with the context's history or start a new one?  A frame without the flag ends it.
// Frame k is traced with seed + k (mod 2^32).  Committed once the stage is enqueued.
void plan_reprojection(rwr_context *ctx, FrameRequest &rq, ReprojectPlan &pp)
{
    if (rq.reproject) {
        pp.key = reproject_key_of(ctx, rq);
        if (pp.key == ctx->reproj.key && ctx->reproj.frames != 0) pp.k = ctx->reproj.frames;
        rq.rp.seed += (uint32_t)pp.k;
    } else {
        ctx->reproj.key.clear();
        ctx->reproj.frames = 0;
        ctx->last_reproject_frames = 0;
    }
}

// What the history keeps of a frame's camera (rwr_hip.h RWR_FLAG_REPROJECT item 3), in the oracle's f32 operations (this unit is
// built without contraction): W(x_nds, y_nds) is pixelToRay's world_vec before the normalise, compute.wgsl:151-159.
RpCamera reproject_camera(const rwr_camera_inv_uniform &cam)
{
    auto mul = [](const float (&m)[4][4], const float (&v)[4], float (&r)[4]) {
        for (int i = 0; i < 4; i++) r[i] = m[0][i] * v[0] + m[1][i] * v[1] + m[2][i] * v[2] + m[3][i] * v[3];
    };
    auto world_vec = [&](float x_nds, float y_nds, float (&w)[4]) {
        const float proj_vec[4] = {x_nds, y_nds, 1.0f, 1.0f};
        float view_vec[4];
        mul(cam.proj_inv, proj_vec, view_vec);
        view_vec[3] = 0.0f;
        mul(cam.viewmodel_inv, view_vec, w);
    };
    float c0[4], wx[4], wy[4];
    world_vec(0.0f, 0.0f, c0);
    world_vec(1.0f, 0.0f, wx);
    world_vec(0.0f, 1.0f, wy);
    RpCamera rc{};
    for (int i = 0; i < 3; i++) {
        rc.o[i] = cam.origin[i];
        rc.c0[i] = c0[i];
        rc.cx[i] = wx[i] - c0[i];
        rc.cy[i] = wy[i] - c0[i];
    }
    rc.nrm[0] = rc.cx[1] * rc.cy[2] - rc.cx[2] * rc.cy[1];
    rc.nrm[1] = rc.cx[2] * rc.cy[0] - rc.cx[0] * rc.cy[2];
    rc.nrm[2] = rc.cx[0] * rc.cy[1] - rc.cx[1] * rc.cy[0];
    rc.nc0 = rc.nrm[0] * rc.c0[0] + rc.nrm[1] * rc.c0[1] + rc.nrm[2] * rc.c0[2];
    rc.nn = rc.nrm[0] * rc.nrm[0] + rc.nrm[1] * rc.nrm[1] + rc.nrm[2] * rc.nrm[2];
    return rc;
}

FrameKernel choose_kernel(const rwr_context *ctx, const FrameRequest &rq, const FrameConsts &fc)
{
    if (rq.dormant) return FrameKernel::kDormant;
    if (rq.wavefront) return FrameKernel::kWavefront;
    const bool one_pixel = (rq.rp.flags & RWR_FLAG_ONE_PIXEL_PER_LANE) || ctx->force_one_pixel;
    // faces much smaller than a tile: the per-ray BVH kernel is the faster way to the same frame (frame_consts.cpp mean_face_pixels)
    const bool auto_bvh = !(rq.rp.flags & RWR_FLAG_NO_CULL) && !one_pixel && ctx->n_tris > ctx->bin_min_faces &&
                          ctx->auto_bvh_face_px > 0.0f && fc.mean_face_px < (double)ctx->auto_bvh_face_px;
    if ((rq.rp.flags & RWR_FLAG_USE_BVH) || auto_bvh) return FrameKernel::kBvh;
    return one_pixel ? FrameKernel::kOnePixel : FrameKernel::kTwoPixel;
}

// The plain reference frame of a small scene: the two-pixel kernel, all faces in one 256-wide batch (no bins), culled.  What its
// special forms — per-tile face sets, the fused launch, the graph — have in common; each adds its own terms.
bool small_culled_frame(const rwr_context *ctx, const FrameRequest &rq, FrameKernel kernel)
{
    return kernel == FrameKernel::kTwoPixel && ctx->n_tris != 0 && ctx->n_tris <= ctx->bin_min_faces && !(rq.rp.flags & RWR_FLAG_NO_CULL);
}

// rows a launch renders: its strips' rows inside [row_begin, row_end) — band_strips with the last strip clipped
uint64_t band_rows(const FrameParams &fp)
{
    const uint32_t strips = band_strips(fp);
    if (strips == 0u) return 0u;
    const uint32_t last = fp.row_begin + (strips - 1u) * fp.row_pitch;
    return (uint64_t)(strips - 1u) * kStripRows + std::min(kStripRows, fp.row_end - last);
}

const float4 *tex0_of(const rwr_context *ctx) { return ctx->d_texs.empty() ? nullptr : ctx->d_texs[0].ptr; }

// Per-frame records and tables (k_frame_setup): they depend on the camera, the screen, the launch's rows and the scene, and
// on nothing else — not on the frame's number — so a slot keeps them while those stand still (launch_records below) and
// makes them again, on the render stream just ahead of the render kernel, when one of them changes.  (Running this small
// kernel on a side stream, double-buffered so that it overlaps the previous frame, was
// measured 4-10 us SLOWER per frame than the 3 us it hides: cross-stream event waits cost
// more than the kernel.)  Here: where they go.
int frame_tables(rwr_context *ctx, FrameSlot &sl, FrameParams &fp, FrameSetupOut &so)
{
    so.ray_pairs = ((ctx->screen.width + 63u) / 64u) * 32u;  // whole 64-pixel workgroup columns
    so.ray_rows = ctx->screen.height + 8u;                   // whole 8-row tiles below any band
    RWR_HIP_CHECK(sl.d_ray_colp.ensure(2u * (size_t)so.ray_pairs));
    RWR_HIP_CHECK(sl.d_ray_row.ensure(so.ray_rows));
    so.ftris = sl.d_ftris.ptr; so.tnum = sl.d_tnum.ptr;
    so.ray_colp = sl.d_ray_colp.ptr; so.ray_row = sl.d_ray_row.ptr;
    fp.ray_colp = so.ray_colp; fp.ray_row = so.ray_row; fp.tnum = so.tnum;
    return RWR_OK;
}

// Everything k_frame_setup reads, and everything that decides where and what it writes: two launches with equal keys write the
// same bytes to the same addresses.  Field by field (no padding bytes); the buffers' addresses are part of it, so a buffer that
// moved between two frames is a different key.
struct RecordsKey {
    rwr_camera_inv_uniform cam;
    CullConsts cc;
    uint64_t scene_generation;
    const void *cull, *tris, *ftris, *tnum, *ray_colp, *ray_row, *zero_a, *zero_b, *tile_lists;
    uint32_t width, height, n_tris, ray_pairs, ray_rows, n_zero_a, n_zero_b, list_gx, list_gy, list_row_begin, list_row_pitch, list_blocks;
    uint32_t row_begin, row_end, row_pitch, pad;   // the launch's rows, with or without face sets: a change of rows is a change of key
    TileClassIn tc;   // the tiles' class words: where they go, and the mesh rectangle, sphere count and sphere rectangles they record
};
static_assert(sizeof(RecordsKey) == sizeof(rwr_camera_inv_uniform) + sizeof(CullConsts) + 8 + 9 * sizeof(void *) + 16 * 4 + sizeof(TileClassIn),
              "RecordsKey has no padding");
static_assert(sizeof(FrameSetupOut) == 96, "a new member of FrameSetupOut belongs in RecordsKey");
static_assert(sizeof(TileClassIn) == 168, "a new member of TileClassIn is a new input of k_frame_setup: RecordsKey holds the whole struct");

// The class words' inputs for a launch whose sets go to so.tile_lists (rwr_internal.h: the words lie behind the sets); all zero
// for a launch without sets.
TileClassIn tile_class_in(const FrameParams &fp, const FrameSetupOut &so)
{
    TileClassIn tc{};
    if (!so.tile_lists) return tc;
    tc.classes = so.tile_lists + (size_t)so.list_gx * so.list_gy * 4u * kTileListWords;
    tc.cover = tc.classes + (size_t)so.list_gx * so.list_gy * 4u;
    for (int k = 0; k < 4; k++) tc.mesh_px[k] = fp.mesh_px[k];
    tc.n_spheres = fp.n_spheres;
    std::memcpy(tc.sphere_rect, fp.sphere_rect, sizeof tc.sphere_rect);
    return tc;
}

// Every k_frame_setup goes through here.  The slot's records are a pure function of the launch's key, so a launch whose key is
// the one the slot's records were made from is not made: camera, screen, rows and scene stand still on most frames of a redraw
// loop (and on all of a progressive accumulation).  Not pure are the words the wavefront integrator wants zeroed (zero_a /
// zero_b: its kernels count in them, every frame from zero), so a launch that carries such words is always made; the records
// it leaves are those of its key all the same.  `captured`: the launch is being recorded into a graph whose replays rewrite the
// records whenever they run — made, not counted (launch_frame_graph counts replays), and it leaves no key.
// This is the only place that leaves a key behind; whatever else writes the slot's records clears it (launch_frame_graph,
// launch_fused_frame, and ensure_frame_buffers when a buffer moves outside a frame).
// *kept (may be null): the launch was not made, the slot's records — and the tiles' class and cover words among them — are the
// ones an earlier launch with this key left.
hipError_t launch_records(rwr_context *ctx, FrameSlot &sl, const FrameConsts &fc, const FrameSetupOut &so, bool captured = false, bool *kept = nullptr)
{
    if (kept) *kept = false;
    const FrameParams &fp = fc.fp;
    const RecordsKey key{fp.cam, fc.cc, ctx->scene_generation, ctx->d_cull.ptr, ctx->d_tris.ptr, so.ftris, so.tnum, so.ray_colp, so.ray_row,
                         so.zero_a, so.zero_b, so.tile_lists, fp.width, fp.height, ctx->n_tris, so.ray_pairs, so.ray_rows, so.n_zero_a,
                         so.n_zero_b, so.list_gx, so.list_gy, so.list_row_begin, so.list_row_pitch, so.list_blocks,
                         fp.row_begin, fp.row_end, fp.row_pitch, 0u, tile_class_in(fp, so)};
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(&key);
    const bool pure = so.n_zero_a == 0u && so.n_zero_b == 0u;
    if (!captured && pure && sl.records_key.size() == sizeof key && std::memcmp(sl.records_key.data(), bytes, sizeof key) == 0) {
        if (kept) *kept = true;
        return hipSuccess;
    }
    sl.records_key.clear();
    sl.cover_frames = 0;   // (the launch zeroes the cover words it reaches: what the frames since the last one learnt is forgotten)
    const hipError_t e = launch_frame_setup(sl.stream, fc.cc, fp.cam, fp.width, fp.height, ctx->d_cull.ptr, ctx->d_tris.ptr, ctx->n_tris, so, key.tc);
    if (e != hipSuccess || captured) return e;
    ctx->setup_launches++;
    if (ctx->setup_cache) sl.records_key.assign(bytes, bytes + sizeof key);   // (RWR_SETUP_CACHE=0: never a key, never a hit)
    return hipSuccess;
}

// What a slot's plane of ray directions (rwr_internal.h RayPlane) is a function of, and where it lies: the camera uniform, the
// screen, the launch's rows (they place the grid's workgroups) and the addresses of the two ray tables it is made from and of
// the plane itself.  No scene generation and no culling constants: the directions survive other spheres, instances or meshes.
// Field by field (no padding bytes).
struct RayPlaneKey {
    rwr_camera_inv_uniform cam;
    const void *ray_colp, *ray_row, *plane;
    uint32_t width, height, row_begin, row_end, row_pitch, pad;
};
static_assert(sizeof(RayPlaneKey) == sizeof(rwr_camera_inv_uniform) + 3 * sizeof(void *) + 6 * 4, "RayPlaneKey has no padding");

// The two-pixel frame kernel's rays for a camera at rest.  A fifth of the kernel's instructions turn the ray tables into the
// normalised directions of its pixel pairs, the same ones every frame while camera, screen and rows stand still — in a redraw
// loop that is most frames, the camera moves only while a key is held.  Per slot, for a frame with key K behind launch_records
// on the slot's stream:
//   the slot's plane was built for K:        the frame kernel loads its directions from it            (returns true)
//   else the slot's frame before had key K:  k_ray_plane fills the plane once, then the same          (returns true)
//   else:                                    K is remembered and the frame computes its rays, as ever (returns false)
// so a moving camera never pays for a plane it would not use, and a camera that comes to rest computes one more frame per
// slot, builds on the next and loads from then on.  Frames that cannot use a plane (another kernel or form, RWR_RAY_PLANE=0, a
// frame beyond kRayPlaneMaxW x kRayPlaneMaxH) pass the slot's key and plane by.  A plane that cannot be allocated is no
// error: the frame computes its rays.  The key is cleared by whatever moves the tables outside a frame (ensure_frame_buffers)
// and by rwr_resize.
bool ray_plane_step(rwr_context *ctx, FrameSlot &sl, const FrameParams &fp, RayPlane &plane)
{
    if (!ctx->ray_plane || fp.width > kRayPlaneMaxW || fp.height > kRayPlaneMaxH || fp.row_end <= fp.row_begin) return false;
    const size_t n = ray_plane_entries(fp);
    auto key_of = [&]() {
        const RayPlaneKey k{fp.cam, fp.ray_colp, fp.ray_row, sl.d_ray_plane.ptr, fp.width, fp.height, fp.row_begin, fp.row_end, fp.row_pitch, 0u};
        const unsigned char *b = reinterpret_cast<const unsigned char *>(&k);
        return std::vector<unsigned char>(b, b + sizeof k);
    };
    std::vector<unsigned char> key = key_of();
    if (key != sl.ray_plane_key) {
        sl.ray_plane_key.swap(key);
        sl.ray_plane_built = false;
        return false;
    }
    if (!sl.ray_plane_built) {
        if (sl.d_ray_plane.count < 3u * n) {   // (a larger plane than the slot has held: the old one goes, and with it the key's address)
            if (sl.d_ray_plane.ensure(3u * n) != hipSuccess) {
                (void)hipGetLastError();
                sl.forget_ray_plane();
                return false;
            }
            sl.ray_plane_key = key_of();
        }
        plane = RayPlane{reinterpret_cast<float4 *>(sl.d_ray_plane.ptr), sl.d_ray_plane.ptr + 2u * n};
        if (launch_ray_plane(sl.stream, fp, plane) != hipSuccess) {
            (void)hipGetLastError();
            sl.forget_ray_plane();
            return false;
        }
        sl.ray_plane_built = true;
        ctx->ray_plane_builds++;
    }
    plane = RayPlane{reinterpret_cast<float4 *>(sl.d_ray_plane.ptr), sl.d_ray_plane.ptr + 2u * n};
    ctx->ray_plane_frames++;
    return true;
}

// k_frame_setup, the screen bins of a large scene, and the start of the frame's timing pair.
int enqueue_records(rwr_context *ctx, FrameSlot &sl, FrameKernel kernel, FrameConsts &fc, const FrameSetupOut &so, FrameTiming &timing,
                    bool *kept = nullptr)
{
    FrameParams &fp = fc.fp;
    const hipStream_t stream = sl.stream;
    RWR_HIP_CHECK(launch_records(ctx, sl, fc, so, false, kept));
    if (ctx->n_tris > ctx->bin_min_faces && !(fp.flags & RWR_FLAG_NO_CULL)) {
        // more faces than one 256-wide batch: bin them per 64x32-pixel screen region, once per frame.  The lists
        // are sized by a count pass on the device; the buffer keeps what the previous frames needed (read back a
        // frame late through pinned memory, never waited for) with headroom, and a frame whose lists do not fit
        // walks the whole scene instead — the same pixels — while the buffer grows for the next one.
        const uint32_t bins_x = (fp.width + kBinW - 1) / kBinW, bins_y = (fp.row_end - fp.row_begin + kBinH - 1) / kBinH;
        const size_t n_bins = (size_t)bins_x * bins_y;
        if (!sl.h_bin_total) {
            RWR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&sl.h_bin_total.h), sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped));   // fine-grained: kernels store to it, the host reads it without a synchronisation
            *sl.h_bin_total = 0u;
        }
        const uint64_t needed = *sl.h_bin_total;
        uint64_t capacity = std::max<uint64_t>(sl.d_bin_lists.count, std::max<uint64_t>(ctx->bin_min_capacity, ctx->bin_min_capacity >= 65536u ? 8ull * ctx->n_tris : 0ull));
        if (needed > capacity || needed + needed / 4u > capacity) capacity = std::max<uint64_t>(capacity, needed + needed / 2u);
        capacity = std::min<uint64_t>(capacity, 0xfffffff0ull);
        if (capacity > sl.d_bin_lists.count) RWR_HIP_CHECK(hipStreamSynchronize(stream));   // the old buffer may still be read
        RWR_HIP_CHECK(sl.d_bin_lists.ensure((size_t)capacity));
        RWR_HIP_CHECK(sl.d_bin_counts.ensure(5u * (size_t)n_bins));   // four wave counts per bin, then the bins' own counts (launch_bin_faces)
        RWR_HIP_CHECK(sl.d_bin_offsets.ensure(n_bins));
        RWR_HIP_CHECK(sl.d_bin_total.ensure(1));
        RWR_HIP_CHECK(launch_bin_faces(stream, sl.d_ftris.ptr, ctx->n_tris, fp.row_begin, sl.d_bin_lists.ptr, sl.d_bin_counts.ptr,
                                       sl.d_bin_offsets.ptr, sl.d_bin_total.ptr, bins_x, bins_y, (uint32_t)sl.d_bin_lists.count, fp.mesh_px,
                                       sl.h_bin_total));   // (the scan writes the total to the pinned word itself: no copy command)
        fp.bins = BinGrid{sl.d_bin_lists.ptr, sl.d_bin_counts.ptr + 4u * (size_t)n_bins, sl.d_bin_offsets.ptr, bins_x, bins_y, (uint32_t)sl.d_bin_lists.count, 1u};
    }
    timing.on = ctx->timing_every && (ctx->timing_calls++ % ctx->timing_every == 0) && ctx->timing_pairs < 256;
    timing.dispatch = timing.on && kernel == FrameKernel::kTwoPixel;
    if (timing.on) {
        while (ctx->timing_events.size() < 2u * (ctx->timing_pairs + 1u)) {
            ctx->timing_events.emplace_back();
            RWR_HIP_CHECK(hipEventCreate(&ctx->timing_events.back().h));
        }
        if (!timing.dispatch) RWR_HIP_CHECK(hipEventRecord(ctx->timing_events[2 * ctx->timing_pairs], stream));
    }
    return RWR_OK;
}

// A/B (RWR_FRAME_GRAPH=1): the plain reference frame — records + frame kernel, nothing else on the stream — as one graph launch
int launch_frame_graph(rwr_context *ctx, FrameSlot &sl, const FrameConsts &fc, const FrameSetupOut &so, const QuadTex &quad_tex, const Targets &tg)
{
    const FrameParams &fp = fc.fp;
    const hipStream_t stream = sl.stream;
    sl.records_key.clear();   // the graph's k_frame_setup writes the slot's records
    std::vector<unsigned char> key(sizeof(FrameParams) + sizeof(CullConsts));
    std::memcpy(key.data(), &fp, sizeof fp);
    std::memcpy(key.data() + sizeof fp, &fc.cc, sizeof fc.cc);
    if (!sl.frame_graph || key != sl.frame_graph_key) {
        hipGraph_t g = nullptr;
        RWR_HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        hipError_t e = launch_records(ctx, sl, fc, so, true);
        if (e == hipSuccess) e = launch_primary_p2(stream, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, sl.d_ftris.ptr, quad_tex, tg);
        const hipError_t e2 = hipStreamEndCapture(stream, &g);
        RWR_HIP_CHECK(e);
        RWR_HIP_CHECK(e2);
        bool updated = false;
        if (sl.frame_graph) {
            hipGraphNode_t bad = nullptr;
            hipGraphExecUpdateResult res;
            updated = hipGraphExecUpdate(sl.frame_graph, g, &bad, &res) == hipSuccess;
            if (!updated) { (void)hipGetLastError(); sl.frame_graph = OwnedGraphExec{}; }
        }
        if (!updated) {
            const hipError_t e3 = hipGraphInstantiate(&sl.frame_graph.h, g, nullptr, nullptr, 0);
            if (e3 != hipSuccess) { (void)hipGraphDestroy(g); RWR_HIP_CHECK(e3); }
        }
        (void)hipGraphDestroy(g);
        sl.frame_graph_key.swap(key);
    }
    RWR_HIP_CHECK(hipGraphLaunch(sl.frame_graph, stream));
    ctx->setup_launches++;
    return RWR_OK;
}

// The plain reference frame — records + frame kernel, nothing else — as ONE launch: the frame kernel's first workgroups
// make the records (kernels_primary_p2.hip, FUSED).
// Where it pays (A/B in one box, tools/fused_ab.py, profiles/r03_fused_ab.txt): SMALL frames with frames in flight, which
// are bound by the host's launches — one rank's share of a multi-GPU 1080p frame: 9.8 -> 6.9 us per frame (1/8), 10.4 -> 8.2
// (1/4), the host's enqueue time 9.8 -> 5.2 us.  A whole 1080p frame is VALU-bound and LOSES (15.0 -> 17.4 us with two slots:
// the next frame's waiting workgroups hold slots the running frame could use; 22.7 -> 23.8 us alone), so it keeps its two
// launches.  RWR_FUSED_SETUP=1 forces the fused form wherever it is possible (tests), 0 switches it off.
bool fused_pays(const rwr_context *ctx, const FrameParams &fp)
{
    const uint32_t render_groups = ((fp.width + 63u) / 64u) * ((fp.row_end - fp.row_begin + fp.row_pitch - 1u) / std::max(1u, fp.row_pitch));
    return ctx->fused_setup_force || (ctx->n_slots > 1u && render_groups <= 1200u);
}

int launch_fused_frame(rwr_context *ctx, FrameSlot &sl, const FrameConsts &fc, const FrameSetupOut &so, const QuadTex &quad_tex, const Targets &tg)
{
    const hipStream_t stream = sl.stream;
    sl.records_key.clear();   // the launch's record makers write the slot's records (and no tile lists)
    FusedSetup fs{};
    fs.cc = fc.cc;
    fs.cull = ctx->d_cull.ptr;
    fs.out = so;
    fs.nb_tris = (ctx->n_tris + 255u) / 256u;
    fs.n_blocks = fs.nb_tris + (so.ray_pairs + so.ray_rows + 255u) / 256u;
    fs.extra_rows = primary_p2_fused_rows(fc.fp, fs.n_blocks);
    if (!sl.d_fused.ptr || sl.fused_blocks != fs.n_blocks) {   // first use, or another scene / frame size: the count starts over
        RWR_HIP_CHECK(hipStreamSynchronize(stream));
        RWR_HIP_CHECK(sl.d_fused.ensure(2));
        RWR_HIP_CHECK(hipMemsetAsync(sl.d_fused.ptr, 0, 2 * sizeof(uint32_t), stream));
        sl.fused_count = 0;
        sl.fused_blocks = fs.n_blocks;
    }
    fs.flag = sl.d_fused.ptr;
    fs.flag_base = sl.fused_count;
    sl.fused_count += fs.n_blocks;   // (modulo 2^32, like the device's count)
    sl.fused_used = true;
    RWR_HIP_CHECK(launch_primary_p2(stream, fc.fp, ctx->d_tris.ptr, ctx->d_shade.ptr, sl.d_ftris.ptr, quad_tex, tg, nullptr, nullptr, &fs));
    return RWR_OK;
}

// The reference frame (one sample per pixel, no bounce): records, bins, the chosen kernel — or, for the plain frame of a small
// scene, the graph or the fused launch in their place.
int enqueue_reference(rwr_context *ctx, FrameSlot &sl, const FrameRequest &rq, FrameKernel kernel, FrameConsts &fc, const Targets &tg,
                      FrameTiming &timing)
{
    FrameParams &fp = fc.fp;
    const hipStream_t stream = sl.stream;
    FrameSetupOut so{};
    int rc = frame_tables(ctx, sl, fp, so);
    if (rc != RWR_OK) return rc;
    const bool small_culled = small_culled_frame(ctx, rq, kernel), band = fp.row_end > fp.row_begin;
    // Unbinned scenes in the two-pixel frame kernel with culling: k_frame_setup's last blocks make every tile's face set
    // (rwr_frame_setup.h frame_tile_lists_block), one wave per region of 4x4 of the kernel's workgroups (recomputing the faces'
    // records per block is the blocks' fixed cost; one region per wave keeps the launch short: it delays this slot's frame kernel).
    // (The fused form ignores them: its record makers run in the frame kernel's own launch.)
    if (small_culled && ctx->tile_lists && ctx->n_tris <= kTileListMaxFaces && band) {
        so.list_gx = (fp.width + 63u) / 64u;
        so.list_gy = band_strips(fp);
        so.list_row_begin = fp.row_begin;
        so.list_row_pitch = fp.row_pitch;
        const uint32_t regions = ((so.list_gx + kListRegionWgs - 1u) / kListRegionWgs) * ((so.list_gy + kListRegionWgs - 1u) / kListRegionWgs);
        so.list_blocks = (regions + 4u * kListRegionsPerWave - 1u) / (4u * kListRegionsPerWave);
        RWR_HIP_CHECK(sl.d_tile_lists.ensure(tile_list_words(so.list_gx, so.list_gy)));   // (the sets, then the tiles' class words)
        so.tile_lists = sl.d_tile_lists.ptr;
        fp.tile_lists = so.tile_lists;
    }
    // the frame kernel takes a tile by its class word (RWR_TILE_CLASS=0: it looks at none; the setup writes them all the same)
    fp.flags &= ~(RWR_FLAG_TILE_CLASS | RWR_FLAG_TILE_COVER);
    if (so.tile_lists && ctx->tile_class) fp.flags |= RWR_FLAG_TILE_CLASS;
    ctx->last_classes = rwr_context::LastClasses{so.tile_lists ? ctx->cur : 0u, so.list_gx, so.tile_lists ? so.list_gy : 0u};
    ctx->last_cover_frames = 0;   // (set below, by the one form that looks at cover words)
    const QuadTex quad_tex{ctx->d_quads.empty() ? nullptr : ctx->d_quads[0].ptr, ctx->d_mat_quads.ptr, ctx->d_srgb_lut.ptr};
    const bool plain = small_culled && !rq.aux && !ctx->timing_every;   // nothing but records + frame kernel on the stream
    if (plain && ctx->frame_graph) return launch_frame_graph(ctx, sl, fc, so, quad_tex, tg);   // (an empty band too: captured as it is)
    if (plain && ctx->fused_setup && fused_pays(ctx, fp) && !(fp.flags & RWR_FLAG_NORMAL_MAP) && band) {
        ctx->last_classes = rwr_context::LastClasses{};   // (the fused form makes no sets)
        return launch_fused_frame(ctx, sl, fc, so, quad_tex, tg);
    }
    bool kept = false;
    if ((rc = enqueue_records(ctx, sl, kernel, fc, so, timing, &kept)) != RWR_OK) return rc;
    switch (kernel) {
    case FrameKernel::kDormant: {
        SingleTriangles st{};
        st.n = ctx->n_triangles;
        for (uint32_t i = 0; i < ctx->n_triangles; i++) st.t[i] = ctx->triangles[i];
        RWR_HIP_CHECK(launch_primary_dormant(stream, fp, st, ctx->d_tris.ptr, ctx->d_shade.ptr, tex0_of(ctx), tg));
        break;
    }
    case FrameKernel::kBvh: {
        const BvhDevice bvh_p{ctx->d_bvh_nodes.ptr, ctx->d_bvh_leaf_faces.ptr, ctx->bvh_n_nodes, 3u * ctx->bvh_depth + 2u, 0.0f, 0u, 0u, 0u, 0u};
        RWR_HIP_CHECK(launch_primary_bvh(stream, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, bvh_p, tex0_of(ctx), tg));
        break;
    }
    case FrameKernel::kOnePixel:
        RWR_HIP_CHECK(launch_primary(stream, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, sl.d_ftris.ptr, tex0_of(ctx), tg));
        break;
    default: {
        // (the forms with a loading twin: culled, no normal maps — launch_primary_p2's own rule for RWR_FLAG_NORMAL_MAP)
        RayPlane plane{};
        const bool can_load = !(fp.flags & RWR_FLAG_NO_CULL) && !((fp.flags & RWR_FLAG_NORMAL_MAP) && fp.tangents);
        const bool load = can_load && ray_plane_step(ctx, sl, fp, plane);
        // Cover words (rwr_internal.h kTileCovered): only a frame served from the slot's kept records looks at them — the first
        // such frame learns them with the straight path's own tests, the frames after it skip those tests on the tiles learnt —
        // so a frame that made its records (a moving camera, RWR_SETUP_CACHE=0) neither reads nor writes one.  RWR_TILE_COVER=0:
        // no frame does.
        // (can_load: no normal maps; one material — the frames whose one-face tiles take the straight path at all)
        if (kept && (fp.flags & RWR_FLAG_TILE_CLASS) && ctx->tile_cover && can_load && fp.n_materials <= 1u) {
            fp.flags |= RWR_FLAG_TILE_COVER;
            ctx->tile_cover_frames++;
            ctx->last_cover_frames = ++sl.cover_frames;
        }
        RWR_HIP_CHECK(launch_primary_p2(stream, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, sl.d_ftris.ptr, quad_tex, tg,
                                        timing.dispatch ? ctx->timing_events[2 * ctx->timing_pairs].h : nullptr,
                                        timing.dispatch ? ctx->timing_events[2 * ctx->timing_pairs + 1].h : nullptr, nullptr,
                                        load ? &plane : nullptr));
    }
    }
    return RWR_OK;
}

// A frame of the wavefront integrator: the samples are traced in launch groups; per group the primary stage (all of the
// group's samples of every pixel, rays into the fixed-slot queue) then the bounce stage (one workgroup per
// 64x8-pixel tile and its ray pool)
int enqueue_wavefront(rwr_context *ctx, FrameSlot &sl, const FrameRequest &rq, AccumPlan &ap, ReprojectPlan &pp, FrameConsts &fc,
                      const Targets &tg, FrameTiming &timing)
{
    FrameParams &fp = fc.fp;
    const rwr_render_params &rp = rq.rp;
    const hipStream_t stream = sl.stream;
    const size_t n = (size_t)fp.width * fp.height;
    const float4 *tex0 = tex0_of(ctx);
    WfState &W = ctx->wf_state[ctx->n_slots > 1u ? ctx->cur : 0u];   // this slot's accumulators and queues
    const uint32_t group = std::min(rp.spp, ctx->wf_group ? ctx->wf_group : (ctx->n_slots > 1u ? 64u : 32u));
    const uint32_t tiles_x = (fp.width + kWfTileW - 1u) / kWfTileW, tiles_y = band_strips(fp);
    const uint32_t n_tiles = tiles_x * tiles_y;
    FrameSetupOut so{};
    int rc = frame_tables(ctx, sl, fp, so);
    if (rc != RWR_OK) return rc;
    // the per-tile ray counts and the live-tile count start every frame from zero: k_frame_setup zeroes them
    RWR_HIP_CHECK(W.d_wave_total.ensure((size_t)n_tiles * 4u));
    RWR_HIP_CHECK(W.d_tiles.ensure(2u * (size_t)n_tiles + 1u));
    so.zero_a = W.d_wave_total.ptr; so.n_zero_a = n_tiles * 4u;
    so.zero_b = W.d_tiles.ptr + 2u * (size_t)n_tiles; so.n_zero_b = 1u;   // live_count (below)
    if ((rc = enqueue_records(ctx, sl, FrameKernel::kWavefront, fc, so, timing)) != RWR_OK) return rc;
    if (W.d_fix.count < 4u * n) W.fix_clean = false;
    RWR_HIP_CHECK(W.d_fix.ensure(4u * n));
    if (!W.fix_clean)   // first use, a new size, or a frame that did not reach its resolve
        RWR_HIP_CHECK(hipMemsetAsync(W.d_fix.ptr, 0, 4u * n * sizeof(unsigned long long), stream));
    W.fix_clean = false;
    // two launch groups in flight (each on its own stream, with its own half of the queue) when the frame has several
    const size_t n_queues = rp.max_bounces ? std::min<size_t>(ctx->wf_queues, (rp.spp + group - 1u) / group) : 1u;
    const bool overlap = n_queues > 1u;
    const size_t slots = (size_t)n_tiles * group * kWfTilePixels;
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
    if (rp.max_bounces) {
        RWR_HIP_CHECK(W.d_rays.ensure(n_queues * 2u * slots));
        RWR_HIP_CHECK(W.d_sorted.ensure(n_queues * slots));
        RWR_HIP_CHECK(W.d_bins.ensure(n_queues * slots));
        RWR_HIP_CHECK(W.d_masks.ensure(n_queues * n_tiles * group * 8u));
        if (rp.max_bounces > 1u) RWR_HIP_CHECK(W.d_masks_next.ensure(n_queues * n_tiles * group * 8u));
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
        RWR_HIP_CHECK(W.d_shadow_masks.ensure(n_queues * n_tiles * group * 8u));
        RWR_HIP_CHECK(W.d_shadow_counts.ensure(2));
        RWR_HIP_CHECK(hipMemsetAsync(W.d_shadow_counts.ptr, 0, 2 * sizeof(unsigned long long), stream));
    }
    // the unit vectors towards the reference's two lights, -normalize(kLightDir) in the oracle's f32 operations
    // (triangle_list/compute.wgsl:55, sphere/compute.wgsl:41)
    float light_mesh[3], light_sphere[3];
    {
        const float km[3] = {1.0f, -1.0f, -5.0f}, ks[3] = {1.0f, -5.0f, 1.0f};
        const float lm = std::sqrt(km[0] * km[0] + km[1] * km[1] + km[2] * km[2]), ls = std::sqrt(ks[0] * ks[0] + ks[1] * ks[1] + ks[2] * ks[2]);
        for (int k = 0; k < 3; k++) { light_mesh[k] = -(km[k] / lm); light_sphere[k] = -(ks[k] / ls); }
    }
    // Did the frame before show LITTLE — fewer than 1 024 live tiles, and at most half of this frame's tiles (a small mesh
    // on an empty screen; not a small frame full of geometry, such as a row band of a multi-GPU frame: measured, that one
    // is best left alone)?  Its count arrives through pinned memory, a frame late, never waited for.  Then several
    // workgroups share a tile's samples in the primary stage (enough of them to fill the chip twice, up to one per
    // sample), and the tiles anything can be seen through are listed first (below).  Any choice gives the same frame: all
    // sums are integers.
    const uint32_t prev_packets = ctx->h_wf_live ? ctx->h_wf_live[0] : 0u, prev_lane = ctx->h_wf_live ? ctx->h_wf_live[1] : 0u;
    const uint32_t live = prev_packets + prev_lane;
    const bool shows_little = live != 0u && live < 1024u && 2u * live <= n_tiles;
    uint32_t z_split = ctx->wf_z_split;
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
    const uint32_t shadow_tiles = live_list ? std::max(1u, live) : n_tiles;
    WfBuffers wfq[kWfMaxQueues];
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
    const BvhDevice bvh{ctx->d_bvh_nodes.ptr, ctx->d_bvh_leaf_faces.ptr, ctx->bvh_n_nodes, 3u * ctx->bvh_depth + 2u,
                        ctx->wf_packet_extent * ctx->bvh_leaf_extent, ctx->wf_min_packet_pools,
                        // work items of the per-lane trace kernel when pools are few: one 256-ray chunk each for a context that
                        // renders one frame at a time (the chip has nothing else to do: as many items as possible), about four
                        // chunks each when frames overlap (a pool's rays grow with the group's samples; measured at configs[3],
                        // 16 samples: 0.625 -> 0.607 ms with 4 096 items, but 0.74 -> 0.79 ms one frame at a time; configs[4]'s
                        // frame, 64 samples: 16 384 is best either way)
                        ctx->wf_lane_items ? ctx->wf_lane_items : (wide_lane ? 256u : ctx->n_slots > 1u ? std::min(16384u, 256u * group) : 16384u),
                        ctx->wf_packet_dense_rays, wide_lane ? 1u : 0u};
    // RWR_FLAG_MIRRORS: this slot's copy of the surface table — a record per part, then one per sphere index — refreshed on the
    // frame's stream (ahead of the fork below: every queue's kernels read it) when the context's attributes have changed since the slot's last copy
    // (ft: what the frame's kernels know, WfFeatures — the surfaces and the sky here, a queue's shadow records per launch group,
    // emit per generation)
    WfFeatures ft;
    ft.surf = rq.gloss ? kSurfGloss : rq.glass ? kSurfGlass : rq.mirrors ? kSurfMirrors : kSurfNone;
    const uint32_t modes = (rq.mirrors ? 1u : 0u) | (rq.glass ? 2u : 0u) | (rq.gloss ? 4u : 0u);   // whose records the frame's copy holds: a flag switches its own surfaces on
    if (modes) {
        const size_t n_parts = ctx->part_mirrors.size(), n_recs = n_parts + RWR_MAX_SPHERES;
        if (W.mirror_version != ctx->mirror_version || W.mirror_modes != modes || W.d_mirror.count < n_recs) {
            if (W.mirror_version != 0u) RWR_HIP_CHECK(hipEventSynchronize(W.mirror_copied));   // the image's last copy has been read
            if (W.h_mirror_count < n_recs) {
                W.h_mirror = PinnedMirror();
                RWR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&W.h_mirror.h), n_recs * sizeof(MirrorRec), hipHostMallocDefault));
                W.h_mirror_count = n_recs;
            }
            RWR_HIP_CHECK(W.d_mirror.ensure(n_recs));
            if (!W.mirror_copied) RWR_HIP_CHECK(hipEventCreateWithFlags(&W.mirror_copied.h, hipEventDisableTiming));
            auto visible = [&](const MirrorRec &m) {   // a surface whose flag the frame lacks is the diffuse surface it was
                const bool on = m.on > 1.0f ? rq.gloss : m.on > 0.0f ? rq.mirrors : m.on < 0.0f ? rq.glass : false;
                return on ? m : MirrorRec{0.0f, 0.0f, 0.0f, 0.0f};
            };
            for (size_t i = 0; i < n_parts; i++) W.h_mirror.h[i] = visible(ctx->part_mirrors[i]);
            for (size_t i = 0; i < RWR_MAX_SPHERES; i++) W.h_mirror.h[n_parts + i] = visible(ctx->sphere_mirrors[i]);
            RWR_HIP_CHECK(hipMemcpyAsync(W.d_mirror.ptr, W.h_mirror.h, n_recs * sizeof(MirrorRec), hipMemcpyHostToDevice, stream));
            RWR_HIP_CHECK(hipEventRecord(W.mirror_copied, stream));
            W.mirror_version = ctx->mirror_version;
            W.mirror_modes = modes;
        }
        ft.mirror = WfMirror{W.d_mirror.ptr, (uint32_t)n_parts, 0u, nullptr};
        // (intended: a frame with RWR_FLAG_GLASS alone also holds and zeroes four counters now, 8 bytes more than its three — one
        // buffer of one size for either flag, so that a context alternating between them never reallocates; no launch is added)
        if (rq.glass || rq.gloss) {   // the frame's event counters — three of glass, then the glossy rays — start from zero
            RWR_HIP_CHECK(W.d_glass_counts.ensure(4));
            RWR_HIP_CHECK(hipMemsetAsync(W.d_glass_counts.ptr, 0, 4 * sizeof(unsigned long long), stream));
            ft.mirror.glass_counts = W.d_glass_counts.ptr;
        }
    }
    if (overlap) {   // the other streams start behind this frame's setup (and so behind the previous frame's resolve)
        RWR_HIP_CHECK(hipEventRecord(W.fork, stream));
        for (size_t q = 1; q < n_queues; q++) RWR_HIP_CHECK(hipStreamWaitEvent(W.streams[q], W.fork, 0));
    }
    if (rq.sky) std::memcpy(&ft.sky, &ctx->sky, sizeof ft.sky);
    ft.sky_on = rq.sky;
    const uint32_t *last_counters = nullptr;
    // (global sample indices: an accumulating frame traces [accum_before, accum_before + spp), keyed like one frame of them all)
    for (uint32_t s0 = 0, g = 0; s0 < ap.trace_spp; s0 += group, g++) {
        const uint32_t cnt = std::min(group, rp.spp - s0);
        const size_t q = g % n_queues;
        hipStream_t gs = q ? W.streams[q].h : stream;
        const size_t mask_words = (size_t)n_tiles * group * 8u;
        if (rq.shadows) ft.shadow = WfShadow{W.d_shadow_recs.ptr + q * slots, W.d_shadow_masks.ptr + q * mask_words, W.d_shadow_counts.ptr};
        ft.shadows = ft.shadow.recs != nullptr;
        RWR_HIP_CHECK(launch_wf_primary(gs, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, sl.d_ftris.ptr, tex0, tg, wfq[q],
                                        (uint32_t)ap.before + s0, cnt, z_split, ft));
        if (rq.shadows)   // h0's shadow rays
            RWR_HIP_CHECK(launch_wf_shadow(gs, fp, ctx->d_tris.ptr, bvh, wfq[q], ft.shadow, n_tiles, shadow_tiles, cnt, light_mesh, light_sphere));
        // the bounce stage: one generation of rays per bounce (RWR_FLAG_MULTI_BOUNCE: up to RWR_MAX_BOUNCES).  Generation k traces
        // ray k of every path that is still alive — the sort and trace kernels run again over the same fixed slots — and, unless
        // it is the last, writes ray k + 1 back into the slot of every hit, with its bit in the other ballot array.
        WfBuffers wg = wfq[q];
        unsigned long long *masks_next = W.d_masks_next.ptr ? W.d_masks_next.ptr + q * n_tiles * group * 8u : nullptr;
        for (uint32_t gen = 1; gen <= rp.max_bounces; gen++) {
            if (gen > 1u)   // the sort counts this generation's live pools from zero (the primary stage zeroed the set of four for the first)
                RWR_HIP_CHECK(hipMemsetAsync(wg.counters, 0, 4u * sizeof(uint32_t), gs));
            const bool emit = gen < rp.max_bounces;
            ft.emits = emit;
            ft.emit = emit ? WfEmit{masks_next, 2u + 16u * gen, (uint32_t)ap.before + s0} : WfEmit{nullptr, 0u, 0u};
            if (emit) RWR_HIP_CHECK(hipMemsetAsync(masks_next, 0, (size_t)n_tiles * group * 8u * sizeof(unsigned long long), gs));
            if (rq.shadows) RWR_HIP_CHECK(hipMemsetAsync(ft.shadow.masks, 0, mask_words * sizeof(unsigned long long), gs));   // the trace kernels set bits
            RWR_HIP_CHECK(launch_wf_bounce(gs, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, bvh, tex0, wg, n_tiles, cnt,
                                           (uint32_t)std::fmax(1.0f, std::ceil(ctx->wf_packet_fill * (float)(cnt * kWfTilePixels))),
                                           W.d_pool_info.ptr + q * n_tiles * wf_pool_info_bytes(), W.d_pool_list.ptr + q * 2u * (size_t)n_tiles, ft));
            if (rq.shadows)   // this generation's hits
                RWR_HIP_CHECK(launch_wf_shadow(gs, fp, ctx->d_tris.ptr, bvh, wg, ft.shadow, n_tiles, shadow_tiles, cnt, light_mesh, light_sphere));
            if (emit) std::swap(wg.masks, masks_next);
        }
        if (rp.max_bounces && s0 + group >= rp.spp) last_counters = wfq[q].counters;   // the last group's live-pool counts, for the next frame's split
    }
    for (size_t q = 1; q < n_queues; q++) {
        RWR_HIP_CHECK(hipEventRecord(W.join[q], W.streams[q]));
        RWR_HIP_CHECK(hipStreamWaitEvent(stream, W.join[q], 0));
    }
    // (the resolve also hands the last group's live pool counts to the host: a store to pinned memory, no copy command.  The
    // same store at the top of the per-lane trace kernel made THAT kernel twice as slow, 453 -> 840 us at configs[3], with the
    // pointer null and the instruction mix unchanged; here it costs nothing measurable.)
    if (!rq.accumulate) {
        RWR_HIP_CHECK(launch_wf_resolve(stream, fp, tg, wfq[0], last_counters, last_counters ? ctx->h_wf_live.h : nullptr));
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
        RWR_HIP_CHECK(launch_wf_resolve_accum(stream, fp, tg, wfq[0], ab, ap.mode, (uint32_t)total, last_counters,
                                              last_counters ? ctx->h_wf_live.h : nullptr));
        RWR_HIP_CHECK(hipEventRecord(A.done, stream));
        A.done_recorded = true;
        A.key.swap(ap.key);
        A.samples = total;
        ctx->last_accum_samples = total;
    }
    W.fix_clean = true;   // (the resolve zeroes what it reads; rows outside the band were never touched)
    // RWR_FLAG_REPROJECT: the stage, behind the resolve on the slot's stream.  The history is the context's, not the slot's: frames
    // in flight trace side by side, their stages run in frame order behind an event.  Frame k gathers from set (k - 1) & 1 and
    // writes set k & 1 — the set frame k - 1 read from, which that frame's stage (the event) has finished with.
    if (rq.reproject) {
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
    }
    // RWR_FLAG_DENOISE: the filter, behind either resolve (and the reprojection stage: it filters `out`, and runs behind the event
    // the next stage waits for — the history never sees the filter) on the slot's stream.  (An accumulating frame: behind the event the next
    // accumulating resolve waits for — the history never sees the filter, and no other slot waits for it.)
    if (rq.denoise) {
        RWR_HIP_CHECK(sl.d_dn_guide.ensure(n));
        RWR_HIP_CHECK(sl.d_dn_a.ensure(n));
        RWR_HIP_CHECK(sl.d_dn_b.ensure(n));
        RWR_HIP_CHECK(launch_wf_denoise(stream, fp.width, fp.height, ctx->d_tris.ptr, tg, ctx->denoise, sl.d_dn_guide.ptr, sl.d_dn_a.ptr, sl.d_dn_b.ptr));
    }
    ctx->last_segments = n_tiles;
    ctx->last_wf_state = ctx->n_slots > 1u ? ctx->cur : 0u;
    return RWR_OK;
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
    ctx->last_bounce = 0;  // filled in lazily by rwr_last_render_stats from the pass counters
    return RWR_OK;
}

}  // namespace

// A frame rendered by the fused frame kernel is complete unless one of its waves waited in vain for the records (the wait is
// bounded; it has never been seen to run out): slot `i` is idle when this is called.
int rwr::check_fused_frame(rwr_context *ctx, uint32_t i)
{
    FrameSlot &sl = ctx->slots[i];
    if (!sl.fused_used || !sl.d_fused.ptr) return RWR_OK;
    uint32_t timed_out = 0;
    RWR_HIP_CHECK(hipMemcpy(&timed_out, sl.d_fused.ptr + 1, sizeof timed_out, hipMemcpyDeviceToHost));
    if (timed_out) {
        sl.fused_blocks = 0;   // the count is no longer what the host expects: start over with the next frame
        return set_error(RWR_ERR_HIP, "a frame is incomplete: workgroups of the fused frame kernel waited in vain for the frame's records "
                         "(RWR_FUSED_SETUP=0 renders with two launches per frame)");
    }
    return RWR_OK;
}

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
