// A render call, validated and planned: what was asked, what it does with the histories, which kernel renders it.
#include <cstring>

#include "rwr_frame.h"

namespace rwr {

namespace {

// validate's rules for the integrator's flags, in the order they are checked (it decides which refusal a call with several
// faults gets).  Every one of them belongs to frames of the mesh and the spheres under the perspective camera.  stage: the flag
// is no flag the frame is traced with but a stage behind the resolve that works on the whole frame's planes — the colour and the
// id / t planes, so RWR_FLAG_AUX_OUTPUTS is implied, and its own bit is not part of rp.flags from there on (nor of a history's key).
// mode: a surface flag switches on the surfaces of its model (surface_mode's bit).
struct FlagRule { uint32_t flag; const char *name, *stage, *why; uint32_t mode; };
constexpr FlagRule kFlagRules[17] = {
    {RWR_FLAG_ACCUMULATE, "RWR_FLAG_ACCUMULATE", nullptr, nullptr, 0u},
    {RWR_FLAG_SHADOWS, "RWR_FLAG_SHADOWS", nullptr, nullptr, 0u},
    {RWR_FLAG_DENOISE, "RWR_FLAG_DENOISE", "filter", "its taps reach 62 pixels", 0u},
    {RWR_FLAG_REPROJECT, "RWR_FLAG_REPROJECT", "stage", "its taps land anywhere in the previous one", 0u},
    {RWR_FLAG_SKY, "RWR_FLAG_SKY", nullptr, nullptr, 0u},
    {RWR_FLAG_MIRRORS, "RWR_FLAG_MIRRORS", nullptr, nullptr, surface_mode(SurfaceModel::kMirror)},
    {RWR_FLAG_GLASS, "RWR_FLAG_GLASS", nullptr, nullptr, surface_mode(SurfaceModel::kGlass)},
    {RWR_FLAG_GLOSSY, "RWR_FLAG_GLOSSY", nullptr, nullptr, surface_mode(SurfaceModel::kGloss)},
    {RWR_FLAG_SOFT_SHADOWS, "RWR_FLAG_SOFT_SHADOWS", nullptr, nullptr, 0u},
    {RWR_FLAG_EMISSIVE, "RWR_FLAG_EMISSIVE", nullptr, nullptr, 0u},
    {RWR_FLAG_LIGHT_SAMPLING, "RWR_FLAG_LIGHT_SAMPLING", nullptr, nullptr, 0u},
    {RWR_FLAG_LIGHT_PARTS, "RWR_FLAG_LIGHT_PARTS", nullptr, nullptr, 0u},
    {RWR_FLAG_LIGHT_MIS, "RWR_FLAG_LIGHT_MIS", nullptr, nullptr, 0u},
    {RWR_FLAG_SOBOL, "RWR_FLAG_SOBOL", nullptr, nullptr, 0u},
    {RWR_FLAG_SKY_IMAGE, "RWR_FLAG_SKY_IMAGE", nullptr, nullptr, 0u},
    {RWR_FLAG_LIGHT_SKY, "RWR_FLAG_LIGHT_SKY", nullptr, nullptr, 0u},
    {RWR_FLAG_TONEMAP, "RWR_FLAG_TONEMAP", "stage", "the exposure is measured over all of it", 0u}};
constexpr uint32_t kSurfaceFlags = RWR_FLAG_MIRRORS | RWR_FLAG_GLASS | RWR_FLAG_GLOSSY;

// What an accumulating frame must share with the frame before for the accumulation to go on (rwr_hip.h RWR_FLAG_ACCUMULATE): the
// camera uniform's bytes, the screen, the rows, bounces, seed, flags but the ACCUMULATE bit, frames in flight and the scene — and, while
// the frame is lit by the sky (RWR_FLAG_SKY), the sky's parameters, and while its lights have a size (RWR_FLAG_SOFT_SHADOWS), theirs.  (Mirror surfaces, RWR_FLAG_MIRRORS: the flag is one of the
// flags, and every call of their setters changes the scene's generation; glass surfaces, RWR_FLAG_GLASS, glossy ones, RWR_FLAG_GLOSSY, and
// emissive ones, RWR_FLAG_EMISSIVE, likewise.)
std::vector<unsigned char> accum_key_of(const rwr_context *ctx, const rwr_camera_inv_uniform &cam, const FrameRequest &rq)
{
    const uint32_t words[9] = {ctx->screen.width, ctx->screen.height, rq.row_begin, rq.row_end, rq.row_pitch, rq.rp.max_bounces, rq.rp.seed,
                               rq.rp.flags & ~(uint32_t)RWR_FLAG_ACCUMULATE, ctx->n_slots};
    std::vector<unsigned char> key(sizeof cam + sizeof words + sizeof ctx->scene_generation + (rq.sky ? sizeof ctx->sky : 0u) + (rq.sky_image ? sizeof ctx->sky_image_generation : 0u) + (rq.soft ? sizeof ctx->shadow : 0u));
    unsigned char *at = key.data();
    std::memcpy(at, &cam, sizeof cam); at += sizeof cam;
    std::memcpy(at, words, sizeof words); at += sizeof words;
    std::memcpy(at, &ctx->scene_generation, sizeof ctx->scene_generation); at += sizeof ctx->scene_generation;
    if (rq.sky) { std::memcpy(at, &ctx->sky, sizeof ctx->sky); at += sizeof ctx->sky; }
    if (rq.sky_image) { std::memcpy(at, &ctx->sky_image_generation, sizeof ctx->sky_image_generation); at += sizeof ctx->sky_image_generation; }   // (RWR_FLAG_SKY_IMAGE: the image's generation next to the sky's parameters)
    if (rq.soft) std::memcpy(at, &ctx->shadow, sizeof ctx->shadow);   // (the flag's bit is among the words: the two optional tails cannot be taken for each other)
    return key;
}

// What a reprojecting frame must share with the one before for the history to go on (rwr_hip.h RWR_FLAG_REPROJECT item 2): the
// screen, spp, bounces, seed, the effective flags (the DENOISE, REPROJECT and TONEMAP bits are not among them), frames in flight, the scene,
// the stage's parameters and, while the sky lights the frame, the sky's, while the lights have a size, theirs.  NOT the camera.
std::vector<unsigned char> reproject_key_of(const rwr_context *ctx, const FrameRequest &rq)
{
    const uint32_t words[7] = {ctx->screen.width, ctx->screen.height, rq.rp.spp, rq.rp.max_bounces, rq.rp.seed, rq.rp.flags, ctx->n_slots};
    std::vector<unsigned char> key(sizeof words + sizeof ctx->scene_generation + sizeof ctx->reproject + (rq.sky ? sizeof ctx->sky : 0u) + (rq.sky_image ? sizeof ctx->sky_image_generation : 0u) + (rq.soft ? sizeof ctx->shadow : 0u));
    unsigned char *at = key.data();
    std::memcpy(at, words, sizeof words); at += sizeof words;
    std::memcpy(at, &ctx->scene_generation, sizeof ctx->scene_generation); at += sizeof ctx->scene_generation;
    std::memcpy(at, &ctx->reproject, sizeof ctx->reproject); at += sizeof ctx->reproject;
    if (rq.sky) { std::memcpy(at, &ctx->sky, sizeof ctx->sky); at += sizeof ctx->sky; }
    if (rq.sky_image) { std::memcpy(at, &ctx->sky_image_generation, sizeof ctx->sky_image_generation); at += sizeof ctx->sky_image_generation; }   // (RWR_FLAG_SKY_IMAGE: the image's generation next to the sky's parameters)
    if (rq.soft) std::memcpy(at, &ctx->shadow, sizeof ctx->shadow);
    return key;
}

}  // namespace

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
    const uint32_t asked = rp.flags;
    const bool off_reference = (asked & (RWR_FLAG_ORTHO_RAYS | RWR_FLAG_USE_BVH)) || ctx->n_triangles != 0;
    const bool whole_frame = row_begin == 0u && row_end == ctx->screen.height && row_pitch == kStripRows;
    for (const FlagRule &f : kFlagRules) {
        if (!(asked & f.flag)) continue;
        if (f.flag == RWR_FLAG_REPROJECT && (asked & RWR_FLAG_ACCUMULATE))
            return set_error(RWR_ERR_UNSUPPORTED, "RWR_FLAG_REPROJECT with RWR_FLAG_ACCUMULATE: a context blends one history, not two");
        if (off_reference)   // (it holds whatever max_bounces is and whatever the scene holds)
            return set_error(RWR_ERR_UNSUPPORTED, "%s: RWR_FLAG_ORTHO_RAYS, RWR_FLAG_USE_BVH and single-triangle passes apply to the reference frame only", f.name);
        if (!f.stage) continue;
        if (!whole_frame)
            return set_error(RWR_ERR_UNSUPPORTED, "%s: the %s needs the whole frame (%s); rows [%u,%u) every %u-th strip is a part of it", f.name,
                             f.stage, f.why, row_begin, row_end, row_pitch / kStripRows);
        rp.flags = (rp.flags & ~f.flag) | RWR_FLAG_AUX_OUTPUTS;
    }
    // A flag without effect is cleared: the frame is the frame without it, in the same kernels.  The sky lights bounce rays alone
    // and a surface model shows in bounce rays alone, so a frame whose paths end at h0 has neither; and a surface flag needs a
    // surface of its model in the scene (looked for only when such a flag is set: the plain reference frame pays for no scan).
    if (rp.max_bounces == 0u) {
        rp.flags &= ~(RWR_FLAG_SKY | kSurfaceFlags);
    } else if (rp.flags & kSurfaceFlags) {
        const uint32_t modes = surface_modes(ctx);
        for (const FlagRule &f : kFlagRules)
            if (f.mode && !(modes & f.mode)) rp.flags &= ~f.flag;
    }
    // The sky's image replaces the gradient's S(D) and nothing else: without the sky in effect, or without an image, there is nothing to replace
    if (!(rp.flags & RWR_FLAG_SKY) || !ctx->sky_image) rp.flags &= ~(uint32_t)RWR_FLAG_SKY_IMAGE;
    // An emitter shows at h0 already, so RWR_FLAG_EMISSIVE stays at max_bounces 0; without an emitting surface it has nothing to add
    if ((rp.flags & RWR_FLAG_EMISSIVE) && !scene_glows(ctx)) rp.flags &= ~(uint32_t)RWR_FLAG_EMISSIVE;
    // Light sampling aims rays from diffuse hits at the emitting spheres: without RWR_FLAG_EMISSIVE in effect, without a bounce (no hit
    // sends a ray on) or without an emitting sphere in use there is nothing to aim at
    if ((rp.flags & RWR_FLAG_LIGHT_SAMPLING) && (!(rp.flags & RWR_FLAG_EMISSIVE) || rp.max_bounces == 0u || scene_lights(ctx).m == 0u))
        rp.flags &= ~(uint32_t)RWR_FLAG_LIGHT_SAMPLING;
    // ... and the mesh light likewise, by its own rule: the list of the emitting parts' faces must not be empty (looked at, and rebuilt
    // if the scene changed it, only when the flag is set and everything else holds)
    if (rp.flags & RWR_FLAG_LIGHT_PARTS) {
        uint32_t n_listed = 0;
        if ((rp.flags & RWR_FLAG_EMISSIVE) && rp.max_bounces != 0u) {
            const int rc = scene_part_lights(ctx, n_listed);
            if (rc != RWR_OK) return rc;
        }
        if (n_listed == 0u) rp.flags &= ~(uint32_t)RWR_FLAG_LIGHT_PARTS;
    }
    // Light rays towards the sky's image need the image in effect and a sampling table of it (an image with weight: looked at, and
    // built if the image changed, only when the flag is set and the image is in effect); they do not need RWR_FLAG_EMISSIVE
    if (rp.flags & RWR_FLAG_LIGHT_SKY) {
        bool have = false;
        if (rp.flags & RWR_FLAG_SKY_IMAGE) {
            const int rc = scene_sky_light(ctx, have);
            if (rc != RWR_OK) return rc;
        }
        if (!have) rp.flags &= ~(uint32_t)RWR_FLAG_LIGHT_SKY;
    }
    // Multiple importance sampling weights the light rays of the three flags above against the bounce rays: without any there is nothing to weight
    if (!(rp.flags & (RWR_FLAG_LIGHT_SAMPLING | RWR_FLAG_LIGHT_PARTS | RWR_FLAG_LIGHT_SKY))) rp.flags &= ~(uint32_t)RWR_FLAG_LIGHT_MIS;
    // Soft shadows change the direction of shadow rays and nothing else: without shadow rays, or with two point lights, there is nothing to change
    if (!(asked & RWR_FLAG_SHADOWS) || (ctx->shadow.mesh_light_radius == 0.0f && ctx->shadow.sphere_light_radius == 0.0f)) rp.flags &= ~(uint32_t)RWR_FLAG_SOFT_SHADOWS;
    auto has = [](uint32_t flags, uint32_t flag) { return (flags & flag) != 0; };
    rq = FrameRequest{rp, row_begin, row_end, row_pitch, has(rp.flags, RWR_FLAG_AUX_OUTPUTS), has(asked, RWR_FLAG_ACCUMULATE), has(asked, RWR_FLAG_SHADOWS),
                      has(asked, RWR_FLAG_DENOISE), has(asked, RWR_FLAG_REPROJECT), has(rp.flags, RWR_FLAG_MIRRORS), has(rp.flags, RWR_FLAG_GLASS),
                      has(rp.flags, RWR_FLAG_GLOSSY), has(rp.flags, RWR_FLAG_SKY), has(rp.flags, RWR_FLAG_SOFT_SHADOWS), has(rp.flags, RWR_FLAG_EMISSIVE), has(rp.flags, RWR_FLAG_LIGHT_SAMPLING), has(rp.flags, RWR_FLAG_LIGHT_PARTS), has(rp.flags, RWR_FLAG_LIGHT_MIS), false, false, false, false, false,
                      has(asked, RWR_FLAG_TONEMAP)};
    // an accumulating frame always takes the wavefront integrator (its samples are jittered even at spp 1), and so does a frame
    // with shadow rays (the integrator's stages trace them), one the filter follows (it runs behind the integrator's resolve) or one
    // with an emitter (the integrator's kernels add its light), and one the tone-mapping stage follows (as the filter)
    rq.wavefront = rp.spp != 1 || rp.max_bounces != 0 || rq.accumulate || rq.shadows || rq.denoise || rq.reproject || rq.glow || rq.tonemap;
    // The sample sequence changes the integrator's random numbers and nothing else: it sends no frame there, and a frame of the
    // reference's kernels draws none (rq.rp.flags is what the histories' keys and the kernels see)
    rq.sky_image = has(rp.flags, RWR_FLAG_SKY_IMAGE);
    rq.light_sky = has(rp.flags, RWR_FLAG_LIGHT_SKY);
    rq.sobol = rq.wavefront && has(rp.flags, RWR_FLAG_SOBOL);
    if (!rq.sobol) rq.rp.flags &= ~(uint32_t)RWR_FLAG_SOBOL;
    rq.dormant = ctx->n_triangles != 0 || (rp.flags & RWR_FLAG_ORTHO_RAYS) != 0;
    if (rq.dormant && (rq.wavefront || (rp.flags & RWR_FLAG_USE_BVH)))
        return set_error(RWR_ERR_UNSUPPORTED, "single-triangle passes and RWR_FLAG_ORTHO_RAYS apply to the reference frame (spp 1, no bounce, no RWR_FLAG_USE_BVH)");
    return RWR_OK;
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

}  // namespace rwr
