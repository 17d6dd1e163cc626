// One frame behind the C ABI, host side only (no .hip file includes this): what the frame units share — a request, its plans,
// and the functions the units call across.  What one unit alone uses stays in that unit.
#pragma once

#include "rwr_context.h"

namespace rwr {

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
    bool soft;        // RWR_FLAG_SOFT_SHADOWS with RWR_FLAG_SHADOWS and a radius that is not 0: k_wf_shadow's SOFT forms (else the bit is cleared from rp.flags)
    bool glow;        // RWR_FLAG_EMISSIVE with an emitting surface in the scene: the GLOW forms (else the bit is cleared from rp.flags)
    bool light;       // RWR_FLAG_LIGHT_SAMPLING with RWR_FLAG_EMISSIVE effective, a bounce and an emitting sphere in use: k_wf_light (else the bit is cleared from rp.flags)
    bool light_parts; // RWR_FLAG_LIGHT_PARTS with RWR_FLAG_EMISSIVE effective, a bounce and a mesh light that is not empty: k_wf_light's PARTS forms (else the bit is cleared from rp.flags)
    bool light_mis;   // RWR_FLAG_LIGHT_MIS with one of the two light flags effective: the light stage and add_glow weight their values (else the bit is cleared from rp.flags)
    bool sky_image;   // RWR_FLAG_SKY_IMAGE with RWR_FLAG_SKY in effect and an image in the context: add_sky fetches S(D) from it (else the bit is cleared from rp.flags)
    bool light_sky;   // RWR_FLAG_LIGHT_SKY with RWR_FLAG_SKY_IMAGE in effect and an image with weight: k_wf_light's SKY forms, and the GLOW forms whatever rq.glow says (else the bit is cleared from rp.flags)
    bool sobol;       // RWR_FLAG_SOBOL in a frame the wavefront integrator renders: its kernels read the bit in FrameParams::flags, beside the seed (else the bit is cleared from rp.flags)
    bool wavefront;   // the wavefront integrator renders it (several samples, a bounce, or an accumulation)
    bool dormant;     // the reference's dormant parts (single-triangle passes, orthographic rays) have their own plain kernel
    bool tonemap;     // RWR_FLAG_TONEMAP: the tone-mapping stage runs last, behind the filter (AUX implied, this bit cleared)
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

// frame_request.cpp: a render call, validated and planned
int validate(rwr_context *ctx, const rwr_camera_inv_uniform *camera, const rwr_render_params *params, uint32_t row_begin, uint32_t row_end, uint32_t row_pitch, FrameRequest &rq);
int plan_accumulation(rwr_context *ctx, const rwr_camera_inv_uniform &cam, const FrameRequest &rq, AccumPlan &ap);
void plan_reprojection(rwr_context *ctx, FrameRequest &rq, ReprojectPlan &pp);
RpCamera reproject_camera(const rwr_camera_inv_uniform &cam);
FrameKernel choose_kernel(const rwr_context *ctx, const FrameRequest &rq, const FrameConsts &fc);
bool small_culled_frame(const rwr_context *ctx, const FrameRequest &rq, FrameKernel kernel);

// frame_records.cpp: what both frame kinds put ahead of their kernels — k_frame_setup, the ray plane, the bins
inline const float4 *tex0_of(const rwr_context *ctx) { return ctx->d_texs.empty() ? nullptr : ctx->d_texs[0].ptr; }
int frame_tables(rwr_context *ctx, FrameSlot &sl, FrameParams &fp, FrameSetupOut &so);
hipError_t launch_records(rwr_context *ctx, FrameSlot &sl, const FrameConsts &fc, const FrameSetupOut &so, bool captured = false, bool *kept = nullptr);
bool ray_plane_step(rwr_context *ctx, FrameSlot &sl, const FrameParams &fp, RayPlane &plane);
int enqueue_records(rwr_context *ctx, FrameSlot &sl, FrameKernel kernel, FrameConsts &fc, const FrameSetupOut &so, FrameTiming &timing, bool *kept = nullptr);

// render_reference.cpp: the reference frame, one sample per pixel and no bounce (check_fused_frame: rwr_context.h)
int enqueue_reference(rwr_context *ctx, FrameSlot &sl, const FrameRequest &rq, FrameKernel kernel, FrameConsts &fc, const Targets &tg, FrameTiming &timing);

// render_wavefront.cpp: a frame of the wavefront integrator
int enqueue_wavefront(rwr_context *ctx, FrameSlot &sl, const FrameRequest &rq, AccumPlan &ap, ReprojectPlan &pp, FrameConsts &fc, const Targets &tg, FrameTiming &timing);

}  // namespace rwr
