// The scene behind the C ABI: staging, upload, the world-space records and the BVH.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh.hpp"
#include "rwr_context.h"

namespace rwr {

int rebuild_tris(rwr_context *ctx)
{
    if (!ctx->tris_dirty) return RWR_OK;
    const uint32_t total = (uint32_t)instanced_faces(ctx->n_faces, ctx->n_instances);
    RWR_HIP_CHECK(ctx->d_tris.ensure(total));
    RWR_HIP_CHECK(ctx->d_shade.ensure(total));
    RWR_HIP_CHECK(ctx->d_cull.ensure(total));
    RWR_HIP_CHECK(ctx->d_tangent.ensure(total));
    RWR_HIP_CHECK(launch_prebake(ctx->stream, ctx->d_verts.ptr, ctx->d_faces.ptr, ctx->d_face_mat.ptr, ctx->n_faces, ctx->d_instances.ptr,
                                 ctx->n_instances, ctx->d_materials.ptr, ctx->d_tris.ptr, ctx->d_shade.ptr, ctx->d_cull.ptr,
                                 ctx->d_tangent.ptr));
    // BVH for incoherent rays, built on the host from the device's own world-space corners
    // (so instancing arithmetic happens in exactly one place, k_prebake)
    std::vector<CullRec> host_cull(total);
    RWR_HIP_CHECK(hipMemcpyAsync(host_cull.data(), ctx->d_cull.ptr, (size_t)total * sizeof(CullRec), hipMemcpyDeviceToHost, ctx->stream));
    RWR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    std::vector<float> corners((size_t)total * 9);
    for (uint32_t i = 0; i < total; i++) {
        std::memcpy(&corners[9 * (size_t)i + 0], host_cull[i].p0, 12);
        std::memcpy(&corners[9 * (size_t)i + 3], host_cull[i].p1, 12);
        std::memcpy(&corners[9 * (size_t)i + 6], host_cull[i].p2, 12);
    }
    for (int k = 0; k < 3; k++) { ctx->aabb_lo[k] = INFINITY; ctx->aabb_hi[k] = -INFINITY; }
    for (size_t v = 0; v < (size_t)total * 3; v++)
        for (int k = 0; k < 3; k++) {
            ctx->aabb_lo[k] = std::fmin(ctx->aabb_lo[k], corners[3 * v + k]);
            ctx->aabb_hi[k] = std::fmax(ctx->aabb_hi[k], corners[3 * v + k]);
        }
    uint32_t max_leaf = kBvhMaxLeafDefault;
    if (const char *e = std::getenv("RWR_BVH_LEAF")) max_leaf = (uint32_t)std::strtoul(e, nullptr, 10);  // tuning knob
    const Bvh bvh = build_bvh(corners.data(), total, max_leaf);
    if (bvh.max_depth > kBvhMaxDepth)
        return set_error(RWR_ERR_UNSUPPORTED, "the scene's BVH is %u levels deep (limit %u): too many faces for the traversal stacks",
                         bvh.max_depth, kBvhMaxDepth);
    RWR_HIP_CHECK(ctx->d_bvh_nodes.ensure(bvh.nodes.size()));
    RWR_HIP_CHECK(ctx->d_bvh_leaf_faces.ensure(bvh.leaf_faces.size() ? bvh.leaf_faces.size() : 1));
    RWR_HIP_CHECK(hipMemcpy(ctx->d_bvh_nodes.ptr, bvh.nodes.data(), bvh.nodes.size() * sizeof(BvhNode4), hipMemcpyHostToDevice));
    if (!bvh.leaf_faces.empty())
        RWR_HIP_CHECK(hipMemcpy(ctx->d_bvh_leaf_faces.ptr, bvh.leaf_faces.data(), bvh.leaf_faces.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    ctx->bvh_n_nodes = (uint32_t)bvh.nodes.size();
    ctx->bvh_depth = bvh.max_depth;
    ctx->bvh_leaf_extent = bvh.mean_leaf_extent;
    ctx->n_tris = total;
    ctx->tris_dirty = false;
    ctx->world_corners = std::move(corners);   // (the mesh light's areas: scene_part_lights)
    ctx->part_lights_dirty = true;
    return RWR_OK;
}

// RWR_FLAG_LIGHT_PARTS item 1: the mesh light changes with the world faces (rebuild_tris) and with a part's emission (set_glow); the
// frame that next asks for the flag rebuilds the list from the corners the device made and uploads it, behind the frames in flight.
int scene_part_lights(rwr_context *ctx, uint32_t &n)
{
    if (ctx->part_lights_dirty) {
        if (ctx->n_tris != 0u && ctx->world_corners.size() == (size_t)ctx->n_tris * 9u && ctx->n_faces != 0u)
            ctx->part_lights = build_part_lights(ctx->world_corners.data(), ctx->n_tris, ctx->st_face_mat.data(), ctx->n_faces,
                                                 &ctx->part_glow.data()->r, (uint32_t)ctx->part_glow.size());
        else
            ctx->part_lights.clear();
        if (!ctx->part_lights.empty()) {
            DeviceGuard g(ctx->device);
            RWR_HIP_CHECK(sync_all(ctx));
            RWR_HIP_CHECK(ctx->d_part_lights.ensure(ctx->part_lights.size()));
            RWR_HIP_CHECK(hipMemcpy(ctx->d_part_lights.ptr, ctx->part_lights.data(), ctx->part_lights.size() * sizeof(PartLightRec), hipMemcpyHostToDevice));
        }
        // RWR_FLAG_LIGHT_MIS item 5: a part's inv_pdf (every listed face of a part stores the same f32) rides in the spare component of
        // its record of the emission table; when one changed, a WfState's copy is refreshed like any other change of that table (a
        // rebuild that leaves them all as they were — the common one under RWR_FLAG_LIGHT_PARTS alone is not: W moves — costs nothing)
        std::vector<float> inv_pdf(ctx->part_glow.size(), 0.0f);
        for (const PartLightRec &r : ctx->part_lights) {
            const uint32_t part = ctx->st_face_mat[r.face % ctx->n_faces];
            if (part < inv_pdf.size()) inv_pdf[part] = r.inv_pdf;
        }
        if (inv_pdf != ctx->part_inv_pdf) {
            ctx->part_inv_pdf = std::move(inv_pdf);
            ctx->glow_version++;
        }
        ctx->part_lights_dirty = false;
    }
    n = (uint32_t)ctx->part_lights.size();
    return RWR_OK;
}

}  // namespace rwr

using namespace rwr;

extern "C" {

int rwr_scene_clear(rwr_context *ctx)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ctx->scene_generation++;
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(sync_all(ctx));
    ctx->st_verts.clear(); ctx->st_faces.clear(); ctx->st_face_mat.clear(); ctx->st_materials.clear();
    ctx->d_texs.clear(); ctx->d_quads.clear(); ctx->d_nmaps.clear();
    ctx->part_surfaces.clear();   // (a new scene: its parts are no mirrors; the sphere attributes are kept per index)
    ctx->surface_version++;
    ctx->part_glow.clear();       // (... and give off no light)
    ctx->glow_version++;
    ctx->world_corners.clear();
    ctx->part_lights_dirty = true;
    ctx->have_mesh = false;
    ctx->n_faces = ctx->n_verts = ctx->n_tris = 0;
    return RWR_OK;
}

int rwr_scene_add_mesh(rwr_context *ctx, const rwr_model_vertex_small *verts, uint32_t n_verts,
                       const rwr_model_face_small *faces, uint32_t n_faces, const rwr_material_data *material,
                       const uint8_t *rgba8_srgb, uint32_t tex_w, uint32_t tex_h)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ctx->scene_generation++;
    if (n_faces == 0) return RWR_OK;  // nothing to add
    if (!verts || !faces || !material || !rgba8_srgb)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL mesh array with n_faces = %u", n_faces);
    if (n_verts == 0 || tex_w == 0 || tex_h == 0)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "empty vertex array or texture with n_faces = %u", n_faces);
    if (tex_w > kMaxTextureDim || tex_h > kMaxTextureDim)  // byte offsets of the taps are 32-bit (rwr_device.h)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "texture %ux%u larger than %ux%u", tex_w, tex_h, kMaxTextureDim, kMaxTextureDim);
    // The shader indexes vertice_list unchecked (compute.wgsl:191-193); an
    // out-of-range index would be a GPU fault here, so it is rejected up front.
    for (uint32_t f = 0; f < n_faces; f++)
        for (int k = 0; k < 3; k++)
            if (faces[f].indices[k] >= n_verts)
                return set_error(RWR_ERR_INVALID_ARGUMENT, "face %u index %u out of range (n_verts %u)", f, faces[f].indices[k], n_verts);
    const uint64_t total_faces = (uint64_t)ctx->st_faces.size() + n_faces;
    if (instanced_faces(total_faces, ctx->n_instances) > 0x7fffffffull || (uint64_t)ctx->st_verts.size() + n_verts > 0xffffffffull)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "too many faces or vertices");
    DeviceGuard g(ctx->device);
    // texture -> linear float4 on the device
    ctx->d_texs.emplace_back();
    DeviceBuffer<float4> &tex = ctx->d_texs.back();
    hipError_t e = tex.ensure((size_t)tex_w * tex_h);
    if (e == hipSuccess) {
        float lut[256];
        build_srgb_lut(lut);
        std::vector<float4> lin((size_t)tex_w * tex_h);
        for (size_t i = 0; i < lin.size(); i++)
            lin[i] = make_float4(lut[rgba8_srgb[4 * i]], lut[rgba8_srgb[4 * i + 1]], lut[rgba8_srgb[4 * i + 2]],
                                 (float)rgba8_srgb[4 * i + 3] / 255.0f);  // alpha is linear in sRGB formats
        e = hipMemcpy(tex.ptr, lin.data(), lin.size() * sizeof(float4), hipMemcpyHostToDevice);
    }
    // ... and as quad records (the frame kernel's form)
    ctx->d_quads.emplace_back();
    DeviceBuffer<uint4> &quad = ctx->d_quads.back();
    if (e == hipSuccess) e = quad.ensure((size_t)(tex_w + 1u) * (tex_h + 1u));
    if (e == hipSuccess) {
        std::vector<uint4> q((size_t)(tex_w + 1u) * (tex_h + 1u));
        build_tex_quads(rgba8_srgb, tex_w, tex_h, reinterpret_cast<uint32_t *>(q.data()));
        e = hipMemcpy(quad.ptr, q.data(), q.size() * sizeof(uint4), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        ctx->d_texs.pop_back();
        ctx->d_quads.pop_back();
        return set_error(RWR_ERR_HIP, "texture upload failed: %s", hipGetErrorString(e));
    }
    const uint32_t vbase = (uint32_t)ctx->st_verts.size(), mid = (uint32_t)ctx->st_materials.size();
    ctx->st_verts.insert(ctx->st_verts.end(), verts, verts + n_verts);
    for (uint32_t f = 0; f < n_faces; f++) {
        rwr_model_face_small fc = faces[f];
        fc.indices[0] += vbase; fc.indices[1] += vbase; fc.indices[2] += vbase;
        ctx->st_faces.push_back(fc);
        ctx->st_face_mat.push_back(mid);
    }
    MaterialRec M{};
    for (int k = 0; k < 3; k++) { M.ambient[k] = material->ambient[k]; M.specular[k] = material->specular[k]; }
    M.tex_w = tex_w; M.tex_h = tex_h; M.tex = tex.ptr;
    M.wmax = (float)(tex_w - 1u); M.hmax = (float)(tex_h - 1u);
    M.nmap = nullptr; M.nmap_w = M.nmap_h = 0u;
    ctx->st_materials.push_back(M);
    ctx->d_nmaps.emplace_back();
    ctx->part_surfaces.push_back(kDiffuseRec);
    ctx->surface_version++;
    ctx->part_glow.push_back(kDiffuseRec);
    ctx->glow_version++;
    if (mid == 0) ctx->material = *material;
    return RWR_OK;
}

int rwr_scene_commit(rwr_context *ctx)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ctx->scene_generation++;
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(sync_all(ctx));
    ctx->n_faces = (uint32_t)ctx->st_faces.size();
    ctx->n_verts = (uint32_t)ctx->st_verts.size();
    ctx->n_tris = 0;
    ctx->have_mesh = true;
    if (ctx->n_faces == 0) {
        ctx->tris_dirty = false;
        return RWR_OK;
    }
    RWR_HIP_CHECK(ctx->d_verts.ensure(ctx->n_verts));
    RWR_HIP_CHECK(ctx->d_faces.ensure(ctx->n_faces));
    RWR_HIP_CHECK(ctx->d_face_mat.ensure(ctx->n_faces));
    RWR_HIP_CHECK(ctx->d_materials.ensure(ctx->st_materials.size()));
    RWR_HIP_CHECK(hipMemcpy(ctx->d_verts.ptr, ctx->st_verts.data(), ctx->st_verts.size() * sizeof(rwr_model_vertex_small), hipMemcpyHostToDevice));
    RWR_HIP_CHECK(hipMemcpy(ctx->d_faces.ptr, ctx->st_faces.data(), ctx->st_faces.size() * sizeof(rwr_model_face_small), hipMemcpyHostToDevice));
    RWR_HIP_CHECK(hipMemcpy(ctx->d_face_mat.ptr, ctx->st_face_mat.data(), ctx->st_face_mat.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    RWR_HIP_CHECK(hipMemcpy(ctx->d_materials.ptr, ctx->st_materials.data(), ctx->st_materials.size() * sizeof(MaterialRec), hipMemcpyHostToDevice));
    {
        std::vector<const uint4 *> mq(ctx->d_quads.size());
        for (size_t i = 0; i < mq.size(); i++) mq[i] = ctx->d_quads[i].ptr;
        RWR_HIP_CHECK(ctx->d_mat_quads.ensure(mq.size()));
        RWR_HIP_CHECK(hipMemcpy(ctx->d_mat_quads.ptr, mq.data(), mq.size() * sizeof(const uint4 *), hipMemcpyHostToDevice));
    }
    ctx->tex_w = ctx->st_materials[0].tex_w;
    ctx->tex_h = ctx->st_materials[0].tex_h;
    ctx->tris_dirty = true;
    const int rc = rebuild_tris(ctx);
    if (rc != RWR_OK) return rc;
    RWR_HIP_CHECK(ensure_frame_buffers(ctx));
    return RWR_OK;
}

int rwr_scene_part_count(rwr_context *ctx, uint32_t *n_parts)
{
    if (!ctx || !n_parts) return set_error(RWR_ERR_INVALID_ARGUMENT, "NULL argument");
    *n_parts = (uint32_t)ctx->st_materials.size();
    return RWR_OK;
}

int rwr_scene_set_normal_map(rwr_context *ctx, uint32_t part, const uint8_t *rgba8_linear, uint32_t tex_w, uint32_t tex_h)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ctx->scene_generation++;
    if (part >= ctx->st_materials.size()) return set_error(RWR_ERR_INVALID_ARGUMENT, "part %u: the scene has %zu parts", part, ctx->st_materials.size());
    if (rgba8_linear && (tex_w == 0 || tex_h == 0)) return set_error(RWR_ERR_INVALID_ARGUMENT, "empty normal map");
    if (tex_w > kMaxTextureDim || tex_h > kMaxTextureDim)
        return set_error(RWR_ERR_INVALID_ARGUMENT, "normal map %ux%u larger than %ux%u", tex_w, tex_h, kMaxTextureDim, kMaxTextureDim);
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(sync_all(ctx));
    DeviceBuffer<float4> &tex = ctx->d_nmaps[part];
    MaterialRec &M = ctx->st_materials[part];
    tex.release();
    if (!rgba8_linear) {
        M.nmap = nullptr; M.nmap_w = M.nmap_h = 0u;
    } else {
        RWR_HIP_CHECK(tex.ensure((size_t)tex_w * tex_h));
        std::vector<float4> lin((size_t)tex_w * tex_h);
        for (size_t i = 0; i < lin.size(); i++)   // rgba8unorm, NOT sRGB: a normal map holds vectors
            lin[i] = make_float4((float)rgba8_linear[4 * i] / 255.0f, (float)rgba8_linear[4 * i + 1] / 255.0f,
                                 (float)rgba8_linear[4 * i + 2] / 255.0f, (float)rgba8_linear[4 * i + 3] / 255.0f);
        RWR_HIP_CHECK(hipMemcpy(tex.ptr, lin.data(), lin.size() * sizeof(float4), hipMemcpyHostToDevice));
        M.nmap = tex.ptr; M.nmap_w = tex_w; M.nmap_h = tex_h;
    }
    if (ctx->have_mesh && ctx->d_materials.ptr && ctx->d_materials.count >= ctx->st_materials.size())   // already committed: refresh the device copy
        RWR_HIP_CHECK(hipMemcpy(ctx->d_materials.ptr, ctx->st_materials.data(), ctx->st_materials.size() * sizeof(MaterialRec), hipMemcpyHostToDevice));
    return RWR_OK;
}

// The surface models (RWR_FLAG_MIRRORS, _GLASS, _GLOSSY; rwr_context.h SurfaceModel).  A part or a sphere index has one record,
// so the twelve entry points — set and get, part and sphere, three models — are one lookup, one setter and one getter.

// the record of part / sphere `index`; NULL: refused, RWR_ERR_INVALID_ARGUMENT is set
static SurfaceRec *surface_at(rwr_context *ctx, bool sphere, uint32_t index)
{
    if (!ctx) {
        set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    } else if (sphere) {
        if (index < RWR_MAX_SPHERES) return &ctx->sphere_surfaces[index];
        set_error(RWR_ERR_INVALID_ARGUMENT, "sphere %u: at most %d spheres", index, RWR_MAX_SPHERES);
    } else {
        if (index < ctx->part_surfaces.size()) return &ctx->part_surfaces[index];
        set_error(RWR_ERR_INVALID_ARGUMENT, "part %u: the scene has %zu parts", index, ctx->part_surfaces.size());
    }
    return nullptr;
}

// rgb: the mirror's or the glossy surface's reflectance, the glass's tint (NULL: the surface is none of the three); param: the
// glass's ior, the glossy surface's roughness.  The record replaces whichever attribute the surface had.
static int set_surface(rwr_context *ctx, bool sphere, uint32_t index, SurfaceModel model, const float *rgb, float param)
{
    SurfaceRec *at = surface_at(ctx, sphere, index);
    if (!at) return RWR_ERR_INVALID_ARGUMENT;
    const char *what = sphere ? "sphere" : "part";
    SurfaceRec m = kDiffuseRec;
    if (rgb) {   // (the range tests are false for NaN)
        if (model == SurfaceModel::kGlass && !(param >= kGlassIorMin && param <= kGlassIorMax))
            return set_error(RWR_ERR_INVALID_ARGUMENT, "%s %u: ior %g: finite, 1 ... 4", what, index, (double)param);
        if (model == SurfaceModel::kGloss && !(param >= kGlossRoughnessMin && param <= kGlossRoughnessMax))
            return set_error(RWR_ERR_INVALID_ARGUMENT, "%s %u: roughness %g: finite, 2^-10 ... 1", what, index, (double)param);
        for (int c = 0; c < 3; c++)
            if (!(rgb[c] >= 0.0f && rgb[c] <= 1.0f))
                return set_error(RWR_ERR_INVALID_ARGUMENT, "%s %u: %s[%d] %g: finite, 0 ... 1", what, index,
                                 model == SurfaceModel::kGlass ? "tint" : "reflectance", c, (double)rgb[c]);
        m = model == SurfaceModel::kGlass ? glass_rec(rgb, param) : model == SurfaceModel::kGloss ? gloss_rec(rgb, param) : mirror_rec(rgb);
    }
    ctx->scene_generation++;   // (a refused call never gets here: it changes nothing, the scene's generation included)
    *at = m;
    ctx->surface_version++;
    return RWR_OK;
}

// is the surface of `model`, and if so its r, g, b and its parameter (zeros if not; any of the three pointers may be NULL)
static int get_surface(rwr_context *ctx, bool sphere, uint32_t index, SurfaceModel model, int *is_model, float rgb[3], float *param)
{
    const SurfaceRec *at = surface_at(ctx, sphere, index);
    if (!at) return RWR_ERR_INVALID_ARGUMENT;
    const bool on = surface_model(*at) == model;
    const SurfaceRec m = on ? *at : kDiffuseRec;
    if (is_model) *is_model = on ? 1 : 0;
    if (rgb) { rgb[0] = m.r; rgb[1] = m.g; rgb[2] = m.b; }
    if (param) *param = surface_param(m);
    return RWR_OK;
}


int rwr_scene_set_part_mirror(rwr_context *ctx, uint32_t part, const float *reflectance) { return set_surface(ctx, false, part, SurfaceModel::kMirror, reflectance, 0.0f); }
int rwr_scene_set_sphere_mirror(rwr_context *ctx, uint32_t sphere, const float *reflectance) { return set_surface(ctx, true, sphere, SurfaceModel::kMirror, reflectance, 0.0f); }
int rwr_scene_get_part_mirror(rwr_context *ctx, uint32_t part, int *is_mirror, float reflectance[3]) { return get_surface(ctx, false, part, SurfaceModel::kMirror, is_mirror, reflectance, nullptr); }
int rwr_scene_get_sphere_mirror(rwr_context *ctx, uint32_t sphere, int *is_mirror, float reflectance[3]) { return get_surface(ctx, true, sphere, SurfaceModel::kMirror, is_mirror, reflectance, nullptr); }
int rwr_scene_set_part_glass(rwr_context *ctx, uint32_t part, float ior, const float *tint) { return set_surface(ctx, false, part, SurfaceModel::kGlass, tint, ior); }
int rwr_scene_set_sphere_glass(rwr_context *ctx, uint32_t sphere, float ior, const float *tint) { return set_surface(ctx, true, sphere, SurfaceModel::kGlass, tint, ior); }
int rwr_scene_get_part_glass(rwr_context *ctx, uint32_t part, int *is_glass, float *ior, float tint[3]) { return get_surface(ctx, false, part, SurfaceModel::kGlass, is_glass, tint, ior); }
int rwr_scene_get_sphere_glass(rwr_context *ctx, uint32_t sphere, int *is_glass, float *ior, float tint[3]) { return get_surface(ctx, true, sphere, SurfaceModel::kGlass, is_glass, tint, ior); }
int rwr_scene_set_part_gloss(rwr_context *ctx, uint32_t part, const float *reflectance, float roughness) { return set_surface(ctx, false, part, SurfaceModel::kGloss, reflectance, roughness); }
int rwr_scene_set_sphere_gloss(rwr_context *ctx, uint32_t sphere, const float *reflectance, float roughness) { return set_surface(ctx, true, sphere, SurfaceModel::kGloss, reflectance, roughness); }
int rwr_scene_get_part_gloss(rwr_context *ctx, uint32_t part, int *is_glossy, float reflectance[3], float *roughness) { return get_surface(ctx, false, part, SurfaceModel::kGloss, is_glossy, reflectance, roughness); }
int rwr_scene_get_sphere_gloss(rwr_context *ctx, uint32_t sphere, int *is_glossy, float reflectance[3], float *roughness) { return get_surface(ctx, true, sphere, SurfaceModel::kGloss, is_glossy, reflectance, roughness); }

// Emission (RWR_FLAG_EMISSIVE): an attribute beside the surface's model, with the same index rules — a record of its own per part
// and per sphere index, so that neither kind of setter touches the other's.

// RWR_FLAG_LIGHT_SAMPLING: the list of the emitting spheres in use — index below the count rwr_scene_set_spheres gave, radiance not
// zero — in index order.  Rebuilt by whatever changes it: the sphere emission setter and rwr_scene_set_spheres.
static void rebuild_lights(rwr_context *ctx)
{
    WfLights l{};
    for (uint32_t i = 0; i < ctx->n_spheres; i++)
        if (glows(ctx->sphere_glow[i])) {
            l.index[l.m] = i;
            l.le[l.m][0] = ctx->sphere_glow[i].r; l.le[l.m][1] = ctx->sphere_glow[i].g; l.le[l.m][2] = ctx->sphere_glow[i].b;
            l.m++;
        }
    ctx->lights = l;
}

// the emission record of part / sphere `index`; NULL: refused, RWR_ERR_INVALID_ARGUMENT is set
static SurfaceRec *glow_at(rwr_context *ctx, bool sphere, uint32_t index)
{
    if (!ctx) {
        set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    } else if (sphere) {
        if (index < RWR_MAX_SPHERES) return &ctx->sphere_glow[index];
        set_error(RWR_ERR_INVALID_ARGUMENT, "sphere %u: at most %d spheres", index, RWR_MAX_SPHERES);
    } else {
        if (index < ctx->part_glow.size()) return &ctx->part_glow[index];
        set_error(RWR_ERR_INVALID_ARGUMENT, "part %u: the scene has %zu parts", index, ctx->part_glow.size());
    }
    return nullptr;
}

static int set_glow(rwr_context *ctx, bool sphere, uint32_t index, const float *radiance)
{
    SurfaceRec *at = glow_at(ctx, sphere, index);
    if (!at) return RWR_ERR_INVALID_ARGUMENT;
    static_assert(kMaxEmission == RWR_MAX_EMISSION, "kMaxEmission is RWR_MAX_EMISSION");
    SurfaceRec g = kDiffuseRec;
    if (radiance) {
        for (int c = 0; c < 3; c++)   // (false for NaN)
            if (!(radiance[c] >= 0.0f && radiance[c] <= kMaxEmission))
                return set_error(RWR_ERR_INVALID_ARGUMENT, "%s %u: radiance[%d] %g: finite, 0 ... %g", sphere ? "sphere" : "part", index, c,
                                 (double)radiance[c], (double)kMaxEmission);
        g = glow_rec(radiance);
    }
    ctx->scene_generation++;   // (a refused call never gets here)
    *at = g;
    ctx->glow_version++;
    if (sphere) rebuild_lights(ctx);
    else ctx->part_lights_dirty = true;
    return RWR_OK;
}

static int get_glow(rwr_context *ctx, bool sphere, uint32_t index, int *emits, float radiance[3])
{
    const SurfaceRec *at = glow_at(ctx, sphere, index);
    if (!at) return RWR_ERR_INVALID_ARGUMENT;
    if (emits) *emits = glows(*at) ? 1 : 0;
    if (radiance) { radiance[0] = at->r; radiance[1] = at->g; radiance[2] = at->b; }
    return RWR_OK;
}

int rwr_scene_set_part_emission(rwr_context *ctx, uint32_t part, const float *radiance) { return set_glow(ctx, false, part, radiance); }
int rwr_scene_set_sphere_emission(rwr_context *ctx, uint32_t sphere, const float *radiance) { return set_glow(ctx, true, sphere, radiance); }
int rwr_scene_get_part_emission(rwr_context *ctx, uint32_t part, int *emits, float radiance[3]) { return get_glow(ctx, false, part, emits, radiance); }
int rwr_scene_get_sphere_emission(rwr_context *ctx, uint32_t sphere, int *emits, float radiance[3]) { return get_glow(ctx, true, sphere, emits, radiance); }

int rwr_scene_upload_mesh(rwr_context *ctx, const rwr_model_vertex_small *verts, uint32_t n_verts,
                          const rwr_model_face_small *faces, uint32_t n_faces, const rwr_material_data *material,
                          const uint8_t *rgba8_srgb, uint32_t tex_w, uint32_t tex_h)
{
    int rc = rwr_scene_clear(ctx);
    if (rc == RWR_OK) rc = rwr_scene_add_mesh(ctx, verts, n_verts, faces, n_faces, material, rgba8_srgb, tex_w, tex_h);
    if (rc == RWR_OK) rc = rwr_scene_commit(ctx);
    return rc;
}

int rwr_scene_set_spheres(rwr_context *ctx, const rwr_sphere_buffer_data *spheres, uint32_t n)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ctx->scene_generation++;
    if (n > RWR_MAX_SPHERES) return set_error(RWR_ERR_INVALID_ARGUMENT, "at most %d spheres", RWR_MAX_SPHERES);
    if (n && !spheres) return set_error(RWR_ERR_INVALID_ARGUMENT, "spheres is NULL");
    for (uint32_t i = 0; i < n; i++) ctx->spheres[i] = spheres[i];
    ctx->n_spheres = n;
    rebuild_lights(ctx);
    return RWR_OK;
}

int rwr_scene_set_triangles(rwr_context *ctx, const rwr_triangle_buffer_data *triangles, uint32_t n)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ctx->scene_generation++;
    if (n > RWR_MAX_TRIANGLES) return set_error(RWR_ERR_INVALID_ARGUMENT, "at most %d single triangles", RWR_MAX_TRIANGLES);
    if (n && !triangles) return set_error(RWR_ERR_INVALID_ARGUMENT, "triangles is NULL with n = %u", n);
    for (uint32_t i = 0; i < n; i++) ctx->triangles[i] = triangles[i];   // passed by value with every launch
    ctx->n_triangles = n;
    return RWR_OK;
}

int rwr_scene_set_instances(rwr_context *ctx, const rwr_instance_raw *instances, uint32_t n)
{
    if (!ctx) return set_error(RWR_ERR_INVALID_ARGUMENT, "ctx is NULL");
    ctx->scene_generation++;
    if (n && !instances) return set_error(RWR_ERR_INVALID_ARGUMENT, "instances is NULL");
    if (instanced_faces(ctx->n_faces, n) > 0x7fffffffull) return set_error(RWR_ERR_INVALID_ARGUMENT, "too many faces");
    DeviceGuard g(ctx->device);
    RWR_HIP_CHECK(sync_all(ctx));
    if (n) {
        RWR_HIP_CHECK(ctx->d_instances.ensure(n));
        RWR_HIP_CHECK(hipMemcpy(ctx->d_instances.ptr, instances, (size_t)n * sizeof *instances, hipMemcpyHostToDevice));
    }
    ctx->n_instances = n;
    if (ctx->have_mesh && ctx->n_faces) {
        ctx->tris_dirty = true;
        return rebuild_tris(ctx);
    }
    return RWR_OK;
}

}  // extern "C"
