/* CPU reference of emissive surfaces (RWR_FLAG_EMISSIVE; include/rwr_hip.h) for the tests.
 *
 * soft_shadow_ref.c's path loop (which it includes unchanged, and with it gloss_ref.c, glass_ref.c, mirror_ref.c, sky_ref.c,
 * shadow_ref.c, path_ref.c and the oracle: every intersection, shading and scattering routine is theirs) with the emission table:
 * `glow` holds {r, g, b, 0} per part, then per sphere index (OR_EM_SPHERES of them), the layout of the surface table.  While a
 * part of the scene or one of its spheres in use emits, the local shading of every hit h the loop shades becomes, in f32 with no
 * contraction,
 *     E'(h) = E(h) + Le(h)            per channel, one add to the value the shader produced;
 *     E'(h) = ambient(h) + Le(h)      where the hit's shadow ray is occluded: a surface's own light is never shadowed;
 * and term k is term_clamp(T(k-1) * E'(h_k)) with the caps of ever ([0, 16] at h0, [0, 64] later) - the sum first, then the product
 * with T, then the clamp.  Both sides of a face emit, a sphere inwards as well as outwards: the table is read by the surface's id
 * alone.  A frame with an emitter takes the integrator's clamped form also at spp 1 without a bounce.  Rays, throughputs, RNG
 * dimensions, nearest hits and every count of soft_render_path are untouched: with glow == NULL, or with no emitter in the scene,
 * this is soft_render_path operation for operation.
 * For the tests: gen_glow_out[k] = shaded hits of generation k (0: h0) on a surface with Le != 0; glow_occluded_out = those whose
 * shadow ray was occluded; capped_out = {terms that reached their cap at h0, at k >= 1} (counted while the rule applies, on any
 * surface); glow_by_surface_out[record] = emitting hits by table record. */
#include "soft_shadow_ref.c"

#define OR_EM_SPHERES 8u         /* RWR_MAX_SPHERES */
#define EM_MAX_SURFACES 72u      /* table records the per-surface counts hold: up to 64 parts and the spheres */

static inline int em_emits(const float *le) { return le[0] != 0.0f || le[1] != 0.0f || le[2] != 0.0f; }

/* the table record of the surface `id` (a face index, or -2 - sphere): mirror_of's indexing */
static inline uint32_t em_surface(uint32_t n_materials, const Mesh *m, int32_t id)
{
    if (id < 0) return n_materials + (uint32_t)(-2 - id);
    return m->face_material ? m->face_material[(uint32_t)id % m->n_base_faces] : 0u;
}

/* soft_render_path's arguments, plus the emission table (NULL: nothing emits) and the counts above (each may be NULL). */
OR_API int emission_render_path(const OrCameraInvUniform *cam, const OrScreen *screen, const OrRenderParams *params,
                             const OrSphere *spheres, uint32_t n_spheres,
                             const OrVertex *verts, uint32_t n_verts, const OrFace *faces, uint32_t n_faces,
                             const OrInstance *instances, uint32_t n_instances,
                             const OrMaterial *materials, uint32_t n_materials, const uint32_t *face_material,
                             const uint8_t *const *tex_ptrs, const uint32_t *tex_ws, const uint32_t *tex_hs,
                             const uint8_t *const *nmap_ptrs, const uint32_t *nmap_ws, const uint32_t *nmap_hs,
                             uint32_t row_begin, uint32_t row_end,
                             uint8_t *color_u8, float *depth_out, float *color_f32, int32_t *obj_id, float *hit_t, uint64_t *rays_out,
                             int shadows, uint64_t *shadow_rays_out, uint64_t *occluded_out, uint8_t *occl0_out,
                             const float *sky_zenith_horizon, uint64_t *sky_terms_out, float *miss_out,
                             const float *mirrors, uint64_t *gen_mirror_out, uint64_t *gen_rays_out, float *first_out,
                             uint64_t *events_out, uint64_t *multi_out, uint64_t *deep_out, uint64_t *gen_glass_out, int thr_unorm16,
                             uint64_t *gen_gloss_out, const float *radii, uint64_t *changed_out, uint32_t *prim_out,
                             const float *glow, uint64_t *gen_glow_out, uint64_t *glow_occluded_out, uint64_t *capped_out,
                             uint64_t *glow_by_surface_out)
{
    /* scene set-up: render_path_core's */
    const OrMaterial *material = materials;
    const uint8_t *tex_rgba8 = n_materials ? tex_ptrs[0] : NULL;
    const uint32_t tex_w = n_materials ? tex_ws[0] : 0u, tex_h = n_materials ? tex_hs[0] : 0u;
    Tex *texs = (Tex *)calloc(n_materials ? n_materials : 1u, sizeof(Tex));
    if (!texs) return -1;
    Tex *nmaps = (Tex *)calloc(n_materials ? n_materials : 1u, sizeof(Tex));
    if (!nmaps) { free(texs); return -1; }
    for (uint32_t k = 0; k < n_materials; k++) {
        texs[k].rgba = tex_ptrs[k]; texs[k].w = tex_ws[k]; texs[k].h = tex_hs[k];
        build_srgb_lut(texs[k].lut);
        if (nmap_ptrs && nmap_ptrs[k] && nmap_ws[k] && nmap_hs[k]) { nmaps[k].rgba = nmap_ptrs[k]; nmaps[k].w = nmap_ws[k]; nmaps[k].h = nmap_hs[k]; }
    }
    const uint32_t W = screen->width, H = screen->height;
    if (row_end > H) row_end = H;
    OrVertex *wverts = NULL; OrFace *wfaces = NULL;
    Scene sc;
    sc.spheres = spheres; sc.n_spheres = n_spheres;
    sc.mesh.material = material;
    sc.mesh.tex.rgba = tex_rgba8; sc.mesh.tex.w = tex_w; sc.mesh.tex.h = tex_h;
    build_srgb_lut(sc.mesh.tex.lut);
    sc.mesh.face_material = (n_materials > 1) ? face_material : NULL;
    sc.mesh.n_base_faces = n_faces ? n_faces : 1u;
    sc.mesh.materials = materials;
    sc.mesh.texs = texs;
    sc.mesh.nmaps = nmaps;
    sc.mesh.use_nmap = (params->flags & OR_FLAG_NORMAL_MAP) != 0u;
    if (n_instances && n_faces) {
        wverts = (OrVertex *)malloc((size_t)n_verts * n_instances * sizeof(OrVertex));
        wfaces = (OrFace *)malloc((size_t)n_faces * n_instances * sizeof(OrFace));
        if (!wverts || !wfaces) { free(wverts); free(wfaces); free(texs); free(nmaps); return -1; }
        for (uint32_t k = 0; k < n_instances; k++) {
            for (uint32_t i = 0; i < n_verts; i++) {
                OrVertex v = verts[i];
                v4 p = {v.position[0], v.position[1], v.position[2], 1.0f};
                v4 q = mat4_mul_v4(instances[k].model, p);
                v.position[0] = q.x; v.position[1] = q.y; v.position[2] = q.z;
                wverts[(size_t)k * n_verts + i] = v;
            }
            for (uint32_t i = 0; i < n_faces; i++) {
                OrFace f = faces[i];
                f.indices[0] += k * n_verts; f.indices[1] += k * n_verts; f.indices[2] += k * n_verts;
                wfaces[(size_t)k * n_faces + i] = f;
            }
        }
        sc.mesh.verts = wverts; sc.mesh.n_verts = n_verts * n_instances;
        sc.mesh.faces = wfaces; sc.mesh.n_faces = n_faces * n_instances;
    } else {
        sc.mesh.verts = verts; sc.mesh.n_verts = n_verts; sc.mesh.faces = faces; sc.mesh.n_faces = n_faces;
    }
    const uint32_t spp = params->spp ? params->spp : 1u;
    const uint32_t max_bounces = params->max_bounces;
    const int bounce = max_bounces >= 1;
    uint64_t rays = 0, shadow_rays = 0, occluded = 0, sky_terms = 0;
    uint64_t gen_mirror[OR_MAX_GEN] = {0}, gen_rays[OR_MAX_GEN] = {0};
    uint64_t ev_refl = 0, ev_trans = 0, ev_tir = 0, multi = 0, deep = 0;
    uint64_t gen_glass[OR_MAX_GEN] = {0};
    uint64_t gen_gloss[OR_MAX_GEN] = {0};
    uint64_t changed_lit = 0, changed_dark = 0;
    uint64_t gen_glow[OR_MAX_GEN] = {0}, glow_surf[EM_MAX_SURFACES] = {0};
    uint64_t glow_occluded = 0, capped0 = 0, capped1 = 0;
    if (n_materials + OR_EM_SPHERES > EM_MAX_SURFACES) { free(texs); free(nmaps); return -2; }
    /* the rule applies when a surface of the scene emits: a part, or a sphere that is in use */
    int glow_on = 0;
    if (glow) {
        for (uint32_t i = 0; i < n_materials; i++) glow_on |= em_emits(glow + 4u * i);
        for (uint32_t i = 0; i < n_spheres; i++) glow_on |= em_emits(glow + 4u * (n_materials + i));
    }
    if (max_bounces >= OR_MAX_GEN) { free(wverts); free(wfaces); free(texs); free(nmaps); return -2; }
    SkyParams skyp;
    const SkyParams *sky = NULL;
    if (sky_zenith_horizon) { memcpy(&skyp, sky_zenith_horizon, sizeof skyp); sky = &skyp; }

#pragma omp parallel for schedule(dynamic, 2) reduction(+ : rays, shadow_rays, occluded, sky_terms, changed_lit, changed_dark, ev_refl, ev_trans, ev_tir, multi, deep, gen_mirror[:OR_MAX_GEN], gen_rays[:OR_MAX_GEN], gen_glass[:OR_MAX_GEN], gen_gloss[:OR_MAX_GEN], gen_glow[:OR_MAX_GEN], glow_surf[:EM_MAX_SURFACES], glow_occluded, capped0, capped1)
    for (int y = (int)row_begin; y < (int)row_end; y++) {
        for (uint32_t x = 0; x < W; x++) {
            const uint32_t pixel = (uint32_t)y * W + x;
            const size_t idx = (size_t)pixel;
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            float depth0 = 0.0f, t0 = 0.0f;
            int32_t id0 = -1;
            for (uint32_t s = 0; s < spp; s++) {
                float jx = 0.5f, jy = 0.5f;
                if (spp > 1) {
                    jx = rng_uniform(pixel, s, 0u, params->seed);
                    jy = rng_uniform(pixel, s, 1u, params->seed);
                }
                Ray ray = pixel_to_ray(cam, screen, x, (uint32_t)y, jx, jy);
                float depth_tex = 0.0f;
                int32_t id = -1;
                HitRecord win = kNoHit;
                for (uint32_t k = 0; k < n_spheres; k++) {
                    HitRecord h = sphere_ray_intersect(v3_from(spheres[k].center), spheres[k].radius, ray);
                    if (!h.hit) continue;
                    float current_depth = 1.0f - depth_tex;
                    float depth = to_non_linear_depth(h.distance);
                    if (depth >= current_depth) continue;
                    depth_tex = 1.0f - depth; id = -2 - (int32_t)k; win = h;
                }
                if (sc.mesh.n_faces) {
                    int i_min;
                    HitRecord h = mesh_nearest(&sc.mesh, ray, &i_min);
                    if (h.hit) {
                        float current_depth = 1.0f - depth_tex;
                        float depth = to_non_linear_depth(h.distance);
                        if (!(depth >= current_depth)) { depth_tex = 1.0f - depth; id = i_min; win = h; }
                    }
                }
                if (s == 0) { depth0 = depth_tex; id0 = id; t0 = win.hit ? win.distance : 0.0f; }
                if (id == -1) continue;
                v3 thr, thr_prev = V3(1.0f, 1.0f, 1.0f);
                v3 e0 = shade_any(&sc, id, &win, ray, &thr);
                int occ0 = 0;
                if (shadows) {
                    shadow_rays++;
                    int hard = 0;
                    const int occ = shadows == 2 ? 1 : radii ? ss_occluded(&sc, id, &win, ray, pixel, s, 0u, params->seed, radii, changed_out ? &hard : NULL)
                                                             : sr_occluded(&sc, id, &win, ray);
                    if (shadows != 2 && radii && changed_out) { changed_lit += (uint64_t)(hard && !occ); changed_dark += (uint64_t)(!hard && occ); }
                    if (prim_out) { prim_out[2 * idx]++; prim_out[2 * idx + 1] += (uint32_t)!occ; }
                    if (occ) {
                        occluded++; e0 = sr_ambient(&sc, id);
                        if (s == 0 && occl0_out) occl0_out[idx] = 1;
                    }
                    occ0 = occ;
                }
                if (glow_on) {   /* E'(h0) = E(h0) + Le(h0), or ambient(h0) + Le(h0): one f32 add per channel */
                    const uint32_t si = em_surface(n_materials, &sc.mesh, id);
                    const float *le = glow + 4u * si;
                    e0 = V3(e0.x + le[0], e0.y + le[1], e0.z + le[2]);
                    if (em_emits(le)) { gen_glow[0]++; glow_surf[si]++; glow_occluded += (uint64_t)occ0; }
                    capped0 += (uint64_t)(e0.x >= OR_PATH_E0_CAP || e0.y >= OR_PATH_E0_CAP || e0.z >= OR_PATH_E0_CAP);
                }
                if (spp != 1 || bounce || shadows || glow_on) {
                    acc[0] += term_clamp(e0.x, OR_PATH_E0_CAP); acc[1] += term_clamp(e0.y, OR_PATH_E0_CAP); acc[2] += term_clamp(e0.z, OR_PATH_E0_CAP);
                } else {
                    acc[0] += e0.x; acc[1] += e0.y; acc[2] += e0.z;
                }
                acc[3] += 2.0f;
                /* the path: (ray, win) is the last segment and its hit, `id` the surface it lies on */
                int32_t idh = id;
                int first_done = 0;
                uint32_t n_trans = 0;
                for (uint32_t k = 1; k <= max_bounces; k++) {
                    v3 P = madd3(win.distance, ray.direction, ray.origin);
                    Ray br;
                    br.origin = V3(P.x + win.normal.x * 1e-4f, P.y + win.normal.y * 1e-4f, P.z + win.normal.z * 1e-4f);
                    const float *mrec = mirror_of(mirrors, n_materials, &sc.mesh, idh);
                    const float *grec = NULL;
                    const float *srec = NULL;
                    if (mrec && mrec[3] < 0.0f) { grec = mrec; mrec = NULL; }
                    else if (mrec && mrec[3] > 1.0f) { srec = mrec; mrec = NULL; }
                    if (grec) {
                        GlassOut g = glass_scatter(win.normal, ray.direction, idh >= 0, idh >= 0 ? face_entering_of(&sc.mesh, idh, ray) : 0, -grec[3],
                                                   pixel, s, 2u + 16u * (k - 1u), params->seed);
                        br.direction = g.dir;
                        br.origin = V3(P.x + g.side.x * 1e-4f, P.y + g.side.y * 1e-4f, P.z + g.side.z * 1e-4f);
                        thr = (k == 1u) ? V3(grec[0], grec[1], grec[2]) : V3(thr_prev.x * grec[0], thr_prev.y * grec[1], thr_prev.z * grec[2]);
                        if (g.event == 0) ev_refl++; else if (g.event == 1) { ev_trans++; if (++n_trans == 2u) multi++; if (n_trans == 4u) deep++; } else ev_tir++;
                        gen_glass[k]++;
                    } else if (srec) {
                        br.direction = gloss_scatter(win.normal, ray.direction, srec[3] - 1.0f, pixel, s, 2u + 16u * (k - 1u), params->seed);
                        thr = (k == 1u) ? V3(srec[0], srec[1], srec[2]) : V3(thr_prev.x * srec[0], thr_prev.y * srec[1], thr_prev.z * srec[2]);
                        gen_gloss[k]++;
                    } else if (mrec) {
                        float d = dot3(win.normal, ray.direction);
                        float two_d = 2.0f * d;
                        br.direction = V3(ray.direction.x - two_d * win.normal.x, ray.direction.y - two_d * win.normal.y,
                                          ray.direction.z - two_d * win.normal.z);
                        /* T(k-1) = T(k-2) * R in place of T(k-2) * albedo(h): thr_prev is T(k-2), the throughput the hit was reached
                           with (kept below, before the albedo goes in); T(0) = R */
                        thr = (k == 1u) ? V3(mrec[0], mrec[1], mrec[2]) : V3(thr_prev.x * mrec[0], thr_prev.y * mrec[1], thr_prev.z * mrec[2]);
                        gen_mirror[k]++;
                    } else {
                        br.direction = pr_bounce_direction_dim(win.normal, pixel, s, params->seed, 2u + 16u * (k - 1u));
                    }
                    if (thr_unorm16) thr = V3(unorm16_round(thr.x), unorm16_round(thr.y), unorm16_round(thr.z));
                    rays++;
                    gen_rays[k]++;
                    HitRecord h;
                    int32_t idk = scene_nearest(&sc, br, &h);
                    if (mrec && !first_done && first_out) {
                        float *m = first_out + ((size_t)idx * spp + s) * 8u;
                        m[0] = br.direction.x; m[1] = br.direction.y; m[2] = br.direction.z;
                        m[3] = thr.x; m[4] = thr.y; m[5] = thr.z; m[6] = idk == -1 ? 0.0f : idk >= 0 ? 1.0f : 2.0f; m[7] = (float)k;
                    }
                    if (mrec) first_done = 1;
                    if (idk == -1) {
                        if (sky) {
                            v3 sk = sky_radiance(sky, br.direction);
                            acc[0] += term_clamp(thr.x * sk.x, OR_PATH_E1_CAP); acc[1] += term_clamp(thr.y * sk.y, OR_PATH_E1_CAP);
                            acc[2] += term_clamp(thr.z * sk.z, OR_PATH_E1_CAP);
                            sky_terms++;
                            if (miss_out) {
                                float *m = miss_out + ((size_t)idx * spp + s) * 8u;
                                m[0] = br.direction.x; m[1] = br.direction.y; m[2] = br.direction.z;
                                m[3] = thr.x; m[4] = thr.y; m[5] = thr.z; m[6] = (float)k; m[7] = 1.0f;
                            }
                        }
                        break;
                    }
                    v3 albedo;
                    v3 ek = shade_any(&sc, idk, &h, br, &albedo);
                    int occk = 0;
                    if (shadows) {
                        shadow_rays++;
                        int hard = 0;
                        const int occ = shadows == 2 ? 1 : radii ? ss_occluded(&sc, idk, &h, br, pixel, s, k, params->seed, radii, changed_out ? &hard : NULL)
                                                                 : sr_occluded(&sc, idk, &h, br);
                        if (shadows != 2 && radii && changed_out) { changed_lit += (uint64_t)(hard && !occ); changed_dark += (uint64_t)(!hard && occ); }
                        if (occ) { occluded++; ek = sr_ambient(&sc, idk); }
                        occk = occ;
                    }
                    if (glow_on) {   /* E'(h_k) = E(h_k) + Le(h_k); the term is T(k-1) * E'(h_k): the sum first, then the product */
                        const uint32_t si = em_surface(n_materials, &sc.mesh, idk);
                        const float *le = glow + 4u * si;
                        ek = V3(ek.x + le[0], ek.y + le[1], ek.z + le[2]);
                        if (em_emits(le)) { gen_glow[k]++; glow_surf[si]++; glow_occluded += (uint64_t)occk; }
                        capped1 += (uint64_t)(thr.x * ek.x >= OR_PATH_E1_CAP || thr.y * ek.y >= OR_PATH_E1_CAP || thr.z * ek.z >= OR_PATH_E1_CAP);
                    }
                    acc[0] += term_clamp(thr.x * ek.x, OR_PATH_E1_CAP); acc[1] += term_clamp(thr.y * ek.y, OR_PATH_E1_CAP);
                    acc[2] += term_clamp(thr.z * ek.z, OR_PATH_E1_CAP);
                    thr_prev = thr;
                    thr = V3(thr.x * albedo.x, thr.y * albedo.y, thr.z * albedo.z);
                    ray = br;
                    win = h;
                    idh = idk;
                }
            }
            const float fs = (float)spp;
            v3 rgb = V3(acc[0] / fs, acc[1] / fs, acc[2] / fs);
            float alpha = acc[3] / fs;
            if (depth_out) depth_out[idx] = depth0;
            if (color_u8) {
                color_u8[4 * idx + 0] = unorm8(rgb.x); color_u8[4 * idx + 1] = unorm8(rgb.y);
                color_u8[4 * idx + 2] = unorm8(rgb.z); color_u8[4 * idx + 3] = unorm8(alpha);
            }
            if (color_f32) {
                color_f32[4 * idx + 0] = rgb.x; color_f32[4 * idx + 1] = rgb.y;
                color_f32[4 * idx + 2] = rgb.z; color_f32[4 * idx + 3] = alpha;
            }
            if (obj_id) obj_id[idx] = id0;
            if (hit_t) hit_t[idx] = t0;
        }
    }
    free(wverts); free(wfaces); free(texs); free(nmaps);
    if (rays_out) *rays_out = rays;
    if (shadow_rays_out) *shadow_rays_out = shadow_rays;
    if (occluded_out) *occluded_out = occluded;
    if (sky_terms_out) *sky_terms_out = sky_terms;
    if (events_out) { events_out[0] = ev_refl; events_out[1] = ev_trans; events_out[2] = ev_tir; }
    if (multi_out) *multi_out = multi;
    if (deep_out) *deep_out = deep;
    if (changed_out) { changed_out[0] = changed_lit; changed_out[1] = changed_dark; }
    for (uint32_t k = 0; k <= max_bounces; k++) {
        if (gen_mirror_out) gen_mirror_out[k] = gen_mirror[k];
        if (gen_rays_out) gen_rays_out[k] = gen_rays[k];
        if (gen_glass_out) gen_glass_out[k] = gen_glass[k];
        if (gen_gloss_out) gen_gloss_out[k] = gen_gloss[k];
        if (gen_glow_out) gen_glow_out[k] = gen_glow[k];
    }
    if (glow_occluded_out) *glow_occluded_out = glow_occluded;
    if (capped_out) { capped_out[0] = capped0; capped_out[1] = capped1; }
    if (glow_by_surface_out)
        for (uint32_t i = 0; i < n_materials + OR_EM_SPHERES; i++) glow_by_surface_out[i] = glow_surf[i];
    return 0;
}
