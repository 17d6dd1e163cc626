/* CPU reference of the shadow rays (RWR_FLAG_SHADOWS; include/rwr_hip.h) for the tests.
 *
 * path_ref.c's path loop (which it includes, and with it the oracle: every intersection and shading routine is the oracle's own)
 * with E_V(h) in place of E(h):
 *   every hit h the loop shades - h0 and every bounce hit - casts one shadow ray from P + 1e-4 n (P = madd3(t, D, O), n the
 *   HitRecord's normal: the origin of the bounce ray that leaves h) towards nl = neg3(normalize3(kLightDir)), kLightDir =
 *   (1, -1, -5) for a mesh hit, (1, -5, 1) for a sphere hit;
 *   occluded(h) = any sphere has sphere_ray_intersect(...).hit or any face has triangle_ray_intersect(...).hit - brute force,
 *   no distance limit, no face excluded;
 *   E_V(h) = E(h), or when occluded its ambient part: the part's MaterialData.ambient (mesh), (0.1, 0, 0) (sphere);
 *   every term is clamped (E_V(h0) to [0, 16] also at spp 1 without a bounce).
 * With `shadows` == 0 it is pr_render_path_nm, operation for operation.  For the tests alone: `shadows` == 2 traces no shadow ray
 * and takes every hit for occluded (the ambient-only path sum, whatever the visibility routine says), and occl0_out receives
 * per pixel whether sample 0's primary hit was occluded (0 where nothing was hit). */
#include "path_ref.c"

/* the shadow ray of the hit `h` (id: >= 0 face, <= -2 sphere) of `ray`: is anything in its way? */
static inline int sr_occluded(const Scene *sc, int32_t id, const HitRecord *h, Ray ray)
{
    const v3 kLightMesh = {1.0f, -1.0f, -5.0f};   /* triangle_list/compute.wgsl:55 */
    const v3 kLightSphere = {1.0f, -5.0f, 1.0f};  /* sphere/compute.wgsl:41 */
    v3 P = madd3(h->distance, ray.direction, ray.origin);
    Ray sr;
    sr.origin = V3(P.x + h->normal.x * 1e-4f, P.y + h->normal.y * 1e-4f, P.z + h->normal.z * 1e-4f);
    sr.direction = neg3(normalize3(id >= 0 ? kLightMesh : kLightSphere));
    for (uint32_t k = 0; k < sc->n_spheres; k++)
        if (sphere_ray_intersect(v3_from(sc->spheres[k].center), sc->spheres[k].radius, sr).hit) return 1;
    const Mesh *m = &sc->mesh;
    for (uint32_t i = 0; i < m->n_faces; i++) {
        const OrFace *f = &m->faces[i];
        if (triangle_ray_intersect(v3_from(m->verts[f->indices[0]].position), v3_from(m->verts[f->indices[1]].position),
                                   v3_from(m->verts[f->indices[2]].position), sr).hit)
            return 1;
    }
    return 0;
}

/* the ambient part of E(h): shade_mesh's (ambient + 0) + 0, shade_sphere's 0.1 * mat_color + 0 */
static inline v3 sr_ambient(const Scene *sc, int32_t id)
{
    if (id < 0) return V3(0.1f, 0.0f, 0.0f);
    const Mesh *m = &sc->mesh;
    const OrMaterial *mat = m->material;
    if (m->face_material) mat = &m->materials[m->face_material[(uint32_t)id % m->n_base_faces]];
    return V3(mat->ambient[0], mat->ambient[1], mat->ambient[2]);
}

/* pr_render_path_nm's arguments, plus the switch and *shadow_rays_out / *occluded_out: the shadow rays traced and how many were occluded. */
OR_API int sr_render_path(const OrCameraInvUniform *cam, const OrScreen *screen, const OrRenderParams *params,
                             const OrSphere *spheres, uint32_t n_spheres,
                             const OrVertex *verts, uint32_t n_verts, const OrFace *faces, uint32_t n_faces,
                             const OrInstance *instances, uint32_t n_instances,
                             const OrMaterial *materials, uint32_t n_materials, const uint32_t *face_material,
                             const uint8_t *const *tex_ptrs, const uint32_t *tex_ws, const uint32_t *tex_hs,
                             const uint8_t *const *nmap_ptrs, const uint32_t *nmap_ws, const uint32_t *nmap_hs,
                             uint32_t row_begin, uint32_t row_end,
                             uint8_t *color_u8, float *depth_out, float *color_f32, int32_t *obj_id, float *hit_t, uint64_t *rays_out,
                             int shadows, uint64_t *shadow_rays_out, uint64_t *occluded_out, uint8_t *occl0_out)
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
    uint64_t rays = 0, shadow_rays = 0, occluded = 0;

#pragma omp parallel for schedule(dynamic, 2) reduction(+ : rays, shadow_rays, occluded)
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
                v3 thr;
                v3 e0 = shade_any(&sc, id, &win, ray, &thr);
                if (shadows) {
                    shadow_rays++;
                    if (shadows == 2 || sr_occluded(&sc, id, &win, ray)) {
                        occluded++; e0 = sr_ambient(&sc, id);
                        if (s == 0 && occl0_out) occl0_out[idx] = 1;
                    }
                }
                if (spp != 1 || bounce || shadows) {
                    acc[0] += term_clamp(e0.x, OR_PATH_E0_CAP); acc[1] += term_clamp(e0.y, OR_PATH_E0_CAP); acc[2] += term_clamp(e0.z, OR_PATH_E0_CAP);
                } else {
                    acc[0] += e0.x; acc[1] += e0.y; acc[2] += e0.z;
                }
                acc[3] += 2.0f;
                /* the path: (ray, win) is the last segment and its hit */
                for (uint32_t k = 1; k <= max_bounces; k++) {
                    v3 P = madd3(win.distance, ray.direction, ray.origin);
                    Ray br;
                    br.origin = V3(P.x + win.normal.x * 1e-4f, P.y + win.normal.y * 1e-4f, P.z + win.normal.z * 1e-4f);
                    br.direction = pr_bounce_direction_dim(win.normal, pixel, s, params->seed, 2u + 16u * (k - 1u));
                    rays++;
                    HitRecord h;
                    int32_t idk = scene_nearest(&sc, br, &h);
                    if (idk == -1) break;
                    v3 albedo;
                    v3 ek = shade_any(&sc, idk, &h, br, &albedo);
                    if (shadows) {
                        shadow_rays++;
                        if (shadows == 2 || sr_occluded(&sc, idk, &h, br)) { occluded++; ek = sr_ambient(&sc, idk); }
                    }
                    acc[0] += term_clamp(thr.x * ek.x, OR_PATH_E1_CAP); acc[1] += term_clamp(thr.y * ek.y, OR_PATH_E1_CAP);
                    acc[2] += term_clamp(thr.z * ek.z, OR_PATH_E1_CAP);
                    thr = V3(thr.x * albedo.x, thr.y * albedo.y, thr.z * albedo.z);
                    ray = br;
                    win = h;
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
    return 0;
}
