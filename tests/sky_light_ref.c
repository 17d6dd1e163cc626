/* CPU reference of the light rays aimed at the sky's image (RWR_FLAG_LIGHT_SKY; include/rwr_hip.h) for the tests.
 *
 * mis_ref.c's path loop (which it includes unchanged, and with it the whole stack down to the oracle; sky_image_ref.c for S_img)
 * with the flag's items, evaluated literally:
 *   - item 1, the table: sky_light_table (double sums, each cdf entry rounded once);
 *   - items 2 and 3: the sky is the last of the L = M + P + 1 lights; its lane draws row, column, point and direction (sl_draw);
 *   - item 4: sl_g, the one factor for both sides; no sample where !(P > 0) or !(n . omega > 0);
 *   - item 5: the light ray reaches when scene_nearest finds nothing; the term is T.c * (S_img(omega).c * g), m(g) under `mis`;
 *   - item 6: the miss of a diffuse ray adds no sky term, or T.c * (S_img(D).c * m(g')) under `mis` (all of S where !(P > 0)).
 * sky_rgb == NULL: this is mis_render_path operation for operation.  With an image the sky is the image's (RWR_FLAG_SKY with
 * RWR_FLAG_SKY_IMAGE; sky_zenith_horizon is not read), with or without sky_light.  sky_out (may be NULL): [0] light rays aimed at the
 * image, [1] those that reached it, [2] misses of diffuse rays silenced or weighted, [3] sky lanes that took no sample because !(P > 0) after the round trip, [4] sky
 * light terms at or above the cap of 64, [5] the weighted misses whose weight is not zero. */
#include "mis_ref.c"
#include "sky_image_ref.c"

/* item 1.  table: n + n * n floats (row cdf, then the rows' conditional cdfs).  Returns W. */
OR_API double sky_light_table(const float *rgb, uint32_t n, float *table)
{
    const size_t N = n;
    double *w = (double *)malloc(N * N * sizeof(double)), *row = (double *)malloc(N * sizeof(double));
    double W = 0.0;
    if (!w || !row) { free(w); free(row); return -1.0; }
    for (size_t j = 0; j < N; j++) {
        row[j] = 0.0;
        for (size_t i = 0; i < N; i++) {
            double b = 0.0;
            for (int dj = -1; dj <= 1; dj++)
                for (int di = -1; di <= 1; di++) {
                    long jj = (long)j + dj, ii = (long)i + di;
                    jj = jj < 0 ? 0 : jj > (long)N - 1 ? (long)N - 1 : jj;
                    ii = ii < 0 ? 0 : ii > (long)N - 1 ? (long)N - 1 : ii;
                    const float *t = rgb + 3u * ((size_t)jj * N + (size_t)ii);
                    b += ((double)t[0] + (double)t[1]) + (double)t[2];
                }
            const double u = ((double)i + 0.5) / (double)n, v = ((double)j + 0.5) / (double)n;
            double px = 2.0 * u - 1.0, pz = 2.0 * v - 1.0;
            const double py = (1.0 - fabs(px)) - fabs(pz);
            if (py < 0.0) {
                const double qx = (1.0 - fabs(pz)) * copysign(1.0, px), qz = (1.0 - fabs(px)) * copysign(1.0, pz);
                px = qx; pz = qz;
            }
            const double l2 = (px * px + py * py) + pz * pz;
            w[j * N + i] = b * (1.0 / (l2 * sqrt(l2)));
            row[j] += w[j * N + i];
        }
        W += row[j];
    }
    for (size_t k = 0; k < N + N * N; k++) table[k] = 1.0f;
    if (W > 0.0) {
        size_t last_row = 0;
        for (size_t j = 0; j < N; j++) if (row[j] > 0.0) last_row = j;
        double run = 0.0;
        for (size_t j = 0; j < last_row; j++) { run += row[j]; table[j] = (float)(run / W); }
        for (size_t j = 0; j < N; j++) {
            if (!(row[j] > 0.0)) continue;
            size_t last = 0;
            for (size_t i = 0; i < N; i++) if (w[j * N + i] > 0.0) last = i;
            double r = 0.0;
            for (size_t i = 0; i < last; i++) { r += w[j * N + i]; table[N + j * N + i] = (float)(r / row[j]); }
        }
    }
    free(w); free(row);
    return W;
}

/* a float coordinate's texel, as the kernels' saturating conversion gives it */
static uint32_t sl_texel(float x, uint32_t n)
{
    if (!(x >= 0.0f)) return 0u;
    if (x >= (float)n) return n - 1u;
    const uint32_t t = (uint32_t)x;
    return t > n - 1u ? n - 1u : t;
}

/* item 3: the draw from four uniforms; tex = {column, row} */
static v3 sl_draw(const float *table, uint32_t n, const float u4[4], uint32_t tex[2])
{
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (u4[0] < table[mid]) hi = mid; else lo = mid + 1u;
    }
    const uint32_t j = lo;
    const float *Cj = table + n + (size_t)j * n;
    lo = 0u; hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (u4[1] < Cj[mid]) hi = mid; else lo = mid + 1u;
    }
    const uint32_t i = lo;
    const float fn = (float)n;
    const float u = ((float)i + u4[2]) / fn, v = ((float)j + u4[3]) / fn;
    float px = 2.0f * u - 1.0f, pz = 2.0f * v - 1.0f;
    const float py = (1.0f - fabsf(px)) - fabsf(pz);
    if (py < 0.0f) {
        const float qx = (1.0f - fabsf(pz)) * copysignf(1.0f, px), qz = (1.0f - fabsf(px)) * copysignf(1.0f, pz);
        px = qx; pz = qz;
    }
    const float len = sqrtf((px * px + py * py) + pz * pz);
    tex[0] = i; tex[1] = j;
    return V3(px / len, py / len, pz / len);
}

/* item 4: the factor of the unit direction w; tex = {column, row} of the texel w maps to, *P its probability */
static float sl_g(const float *table, uint32_t n, v3 w, float ndw, uint32_t L, uint32_t tex[2], float *P)
{
    const float d[3] = {w.x, w.y, w.z};
    const float a = (fabsf(w.x) + fabsf(w.y)) + fabsf(w.z);
    float uv[2];
    sky_image_ref_uv(d, uv);
    const float fn = (float)n;
    const uint32_t i = sl_texel(uv[0] * fn, n), j = sl_texel(uv[1] * fn, n);
    const float *Cj = table + n + (size_t)j * n;
    const float r1 = table[j], r0 = j ? table[j - 1u] : 0.0f;
    const float c1 = Cj[i], c0 = i ? Cj[i - 1u] : 0.0f;
    *P = (r1 - r0) * (c1 - c0);
    tex[0] = i; tex[1] = j;
    return ((((float)L * ndw) * 0.318309886f) * (4.0f * ((a * a) * a))) / ((fn * fn) * *P);
}

/* The draw and the factor for `count` four-tuples against the normal nrm among L lights: out[12 k ...] = {omega (3), the drawn
 * texel's column and row, the texel omega maps back to (column, row; as floats: exact below 2^24), P, g, ndw, 0, 0}. */
OR_API void sky_light_samples(const float *table, uint32_t n, const float *u4, size_t count, const float *nrm, uint32_t L, float *out)
{
    for (size_t k = 0; k < count; k++) {
        uint32_t td[2], tf[2];
        const v3 w = sl_draw(table, n, u4 + 4u * k, td);
        const float ndw = dot3(V3(nrm[0], nrm[1], nrm[2]), w);
        float P;
        const float g = sl_g(table, n, w, ndw, L, tf, &P);
        float *o = out + 12u * k;
        o[0] = w.x; o[1] = w.y; o[2] = w.z; o[3] = (float)td[0]; o[4] = (float)td[1]; o[5] = (float)tf[0]; o[6] = (float)tf[1];
        o[7] = P; o[8] = g; o[9] = ndw; o[10] = 0.0f; o[11] = 0.0f;
    }
}

static v3 sl_image(const float *rgb, uint32_t n, v3 d)
{
    const float dir[3] = {d.x, d.y, d.z};
    float out[3];
    sky_image_ref_radiance(rgb, n, dir, 1u, out);
    return V3(out[0], out[1], out[2]);
}

/* mis_render_path's arguments, plus the image (sky_rgb: n * n * 3 floats, NULL: none), the flag and sky_out (may be NULL). */
OR_API int sky_light_render_path(const OrCameraInvUniform *cam, const OrScreen *screen, const OrRenderParams *params,
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
                             uint64_t *glow_by_surface_out, int light, uint64_t *light_out, float *sample_out, float *hit_out,
                             int parts, uint64_t *part_out, uint64_t *light_capped_out,
                             int mis, uint64_t *mis_out,
                             const float *sky_rgb, uint32_t sky_n, int sky_light, uint64_t *sky_out)
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
    /* item 1: the emitting spheres in use, s_0 < ... < s_{M-1}; effective with RWR_FLAG_EMISSIVE's rule on and a bounce */
    uint32_t lights[OR_EM_SPHERES], M = 0;
    if (glow)
        for (uint32_t i = 0; i < n_spheres && i < OR_EM_SPHERES; i++)
            if (em_emits(glow + 4u * (n_materials + i))) lights[M++] = i;
    const int light_on = light && glow_on && max_bounces >= 1u && M > 0u;
    uint64_t lt_rays[OR_MAX_GEN] = {0}, lt_reached[OR_MAX_GEN] = {0}, lt_silenced[OR_MAX_GEN] = {0};
    uint64_t pl_rays[OR_MAX_GEN] = {0}, pl_reached[OR_MAX_GEN] = {0}, pl_silenced[OR_MAX_GEN] = {0}, lt_capped = 0;
    if (max_bounces >= OR_MAX_GEN) { free(wverts); free(wfaces); free(texs); free(nmaps); return -2; }
    /* items 1-3: the mesh light; effective with RWR_FLAG_EMISSIVE's rule on, a bounce and a list that is not empty */
    PlRec *table = NULL;
    uint32_t n_listed = 0;
    if (parts && glow_on && max_bounces >= 1u) {
        n_listed = pl_build_table(&sc.mesh, n_materials, glow, NULL, 0u);
        if (n_listed) {
            table = (PlRec *)malloc((size_t)n_listed * sizeof(PlRec));
            if (!table) { free(wverts); free(wfaces); free(texs); free(nmaps); return -1; }
            pl_build_table(&sc.mesh, n_materials, glow, table, n_listed);
        }
    }
    const int parts_on = n_listed > 0u;
    if (!light_on) M = 0u;
    /* RWR_FLAG_LIGHT_SKY items 1 and 7: effective with the image in effect (a bounce) and W > 0 */
    float *sky_table = NULL;
    int sky_on = 0;
    if (sky_rgb && sky_light && max_bounces >= 1u) {
        sky_table = (float *)malloc(((size_t)sky_n + (size_t)sky_n * sky_n) * sizeof(float));
        if (!sky_table) { free(wverts); free(wfaces); free(texs); free(nmaps); free(table); return -1; }
        sky_on = sky_light_table(sky_rgb, sky_n, sky_table) > 0.0;
    }
    const uint32_t Ln = M + (parts_on ? 1u : 0u) + (sky_on ? 1u : 0u);
    /* item 1: effective while one of the three light flags is */
    const int mis_on = mis && (light_on || parts_on || sky_on);
    uint64_t sl_rays = 0, sl_reached = 0, sl_quiet = 0, sl_dropped = 0, sl_capped = 0, sl_weighted = 0;
    /* item 5: inv_pdf per part - every listed face of a part stores the same f32 */
    float part_inv_pdf[EM_MAX_SURFACES] = {0.0f};
    for (uint32_t j = 0; j < n_listed; j++) part_inv_pdf[em_surface(n_materials, &sc.mesh, (int32_t)table[j].face)] = table[j].inv_pdf;
    uint64_t w_sphere = 0, w_face = 0, w_inside = 0, w_nonzero = 0;
    SkyParams skyp;
    const SkyParams *sky = NULL;
    if (sky_zenith_horizon) { memcpy(&skyp, sky_zenith_horizon, sizeof skyp); sky = &skyp; }

#pragma omp parallel for schedule(dynamic, 2) reduction(+ : rays, shadow_rays, occluded, sky_terms, changed_lit, changed_dark, ev_refl, ev_trans, ev_tir, multi, deep, gen_mirror[:OR_MAX_GEN], gen_rays[:OR_MAX_GEN], gen_glass[:OR_MAX_GEN], gen_gloss[:OR_MAX_GEN], gen_glow[:OR_MAX_GEN], lt_rays[:OR_MAX_GEN], lt_reached[:OR_MAX_GEN], lt_silenced[:OR_MAX_GEN], pl_rays[:OR_MAX_GEN], pl_reached[:OR_MAX_GEN], pl_silenced[:OR_MAX_GEN], lt_capped, w_sphere, w_face, w_inside, w_nonzero, sl_rays, sl_reached, sl_quiet, sl_dropped, sl_capped, sl_weighted, glow_surf[:EM_MAX_SURFACES], glow_occluded, capped0, capped1)
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
                    int diffuse_ray = 0;   /* ray k is the cosine-distributed bounce ray: its hit h_(k-1) is eligible (item 2) */
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
                        diffuse_ray = 1;
                    }
                    if (thr_unorm16) thr = V3(unorm16_round(thr.x), unorm16_round(thr.y), unorm16_round(thr.z));
                    uint32_t li = 0u;   /* item 5: which of the L lights */
                    if (Ln && diffuse_ray) {
                        const float u = rng_uniform(pixel, s, 274u + 17u * (k - 1u), params->seed);
                        li = (uint32_t)(u * (float)Ln);
                        if (li > Ln - 1u) li = Ln - 1u;
                    }
                    if (sky_on && diffuse_ray && li == Ln - 1u) {   /* RWR_FLAG_LIGHT_SKY items 3-5: the sky lane (the sky is the last of the L) */
                        const uint32_t d = 274u + 17u * (k - 1u);
                        const v3 n = win.normal;
                        const float u4[4] = {rng_uniform(pixel, s, d + 1u, params->seed), rng_uniform(pixel, s, d + 2u, params->seed),
                                             rng_uniform(pixel, s, d + 3u, params->seed), rng_uniform(pixel, s, d + 4u, params->seed)};
                        uint32_t td[2], tf[2];
                        Ray lr;
                        lr.origin = br.origin;
                        lr.direction = sl_draw(sky_table, sky_n, u4, td);
                        const float ndw = dot3(n, lr.direction);
                        float P;
                        const float g = sl_g(sky_table, sky_n, lr.direction, ndw, Ln, tf, &P);
                        if (P > 0.0f && ndw > 0.0f) {
                            lt_rays[k - 1u]++; sl_rays++;
                            HitRecord lh;
                            const int32_t got = scene_nearest(&sc, lr, &lh);
                            if (sample_out) {
                                float *m = sample_out + (((size_t)idx * spp + s) * max_bounces + (k - 1u)) * 4u;
                                m[0] = lr.direction.x; m[1] = lr.direction.y; m[2] = lr.direction.z; m[3] = g;
                            }
                            if (got == -1) {
                                const v3 S = sl_image(sky_rgb, sky_n, lr.direction);
                                lt_reached[k - 1u]++; sl_reached++;
                                const float gw = mis_on ? mis_m(g) : g;
                                const float tr = thr.x * (S.x * gw), tg = thr.y * (S.y * gw), tb = thr.z * (S.z * gw);
                                sl_capped += (uint64_t)(tr >= OR_PATH_E1_CAP || tg >= OR_PATH_E1_CAP || tb >= OR_PATH_E1_CAP);
                                lt_capped += (uint64_t)(tr >= OR_PATH_E1_CAP || tg >= OR_PATH_E1_CAP || tb >= OR_PATH_E1_CAP);
                                acc[0] += term_clamp(tr, OR_PATH_E1_CAP); acc[1] += term_clamp(tg, OR_PATH_E1_CAP); acc[2] += term_clamp(tb, OR_PATH_E1_CAP);
                            }
                        } else sl_dropped += (uint64_t)!(P > 0.0f);   /* (a direction below the surface is no ray either, and not counted) */
                    } else if (parts_on && diffuse_ray && li == M) {   /* item 6: the face sample */
                        const uint32_t d = 274u + 17u * (k - 1u);
                        const v3 O = br.origin, n = win.normal;
                        const float uf = rng_uniform(pixel, s, d + 1u, params->seed);
                        uint32_t lo = 0u, hi = n_listed - 1u;
                        while (lo < hi) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (uf < table[mid].cdf) hi = mid; else lo = mid + 1u;
                        }
                        const uint32_t fi = table[lo].face;
                        const float inv_pdf = table[lo].inv_pdf;
                        float u1 = rng_uniform(pixel, s, d + 2u, params->seed), u2 = rng_uniform(pixel, s, d + 3u, params->seed);
                        if (u1 + u2 > 1.0f) { u1 = 1.0f - u1; u2 = 1.0f - u2; }
                        const OrFace *fc = &sc.mesh.faces[fi];
                        const v3 p0 = v3_from(sc.mesh.verts[fc->indices[0]].position), p1 = v3_from(sc.mesh.verts[fc->indices[1]].position),
                                 p2 = v3_from(sc.mesh.verts[fc->indices[2]].position);
                        const v3 P = V3((p0.x + u1 * (p1.x - p0.x)) + u2 * (p2.x - p0.x), (p0.y + u1 * (p1.y - p0.y)) + u2 * (p2.y - p0.y),
                                        (p0.z + u1 * (p1.z - p0.z)) + u2 * (p2.z - p0.z));
                        const v3 v = V3(P.x - O.x, P.y - O.y, P.z - O.z);
                        const float d2 = dot3(v, v);
                        if (d2 > 0.0f) {
                            const float dl = sqrtf(d2);
                            Ray lr;
                            lr.origin = O;
                            lr.direction = V3(v.x / dl, v.y / dl, v.z / dl);
                            const float ndw = dot3(n, lr.direction);
                            if (ndw > 0.0f) {
                                lt_rays[k - 1u]++; pl_rays[k - 1u]++;
                                const v3 Nf = normalize3(cross3(sub3(p1, p0), sub3(p2, p0)));
                                const float cf = fabsf(dot3(Nf, lr.direction));
                                const float g = (float)Ln * inv_pdf * ndw * cf * 0.318309886f / d2;
                                HitRecord lh;
                                const int32_t got = scene_nearest(&sc, lr, &lh);
                                if (sample_out) {
                                    float *m = sample_out + (((size_t)idx * spp + s) * max_bounces + (k - 1u)) * 4u;
                                    m[0] = lr.direction.x; m[1] = lr.direction.y; m[2] = lr.direction.z; m[3] = g;
                                }
                                if (got == (int32_t)fi) {
                                    const float *le = glow + 4u * em_surface(n_materials, &sc.mesh, (int32_t)fi);
                                    lt_reached[k - 1u]++; pl_reached[k - 1u]++;
                                    const float gw = mis_on ? mis_m(g) : g;   /* item 4 */
                                    const float tr = thr.x * (le[0] * gw), tg = thr.y * (le[1] * gw), tb = thr.z * (le[2] * gw);
                                    lt_capped += (uint64_t)(tr >= OR_PATH_E1_CAP || tg >= OR_PATH_E1_CAP || tb >= OR_PATH_E1_CAP);
                                    acc[0] += term_clamp(tr, OR_PATH_E1_CAP); acc[1] += term_clamp(tg, OR_PATH_E1_CAP); acc[2] += term_clamp(tb, OR_PATH_E1_CAP);
                                }
                            }
                        }
                    } else if (light_on && diffuse_ray) {   /* RWR_FLAG_LIGHT_SAMPLING's item 3, L in M's place: the light sample of hit h_(k-1) */
                        const uint32_t d = 274u + 17u * (k - 1u);
                        const v3 O = br.origin, n = win.normal;
                        const uint32_t i = li;
                        const uint32_t si = lights[i];
                        const v3 Cc = v3_from(spheres[si].center);
                        const float R = spheres[si].radius;
                        v3 w = V3(Cc.x - O.x, Cc.y - O.y, Cc.z - O.z);
                        const float d2 = dot3(w, w);
                        float *hrec = hit_out ? hit_out + (((size_t)idx * spp + s) * max_bounces + (k - 1u)) * 8u : NULL;
                        if (hrec) { hrec[0] = O.x; hrec[1] = O.y; hrec[2] = O.z; hrec[3] = n.x; hrec[4] = n.y; hrec[5] = n.z; hrec[6] = 1.0f; }
                        if (d2 > R * R) {
                            const float dl = sqrtf(d2);
                            w = V3(w.x / dl, w.y / dl, w.z / dl);
                            const float s2 = R * R / d2;
                            const float cmax = sqrtf(fmaxf(0.0f, 1.0f - s2));
                            const float kc = s2 / (1.0f + cmax);
                            float a = 0.0f, b = 0.0f;
                            for (uint32_t j = 0; j < 8u; j++) {
                                float ua = 2.0f * rng_uniform(pixel, s, d + 1u + 2u * j, params->seed) - 1.0f;
                                float ub = 2.0f * rng_uniform(pixel, s, d + 2u + 2u * j, params->seed) - 1.0f;
                                if (ua * ua + ub * ub <= 1.0f) { a = ua; b = ub; break; }
                            }
                            const float q = a * a + b * b;
                            const float c = 1.0f - q * kc;
                            const float r = q > 0.0f ? sqrtf(fmaxf(0.0f, 1.0f - c * c) / q) : 0.0f;
                            const float sign = copysignf(1.0f, w.z);
                            const float aa = -1.0f / (sign + w.z);
                            const float bb = w.x * w.y * aa;
                            const v3 b1 = V3(1.0f + sign * w.x * w.x * aa, sign * bb, -sign * w.x);
                            const v3 b2 = V3(bb, sign + w.y * w.y * aa, -w.y);
                            Ray lr;
                            lr.origin = O;
                            lr.direction = V3(r * (a * b1.x + b * b2.x) + c * w.x, r * (a * b1.y + b * b2.y) + c * w.y, r * (a * b1.z + b * b2.z) + c * w.z);
                            const float ndw = dot3(n, lr.direction);
                            if (hrec) hrec[6] = ndw > 0.0f ? 3.0f : 2.0f;
                            if (ndw > 0.0f) {
                                lt_rays[k - 1u]++;
                                HitRecord lh;
                                const int32_t got = scene_nearest(&sc, lr, &lh);
                                const float g = 2.0f * (float)Ln * kc * ndw;
                                if (sample_out) {
                                    float *m = sample_out + (((size_t)idx * spp + s) * max_bounces + (k - 1u)) * 4u;
                                    m[0] = lr.direction.x; m[1] = lr.direction.y; m[2] = lr.direction.z; m[3] = g;
                                }
                                if (got == -2 - (int32_t)si) {
                                    const float *le = glow + 4u * (n_materials + si);
                                    lt_reached[k - 1u]++;
                                    const float gw = mis_on ? mis_m(g) : g;   /* item 4 */
                                    lt_capped += (uint64_t)(thr.x * (le[0] * gw) >= OR_PATH_E1_CAP || thr.y * (le[1] * gw) >= OR_PATH_E1_CAP || thr.z * (le[2] * gw) >= OR_PATH_E1_CAP);
                                    acc[0] += term_clamp(thr.x * (le[0] * gw), OR_PATH_E1_CAP); acc[1] += term_clamp(thr.y * (le[1] * gw), OR_PATH_E1_CAP);
                                    acc[2] += term_clamp(thr.z * (le[2] * gw), OR_PATH_E1_CAP);
                                }
                            }
                        }
                    }
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
                    if (idk == -1 && sky_rgb) {   /* RWR_FLAG_SKY_IMAGE's term, under RWR_FLAG_LIGHT_SKY's item 6 */
                        v3 sk = sl_image(sky_rgb, sky_n, br.direction);
                        if (sky_on && diffuse_ray) {
                            float mw = 0.0f;
                            int quiet = 1;
                            if (mis_on) {
                                uint32_t tf[2];
                                float P;
                                const float gp = sl_g(sky_table, sky_n, br.direction, dot3(win.normal, br.direction), Ln, tf, &P);
                                mw = mis_m(gp);
                                if (!(P > 0.0f)) { mw = 1.0f; quiet = 0; }
                            }
                            sk = V3(sk.x * mw, sk.y * mw, sk.z * mw);
                            if (quiet) { sl_quiet++; lt_silenced[k]++; sl_weighted += (uint64_t)(mw != 0.0f); }
                        }
                        acc[0] += term_clamp(thr.x * sk.x, OR_PATH_E1_CAP); acc[1] += term_clamp(thr.y * sk.y, OR_PATH_E1_CAP);
                        acc[2] += term_clamp(thr.z * sk.z, OR_PATH_E1_CAP);
                        sky_terms++;
                        break;
                    }
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
                        static const float kDark[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                        float lw[4] = {0.0f, 0.0f, 0.0f, 0.0f};   /* item 5: Le m(g') */
                        float gp = 0.0f;
                        int weighted = 0;
                        const float nd = dot3(win.normal, br.direction);   /* n: the normal of the hit that sent the ray (win is still that hit) */
                        if (light_on && diffuse_ray && idk < -1 && em_emits(le)) {   /* item 4: O's light sample has this light already */
                            const v3 Cc = v3_from(spheres[-2 - idk].center);
                            const float R = spheres[-2 - idk].radius;
                            const v3 w = V3(Cc.x - br.origin.x, Cc.y - br.origin.y, Cc.z - br.origin.z);
                            const float d2 = dot3(w, w);
                            if (d2 > R * R) {
                                lt_silenced[k]++;
                                if (mis_on) {
                                    const float s2 = R * R / d2;
                                    const float cmax = sqrtf(fmaxf(0.0f, 1.0f - s2));
                                    const float kc = s2 / (1.0f + cmax);
                                    gp = 2.0f * (float)Ln * kc * nd;
                                    weighted = 1; w_sphere++;
                                } else le = kDark;
                            } else w_inside++;
                        }
                        if (parts_on && diffuse_ray && idk >= 0 && em_emits(le)) {   /* item 8 */
                            lt_silenced[k]++; pl_silenced[k]++;
                            if (mis_on) {
                                const OrFace *fc = &sc.mesh.faces[idk];
                                const v3 p0 = v3_from(sc.mesh.verts[fc->indices[0]].position), p1 = v3_from(sc.mesh.verts[fc->indices[1]].position),
                                         p2 = v3_from(sc.mesh.verts[fc->indices[2]].position);
                                const v3 Nf = normalize3(cross3(sub3(p1, p0), sub3(p2, p0)));
                                const float cf = fabsf(dot3(Nf, br.direction));
                                const float d2 = h.distance * h.distance;
                                gp = (float)Ln * part_inv_pdf[si] * nd * cf * 0.318309886f / d2;
                                weighted = 1; w_face++;
                            } else le = kDark;
                        }
                        if (weighted) {
                            const float m = mis_m(gp);
                            lw[0] = le[0] * m; lw[1] = le[1] * m; lw[2] = le[2] * m;
                            le = lw;
                            w_nonzero += (uint64_t)em_emits(le);
                        }
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
    free(wverts); free(wfaces); free(texs); free(nmaps); free(table); free(sky_table);
    if (sky_out) { sky_out[0] = sl_rays; sky_out[1] = sl_reached; sky_out[2] = sl_quiet; sky_out[3] = sl_dropped; sky_out[4] = sl_capped; sky_out[5] = sl_weighted; }
    if (rays_out) *rays_out = rays;
    if (light_capped_out) *light_capped_out = lt_capped;
    if (mis_out) { mis_out[0] = w_sphere; mis_out[1] = w_face; mis_out[2] = w_inside; mis_out[3] = w_nonzero; }
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
        if (light_out) { light_out[3u * k] = lt_rays[k]; light_out[3u * k + 1u] = lt_reached[k]; light_out[3u * k + 2u] = lt_silenced[k]; }
        if (part_out) { part_out[3u * k] = pl_rays[k]; part_out[3u * k + 1u] = pl_reached[k]; part_out[3u * k + 2u] = pl_silenced[k]; }
    }
    if (glow_occluded_out) *glow_occluded_out = glow_occluded;
    if (capped_out) { capped_out[0] = capped0; capped_out[1] = capped1; }
    if (glow_by_surface_out)
        for (uint32_t i = 0; i < n_materials + OR_EM_SPHERES; i++) glow_by_surface_out[i] = glow_surf[i];
    return 0;
}
