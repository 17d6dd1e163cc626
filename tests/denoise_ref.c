/* CPU reference of the a-trous denoiser (RWR_FLAG_DENOISE; include/rwr_hip.h) for the tests: the definition, literally.
 *
 * It includes the oracle for its vector routines and its rgba8 store, so that the face normals are the oracle's own
 * normalize(cross(p1 - p0, p2 - p0)) of the faces as wound, under instances the oracle's own mat4_mul_v4 of the corners.
 *
 *   c0 = the colour plane handed in.  For i = 0 ... N-1, step s = 2^i, every pixel p:
 *     id(p) = -1: c(i+1)(p) = c(i)(p).  Otherwise, over the taps (dx, dy) in {-2 ... 2}^2, dy outer, q = p + s (dx, dy) inside the
 *     frame, with g(p, q) = 1:  sum += (h w) c(i)(q),  norm += h w;  c(i+1)(p).rgb = sum / norm; alpha stays c0's.
 *     h = k[|dx|] k[|dy|], k = {3/8, 1/4, 1/16};  w = 1 / (1 + d2 inv_i), d2 = (dr dr + dg dg) + db db, inv_0 = 1 / (sigma sigma),
 *     inv_(i+1) = 4 inv_i;  g = 0 for id(q) = -1, 1 for id(q) = id(p), for two faces: dot3(nhat p, nhat q) >= normal_cos_min and
 *     fabsf(t(p) - t(q)) <= depth_rel * fminf(t(p), t(q)); 0 otherwise.
 * Built with the oracle's flags (-ffp-contract=off: every operation rounds once). */
#include "../oracle/rt_oracle.c"

/* nhat of every face the kernels see: faces of instance 0, then instance 1, ... (no instances: the mesh once); out: 3 floats each */
OR_API void dr_face_normals(const OrVertex *verts, const OrFace *faces, uint32_t n_faces,
                            const OrInstance *instances, uint32_t n_instances, float *out)
{
    const uint32_t copies = n_instances ? n_instances : 1u;
    for (uint32_t k = 0; k < copies; k++) {
        for (uint32_t i = 0; i < n_faces; i++) {
            v3 p[3];
            for (int c = 0; c < 3; c++) {
                const float *v = verts[faces[i].indices[c]].position;
                p[c] = v3_from(v);
                if (n_instances) {
                    v4 h = {v[0], v[1], v[2], 1.0f};
                    v4 q = mat4_mul_v4(instances[k].model, h);
                    p[c] = V3(q.x, q.y, q.z);
                }
            }
            v3 n = normalize3(cross3(sub3(p[1], p[0]), sub3(p[2], p[0])));
            float *o = out + 3u * ((size_t)k * n_faces + i);
            o[0] = n.x; o[1] = n.y; o[2] = n.z;
        }
    }
}

static inline int dr_same_surface(int32_t idp, int32_t idq, float tp, float tq, const float *nhat, float cos_min, float depth_rel)
{
    if (idq == -1) return 0;
    if (idq == idp) return 1;
    if (idp < 0 || idq < 0) return 0;
    v3 np = v3_from(nhat + 3u * (size_t)idp), nq = v3_from(nhat + 3u * (size_t)idq);
    return dot3(np, nq) >= cos_min && fabsf(tp - tq) <= depth_rel * fminf(tp, tq);
}

/* color_in / color_out: W*H*4 floats (may not alias); color_u8: W*H*4 bytes or NULL; nhat: dr_face_normals' array.  0, or -1 when
 * out of memory. */
OR_API int dr_denoise(uint32_t W, uint32_t H, const float *color_in, const int32_t *obj_id, const float *hit_t, const float *nhat,
                      uint32_t iterations, float sigma_color, float normal_cos_min, float depth_rel, float *color_out, uint8_t *color_u8)
{
    static const float kern[3] = {0.375f, 0.25f, 0.0625f};
    const size_t n = (size_t)W * H;
    float *a = (float *)malloc(n * 4u * sizeof(float)), *b = (float *)malloc(n * 4u * sizeof(float));
    if (!a || !b) { free(a); free(b); return -1; }
    memcpy(a, color_in, n * 4u * sizeof(float));
    float inv = 1.0f / (sigma_color * sigma_color);
    for (uint32_t i = 0; i < iterations; i++) {
        const int s = 1 << i;
#pragma omp parallel for schedule(static)
        for (int y = 0; y < (int)H; y++) {
            for (int x = 0; x < (int)W; x++) {
                const size_t p = (size_t)y * W + (size_t)x;
                const float *cp = a + 4u * p;
                float *o = b + 4u * p;
                o[3] = cp[3];
                if (obj_id[p] == -1) { o[0] = cp[0]; o[1] = cp[1]; o[2] = cp[2]; continue; }
                float sum[3] = {0.0f, 0.0f, 0.0f}, norm = 0.0f;
                for (int dy = -2; dy <= 2; dy++) {
                    for (int dx = -2; dx <= 2; dx++) {
                        const int qx = x + s * dx, qy = y + s * dy;
                        if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)H) continue;
                        const size_t q = (size_t)qy * W + (size_t)qx;
                        if (!dr_same_surface(obj_id[p], obj_id[q], hit_t[p], hit_t[q], nhat, normal_cos_min, depth_rel)) continue;
                        const float *cq = a + 4u * q;
                        const float h = kern[abs(dx)] * kern[abs(dy)];
                        const float dr = cp[0] - cq[0], dg = cp[1] - cq[1], db = cp[2] - cq[2];
                        const float d2 = (dr * dr + dg * dg) + db * db;
                        const float w = 1.0f / (1.0f + d2 * inv);
                        const float hw = h * w;
                        sum[0] += hw * cq[0]; sum[1] += hw * cq[1]; sum[2] += hw * cq[2];
                        norm += hw;
                    }
                }
                o[0] = sum[0] / norm; o[1] = sum[1] / norm; o[2] = sum[2] / norm;
            }
        }
        float *tmp = a; a = b; b = tmp;
        inv = inv * 4.0f;
    }
    memcpy(color_out, a, n * 4u * sizeof(float));
    if (color_u8)
        for (size_t k = 0; k < n * 4u; k++) color_u8[k] = unorm8(a[k]);
    free(a); free(b);
    return 0;
}
