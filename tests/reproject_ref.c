/* CPU reference of temporal reprojection (RWR_FLAG_REPROJECT; include/rwr_hip.h) for the tests: the definition,
 * operation for operation.  It includes the oracle for pixel_to_ray, its vector routines and its rgba8 store.
 *
 * Per frame, from a camera uniform alone (rr_camera):  W(x_nds, y_nds) = pixel_to_ray's world_vec before the normalise;
 *   c0 = W(0,0), cx = W(1,0) - c0, cy = W(0,1) - c0, nrm = cross3(cx, cy), nc0 = dot3(nrm, c0), nn = dot3(nrm, nrm).
 * Per pixel p = (x, y) of a frame with a previous one (rr_frame), id = obj_id(p), t = hit_t(p):
 *   id = -1: out = c_now, n' = 0, background.  Otherwise P = madd3(t, Dc, O) on the PIXEL-CENTRE ray, d = sub3(P, o'),
 *   den = dot3(nrm', d), mu = nc0' / den; no history unless mu > 0.  r = mu d - c0',
 *   xn = dot3(cross3(r, cy'), nrm') / nn', yn = dot3(cross3(cx', r), nrm') / nn', fx = (xn + 1) 0.5 W - 0.5, fy likewise,
 *   te = sqrtf(dot3(d, d)).  Taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), x0 = floorf(fx), a = fx - x0, bilinear weights.
 *   A tap counts if it lies inside the frame (no clamping), id'(q) == id or both >= 0 and dot3(nhat[id], nhat[id'(q)]) >= cos_min,
 *   and fabsf(te - t'(q)) <= depth_rel * te.  sw += w, sc += w h(q), sn += w n(q) in tap order.
 *   Not sw > 0 (or fx / fy not finite): out = c_now, n' = 1, fresh.  Else hist = sc / sw, n' = fminf(sn / sw + 1, max_history),
 *   out = hist + (c_now - hist) / n' — and c_now itself when n' == 1; reused.  Alpha is c_now's.
 * Built with the oracle's flags (-ffp-contract=off: every operation rounds once). */
#include "../oracle/rt_oracle.c"

typedef struct { float o[3], c0[3], cx[3], cy[3], nrm[3]; float nc0, nn; } RrCamera;

static v3 rr_world_vec(const OrCameraInvUniform *cam, float x_nds, float y_nds)
{
    v4 proj_vec = {x_nds, y_nds, 1.0f, 1.0f};
    v4 view_vec = mat4_mul_v4(cam->proj_inv, proj_vec);
    view_vec.w = 0.0f;
    v4 world_vec = mat4_mul_v4(cam->viewmodel_inv, view_vec);
    return V3(world_vec.x, world_vec.y, world_vec.z);
}

static void rr_put(float *dst, v3 a) { dst[0] = a.x; dst[1] = a.y; dst[2] = a.z; }

OR_API void rr_camera(const OrCameraInvUniform *cam, RrCamera *out)
{
    v3 c0 = rr_world_vec(cam, 0.0f, 0.0f);
    v3 cx = sub3(rr_world_vec(cam, 1.0f, 0.0f), c0);
    v3 cy = sub3(rr_world_vec(cam, 0.0f, 1.0f), c0);
    v3 nrm = cross3(cx, cy);
    rr_put(out->o, v3_from(cam->origin));
    rr_put(out->c0, c0); rr_put(out->cx, cx); rr_put(out->cy, cy); rr_put(out->nrm, nrm);
    out->nc0 = dot3(nrm, c0);
    out->nn = dot3(nrm, nrm);
}

/* P of pixel (x, y) at distance t on its pixel-centre ray */
OR_API void rr_centre_point(const OrCameraInvUniform *cam, uint32_t W, uint32_t H, uint32_t x, uint32_t y, float t, float *P)
{
    OrScreen screen = {W, H};
    Ray ray = pixel_to_ray(cam, &screen, x, y, 0.5f, 0.5f);
    rr_put(P, madd3(t, ray.direction, ray.origin));
}

/* where P lands in the frame of camera `prev`: 1 and (fx, fy, te) when mu > 0, else 0 */
static int rr_project_point(const RrCamera *prev, v3 P, float W, float H, float *fx, float *fy, float *te)
{
    v3 nrm = v3_from(prev->nrm);
    v3 d = sub3(P, v3_from(prev->o));
    float den = dot3(nrm, d);
    float mu = prev->nc0 / den;
    if (!(mu > 0.0f)) return 0;
    v3 r = V3(mu * d.x - prev->c0[0], mu * d.y - prev->c0[1], mu * d.z - prev->c0[2]);
    float xn = dot3(cross3(r, v3_from(prev->cy)), nrm) / prev->nn;
    float yn = dot3(cross3(v3_from(prev->cx), r), nrm) / prev->nn;
    *fx = (xn + 1.0f) * 0.5f * W - 0.5f;
    *fy = (yn + 1.0f) * 0.5f * H - 0.5f;
    *te = sqrtf(dot3(d, d));
    return 1;
}

OR_API int rr_project(const RrCamera *prev, const float *P, uint32_t W, uint32_t H, float *fx_fy_te)
{
    return rr_project_point(prev, v3_from(P), (float)W, (float)H, fx_fy_te, fx_fy_te + 1, fx_fy_te + 2);
}

enum { RR_COUNTING = 0, RR_OUTSIDE = 1, RR_REFUSED_ID = 2, RR_REFUSED_DEPTH = 3, RR_BY_NORMAL = 4, RR_BEHIND = 5, RR_REUSED = 6, RR_DIAG = 7 };

/* One frame.  c_now: W*H*4; obj_id, hit_t: W*H; nhat: 3 floats per face (denoise_ref.c dr_face_normals); prev = NULL: frame 0 of a
 * history (every hit pixel fresh), else the previous frame's camera and its planes prev_out (W*H*4), prev_n, prev_id, prev_t.
 * out: W*H*4, out_u8: W*H*4 or NULL, n1: W*H, counts: {reused, fresh, background}, diag: NULL or RR_DIAG ints per pixel —
 * {counting taps, taps outside the frame, taps refused by the id / normal rule, taps refused by the depth rule, counting taps
 * with id' != id (the normal rule's), 1 when mu > 0 failed, 1 when the pixel is reused (sw > 0: a counting tap may weigh nothing)}. */
OR_API void rr_frame(uint32_t W, uint32_t H, const float *c_now, const int32_t *obj_id, const float *hit_t, const float *nhat,
                     const OrCameraInvUniform *cam, uint32_t max_history, float normal_cos_min, float depth_rel,
                     const RrCamera *prev, const float *prev_out, const float *prev_n, const int32_t *prev_id, const float *prev_t,
                     float *out, uint8_t *out_u8, float *n1_plane, uint64_t *counts, int32_t *diag)
{
    const float fw = (float)W, fh = (float)H;
    OrScreen screen = {W, H};
    counts[0] = counts[1] = counts[2] = 0u;
    for (uint32_t y = 0; y < H; y++) {
        for (uint32_t x = 0; x < W; x++) {
            const size_t p = (size_t)y * W + x;
            const float *c = c_now + 4u * p;
            float *o = out + 4u * p;
            int32_t dg[RR_DIAG] = {0, 0, 0, 0, 0, 0, 0};
            const int32_t id = obj_id[p];
            o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
            if (id == -1) {
                n1_plane[p] = 0.0f;
                counts[2]++;
            } else {
                float n1 = 1.0f;
                int reused = 0;
                if (prev) {
                    Ray ray = pixel_to_ray(cam, &screen, x, y, 0.5f, 0.5f);
                    v3 P = madd3(hit_t[p], ray.direction, ray.origin);
                    float fx, fy, te;
                    if (!rr_project_point(prev, P, fw, fh, &fx, &fy, &te)) {
                        dg[RR_BEHIND] = 1;
                    } else if (!(fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh)) {
                        dg[RR_OUTSIDE] = 4;   /* every tap lies outside the frame (or fx / fy is not finite) */
                    } else {
                        const float x0f = floorf(fx), y0f = floorf(fy);
                        const float a = fx - x0f, b = fy - y0f;
                        const int x0 = (int)x0f, y0 = (int)y0f;
                        const float tol = depth_rel * te;
                        float sw = 0.0f, sc[3] = {0.0f, 0.0f, 0.0f}, sn = 0.0f;
                        for (int j = 0; j < 4; j++) {
                            const int qx = x0 + (j & 1), qy = y0 + (j >> 1);
                            if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)H) { dg[RR_OUTSIDE]++; continue; }
                            const size_t q = (size_t)qy * W + (size_t)qx;
                            const int32_t idq = prev_id[q];
                            int by_normal = 0;
                            if (idq != id) {
                                if (!(id >= 0 && idq >= 0)) { dg[RR_REFUSED_ID]++; continue; }
                                if (!(dot3(v3_from(nhat + 3u * (size_t)id), v3_from(nhat + 3u * (size_t)idq)) >= normal_cos_min)) {
                                    dg[RR_REFUSED_ID]++;
                                    continue;
                                }
                                by_normal = 1;
                            }
                            if (!(fabsf(te - prev_t[q]) <= tol)) { dg[RR_REFUSED_DEPTH]++; continue; }
                            const float w = ((j & 1) ? a : 1.0f - a) * ((j >> 1) ? b : 1.0f - b);
                            const float *hq = prev_out + 4u * q;
                            sw += w;
                            sc[0] += w * hq[0]; sc[1] += w * hq[1]; sc[2] += w * hq[2];
                            sn += w * prev_n[q];
                            dg[RR_COUNTING]++;
                            dg[RR_BY_NORMAL] += by_normal;
                        }
                        if (sw > 0.0f) {
                            reused = 1;
                            n1 = fminf(sn / sw + 1.0f, (float)max_history);
                            if (n1 != 1.0f) {
                                for (int k = 0; k < 3; k++) {
                                    const float hist = sc[k] / sw;
                                    o[k] = hist + (c[k] - hist) / n1;
                                }
                            }
                        }
                    }
                }
                n1_plane[p] = n1;
                dg[RR_REUSED] = reused;
                counts[reused ? 0 : 1]++;
            }
            if (out_u8)
                for (int k = 0; k < 4; k++) out_u8[4u * p + k] = unorm8(o[k]);
            if (diag)
                for (int k = 0; k < RR_DIAG; k++) diag[RR_DIAG * p + k] = dg[k];
        }
    }
}
