/* CPU reference of the sky's image (RWR_FLAG_SKY_IMAGE; include/rwr_hip.h) for the tests: S_img(D) written from the
 * header's definition, f32 throughout, built with the oracle's flags (no contraction; fmaf is the one fused operation, where the
 * definition names it).
 *
 *   a  = (|D.x| + |D.y|) + |D.z|;  px = D.x / a;  pz = D.z / a
 *   D.y < 0:  (px, pz) <- ((1 - |pz|) * copysignf(1, px), (1 - |px|) * copysignf(1, pz))
 *   u = px * 0.5 + 0.5;  v = pz * 0.5 + 0.5
 *   the mesh textures' bilinear fetch of the n x n image at (u * n - 0.5, v * n - 0.5): taps at floor and floor + 1, each clamped
 *   to [0, n - 1] (ClampToEdge), fractions a = position - floor, weights w00 = (1 - a.x)(1 - a.y), w10 = a.x (1 - a.y),
 *   w01 = (1 - a.x) a.y, w11 = a.x a.y, value fma(t11, w11, fma(t01, w01, fma(t10, w10, t00 * w00))) per channel.
 * The image is n * n * 3 floats, row j <-> v, column i <-> u. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(_WIN32)
#define SI_API __declspec(dllexport)
#else
#define SI_API __attribute__((visibility("default")))
#endif

SI_API void sky_image_ref_uv(const float d[3], float uv[2])
{
    const float a = (fabsf(d[0]) + fabsf(d[1])) + fabsf(d[2]);
    float px = d[0] / a, pz = d[2] / a;
    if (d[1] < 0.0f) {
        const float qx = (1.0f - fabsf(pz)) * copysignf(1.0f, px);
        const float qz = (1.0f - fabsf(px)) * copysignf(1.0f, pz);
        px = qx; pz = qz;
    }
    uv[0] = px * 0.5f + 0.5f;
    uv[1] = pz * 0.5f + 0.5f;
}

/* a tap's index: the texel coordinate clamped to the image; a NaN coordinate (a zero or NaN direction) takes texel 0 — the value
 * is NaN whichever texel it is, since the weights are */
static uint32_t si_tap(float f, float max)
{
    if (!(f >= 0.0f)) return 0u;
    return (uint32_t)(f > max ? max : f);
}

SI_API void sky_image_ref_radiance(const float *rgb, uint32_t n, const float *dirs, size_t count, float *out)
{
    const float fn = (float)n, max = fn - 1.0f;
    for (size_t k = 0; k < count; k++) {
        float uv[2];
        sky_image_ref_uv(dirs + 3u * k, uv);
        const float x = uv[0] * fn - 0.5f, y = uv[1] * fn - 0.5f;
        const float x0 = floorf(x), y0 = floorf(y);
        const float ax = x - x0, ay = y - y0, bx = 1.0f - ax, by = 1.0f - ay;
        const uint32_t i0 = si_tap(x0, max), i1 = si_tap(x0 + 1.0f, max), j0 = si_tap(y0, max), j1 = si_tap(y0 + 1.0f, max);
        const float w00 = bx * by, w10 = ax * by, w01 = bx * ay, w11 = ax * ay;
        for (int c = 0; c < 3; c++) {
            const float t00 = rgb[((size_t)j0 * n + i0) * 3u + c], t10 = rgb[((size_t)j0 * n + i1) * 3u + c];
            const float t01 = rgb[((size_t)j1 * n + i0) * 3u + c], t11 = rgb[((size_t)j1 * n + i1) * 3u + c];
            out[3u * k + c] = fmaf(t11, w11, fmaf(t01, w01, fmaf(t10, w10, t00 * w00)));
        }
    }
}
