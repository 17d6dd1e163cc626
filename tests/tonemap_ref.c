/* The tests' CPU reference of the tone-mapping stage (RWR_FLAG_TONEMAP, include/rwr_hip.h items 3-5), written from the definition:
 * the measure, the exposure and the map, all f32 in the stated order.  Built by tonemap_ref.py with the oracle's compiler flags
 * (-ffp-contract=off among them).  Nothing here includes the library's sources. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define TR_API __attribute__((visibility("default")))   /* the oracle's flags hide the rest */

static int32_t bits_of(float v)
{
    int32_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

static float float_of(int32_t b)
{
    float v;
    memcpy(&v, &b, sizeof v);
    return v;
}

/* item 3: L of one pixel */
TR_API int32_t tr_luma_bits(float r, float g, float b)
{
    const float y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    float yc = y;
    if (!(yc >= 0x1p-16f)) yc = 0x1p-16f;   /* fmaxf(Y, 2^-16): a NaN gives 2^-16 */
    if (yc > 0x1p16f) yc = 0x1p16f;
    return bits_of(yc) - 0x3f800000;
}

/* item 3 over a plane of n rgba pixels */
TR_API void tr_measure(const float *rgba, uint64_t n, int64_t *log_sum, uint32_t *count)
{
    int64_t s = 0;
    uint32_t c = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (rgba[4 * i + 3] == 0.0f) continue;   /* (a NaN alpha counts: it is not 0) */
        s += tr_luma_bits(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]);
        c++;
    }
    *log_sum = s;
    *count = c;
}

/* item 4 */
TR_API float tr_exposure(int64_t log_sum, uint32_t count, uint32_t auto_exposure, float key, float exposure)
{
    if (!auto_exposure || count == 0) return exposure;
    int64_t q = log_sum / (int64_t)count, r = log_sum % (int64_t)count;
    if (r < 0) q -= 1;   /* floor: C truncates towards zero */
    const float G = float_of(0x3f800000 + (int32_t)q);
    return (key / G) * exposure;
}

/* item 5: one component's y */
TR_API float tr_curve(float c, float E, uint32_t curve, float white)
{
    const float x = c * E;
    if (curve == 1u) {
        const float iw2 = 1.0f / (white * white);
        return (x * (1.0f + x * iw2)) / (1.0f + x);
    }
    if (curve == 2u) return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    return x;
}

/* the rgba8 store's rule: times 255, saturated, nearest-even, NaN gives 0 */
TR_API uint8_t tr_byte(float y)
{
    const float v = y * 255.0f;
    if (v != v || v <= 0.0f) return 0;
    if (v >= 255.0f) return 255;
    return (uint8_t)rintf(v);
}

/* items 3-5 over a plane: out8 gets n rgba8 pixels; returns E */
TR_API float tr_tonemap(const float *rgba, uint64_t n, uint32_t curve, uint32_t auto_exposure, float exposure, float key, float white,
                 uint8_t *out8, int64_t *log_sum, uint32_t *count)
{
    *log_sum = 0;
    *count = 0;
    if (auto_exposure) tr_measure(rgba, n, log_sum, count);
    const float E = tr_exposure(*log_sum, *count, auto_exposure, key, exposure);
    for (uint64_t i = 0; i < n; i++) {
        for (int c = 0; c < 3; c++) out8[4 * i + c] = tr_byte(tr_curve(rgba[4 * i + c], E, curve, white));
        out8[4 * i + 3] = tr_byte(rgba[4 * i + 3]);
    }
    return E;
}

/* a grid of `n` inputs x_i = (float)i * step under one curve with E = 1: the bytes (the monotonicity test reads them) */
TR_API void tr_curve_bytes(uint32_t curve, float white, float step, uint64_t n, uint8_t *out)
{
    for (uint64_t i = 0; i < n; i++) out[i] = tr_byte(tr_curve((float)i * step, 1.0f, curve, white));
}
