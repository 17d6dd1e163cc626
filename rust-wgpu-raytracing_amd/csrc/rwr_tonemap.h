// Tone mapping and exposure of a path-traced frame (RWR_FLAG_TONEMAP; definition: include/rwr_hip.h): the three
// functions of the definition, one statement for both sides.  The kernels (kernels_wf_tonemap.hip) call them per pixel,
// rwr_last_tonemap_stats computes the frame's exposure with the same tonemap_exposure, and the host half compiles without HIP
// (tests/tonemap_host.cpp).  Every unit that includes this is built without contraction and with IEEE division: a result is the
// same 32 bits wherever it is computed.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define RWR_HD __host__ __device__
#else
#define RWR_HD
#endif

namespace rwr {

// the curves (rwr_hip.h RWR_TONEMAP_*: the same numbers)
constexpr uint32_t kTonemapClamp = 0u, kTonemapReinhard = 1u, kTonemapAces = 2u;
constexpr float kTonemapLumaMin = 1.52587890625e-05f, kTonemapLumaMax = 65536.0f;   // 2^-16, 2^16: the measure's clamp
constexpr int32_t kTonemapOneBits = 0x3f800000;

RWR_HD inline int32_t tonemap_bits_of(float v)
{
    int32_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}
RWR_HD inline float tonemap_float_of(int32_t b)
{
    float v;
    __builtin_memcpy(&v, &b, sizeof v);
    return v;
}

// Item 3: the pixel's luminance as the piecewise-linear log2 in units of 2^-23 — the bits of the clamped luminance above those of
// 1.0f, an exact integer in [-2^27, 2^27].  A NaN luminance counts as the lower clamp (fmaxf returns the other operand).
RWR_HD inline int32_t tonemap_luma_bits(float r, float g, float b)
{
    const float y = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    const float yc = __builtin_fminf(__builtin_fmaxf(y, kTonemapLumaMin), kTonemapLumaMax);
    return tonemap_bits_of(yc) - kTonemapOneBits;
}

// Item 4: the frame's exposure from the measure's sums.  M = floor(log_sum / count) — floor, not C's truncation: scaling the image by
// 2^j then shifts M by exactly j 2^23 on either side of zero — and G, the log-average luminance, is the float whose bits are M above 1.0f's.
RWR_HD inline float tonemap_exposure(int64_t log_sum, uint32_t count, uint32_t auto_exposure, float key, float exposure)
{
    if (!auto_exposure || count == 0u) return exposure;
    const int64_t n = (int64_t)count;
    int64_t m = log_sum / n;
    if (log_sum % n != 0 && log_sum < 0) m -= 1;
    const float G = tonemap_float_of(kTonemapOneBits + (int32_t)m);
    return (key / G) * exposure;
}

// Item 5: one component through the curve.  T: float, or two pixels' components side by side (the kernels' f2).
template <typename T>
RWR_HD inline T tonemap_curve(T c, float E, uint32_t curve, float iw2)
{
    const T x = c * E;
    if (curve == kTonemapReinhard) return (x * (1.0f + x * iw2)) / (1.0f + x);
    if (curve == kTonemapAces) return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    return x;
}

// pack_rgba8's rule for one channel (rwr_device.h): times 255, saturated to [0, 255], nearest, ties to even, NaN gives 0
RWR_HD inline uint32_t tonemap_byte(float y)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_cvt_pk_u8_f32(y * 255.0f, 0, 0u);
#else
    const float v = y * 255.0f;
    if (!(v > 0.0f)) return 0u;
    if (v >= 255.0f) return 255u;
    return (uint32_t)__builtin_rintf(v);   // (the default rounding mode: nearest, ties to even)
#endif
}

// Item 5: a pixel of colour_f32 to its rgba8 word (r in the low byte).  The alpha byte is the one the resolve wrote: its rule on a.
RWR_HD inline uint32_t tonemap_pixel(float r, float g, float b, float a, float E, uint32_t curve, float iw2)
{
    return tonemap_byte(tonemap_curve(r, E, curve, iw2)) | (tonemap_byte(tonemap_curve(g, E, curve, iw2)) << 8) |
           (tonemap_byte(tonemap_curve(b, E, curve, iw2)) << 16) | (tonemap_byte(a) << 24);
}

}  // namespace rwr
