// csrc/rwr_tonemap.h for the host test (test_tonemap_host.py): the library's own luminance log, exposure and pixel map
// (RWR_FLAG_TONEMAP items 3-5), compiled without HIP, so that their results can be held against the reference's bit for bit.
// With TONEMAP_HOST_MAIN: a stand-alone program that walks the functions over their ranges' edges and checks their properties,
// for a run under -fsanitize=address,undefined.
#include <stdint.h>
#include <string.h>

#include "rwr_tonemap.h"

extern "C" {

// n pixels of 4 floats: L per pixel
void tonemap_host_luma_bits(const float *rgba, uint64_t n, int32_t *out)
{
    for (uint64_t i = 0; i < n; i++) out[i] = rwr::tonemap_luma_bits(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]);
}

float tonemap_host_exposure(int64_t log_sum, uint32_t count, uint32_t auto_exposure, float key, float exposure)
{
    return rwr::tonemap_exposure(log_sum, count, auto_exposure, key, exposure);
}

// n pixels of 4 floats: the rgba8 word per pixel, and (y may be null) the three curve values as floats
void tonemap_host_pixels(const float *rgba, uint64_t n, float E, uint32_t curve, float white, uint32_t *out, float *y)
{
    const float iw2 = 1.0f / (white * white);   // computed once, as the launcher does
    for (uint64_t i = 0; i < n; i++) {
        out[i] = rwr::tonemap_pixel(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], rgba[4 * i + 3], E, curve, iw2);
        if (y)
            for (int c = 0; c < 3; c++) y[3 * i + c] = rwr::tonemap_curve(rgba[4 * i + c], E, curve, iw2);
    }
}

}  // extern "C"

#ifdef TONEMAP_HOST_MAIN
#include <math.h>
#include <stdio.h>

#include <vector>

static int fail(const char *what, double a, double b)
{
    printf("%s: %.9g, %.9g\n", what, a, b);
    return 1;
}

int main()
{
    int bad = 0;
    // the log of a grey 2^k is k 2^23 (the three weights add up to 1.0f exactly, in the definition's order); the clamps; NaN counts
    // as the lower clamp
    for (int k = -16; k <= 16; k++) {
        const float v = ldexpf(1.0f, k);
        const int32_t L = rwr::tonemap_luma_bits(v, v, v);
        if (L != k * (1 << 23)) bad += fail("log of a power of two", L, k);
    }
    if (rwr::tonemap_luma_bits(0.0f, 0.0f, 0.0f) != -16 * (1 << 23)) bad += fail("lower clamp", rwr::tonemap_luma_bits(0.0f, 0.0f, 0.0f), 0);
    if (rwr::tonemap_luma_bits(1e30f, 1e30f, 1e30f) != 16 * (1 << 23)) bad += fail("upper clamp", rwr::tonemap_luma_bits(1e30f, 1e30f, 1e30f), 0);
    if (rwr::tonemap_luma_bits(NAN, 1.0f, 1.0f) != -16 * (1 << 23)) bad += fail("NaN luminance", rwr::tonemap_luma_bits(NAN, 1.0f, 1.0f), 0);
    if (rwr::tonemap_luma_bits(-5.0f, -5.0f, -5.0f) != -16 * (1 << 23)) bad += fail("negative luminance", 0, 0);
    // floor division on both sides of zero, the extreme sums, count 0 and manual mode
    const int64_t unit = 1 << 23;
    if (rwr::tonemap_exposure(-1, 2u, 1u, 1.0f, 1.0f) != 1.0f / rwr::tonemap_float_of(0x3f800000 - 1)) bad += fail("floor below zero", 0, 0);
    if (rwr::tonemap_exposure(1, 2u, 1u, 1.0f, 1.0f) != 1.0f) bad += fail("floor above zero", 0, 0);
    if (rwr::tonemap_exposure(-3 * unit, 1u, 1u, 0.5f, 2.0f) != 8.0f) bad += fail("G = 2^-3", rwr::tonemap_exposure(-3 * unit, 1u, 1u, 0.5f, 2.0f), 8.0);
    if (rwr::tonemap_exposure(16 * unit * (int64_t)(1u << 30), 1u << 30, 1u, 1.0f, 1.0f) != ldexpf(1.0f, -16)) bad += fail("largest sum", 0, 0);
    if (rwr::tonemap_exposure(-16 * unit * (int64_t)(1u << 30), 1u << 30, 1u, 1.0f, 1.0f) != ldexpf(1.0f, 16)) bad += fail("smallest sum", 0, 0);
    if (rwr::tonemap_exposure(12345, 0u, 1u, 0.18f, 3.0f) != 3.0f) bad += fail("count 0", 0, 0);
    if (rwr::tonemap_exposure(12345, 7u, 0u, 0.18f, 3.0f) != 3.0f) bad += fail("manual", 0, 0);
    // every curve over the edge values and a dense grid: bytes in range and monotone, 0 stays 0, NaN gives 0
    const float edges[] = {0.0f, ldexpf(1.0f, -50), ldexpf(1.0f, -16), 1.0f, 4.0f, 64.0f * 17.0f, 1e30f, INFINITY, -1.0f, -INFINITY, NAN};
    for (uint32_t curve = 0; curve < 3u; curve++) {
        for (float white : {1.0f / 256.0f, 4.0f, 65536.0f}) {
            const float iw2 = 1.0f / (white * white);
            for (float E : {ldexpf(1.0f, -16), 1.0f, ldexpf(1.0f, 48)}) {
                for (float c : edges) {
                    const uint32_t px = rwr::tonemap_pixel(c, c, c, 1.0f, E, curve, iw2);
                    if ((px >> 24) != 255u) bad += fail("alpha byte", px, c);
                    // (a negative radiance, which no frame holds, gives 0 under the clamp; the two rational curves are not cut off below 0)
                    if ((c == 0.0f || c != c || (curve == rwr::kTonemapClamp && c < 0.0f)) && (px & 0xffffffu) != 0u) bad += fail("0, NaN and the clamp's negatives give 0", px, c);
                }
            }
            uint32_t prev = 0;
            for (uint32_t i = 0; i <= 200000u; i++) {
                const uint32_t b = rwr::tonemap_byte(rwr::tonemap_curve((float)i * (64.0f / 200000.0f), 1.0f, curve, iw2));
                if (b > 255u || b < prev) { bad += fail("bytes are monotone", b, prev); break; }
                prev = b;
            }
        }
    }
    // the measure over a plane on the heap, as the kernel walks it: sums stay exact
    std::vector<float> plane(4u * 4099u);
    for (size_t i = 0; i < plane.size() / 4u; i++) {
        plane[4 * i] = (float)(i % 97u) * 0.37f; plane[4 * i + 1] = (float)(i % 13u) * 5.0f; plane[4 * i + 2] = (float)(i % 7u) * 0.01f;
        plane[4 * i + 3] = i % 5u ? 1.0f : 0.0f;
    }
    std::vector<int32_t> L(plane.size() / 4u);
    tonemap_host_luma_bits(plane.data(), L.size(), L.data());
    int64_t sum = 0, rsum = 0;
    for (size_t i = 0; i < L.size(); i++) sum += L[i];
    for (size_t i = L.size(); i-- > 0;) rsum += L[i];
    if (sum != rsum) bad += fail("order of the sum", (double)sum, (double)rsum);
    std::vector<uint32_t> px(L.size());
    std::vector<float> y(3u * L.size());
    tonemap_host_pixels(plane.data(), px.size(), rwr::tonemap_exposure(sum, (uint32_t)L.size(), 1u, 0.18f, 1.0f), rwr::kTonemapAces, 4.0f, px.data(), y.data());
    printf(bad ? "FAILED\n" : "tonemap_host ok\n");
    return bad ? 1 : 0;
}
#endif
