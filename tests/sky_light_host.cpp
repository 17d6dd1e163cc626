// csrc/rwr_sky_light.h for the host test (test_sky_light_host.py): the library's own builder of the sky image's sampling table
// (RWR_FLAG_LIGHT_SKY item 1), compiled without HIP, so that its entries can be held against the reference's bit for bit.
// With SKY_LIGHT_HOST_MAIN: a stand-alone program that builds the tables of a few maps and checks their shape, for a run under
// -fsanitize=address,undefined.
#include <stdint.h>
#include <string.h>

#include "rwr_sky_light.h"

// rgb: n * n texels of `stride` floats.  Writes the n + n * n floats when there is a table (W > 0) and returns W.
extern "C" double sky_light_host_build(const float *rgb, uint32_t n, uint32_t stride, float *out)
{
    double W = 0.0;
    const std::vector<float> table = rwr::build_sky_light(rgb, n, stride, &W);
    if (!table.empty()) memcpy(out, table.data(), table.size() * sizeof(float));
    return W;
}

#ifdef SKY_LIGHT_HOST_MAIN
#include <stdio.h>

static int check(const char *what, const std::vector<float> &rgb, uint32_t n, uint32_t stride, bool want_table)
{
    double W = -1.0;
    const std::vector<float> t = rwr::build_sky_light(rgb.data(), n, stride, &W);
    if (want_table != !t.empty()) { printf("%s: table %s, W %g\n", what, t.empty() ? "missing" : "unexpected", W); return 1; }
    if (t.empty()) return 0;
    if (t.size() != (size_t)n + (size_t)n * n) { printf("%s: %zu entries\n", what, t.size()); return 1; }
    for (uint32_t c = 0; c <= n; c++) {   // the row cdf, then every row's
        const float *cdf = c == 0u ? t.data() : t.data() + n + (size_t)(c - 1u) * n;
        float prev = 0.0f;
        for (uint32_t i = 0; i < n; i++) {
            if (!(cdf[i] >= prev) || cdf[i] > 1.0f) { printf("%s: cdf %u entry %u is %g after %g\n", what, c, i, cdf[i], prev); return 1; }
            prev = cdf[i];
        }
        if (cdf[n - 1u] != 1.0f) { printf("%s: cdf %u ends at %g\n", what, c, cdf[n - 1u]); return 1; }
    }
    return 0;
}

int main()
{
    int bad = 0;
    for (uint32_t n : {2u, 5u, 16u, 64u}) {
        for (uint32_t stride : {3u, 4u}) {
            std::vector<float> rgb((size_t)n * n * stride, 0.0f);
            bad += check("black", rgb, n, stride, false);
            rgb[0] = 40.0f;                                                    // one bright texel in a corner: the clamped neighbourhood
            bad += check("corner", rgb, n, stride, true);
            rgb[((size_t)n * n - 1u) * stride + 2u] = 64.0f;                   // and the opposite one
            bad += check("corners", rgb, n, stride, true);
            for (size_t t = 0; t < (size_t)n * n; t++)
                for (uint32_t c = 0; c < 3u; c++) rgb[t * stride + c] = (float)((t * 7u + c * 3u) % 11u) * 0.25f;
            bad += check("pattern", rgb, n, stride, true);
        }
    }
    bad += check("no image", std::vector<float>(), 0u, 3u, false);
    printf(bad ? "FAILED\n" : "sky_light_host ok\n");
    return bad ? 1 : 0;
}
#endif
