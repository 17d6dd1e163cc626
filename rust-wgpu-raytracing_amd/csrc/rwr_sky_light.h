// The sky's image as a light of the path tracer (RWR_FLAG_LIGHT_SKY; definition: include/rwr_hip.h): the sampling
// distribution over the n x n octahedral map the light stage draws a texel from (kernels_wf_light.hip, the SKY forms) and both
// sides read a texel's probability from (rwr_device.h sky_light_g).  The builder compiles without HIP (tests/sky_light_host.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace rwr {

// The table, n + n * n floats: the row cdf R_j at [j], then row j's conditional cdf C_ji at [n + j * n + i].  rgb: the image as
// rwr_sky_set_image takes it (row j <-> v, column i <-> u), `stride` floats per texel (3: the caller's array; 4: the float4 texels
// the context keeps).  Texel (j, i) weighs w_ji = b_ji * O_ji: b_ji the sum of r + g + b over its 3 x 3 neighbourhood, indices
// clamped to the map (S_img's bilinear fetch reads exactly those texels from inside the cell, so the density is positive wherever
// S_img is), O_ji = 1 / |p_c|^3 the cell's solid angle up to a constant, p_c the cell centre's point on |x| + |y| + |z| = 1.
// All sums in double, rounded to f32 once, on storing; every entry of a cdf from its last texel (row) of non-zero weight on is 1.0f,
// and a row without weight holds 1.0f throughout (its step of the row cdf is 0: it is never drawn).  total (may be null): W, the
// sum of all weights; an empty table is returned when W is not greater than 0 — the flag is not effective then.
inline std::vector<float> build_sky_light(const float *rgb, uint32_t n, uint32_t stride, double *total = nullptr)
{
    std::vector<float> table;
    if (total) *total = 0.0;
    if (!rgb || n == 0u) return table;
    const size_t N = n;
    std::vector<double> lum(N * N), w(N * N), row(N);
    for (size_t t = 0; t < N * N; t++) lum[t] = ((double)rgb[stride * t] + (double)rgb[stride * t + 1u]) + (double)rgb[stride * t + 2u];
    double W = 0.0;
    for (size_t j = 0; j < N; j++) {
        double Wj = 0.0;
        for (size_t i = 0; i < N; i++) {
            double b = 0.0;
            for (int dj = -1; dj <= 1; dj++)
                for (int di = -1; di <= 1; di++) {
                    const size_t jj = (size_t)std::min<long>(std::max<long>((long)j + dj, 0), (long)N - 1);
                    const size_t ii = (size_t)std::min<long>(std::max<long>((long)i + di, 0), (long)N - 1);
                    b += lum[jj * N + ii];
                }
            // the cell centre on the octahedron: the inverse of S_img's mapping
            const double u = ((double)i + 0.5) / (double)n, v = ((double)j + 0.5) / (double)n;
            double px = 2.0 * u - 1.0, pz = 2.0 * v - 1.0;
            const double py = (1.0 - std::fabs(px)) - std::fabs(pz);
            if (py < 0.0) {
                const double qx = (1.0 - std::fabs(pz)) * std::copysign(1.0, px), qz = (1.0 - std::fabs(px)) * std::copysign(1.0, pz);
                px = qx; pz = qz;
            }
            const double l2 = (px * px + py * py) + pz * pz;
            w[j * N + i] = b * (1.0 / (l2 * std::sqrt(l2)));
            Wj += w[j * N + i];
        }
        row[j] = Wj;
        W += Wj;
    }
    if (total) *total = W;
    if (!(W > 0.0)) return table;
    table.assign(N + N * N, 1.0f);
    size_t last_row = 0;
    for (size_t j = 0; j < N; j++)
        if (row[j] > 0.0) last_row = j;
    double run = 0.0;
    for (size_t j = 0; j < last_row; j++) {
        run += row[j];
        table[j] = (float)(run / W);
    }
    for (size_t j = 0; j < N; j++) {
        if (!(row[j] > 0.0)) continue;
        size_t last = 0;
        for (size_t i = 0; i < N; i++)
            if (w[j * N + i] > 0.0) last = i;
        double r = 0.0;
        for (size_t i = 0; i < last; i++) {
            r += w[j * N + i];
            table[N + j * N + i] = (float)(r / row[j]);
        }
    }
    return table;
}

}  // namespace rwr
