// The mesh light of the path tracer (RWR_FLAG_LIGHT_PARTS; definition: include/rwr_hip.h): the list of the world faces
// whose part emits, as an area distribution the light stage draws a face from (kernels_wf_light.hip, the PARTS forms).  Host and
// device share this header; the builder compiles without HIP (tests/part_light_host.cpp).
#pragma once

#include <stdint.h>

#include <cmath>
#include <vector>

namespace rwr {

// One listed face, 16 bytes: the running sum of the weights up to and including it over their total (non-decreasing, the last one
// 1.0f), the world face's index, and the reciprocal of the area density of a point drawn on it — choice w_f / W times 1 / A_f,
// w_f = A_f (Le_r + Le_g + Le_b): W / (Le_r + Le_g + Le_b), the same for every face of a part.
struct PartLightRec { float cdf; uint32_t face; float inv_pdf; uint32_t pad; };
static_assert(sizeof(PartLightRec) == 16, "PartLightRec is 16 B");

// The list, in face-index order: the world faces (after instancing: world face i is base face i % n_base_faces) whose part's radiance
// is not zero and whose area is greater than 0.  corners: 9 floats per world face, the world-space p0, p1, p2 the kernels hold;
// face_part: the part of every base face; glow: 4 floats {r, g, b, -} per part (the emission table's records).
// All sums in double, rounded to f32 once, on storing: A_f = 0.5 |(p1 - p0) x (p2 - p0)|, W the running sum of the w_f in list order,
// cdf_f that running sum over W.  (Built without contraction, like every unit of the library and tests/part_light_ref.c.)
inline std::vector<PartLightRec> build_part_lights(const float *corners, uint32_t n_world_faces, const uint32_t *face_part, uint32_t n_base_faces,
                                                   const float *glow, uint32_t n_parts)
{
    std::vector<PartLightRec> list;
    std::vector<double> running;
    if (n_base_faces == 0u) return list;
    double W = 0.0;
    for (uint32_t i = 0; i < n_world_faces; i++) {
        const uint32_t part = face_part[i % n_base_faces];
        if (part >= n_parts) continue;
        const float *le = glow + 4u * (size_t)part;
        if (!(le[0] != 0.0f || le[1] != 0.0f || le[2] != 0.0f)) continue;
        const float *c = corners + 9u * (size_t)i;
        const double ax = (double)c[3] - (double)c[0], ay = (double)c[4] - (double)c[1], az = (double)c[5] - (double)c[2];
        const double bx = (double)c[6] - (double)c[0], by = (double)c[7] - (double)c[1], bz = (double)c[8] - (double)c[2];
        const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const double area = 0.5 * std::sqrt(nx * nx + ny * ny + nz * nz);
        if (!(area > 0.0)) continue;
        const double sum = (double)le[0] + (double)le[1] + (double)le[2];
        W += area * sum;
        running.push_back(W);
        list.push_back(PartLightRec{0.0f, i, 0.0f, 0u});
    }
    for (size_t j = 0; j < list.size(); j++) {
        const float *le = glow + 4u * (size_t)face_part[list[j].face % n_base_faces];
        list[j].cdf = (float)(running[j] / W);
        list[j].inv_pdf = (float)(W / ((double)le[0] + (double)le[1] + (double)le[2]));
    }
    if (!list.empty()) list.back().cdf = 1.0f;
    return list;
}

}  // namespace rwr
