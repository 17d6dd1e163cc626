// RWR_FLAG_DENOISE: the edge-avoiding a-trous filter behind the wavefront integrator's resolve (include/rwr_hip.h).
//
// k_dn_guide, once per frame, packs what a tap needs into two 16-byte records per pixel: the guide {nhat.xyz of the face (zeros for
// spheres and background), t} and the colour {r, g, b, object id (its bits)} — a tap is two coalesced 16-byte loads and never
// gathers through obj_id -> TriRecord.  One launch per iteration then reads one colour plane and writes the other (two scratch
// planes of the frame slot, ping-pong); the last iteration writes the frame's colour_f32 and rgba8 planes.
//   steps 1 and 2 (k_dn_tile): the 64x8 tile and its halo of 2 * step pixels are staged in LDS, colour and guide as two arrays
//     of 16-byte records.  A wave reads one tile row per instruction — 64 consecutive records, 256 B per 16-lane group, one bank
//     row: ds_read_b128 without conflicts, whatever the row pitch — and the fill writes consecutive records.
//     26 KiB (step 1) / 36 KiB (step 2) per workgroup: 6 / 4 workgroups per CU.
//   steps 4, 8, 16 (k_dn_far): taps straight from memory; neighbouring lanes read neighbouring pixels, and the three planes of a
//     frame stay in the last-level cache between the launches.
// The arithmetic is the definition's, operation for operation (this translation unit: no contraction, IEEE division), so a frame
// equals tests/denoise_ref.c on the same planes.
#include "rwr_device.h"

namespace rwr {

namespace {

struct DnConsts {
    float inv;          // inv_i = 1 / (sigma * sigma) * 4^i
    float cos_min;
    float depth_rel;
    uint32_t width, height;
};

// the tap's geometry weight, for a centre pixel on a surface (idp != -1)
RWR_DEV bool dn_same_surface(int32_t idp, const float4 gp, int32_t idq, const float4 gq, const DnConsts &k)
{
    if (idq == -1) return false;
    if (idq == idp) return true;
    if (idp < 0 || idq < 0) return false;   // a sphere against another sphere or against the mesh
    const float d = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
    return d >= k.cos_min && __builtin_fabsf(gp.w - gq.w) <= k.depth_rel * __builtin_fminf(gp.w, gq.w);
}

struct DnSum {
    float r, g, b, norm;
};

RWR_DEV void dn_tap(DnSum &s, const float4 cp, const float4 cq, float h, float inv)
{
    const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z;
    const float d2 = (dr * dr + dg * dg) + db * db;
    const float w = 1.0f / (1.0f + d2 * inv);
    const float hw = h * w;
    s.r += hw * cq.x; s.g += hw * cq.y; s.b += hw * cq.z;
    s.norm += hw;
}

RWR_DEV float dn_kernel(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// the iteration's result for one pixel goes to the other scratch plane or, from the last iteration, to the frame's planes (alpha
// is the resolve's: colour_f32 still holds it)
template <bool LAST>
RWR_DEV void dn_store(const Targets &tg, float4 *__restrict__ out, size_t pixel, float r, float g, float b, float id_bits)
{
    if (LAST) {
        float4 *dst = reinterpret_cast<float4 *>(tg.color_f32) + pixel;
        const float a = dst->w;
        *dst = make_float4(r, g, b, a);
        reinterpret_cast<uint32_t *>(tg.color)[pixel] = pack_rgba8(r, g, b, a);
    } else {
        out[pixel] = make_float4(r, g, b, id_bits);
    }
}

}  // namespace

__global__ void __launch_bounds__(256)
k_dn_guide(const TriRecord *__restrict__ tris, const Targets tg, float4 *__restrict__ guide, float4 *__restrict__ colour, uint32_t n)
{
    const uint32_t pixel = blockIdx.x * 256u + threadIdx.x;
    if (pixel >= n) return;
    const int32_t id = tg.obj_id[pixel];
    const float4 c = reinterpret_cast<const float4 *>(tg.color_f32)[pixel];
    float4 g = make_float4(0.0f, 0.0f, 0.0f, tg.hit_t[pixel]);
    if (id >= 0) {
        const float4 nh = *reinterpret_cast<const float4 *>(tris[id].nhat);
        g.x = nh.x; g.y = nh.y; g.z = nh.z;
    }
    guide[pixel] = g;
    colour[pixel] = make_float4(c.x, c.y, c.z, __int_as_float(id));
}

// steps 1 and 2: workgroup = 64x8 tile, wave w filters rows w and w + 4
template <int STEP, bool LAST>
__global__ void __launch_bounds__(256)
k_dn_tile(const DnConsts k, const float4 *__restrict__ in, const float4 *__restrict__ guide, float4 *__restrict__ out, const Targets tg)
{
    constexpr int R = 2 * STEP, PW = 64 + 2 * R, PH = 8 + 2 * R;
    __shared__ float4 s_c[PW * PH];
    __shared__ float4 s_g[PW * PH];
    const int x0 = (int)(blockIdx.x * 64u) - R, y0 = (int)(blockIdx.y * 8u) - R;
    for (int i = (int)threadIdx.x; i < PW * PH; i += 256) {
        const int ly = i / PW, lx = i - ly * PW;
        const int x = x0 + lx, y = y0 + ly;
        // a record outside the frame reads as background: its taps are skipped
        float4 c = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)), g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (x >= 0 && y >= 0 && x < (int)k.width && y < (int)k.height) {
            const size_t q = (size_t)y * k.width + (uint32_t)x;
            c = in[q];
            g = guide[q];
        }
        s_c[i] = c;
        s_g[i] = g;
    }
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int ry = wave + 4 * half;
        const uint32_t x = blockIdx.x * 64u + (uint32_t)lane, y = blockIdx.y * 8u + (uint32_t)ry;
        if (x >= k.width || y >= k.height) continue;
        const int centre = (ry + R) * PW + lane + R;
        const float4 cp = s_c[centre], gp = s_g[centre];
        const int32_t idp = __float_as_int(cp.w);
        float r = cp.x, g = cp.y, b = cp.z;
        if (idp != -1) {
            DnSum s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                for (int dx = -2; dx <= 2; dx++) {
                    const int q = centre + STEP * (dy * PW + dx);
                    const float4 cq = s_c[q];
                    if (dn_same_surface(idp, gp, __float_as_int(cq.w), s_g[q], k)) dn_tap(s, cp, cq, dn_kernel(dx) * dn_kernel(dy), k.inv);
                }
            }
            r = s.r / s.norm; g = s.g / s.norm; b = s.b / s.norm;
        }
        dn_store<LAST>(tg, out, (size_t)y * k.width + x, r, g, b, cp.w);
    }
}

// steps 4 and up: workgroup = 64x4 pixels, one row per wave
template <bool LAST>
__global__ void __launch_bounds__(256)
k_dn_far(const DnConsts k, int step, const float4 *__restrict__ in, const float4 *__restrict__ guide, float4 *__restrict__ out, const Targets tg)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= k.width || y >= k.height) return;
    const size_t pixel = (size_t)y * k.width + x;
    const float4 cp = in[pixel];
    const int32_t idp = __float_as_int(cp.w);
    float r = cp.x, g = cp.y, b = cp.z;
    if (idp != -1) {
        const float4 gp = guide[pixel];
        DnSum s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
            const int qy = (int)y + step * dy;
            if (qy < 0 || qy >= (int)k.height) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const int qx = (int)x + step * dx;
                if (qx < 0 || qx >= (int)k.width) continue;
                const size_t q = (size_t)qy * k.width + (uint32_t)qx;
                const float4 cq = in[q];
                const int32_t idq = __float_as_int(cq.w);
                if (idq == -1) continue;
                if (dn_same_surface(idp, gp, idq, guide[q], k)) dn_tap(s, cp, cq, dn_kernel(dx) * dn_kernel(dy), k.inv);
            }
        }
        r = s.r / s.norm; g = s.g / s.norm; b = s.b / s.norm;
    }
    dn_store<LAST>(tg, out, pixel, r, g, b, cp.w);
}

hipError_t launch_wf_denoise(hipStream_t s, uint32_t width, uint32_t height, const TriRecord *tris, const Targets &tg,
                             const rwr_denoise_params &dp, float4 *guide, float4 *plane_a, float4 *plane_b)
{
    if (width == 0u || height == 0u) return hipSuccess;
    const uint32_t n = width * height;   // at most 2^30 (rwr_resize)
    hipLaunchKernelGGL(k_dn_guide, dim3((n + 255u) / 256u), dim3(256), 0, s, tris, tg, guide, plane_a, n);
    DnConsts k{1.0f / (dp.sigma_color * dp.sigma_color), dp.normal_cos_min, dp.depth_rel, width, height};
    const float4 *in = plane_a;
    float4 *out = plane_b;
    for (uint32_t i = 0; i < dp.iterations; i++) {
        const bool last = i + 1u == dp.iterations;
        const dim3 tiles((width + 63u) / 64u, (height + 7u) / 8u), rows((width + 63u) / 64u, (height + 3u) / 4u);
        if (i == 0u) {
            if (last) hipLaunchKernelGGL((k_dn_tile<1, true>), tiles, dim3(256), 0, s, k, in, guide, out, tg);
            else hipLaunchKernelGGL((k_dn_tile<1, false>), tiles, dim3(256), 0, s, k, in, guide, out, tg);
        } else if (i == 1u) {
            if (last) hipLaunchKernelGGL((k_dn_tile<2, true>), tiles, dim3(256), 0, s, k, in, guide, out, tg);
            else hipLaunchKernelGGL((k_dn_tile<2, false>), tiles, dim3(256), 0, s, k, in, guide, out, tg);
        } else {
            if (last) hipLaunchKernelGGL((k_dn_far<true>), rows, dim3(256), 0, s, k, 1 << i, in, guide, out, tg);
            else hipLaunchKernelGGL((k_dn_far<false>), rows, dim3(256), 0, s, k, 1 << i, in, guide, out, tg);
        }
        float4 *next_out = const_cast<float4 *>(in);
        in = out;
        out = next_out;
        k.inv = k.inv * 4.0f;   // the colour tolerance halves per level
    }
    return hipGetLastError();
}

}  // namespace rwr
