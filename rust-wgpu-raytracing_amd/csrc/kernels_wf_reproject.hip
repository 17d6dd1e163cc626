// RWR_FLAG_REPROJECT: temporal reprojection of the context's history behind the wavefront integrator's resolve and ahead of the
// filter (include/rwr_hip.h).
//
// One launch per frame, one pixel per lane, a wave per 64-pixel row piece.  A hit pixel's point P on its pixel-centre ray is
// projected into the previous frame through that frame's camera constants (RpCamera: kernel arguments, wave-uniform), and the
// four pixels around the landing point are the taps.  The history is laid out for the taps, as k_dn_guide lays out the filter's
// planes: per pixel a record {r, g, b, n}, a record {nhat.xyz of the face (zeros for spheres and background), t} and the id — a
// tap is two 16-byte loads and a 4-byte one, coalesced across the wave under any coherent camera move, and never gathers
// through obj_id -> TriRecord.  The pixel itself reads its resolved colour, id and t once and its face's nhat (the only gather),
// and writes the next history once; colour_f32 and rgba8 are rewritten only where a blend changed them (a fresh, background or
// n' = 1 pixel keeps the resolve's bytes).  Two history sets alternate (the stage gathers, so it cannot work in place).
// The three counts: ballot + popcount per wave, one atomic per count from the wave's first lane.
// The arithmetic is the definition's, operation for operation (this translation unit: no contraction, IEEE division and square
// root), so n' and the counts equal tests/reproject_ref.c exactly.
#include "rwr_device.h"

namespace rwr {

namespace {

struct RpConsts {
    RpCamera prev;               // the previous reprojecting frame's camera
    float cos_min, depth_rel, max_history;
    uint32_t width, height;
    uint32_t have_prev;          // 0: frame 0 of a history — every hit pixel is fresh
};

enum : uint32_t { kRpReused = 0u, kRpFresh = 1u, kRpBackground = 2u, kRpOutside = 3u };

}  // namespace

__global__ void __launch_bounds__(256)
k_wf_reproject(const RpConsts k, const rwr_camera_inv_uniform cam, const TriRecord *__restrict__ tris, const Targets tg,
               const RpHistory hp, const RpHistory hn, unsigned long long *__restrict__ counts)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    uint32_t kind = kRpOutside;
    if (x < k.width && y < k.height) {
        const size_t p = (size_t)y * k.width + x;
        const int32_t id = tg.obj_id[p];
        const float t = tg.hit_t[p];
        const float4 c = reinterpret_cast<const float4 *>(tg.color_f32)[p];
        float r = c.x, g = c.y, b = c.z, n1 = 0.0f;
        f3 nh = mk3(0.0f, 0.0f, 0.0f);
        kind = kRpBackground;
        if (id != -1) {
            kind = kRpFresh;
            n1 = 1.0f;
            if (id >= 0) {
                const float4 v = *reinterpret_cast<const float4 *>(tris[id].nhat);
                nh = mk3(v.x, v.y, v.z);
            }
            if (k.have_prev) {
                const float fw = (float)k.width, fh = (float)k.height;
                const f3 Dc = normalize3(ray_dir_unnormalized(cam, (float)x + 0.5f, (float)y + 0.5f, fw, fh));
                const f3 P = along(ld3(cam.origin), t, Dc);
                const f3 d = sub3(P, ld3(k.prev.o));
                const f3 nrm = ld3(k.prev.nrm);
                const float den = dot3(nrm, d);
                const float mu = k.prev.nc0 / den;
                if (mu > 0.0f) {   // (false for NaN: den = 0 has no history)
                    const f3 rr = mk3(mu * d.x - k.prev.c0[0], mu * d.y - k.prev.c0[1], mu * d.z - k.prev.c0[2]);
                    const float xn = dot3(cross3(rr, ld3(k.prev.cy)), nrm) / k.prev.nn;
                    const float yn = dot3(cross3(ld3(k.prev.cx), rr), nrm) / k.prev.nn;
                    const float fx = (xn + 1.0f) * 0.5f * fw - 0.5f, fy = (yn + 1.0f) * 0.5f * fh - 0.5f;
                    // beyond these bounds (or not finite) all four taps lie outside the frame
                    if (fx >= -1.0f && fx < fw && fy >= -1.0f && fy < fh) {
                        const float x0f = floorf(fx), y0f = floorf(fy);
                        const float a = fx - x0f, bb = fy - y0f;
                        const int x0 = (int)x0f, y0 = (int)y0f;
                        const float te = sqrtf(dot3(d, d));
                        const float tol = k.depth_rel * te;
                        float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f;
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const int qx = x0 + (j & 1), qy = y0 + (j >> 1);
                            if (qx < 0 || qy < 0 || qx >= (int)k.width || qy >= (int)k.height) continue;   // skipped, not clamped
                            const size_t q = (size_t)qy * k.width + (uint32_t)qx;
                            const int32_t idq = hp.id[q];
                            const float4 gq = hp.guide[q];
                            const bool same = idq == id || (id >= 0 && idq >= 0 && dot3(nh, mk3(gq.x, gq.y, gq.z)) >= k.cos_min);
                            if (!same || !(__builtin_fabsf(te - gq.w) <= tol)) continue;
                            const float4 hq = hp.colour[q];
                            const float w = ((j & 1) ? a : 1.0f - a) * ((j >> 1) ? bb : 1.0f - bb);
                            sw += w;
                            sr += w * hq.x; sg += w * hq.y; sb += w * hq.z;
                            sn += w * hq.w;
                        }
                        if (sw > 0.0f) {
                            kind = kRpReused;
                            const float hr = sr / sw, hg = sg / sw, hb = sb / sw;
                            n1 = __builtin_fminf(sn / sw + 1.0f, k.max_history);
                            if (n1 != 1.0f) {   // (n' = 1: out is c_now itself)
                                r = hr + (c.x - hr) / n1; g = hg + (c.y - hg) / n1; b = hb + (c.z - hb) / n1;
                                reinterpret_cast<float4 *>(tg.color_f32)[p] = make_float4(r, g, b, c.w);
                                reinterpret_cast<uint32_t *>(tg.color)[p] = pack_rgba8(r, g, b, c.w);
                            }
                        }
                    }
                }
            }
        }
        hn.colour[p] = make_float4(r, g, b, n1);
        hn.guide[p] = make_float4(nh.x, nh.y, nh.z, t);
        hn.id[p] = id;
    }
    const unsigned long long active = __ballot(true);
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t e = 0; e < 3u; e++) {
        const uint32_t n = (uint32_t)__popcll(__ballot(kind == e));
        if (n && lane == (uint32_t)__builtin_ctzll(active)) atomicAdd(&counts[e], (unsigned long long)n);
    }
}

hipError_t launch_wf_reproject(hipStream_t s, uint32_t width, uint32_t height, const TriRecord *tris, const Targets &tg,
                               const rwr_camera_inv_uniform &cam, const RpCamera *prev, const rwr_reproject_params &rp,
                               const RpHistory &from, const RpHistory &to, unsigned long long *counts)
{
    if (width == 0u || height == 0u) return hipSuccess;
    RpConsts k{};
    if (prev) k.prev = *prev;
    k.cos_min = rp.normal_cos_min;
    k.depth_rel = rp.depth_rel;
    k.max_history = (float)rp.max_history;
    k.width = width;
    k.height = height;
    k.have_prev = prev ? 1u : 0u;
    hipLaunchKernelGGL(k_wf_reproject, dim3((width + 63u) / 64u, (height + 3u) / 4u), dim3(256), 0, s, k, cam, tris, tg, from, to, counts);
    return hipGetLastError();
}

}  // namespace rwr
