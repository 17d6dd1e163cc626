// RWR_FLAG_TONEMAP: exposure and a tone curve, the last stage behind the wavefront integrator's resolve (include/rwr_hip.h,
// DESIGN.md §6).  The stage reads the frame's colour_f32 plane and rewrites its rgba8 plane; nothing else moves.
//   k_tm_measure (auto-exposure only): the frame's sum of luminance logs and its count of pixels with alpha.  Every lane loads whole
//     16-byte pixels, a wave one 1 KiB row of the plane per instruction; the logs are exact integers (rwr_tonemap.h), so lanes,
//     waves and workgroups add them in any order to the same bits.  A wave reduces across its lanes, the four waves through LDS,
//     and the workgroup adds once to the slot's record: one 64-bit and one 32-bit atomic.  The grid is capped and strides, so a
//     4K frame issues 4 096 atomics, not 65 000.
//   k_tm_exposure: one lane turns the record into the frame's exposure E (a 64-bit floor division, once per frame).
//   k_tm_apply: two pixels per lane, 256 apart, their components side by side in an f2 — v_pk_mul_f32 / v_pk_add_f32 for the
//     curves' polynomials, two IEEE divisions per channel — and one 4-byte store per pixel.  In manual mode E is an argument and
//     this is the stage's only launch.
// The arithmetic is the definition's, operation for operation (this translation unit: no contraction, IEEE division), so a frame's
// bytes equal tests/tonemap_ref.c on the same plane.
#include "rwr_device.h"
#include "rwr_tonemap.h"

namespace rwr {

namespace {

constexpr uint32_t kTmMeasureGroups = 2048u;   // k_tm_measure's grid at most: two atomics each

}  // namespace

__global__ void __launch_bounds__(256)
k_tm_measure(const float4 *__restrict__ colour, uint32_t n, TonemapRecord *__restrict__ rec)
{
    __shared__ long long s_sum[4];
    __shared__ uint32_t s_count[4];
    long long sum = 0;
    uint32_t count = 0u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {   // (n <= 2^30: i never wraps)
        const float4 c = colour[i];
        if (c.w != 0.0f) {
            sum += (long long)tonemap_luma_bits(c.x, c.y, c.z);
            count += 1u;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sum += __shfl_down(sum, off, 64);
        count += __shfl_down(count, off, 64);
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) { s_sum[wave] = sum; s_count[wave] = count; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        const long long total = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        const uint32_t counted = (s_count[0] + s_count[1]) + (s_count[2] + s_count[3]);
        if (counted != 0u) {   // (a workgroup of background pixels adds nothing)
            atomicAdd(reinterpret_cast<unsigned long long *>(&rec->log_sum), (unsigned long long)total);   // two's complement: the signed sum
            atomicAdd(&rec->count, counted);
        }
    }
}

__global__ void __launch_bounds__(64)
k_tm_exposure(TonemapRecord *__restrict__ rec, float key, float exposure)
{
    if (threadIdx.x == 0u) rec->exposure = tonemap_exposure(rec->log_sum, rec->count, 1u, key, exposure);
}

// rec: the measured frame's record (E is its last word), or null — E is the argument
template <uint32_t CURVE>
__global__ void __launch_bounds__(256)
k_tm_apply(const float4 *__restrict__ colour, uint32_t *__restrict__ rgba8, uint32_t n, const TonemapRecord *__restrict__ rec, float exposure, float iw2)
{
    const float E = rec ? rec->exposure : exposure;
    const uint32_t i0 = blockIdx.x * 512u + threadIdx.x, i1 = i0 + 256u;
    if (i0 >= n) return;
    const bool two = i1 < n;
    const float4 c0 = colour[i0];
    const float4 c1 = two ? colour[i1] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const f2 r = tonemap_curve(f2{c0.x, c1.x}, E, CURVE, iw2);
    const f2 g = tonemap_curve(f2{c0.y, c1.y}, E, CURVE, iw2);
    const f2 b = tonemap_curve(f2{c0.z, c1.z}, E, CURVE, iw2);
    rgba8[i0] = pack_rgba8(r.x, g.x, b.x, c0.w);
    if (two) rgba8[i1] = pack_rgba8(r.y, g.y, b.y, c1.w);
}

hipError_t launch_wf_tonemap(hipStream_t s, uint32_t width, uint32_t height, const Targets &tg, const rwr_tonemap_params &tp, TonemapRecord *rec)
{
    if (width == 0u || height == 0u) return hipSuccess;
    const uint32_t n = width * height;   // at most 2^30 (rwr_resize)
    const float4 *colour = reinterpret_cast<const float4 *>(tg.color_f32);
    uint32_t *rgba8 = reinterpret_cast<uint32_t *>(tg.color);
    const float iw2 = 1.0f / (tp.white * tp.white);
    if (tp.auto_exposure) {
        const hipError_t e = hipMemsetAsync(rec, 0, sizeof(TonemapRecord), s);
        if (e != hipSuccess) return e;
        const uint32_t groups = (n + 255u) / 256u;
        hipLaunchKernelGGL(k_tm_measure, dim3(groups < kTmMeasureGroups ? groups : kTmMeasureGroups), dim3(256), 0, s, colour, n, rec);
        hipLaunchKernelGGL(k_tm_exposure, dim3(1), dim3(64), 0, s, rec, tp.key, tp.exposure);
    } else {
        rec = nullptr;
    }
    const dim3 grid((n + 511u) / 512u);
    switch (tp.curve) {
    case kTonemapClamp: hipLaunchKernelGGL((k_tm_apply<kTonemapClamp>), grid, dim3(256), 0, s, colour, rgba8, n, rec, tp.exposure, iw2); break;
    case kTonemapReinhard: hipLaunchKernelGGL((k_tm_apply<kTonemapReinhard>), grid, dim3(256), 0, s, colour, rgba8, n, rec, tp.exposure, iw2); break;
    default: hipLaunchKernelGGL((k_tm_apply<kTonemapAces>), grid, dim3(256), 0, s, colour, rgba8, n, rec, tp.exposure, iw2); break;
    }
    return hipGetLastError();
}

}  // namespace rwr
