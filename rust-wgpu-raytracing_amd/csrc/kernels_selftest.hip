// Self-test of the short exact forms (rwr_device.h): they must return the very bits of the
// expressions they stand in for, on this GPU, for every input of their stated domain.
//   * to_non_linear_depth_fast vs to_non_linear_depth, sqrt_fast vs sqrtf: ALL 2^32 float bit patterns
//     are visited and every one inside the form's domain is compared (scalar and two-wide forms);
//   * normalize3_fast vs normalize3: 2^30 pseudo-random vectors spread over the whole domain of
//     normalize_fast_domain and a little beyond it (exponents 2^-44 .. 2^43 per component, all sign combinations;
//     vectors outside the domain are skipped, as the kernel skips them), plus the
//     two-wide form;
//   * the hit test's t = tnum / ndotd (rwr_device_p2.h hit_t): 2^30 rounds of pseudo-random pairs and the domain edges.
// Run through rwr_selftest_exact_math() by tests/test_gpu_exact_math.py and rwr_selftest_exact_div() by
// tests/test_gpu_exact_div.py.
#include "rwr_device_p2.h"

namespace rwr {

RWR_DEV bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

__global__ void __launch_bounds__(256)
k_selftest_depth(unsigned long long *out)  // out[0] compared, out[1] mismatches
{
    unsigned long long n = 0, bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float t = __uint_as_float((uint32_t)i);
        if (t >= 0x1p-100f && t <= 0x1p100f) {  // sqrt_fast's range
            const f2 sq = sqrt_fast(f2{t, t});
            const float want_sq = sqrtf(t);
            bad += !(same_bits(sqrt_fast(t), want_sq) && same_bits(sq.x, want_sq) && same_bits(sq.y, want_sq));
        }
        if (!depth_fast_domain(t)) continue;
        const float want = to_non_linear_depth(t);
        const f2 pair = to_non_linear_depth_fast(f2{t, t});
        n++;
        bad += !(same_bits(to_non_linear_depth_fast(t), want) && same_bits(pair.x, want) && same_bits(pair.y, want));
    }
    atomicAdd(&out[0], n);
    atomicAdd(&out[1], bad);
}

// component k of pseudo-random vector i: sign, exponent in [-44, 43], 23 random mantissa bits
RWR_DEV float selftest_component(uint32_t i, uint32_t k, uint32_t seed)
{
    const uint32_t h = rng_hash(i, k, 0u, seed), g = rng_hash(i, k, 1u, seed);
    const uint32_t expo = 127u - 44u + g % 88u;
    return __uint_as_float((h & 0x80000000u) | (expo << 23) | (h & 0x007fffffu));
}

__global__ void __launch_bounds__(256)
k_selftest_normalize(unsigned long long *out, uint32_t count, uint32_t seed)  // out[2] compared, out[3] mismatches
{
    unsigned long long n = 0, bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;   // (64-bit: a count near 2^32 must not wrap the loop)
    for (uint64_t i64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < count; i64 += stride) {
        const uint32_t i = (uint32_t)i64;
        f3 a = mk3(selftest_component(i, 0u, seed), selftest_component(i, 1u, seed), selftest_component(i, 2u, seed));
        if ((i & 7u) == 0u) {  // every eighth vector: comparable magnitudes (what a camera produces)
            const float s = __builtin_fabsf(a.x);
            a.y = __builtin_copysignf(s * (1.0f + (float)(i >> 3 & 1023u) * 0x1p-10f), a.y);
            a.z = __builtin_copysignf(s * (0.5f + (float)(i >> 13 & 1023u) * 0x1p-11f), a.z);
        }
        if (!normalize_fast_domain(a)) continue;
        const f3 want = normalize3(a), got = normalize3_fast(a);
        const v3 a2 = v3{f2{a.x, a.y}, f2{a.y, a.z}, f2{a.z, a.x}};  // two different vectors side by side
        const bool ok2 = normalize_fast_domain(a2);
        const v3 got2 = normalize3_fast(a2);
        const f3 want2 = normalize3(mk3(a.y, a.z, a.x));
        n++;
        bool ok = same_bits(got.x, want.x) && same_bits(got.y, want.y) && same_bits(got.z, want.z);
        ok = ok && ok2 && same_bits(got2.x.x, want.x) && same_bits(got2.y.x, want.y) && same_bits(got2.z.x, want.z);
        ok = ok && same_bits(got2.x.y, want2.x) && same_bits(got2.y.y, want2.y) && same_bits(got2.z.y, want2.z);
        bad += !ok;
    }
    atomicAdd(&out[2], n);
    atomicAdd(&out[3], bad);
}

// arbitrary float: sign, exponent in [emin, emin + span), 23 random mantissa bits
RWR_DEV float selftest_float(uint32_t i, uint32_t k, uint32_t seed, int emin, uint32_t span)
{
    const uint32_t h = rng_hash(i, k, 0u, seed), g = rng_hash(i, k, 1u, seed);
    const uint32_t expo = (uint32_t)(127 + emin) + g % span;
    return __uint_as_float((h & 0x80000000u) | (expo << 23) | (h & 0x007fffffu));
}

// operands at and just beyond the edges of hit_t's domain, and the special values
__constant__ const float kDivEdgeNum[] = {0x1p-40f, -0x1p-40f, 0x1.fffffep-41f, -0x1.fffffep-41f, 0x1p40f, -0x1p40f, 0x1.000002p40f,
                                          -0x1.000002p40f, 0.0f, -0.0f, 0x1p-126f, 0x1p-149f, -0x1p-140f, __builtin_inff(), -__builtin_inff(),
                                          __builtin_nanf(""), 1.0f, -3.0f, 0x1.234566p-20f, 0x1.fffffep39f};
__constant__ const float kDivEdgeDen[] = {kEpsilon, -kEpsilon, 0x1.0c6f7ap-20f, -0x1.0c6f7ap-20f, 0x1p40f, -0x1p40f, 0x1.000002p40f,
                                          -0x1.000002p40f, 0x1p-40f, 0.0f, -0.0f, 0x1p-149f, -0x1p-126f, __builtin_inff(), -__builtin_inff(),
                                          __builtin_nanf(""), 1.0f, -1.0f, 0x1.fffffep-1f, 0x1p-19f};
constexpr uint32_t kDivEdges = sizeof(kDivEdgeNum) / sizeof(float);
static_assert(sizeof(kDivEdgeDen) == sizeof(kDivEdgeNum), "edge lists");

// hit_t (rwr_device_p2.h) against the IEEE quotient tnum / ndotd.  Every round: a wave-uniform numerator (as the face's
// is in the hit test) and a pair of denominators per lane, exponents 2^-44 .. 2^43 and 2^-24 .. 2^43 (so that some waves
// leave the domain).  out[0] / out[1]: in-domain elements compared through div_fast / mismatches; out[2] / out[3]: elements
// with |ndotd| >= kEpsilon or NaN (those whose t the hit test takes) compared through hit_t, the wave-uniform choice of
// short form or IEEE division / mismatches of t's bits or of its t < 0 mask.  Every eighth round puts edge operands in
// the numerator and in a quarter of the lanes; three rounds in eight draw every operand of the wave inside the domain
// (exponents 2^-40 .. 2^39 and 2^-19 .. 2^39), so that hit_t's own choice takes the short form there.
__global__ void __launch_bounds__(256)
k_selftest_div(unsigned long long *out, uint32_t count, uint32_t seed)
{
    unsigned long long n = 0, bad = 0, n_sel = 0, bad_sel = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;   // (64-bit: a count near 2^32 must not wrap the loop)
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < count; i0 += stride) {   // (wave-uniform loop)
        const bool spare = i0 + threadIdx.x >= count;
        const uint32_t i = (uint32_t)(i0 + threadIdx.x);
        const uint32_t w = __builtin_amdgcn_readfirstlane(i >> 6);
        const bool inside = (w & 7u) >= 1u && (w & 7u) <= 3u;
        float tnum = inside ? selftest_float(w, 0u, seed, -40, 80u) : selftest_float(w, 0u, seed, -44, 88u);
        f2 d = inside ? f2{selftest_float(i, 1u, seed, -19, 59u), selftest_float(i, 2u, seed, -19, 59u)}
                      : f2{selftest_float(i, 1u, seed, -24, 68u), selftest_float(i, 2u, seed, -24, 68u)};
        if ((w & 7u) == 0u) {
            const uint32_t r = w >> 3;
            tnum = kDivEdgeNum[r % kDivEdges];
            if ((lane & 3u) == 0u) d = f2{kDivEdgeDen[(r / kDivEdges + lane) % kDivEdges], kDivEdgeDen[(r + lane / 4u) % kDivEdges]};
        }
        if (spare) d = splat(1.0f);   // (the last round's spare lanes: in the domain, not counted)
        const f2 q = div_fast(splat(tnum), d);
        const f2 t = hit_t(tnum, d, abs2(d));
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const float dk = k ? d.y : d.x, want = tnum / dk;
            if (spare) continue;
            const float ad = __builtin_fabsf(dk);
            if (hit_div_num_domain(tnum) && ad >= kEpsilon && ad <= 0x1p40f) {
                n++;
                bad += !same_bits(k ? q.y : q.x, want);
            }
            if (!(ad < kEpsilon)) {
                const float got = k ? t.y : t.x;
                n_sel++;
                bad_sel += !same_bits(got, want) || ((got < 0.0f) != (want < 0.0f));
            }
        }
    }
    atomicAdd(&out[0], n);
    atomicAdd(&out[1], bad);
    atomicAdd(&out[2], n_sel);
    atomicAdd(&out[3], bad_sel);
}

// Shader clock and f32 VALU issue rate under load, for the roofline accounting of bench.py: every wave runs
// `iters` rounds of eight independent v_fma_f32 (MODE 0) or v_pk_fma_f32 (MODE 1) chains and stamps the shader
// cycle counter (s_memtime, one tick per shader cycle) and the constant 100 MHz counter (s_memrealtime) around
// them (MI355X_MICROARCH.md: in-kernel clock = d s_memtime / d s_memrealtime * 100 MHz).  out[wave] =
// {cycles, realtime ticks}.  The launch puts `waves_per_simd` waves on every SIMD at once.
template <int MODE>
__global__ void __launch_bounds__(256)
k_measure_valu(ulonglong2 *out, uint32_t iters, float s)
{
    float a0 = (float)threadIdx.x, a1 = a0 + 1.0f, a2 = a0 + 2.0f, a3 = a0 + 3.0f, a4 = a0 + 4.0f, a5 = a0 + 5.0f, a6 = a0 + 6.0f, a7 = a0 + 7.0f;
    f2 p0 = {a0, a1}, p1 = {a2, a3}, p2 = {a4, a5}, p3 = {a6, a7}, p4 = {a1, a0}, p5 = {a3, a2}, p6 = {a5, a4}, p7 = {a7, a6};
    const f2 sv = {s, s};
    __builtin_amdgcn_sched_barrier(0);
    const uint64_t c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    for (uint32_t i = 0; i < iters; i++) {
        if (MODE == 0) {   // (inline assembly: the compiler would pair adjacent scalar FMAs into v_pk_fma_f32)
            asm volatile("v_fma_f32 %0, %0, %8, %0\n\tv_fma_f32 %1, %1, %8, %1\n\tv_fma_f32 %2, %2, %8, %2\n\tv_fma_f32 %3, %3, %8, %3\n\t"
                         "v_fma_f32 %4, %4, %8, %4\n\tv_fma_f32 %5, %5, %8, %5\n\tv_fma_f32 %6, %6, %8, %6\n\tv_fma_f32 %7, %7, %8, %7"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(s));
        } else {
            p0 = fma2(p0, sv, p0); p1 = fma2(p1, sv, p1); p2 = fma2(p2, sv, p2); p3 = fma2(p3, sv, p3);
            p4 = fma2(p4, sv, p4); p5 = fma2(p5, sv, p5); p6 = fma2(p6, sv, p6); p7 = fma2(p7, sv, p7);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    const uint64_t c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    const float sink = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + p0.x + p0.y + p1.x + p1.y + p2.x + p2.y + p3.x + p3.y + p4.x + p4.y +
                       p5.x + p5.y + p6.x + p6.y + p7.x + p7.y;
    if ((threadIdx.x & 63u) == 0u || sink == 12345.678f)  // the sink keeps the chains alive
        out[(blockIdx.x * blockDim.x + threadIdx.x) >> 6] = make_ulonglong2(c1 - c0, r1 - r0);
}

// One wave that does nothing but watch the two counters for `ticks` ticks of the 100 MHz counter: launched on a
// side stream while frames render, it reports the shader clock the chip runs at UNDER THAT WORKLOAD (a pure FMA
// loop pulls the clock lower than the frame kernel does).
__global__ void __launch_bounds__(64)
k_clock_probe(ulonglong2 *out, uint32_t ticks)
{
    const uint64_t r0 = __builtin_amdgcn_s_memrealtime(), c0 = __builtin_amdgcn_s_memtime();
    uint64_t r1 = r0;
    while (r1 - r0 < ticks) {
        __builtin_amdgcn_s_sleep(32);
        r1 = __builtin_amdgcn_s_memrealtime();
    }
    const uint64_t c1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) out[0] = make_ulonglong2(c1 - c0, r1 - r0);
}

// RWR_FLAG_SOBOL: out[i] = rng_sobol of tuple i (rwr_device.h), for rwr_selftest_sobol and tests/test_gpu_sobol.py.
// in: the four columns one after the other, n words each (pixel, sample, dim, seed).
__global__ void __launch_bounds__(256)
k_selftest_sobol(const uint32_t *__restrict__ in, uint32_t n, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = rng_sobol(in[i], in[n + i], in[2u * n + i], in[3u * n + i]);
}

hipError_t launch_selftest_sobol(hipStream_t s, const uint32_t *d_in, uint32_t n, uint32_t *d_out)
{
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_sobol, dim3((n + 255u) / 256u), dim3(256), 0, s, d_in, n, d_out);
    return hipGetLastError();
}

// RWR_FLAG_SKY_IMAGE: out[3 i ...] = sky_image_radiance of direction i (rwr_device.h), for rwr_selftest_sky_image and
// tests/test_gpu_sky_image.py.
__global__ void __launch_bounds__(256)
k_selftest_sky_image(const WfSkyImage si, const float *__restrict__ dirs, uint32_t n, float *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const f3 s = sky_image_radiance(si.image, si.n, mk3(dirs[3u * i], dirs[3u * i + 1u], dirs[3u * i + 2u]));
    out[3u * i] = s.x; out[3u * i + 1u] = s.y; out[3u * i + 2u] = s.z;
}

hipError_t launch_selftest_sky_image(hipStream_t s, const WfSkyImage &si, const float *d_dirs, uint32_t count, float *d_out)
{
    if (count == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_sky_image, dim3((count + 255u) / 256u), dim3(256), 0, s, si, d_dirs, count, d_out);
    return hipGetLastError();
}

// RWR_FLAG_LIGHT_SKY: out[8 i ...] = the direction sky_light_draw makes of the four uniforms u4[4 i ...], its texel's column and row (as
// uint32 bits), P and g = sky_light_g of that direction against the normal (nx, ny, nz) among n_lights lights, 0 (rwr_device.h), for
// rwr_selftest_sky_light and tests/test_gpu_sky_light.py.
__global__ void __launch_bounds__(256)
k_selftest_sky_light(const WfSkyImage si, const float *__restrict__ u4, uint32_t n, float nx, float ny, float nz, uint32_t n_lights, float *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t ti, tj;
    const f3 w = sky_light_draw(si.table, si.n, u4[4u * i], u4[4u * i + 1u], u4[4u * i + 2u], u4[4u * i + 3u], true, ti, tj);
    float P = 0.0f;
    const float g = sky_light_g(si.table, si.n, w, dot3(mk3(nx, ny, nz), w), (float)n_lights, ti, tj, P);
    out[8u * i] = w.x; out[8u * i + 1u] = w.y; out[8u * i + 2u] = w.z;
    out[8u * i + 3u] = __uint_as_float(ti); out[8u * i + 4u] = __uint_as_float(tj);
    out[8u * i + 5u] = P; out[8u * i + 6u] = g; out[8u * i + 7u] = 0.0f;
}

hipError_t launch_selftest_sky_light(hipStream_t s, const WfSkyImage &si, const float *d_u4, uint32_t count, const float nrm[3], uint32_t n_lights, float *d_out)
{
    if (count == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_selftest_sky_light, dim3((count + 255u) / 256u), dim3(256), 0, s, si, d_u4, count, nrm[0], nrm[1], nrm[2], n_lights, d_out);
    return hipGetLastError();
}

hipError_t launch_selftest_exact_div(hipStream_t s, unsigned long long *d_out4, uint32_t count, uint32_t seed)
{
    hipLaunchKernelGGL(k_selftest_div, dim3(8192), dim3(256), 0, s, d_out4, count, seed);
    return hipGetLastError();
}

hipError_t launch_clock_probe(hipStream_t s, ulonglong2 *d_out, uint32_t ticks)
{
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, s, d_out, ticks);
    return hipGetLastError();
}

hipError_t launch_measure_valu(hipStream_t s, int mode, ulonglong2 *d_out, uint32_t n_workgroups, uint32_t iters)
{
    if (mode == 0) hipLaunchKernelGGL((k_measure_valu<0>), dim3(n_workgroups), dim3(256), 0, s, d_out, iters, 1.0001f);
    else hipLaunchKernelGGL((k_measure_valu<1>), dim3(n_workgroups), dim3(256), 0, s, d_out, iters, 1.0001f);
    return hipGetLastError();
}

hipError_t launch_selftest_exact_math(hipStream_t s, unsigned long long *d_out4, uint32_t normalize_count, uint32_t seed)
{
    hipLaunchKernelGGL(k_selftest_depth, dim3(8192), dim3(256), 0, s, d_out4);
    hipLaunchKernelGGL(k_selftest_normalize, dim3(8192), dim3(256), 0, s, d_out4, normalize_count, seed);
    return hipGetLastError();
}

}  // namespace rwr
