// Wavefront integrator, first stage (extension; BASELINE.json configs 2-4 — the reference traces one centre
// ray per pixel and has no samples or bounces; specification: DESIGN.md "Extended integrator",
// restated brute force in oracle/rt_oracle.c or_render_path).
//
//   k_wf_primary   ONE launch traces a whole GROUP of samples (up to 32) of every pixel.  Same mapping as the
//                  fused frame kernel (kernels_primary_p2.hip): wave64 = 32x4-pixel tile, two horizontally
//                  adjacent pixels per lane (v_pk_* arithmetic), per-wave culling against the per-frame
//                  FrameTri records, face records in scalar registers, no LDS, no barrier.  Per sample: jittered
//                  ray (counter-based RNG keyed by GLOBAL pixel, sample, seed), spheres + mesh with the
//                  reference's depth compositing, local shading E(h0); the group's E(h0) are summed in
//                  registers as fixed point and added to the frame's integer planes ONCE per group (not per
//                  sample).  A pixel that hit a surface builds
//                  its cosine-distributed bounce ray and stores it at its FIXED slot of the ray queue in HBM
//                  (coalesced 16-byte stores, rwr_internal.h WfBuffers); the wave publishes the ballot of the
//                  lanes that emitted.  Compaction — ballot + prefix popcount — happens in the consumer
//                  (kernels_wf_bounce.hip), folded into the sort of the tile's ray pool by direction.
//                  Rays that left the scene cost nothing downstream.
//   k_wf_classify  frames that show little: lists the tiles anything can be seen through, so that k_wf_primary<LIST>
//                  takes (listed tile, share of its samples) items instead of grid coordinates (see there).
//
// Everything that decides what a sample sees (ray, hit tests, selection, depth, bounce ray) is written operation
// for operation like the oracle, so sample-0 planes are bit-exact and every bounce ray is the oracle's.
#include <hip/hip_ext.h>

#include <algorithm>

#include "rwr_primary.h"
#include "rwr_shade_p2.h"
#include "rwr_wf_cull.h"
#include "rwr_wf_forms.h"

namespace rwr {

// rng_hash (rwr_device.h) in two steps: everything up to the dimension is shared by the uniforms of one
// (pixel, sample).  rng_dim(rng_base(pixel, sample, seed), dim) == rng_hash(pixel, sample, dim, seed).
RWR_DEV uint32_t rng_base(uint32_t pixel, uint32_t sample, uint32_t seed)
{
    uint32_t h = seed ^ 0x9E3779B9u;
    h = rng_mix(h ^ pixel);
    return rng_mix(h ^ (sample * 0x85EBCA6Bu));
}
RWR_DEV float rng_dim(uint32_t base, uint32_t dim)
{
    return (float)(rng_mix(base ^ (dim * 0xC2B2AE35u)) >> 8) * (1.0f / 16777216.0f);
}
// RWR_FLAG_SOBOL (sobol: wave-uniform): `base` is sobol_pixel of the pixel instead, which the sample does not enter — the
// sequence's steps take it.  rng_draw2: the uniforms of dimensions dim and dim + 1, dim even, one pair of the sequence.
RWR_DEV uint32_t rng_base(uint32_t pixel, uint32_t sample, uint32_t seed, bool sobol)
{
    return sobol ? sobol_pixel(pixel, seed) : rng_base(pixel, sample, seed);
}
RWR_DEV float rng_draw(uint32_t base, uint32_t sample, uint32_t dim, bool sobol)
{
    return sobol ? rng_to_unit(sobol_coord(sobol_pair(base, sample, dim), dim & 1u)) : rng_dim(base, dim);
}
RWR_DEV void rng_draw2(uint32_t base, uint32_t sample, uint32_t dim, bool sobol, float &u0, float &u1)
{
    if (sobol) {
        const SobolPair q = sobol_pair(base, sample, dim);
        u0 = rng_to_unit(sobol_coord(q, 0u));
        u1 = rng_to_unit(sobol_coord(q, 1u));
    } else {
        u0 = rng_dim(base, dim);
        u1 = rng_dim(base, dim + 1u);
    }
}

// n / d for a wave-uniform positive integer-valued d (the frame's width or height) and 0 <= n < 2^16: the
// compiler's IEEE expansion of the quotient with the reciprocal refined once per wave and the instructions that
// are the identity on such operands left out (rwr_device.h div_shared_rcp; zero numerators give +0 either way).
RWR_DEV float refined_rcp(float d)
{
    const float r = __builtin_amdgcn_rcpf(d);
    return __builtin_fmaf(__builtin_fmaf(-d, r, 1.0f), r, r);
}

// pixelToRay (compute.wgsl:150-164) for the pixel-space points (fx.x, fy.x) and (fx.y, fy.y).
template <typename Cam>   // rwr_camera_inv_uniform, possibly in the kernel-argument address space
RWR_DEV v3 pixel_pair_ray_dir_at(const Cam &cam, f2 fx, f2 fy, float width, float height, float rw, float rh)
{
    const f2 x_nds = div_shared_rcp(2.0f * fx, splat(width), splat(rw)) - 1.0f;
    const f2 y_nds = div_shared_rcp(2.0f * fy, splat(height), splat(rh)) - 1.0f;
    const auto &p = cam.proj_inv;
    const f2 vx = p[0][0] * x_nds + p[1][0] * y_nds + p[2][0] * 1.0f + p[3][0] * 1.0f;
    const f2 vy = p[0][1] * x_nds + p[1][1] * y_nds + p[2][1] * 1.0f + p[3][1] * 1.0f;
    const f2 vz = p[0][2] * x_nds + p[1][2] * y_nds + p[2][2] * 1.0f + p[3][2] * 1.0f;
    const f2 vw = splat(0.0f);
    const auto &m = cam.viewmodel_inv;
    v3 w;
    w.x = m[0][0] * vx + m[1][0] * vy + m[2][0] * vz + m[3][0] * vw;
    w.y = m[0][1] * vx + m[1][1] * vy + m[2][1] * vz + m[3][1] * vw;
    w.z = m[0][2] * vx + m[1][2] * vy + m[2][2] * vz + m[3][2] * vw;
    if (__all(normalize_fast_domain(w))) return normalize3_fast(w);
    return normalize3(w);
}

// bounce_direction (rwr_device.h) for a pixel pair; lanes / elements whose `want` is 0 still compute (cheaply
// wrong values are never stored).  base: rng_base of each pixel for this sample.
RWR_DEV v3 bounce_direction_pair(v3 n, u2 base, i2 want, uint32_t sample, bool sobol)
{
    // Rejection-sample the unit disk (up to 8 tries per pixel, a = b = 0 when all fail).  78.5 % of the tries
    // succeed: the first try runs for both pixels at once; for the rest a lane takes ONE try of ONE pixel per
    // iteration (first its left pixel's, then its right pixel's), so a wave iterates max over lanes of the tries
    // both pixels still need, not 2 x max over pixels.
    f2 a = splat(0.0f), b = splat(0.0f);
    i2 need = want;
    {
        float x0, x1, y0, y1;
        rng_draw2(base.x, sample, 2u, sobol, x0, x1);
        rng_draw2(base.y, sample, 2u, sobol, y0, y1);
        const f2 ua = 2.0f * f2{x0, y0} - 1.0f;
        const f2 ub = 2.0f * f2{x1, y1} - 1.0f;
        const i2 ok = need & ((ua * ua + ub * ub) <= 1.0f);
        a = ok ? ua : a;
        b = ok ? ub : b;
        need &= ~ok;
    }
    bool busy = any2(need);
    uint32_t sel = need.x ? 0u : 1u, k = 1u;
    while (__any(busy)) {
        if (busy) {
            const uint32_t bs = sel ? base.y : base.x;
            float u0, u1;
            rng_draw2(bs, sample, 2u + 2u * k, sobol, u0, u1);
            const float ua = 2.0f * u0 - 1.0f;
            const float ub = 2.0f * u1 - 1.0f;
            const bool ok = (ua * ua + ub * ub) <= 1.0f;
            if (ok) {
                if (sel) { a.y = ua; b.y = ub; } else { a.x = ua; b.x = ub; }
            }
            if (ok || k == 7u) {          // this pixel is done: on to the lane's other pixel, or out
                if (sel == 0u && need.y) { sel = 1u; k = 1u; }
                else busy = false;
            } else {
                k++;
            }
        }
    }
    const f2 rad = 1.0f - a * a - b * b;
    const f2 clamped = f2{fmaxf(0.0f, rad.x), fmaxf(0.0f, rad.y)};
    // sqrt_fast returns sqrtf's bits on [2^-100, 2^100] (rwr_device.h); 0 and the rare tiny radicand take the long form
    const bool sq_fast = __all(clamped.x >= 0x1p-100f && clamped.y >= 0x1p-100f);
    const f2 dz = sq_fast ? sqrt_fast(clamped) : sqrt2(clamped);
    const f2 sign = f2{copysignf(1.0f, n.z.x), copysignf(1.0f, n.z.y)};
    const f2 aa = -1.0f / (sign + n.z);
    const f2 bb = n.x * n.y * aa;
    const v3 b1 = v3{1.0f + sign * n.x * n.x * aa, sign * bb, -sign * n.x};
    const v3 b2 = v3{bb, sign + n.y * n.y * aa, -n.y};
    v3 d = v3{a * b1.x + b * b2.x + dz * n.x, a * b1.y + b * b2.y + dz * n.y, a * b1.z + b * b2.z + dz * n.z};
    // elements nobody wants get a harmless in-domain vector, so that they do not push the wave onto the long form
    d.x = want ? d.x : splat(1.0f); d.y = want ? d.y : splat(1.0f); d.z = want ? d.z : splat(1.0f);
    if (__all(normalize_fast_domain(d))) return normalize3_fast(d);
    return normalize3(d);
}

// gloss_direction (rwr_device.h) for a pixel pair: X is the pair's diffuse direction (bounce_direction_pair), rho each pixel's
// roughness.  Elements that are not glossy still compute; the caller selects.
RWR_DEV v3 gloss_direction_pair(v3 n, v3 D, v3 X, f2 rho)
{
    const v3 Dh = normalize3(D);
    const f2 two_d = 2.0f * dot3(n, Dh);
    const v3 Rf = v3{Dh.x - two_d * n.x, Dh.y - two_d * n.y, Dh.z - two_d * n.z};
    const f2 om = 1.0f - rho;
    const v3 S = v3{om * Rf.x + rho * X.x, om * Rf.y + rho * X.y, om * Rf.z + rho * X.z};
    const i2 ok = dot3(S, S) > 0.0f;
    return v3{ok ? S.x : Rf.x, ok ? S.y : Rf.y, ok ? S.z : Rf.z};
}

#ifndef RWR_WF_OCC
#define RWR_WF_OCC 4
#endif
// The kernel's ONE argument.  The sample loop is long and uses some 130 wave-uniform words — camera matrices, spheres and their
// rectangles, a dozen pointers, the face record under test — against 102 scalar registers; the compiler hoists every
// kernel-argument load out of the loop and then spills (round 2: 86-135 scalar spills through v_writelane / v_readlane, 11-26
// vector registers in scratch).  So the loop reads what a phase needs through a pointer to the kernel-argument segment that is
// RE-DERIVED at the phase (wf_args_again: an empty asm the compiler cannot see through), i.e. by scalar loads from the constant
// cache where the values are used; they are dead again before the next phase.
struct WfPrimaryArgs {
    const FrameTri *ftris;
    uint32_t n_tris, row_begin, bins_enabled;
    int32_t mesh_x0, mesh_y0, mesh_x1, mesh_y1;
    uint32_t sample_begin, sample_count, z_split;
    FrameParams p;
    const TriRecord *tris;
    const ShadeRec *shade;
    const float4 *tex;
    Targets tg;
    WfBuffers wf;
    WfShadow sw;   // RWR_FLAG_SHADOWS (the SHADOW forms); behind the rest, so that the other forms read their arguments where they always did
    WfSurfaces surfaces;   // RWR_FLAG_MIRRORS, _GLASS, _GLOSSY (the surface forms); behind the rest, for the same reason
    WfGlow glow;           // RWR_FLAG_EMISSIVE (the GLOW forms); last, for the same reason
};
template <typename T> using kernarg = const __attribute__((address_space(4))) T;
RWR_DEV kernarg<WfPrimaryArgs> *wf_args_again(kernarg<WfPrimaryArgs> *q)
{
    asm volatile("" : "+s"(q));
    return q;
}
RWR_DEV f3 ld3(kernarg<float> *q) { return mk3(q[0], q[1], q[2]); }

// SHADOW (RWR_FLAG_SHADOWS): a hit adds the AMBIENT part of E(h0) to the group's sums and leaves a shadow record — the bounce
// ray's origin, the light of the shader that shaded it, fix(E) - fix(ambient) — at its queue slot, with its bit in the shadow
// ballots, for k_wf_shadow (kernels_wf_shadow.hip).  Forms of their own: the others keep their registers.
// MIRROR (RWR_FLAG_MIRRORS): a hit on a mirror surface (WfSurfaces' table: per part, per sphere) emits the reflection of its ray
// with throughput R instead of the cosine-distributed ray with the albedo, decided per pixel of the lane's pair.  A tile without
// a mirror hit skips the reflection, a tile whose emitting pixels are all mirror hits skips the RNG and the disk-to-hemisphere
// arithmetic (wave-uniform branches on ballots), a mixed tile computes both and selects.  Forms of their own again.
// SURF (rwr_surface.h): kSurfNone, kSurfMirrors — the MIRROR forms — or kSurfGlass (RWR_FLAG_GLASS, with or without mirrors): a hit
// on glass emits the reflected or the refracted ray of refract_or_reflect from P + 1e-4 m with throughput C, decided per pixel too.
// A tile without a glass hit skips that arithmetic, a tile whose emitting pixels are all specular skips the RNG disk loop.
// kSurfGloss (RWR_FLAG_GLOSSY, with or without the other two): a glossy hit draws the diffuse direction like a diffuse one and
// sends gloss_direction_pair's ray on with throughput R; a tile without a glossy hit skips that arithmetic.
// GLOW (RWR_FLAG_EMISSIVE): the radiance Le of the hit's surface (WfGlow's table, rwr_surface.h glow_record) is added to the shader's
// E(h0) — and, under SHADOW, to its ambient part: a surface's own light is not shadowed — ahead of the conversion, one f32 add per
// channel; the hits with Le != 0 are counted.  Rays, planes and counts are the twin's.  Forms of their own again.
template <bool AUX, bool CULL, bool NMAP, bool LIST = false, bool SHADOW = false, int SURF = kSurfNone, bool GLOW = false>
// (LIST — frames that show little — keeps an item loop's state on top of everything else and needs 142 registers: three waves
// per SIMD like the AUX / NMAP forms; such a frame does not fill the chip anyway.  MIRROR does not loosen the bound: the plain
// mirror forms hold RWR_WF_OCC waves like their twins, profiles/mirror_kernel_resources.txt)
__global__ void __launch_bounds__(256, (AUX || NMAP || LIST || SHADOW) ? 3 : RWR_WF_OCC)
k_wf_primary(const WfPrimaryArgs a)
{
    constexpr bool MIRROR = SURF != kSurfNone, GLASS = SURF == kSurfGlass || SURF == kSurfGloss, GLOSS = SURF == kSurfGloss;
    kernarg<WfPrimaryArgs> *const ka = (kernarg<WfPrimaryArgs> *)__builtin_amdgcn_kernarg_segment_ptr();
    const uint32_t sample_begin = a.sample_begin, sample_count = a.sample_count, z_split = a.z_split;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    // the bounce stage's counters for this queue start from zero (nothing reads them before this kernel has ended)
    if (a.wf.counters && (blockIdx.x | blockIdx.y | blockIdx.z) == 0u && threadIdx.x < 4u) a.wf.counters[threadIdx.x] = 0u;
    // which tile, which share of its samples: the launch grid's (x, y, z) — or, on a frame that shows little, item after item
    // of (live tile of k_wf_classify's list) x (share), so that no workgroup is spent on finding its tile empty
    uint32_t bx = blockIdx.x, by = blockIdx.y, z = blockIdx.z;
    uint32_t item = blockIdx.x, n_items = 0u;
    if (LIST) n_items = (uint32_t)__builtin_amdgcn_readfirstlane((int)*a.wf.live_count) * z_split;
    do {
    kernarg<WfPrimaryArgs> *const qi = wf_args_again(ka);   // this tile's set-up: culling inputs, the frame's size and band
    const uint32_t tiles_x = qi->wf.tiles_x;
    if (LIST) {
        if (item >= n_items) break;
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)qi->wf.live_list[item / z_split]);
        z = item % z_split;
        by = t / tiles_x;
        bx = t - by * tiles_x;
        item += gridDim.x;
    }
    const uint32_t row_begin = qi->row_begin, width = qi->p.width;
    const uint32_t blk_x0 = bx * kWfTileW;
    const uint32_t tile_x0 = blk_x0 + (wave & 1u) * 32u;
    const uint32_t tile_y0 = row_begin + by * qi->p.row_pitch + (wave >> 1) * 4u;
    const uint32_t px0 = tile_x0 + 2u * (lane & 15u), py = tile_y0 + (lane >> 4);
    constexpr float kTileWf = 32.0f, kTileHf = 4.0f;
    const bool in0 = py < qi->p.row_end && px0 < width, in1 = in0 && (px0 + 1u < width);
    const uint32_t pix0 = py * width + px0;  // GLOBAL pixel index: RNG key and accumulator slot (< 2^30, rwr_resize)
    const uint32_t tile = by * tiles_x + bx;

    // candidate faces of this wave's tile: rwr_wf_cull.h (shared with k_wf_classify)
    const FrameTri *__restrict__ ftris = qi->ftris;
    const WfWaveCull wc = wf_wave_cull<CULL>(ftris, qi->n_tris, row_begin, qi->bins_enabled, qi->mesh_x0, qi->mesh_y0, qi->mesh_x1, qi->mesh_y1,
                                             qi->p.bins, blk_x0, row_begin + by * qi->p.row_pitch, wave, lane);
    const uint32_t n_src = wc.n_src;
    const uint32_t *__restrict__ src = wc.src;
    const float tx0 = (float)tile_x0, ty0 = (float)tile_y0;
    const TileRect tile_rect = {tx0, ty0, tx0 + kTileWf, ty0 + kTileHf};
    const bool cached = wc.cached;
    const unsigned long long cm0 = wc.cm0, cm1 = wc.cm1;
    const uint32_t cf0 = wc.cf0, cf1 = wc.cf1;

    // the group's sums of E(h0) per pixel as 2^-22 fixed point in 32 bits (a sample's term is clamped to kWfE0Cap = 16 — part of
    // the integrator's definition, rwr_hip.h / oracle render_path_core — so a whole group of <= 64 fits; shifted into the planes'
    // 2^-26 units at the end: WfBuffers::fix), and its primary hits
    uint32_t fr0 = 0, fg0 = 0, fb0 = 0, fr1 = 0, fg1 = 0, fb1 = 0;
    uint32_t hits0 = 0, hits1 = 0;
    uint32_t emitted = 0;  // rays this wave emitted in this launch (wave-uniform)
    // z_split workgroups share a tile's samples (sample z, z + z_split, ...): on a frame that shows a small mesh a wave
    // would otherwise trace all the group's samples one after the other while most of the chip idles

    // A tile no face and no sphere can be seen through (conservative bounds: nothing any jittered ray of its pixels could
    // hit) has nothing to trace in any sample: its pixels keep the clear values.  On a frame that shows a small mesh
    // that is most tiles.
    const bool empty_tile = wf_wave_empty<CULL>(wc, qi->p, tx0, ty0);
    if (empty_tile && sample_begin == 0u && z == 0u && in0) {   // sample 0's planes
        qi->tg.depth[pix0] = 0.0f;
        if (AUX) { qi->tg.obj_id[pix0] = -1; qi->tg.hit_t[pix0] = 0.0f; }
        if (in1) {
            qi->tg.depth[pix0 + 1u] = 0.0f;
            if (AUX) { qi->tg.obj_id[pix0 + 1u] = -1; qi->tg.hit_t[pix0 + 1u] = 0.0f; }
        }
    }
    if (empty_tile && qi->p.bounces != 0u && lane == 0u && z == 0u)    // nothing emitted: the bounce stage sees empty ballots
        for (uint32_t sidx = 0; sidx < sample_count; sidx++) {
            unsigned long long *mk = qi->wf.masks + (size_t)(tile * qi->wf.group + sidx) * 8u + wave * 2u;
            mk[0] = 0ull; mk[1] = 0ull;
        }
    if (SHADOW && empty_tile && lane == 0u && z == 0u)   // ... and no shadow records
        for (uint32_t sidx = 0; sidx < sample_count; sidx++) {
            unsigned long long *mk = qi->sw.masks + (size_t)(tile * qi->wf.group + sidx) * 8u + wave * 2u;
            mk[0] = 0ull; mk[1] = 0ull;
        }

    for (uint32_t sidx = z; sidx < (empty_tile ? 0u : sample_count); sidx += z_split) {
        const uint32_t sample = sample_begin + sidx;
        // -- the sample's ray: pixel centre at spp = 1, else (and in every accumulating frame) two uniforms of the counter-based RNG
        kernarg<WfPrimaryArgs> *const qr = wf_args_again(ka);   // this phase's kernel arguments: seed, jitter rule, the camera
        const bool sobol = (qr->p.flags & RWR_FLAG_SOBOL) != 0u;   // (scalar) the sequence's numbers in place of the hash's
        const u2 base = u2{rng_base(pix0, sample, qr->p.seed, sobol), rng_base(pix0 + 1u, sample, qr->p.seed, sobol)};
        f2 jx = splat(0.5f), jy = splat(0.5f);
        if (qr->p.jitter_spp > 1u) {
            float x0, x1, y0, y1;
            rng_draw2(base.x, sample, 0u, sobol, x0, x1);
            rng_draw2(base.y, sample, 0u, sobol, y0, y1);
            jx = f2{x0, y0};
            jy = f2{x1, y1};
        }
        const f2 fx = f2{(float)px0, (float)(px0 + 1u)} + jx;
        const f2 fy = splat((float)py) + jy;
        const float fw = (float)qr->p.width, fh = (float)qr->p.height;   // (8 instructions a sample against 4-8 registers across the loop)
        const v3 D = pixel_pair_ray_dir_at(qr->p.cam, fx, fy, fw, fh, refined_rcp(fw), refined_rcp(fh));
        const f3 O = ld3(qr->p.cam.origin);

        f2 depth_tex = splat(0.0f), win_t = splat(0.0f);
        i2 obj = i2{-1, -1};
        // -- analytic sphere passes, in order (lib.rs:1106-1173) ------------------------------------------------
        kernarg<WfPrimaryArgs> *const qs = wf_args_again(ka);   // the spheres and their screen rectangles
        const uint32_t n_spheres = qs->p.n_spheres;
        for (uint32_t s = 0; s < n_spheres; s++) {
            if (CULL && ((tx0 + kTileWf < qs->p.sphere_rect[s][0]) || (tx0 > qs->p.sphere_rect[s][2]) ||
                         (ty0 + kTileHf < qs->p.sphere_rect[s][1]) || (ty0 > qs->p.sphere_rect[s][3])))
                continue;
            f2 t = splat(0.0f);
            const i2 hit = sphere_ray_intersect_t(ld3(qs->p.spheres[s].center), qs->p.spheres[s].radius, O, D, t);
            if (any2(hit)) {
                const f2 current_depth = 1.0f - depth_tex;  // sphere/compute.wgsl:130
                const f2 depth = to_non_linear_depth(t);
                const i2 win = hit & ~(depth >= current_depth);
                depth_tex = win ? (1.0f - depth) : depth_tex;
                obj = win ? i2{-2 - (int)s, -2 - (int)s} : obj;
                win_t = win ? t : win_t;
            }
        }
        // -- mesh pass (lib.rs:1174-1184): per-wave culling, survivors in ascending face order ------------------
        MeshHit2 best;
        best.have = i2{0, 0};
        best.t = best.u = best.v = best.ndotd = splat(0.0f);
        best.idx = u2{0u, 0u};
        uint32_t n_tested = 0;
        ShadeRec last_shade = {};
        // survivors in ascending face order; wave-uniform face index: the record comes in through scalar loads.
        // Samples jitter the ray, never the origin: the plane numerator is the frame's per-face table.
        kernarg<WfPrimaryArgs> *const qm = wf_args_again(ka);   // the face records, the shading records, the numerators
        const const_ptr<TriRecord> tris_c = to_const_space(qm->tris);
        const const_ptr<ShadeRec> shade_c = to_const_space(qm->shade);
        const const_ptr<float> tnum_c = to_const_space(qm->p.tnum);
        auto walk = [&](unsigned long long m, uint32_t faces_v) {
            while (m) {
                const uint32_t b = (uint32_t)__builtin_ctzll(m);
                m &= m - 1ull;
                const uint32_t idx = (uint32_t)__builtin_amdgcn_readlane((int)faces_v, (int)b);
                intersect_and_select(load_tri_record(tris_c + idx), tnum_c[idx], idx, O, D, best);
                n_tested++;
                last_shade = load_shade_record(shade_c + idx);
            }
        };
        if (cached) {
            walk(cm0, cf0);
            walk(cm1, cf1);
        } else {
            for (uint32_t base_f = 0; base_f < n_src; base_f += 64u) {
                const uint32_t e = base_f + lane;
                bool keep = e < n_src;
                const uint32_t my_face = (keep && src) ? src[e] : e;
                if (CULL && keep) keep = !rect_culls(ftris[my_face], tile_rect);
                walk(__ballot(keep), my_face);
            }
        }
        if (any2(best.have)) {
            const f2 current_depth = 1.0f - depth_tex;  // compute.wgsl:210
            const bool fast = !__any(any2(best.have & ~depth_fast_domain(best.t)));
            const f2 depth = fast ? to_non_linear_depth_fast(best.t) : to_non_linear_depth(best.t);
            const i2 win = best.have & ~(depth >= current_depth);
            depth_tex = win ? (1.0f - depth) : depth_tex;
            obj = win ? i2{(int)best.idx.x, (int)best.idx.y} : obj;
            win_t = win ? best.t : win_t;
        }
        if (sample == 0u && in0) {  // depth / aux planes report sample 0
            kernarg<WfPrimaryArgs> *const qt = wf_args_again(ka);   // the targets (once per frame and pixel: addresses made here, not kept)
            float *const depth_plane = qt->tg.depth;
            depth_plane[pix0] = depth_tex.x;
            if (AUX) { qt->tg.obj_id[pix0] = obj.x; qt->tg.hit_t[pix0] = win_t.x; }
            if (in1) {
                uint32_t pix1 = pix0 + 1u;
                // (glossy forms: the right pixel's index is made here, once per frame, not kept in a register pair across the sample loop)
                if (GLOSS) asm volatile("" : "+v"(pix1));
                depth_plane[pix1] = depth_tex.y;
                if (AUX) { qt->tg.obj_id[pix1] = obj.y; qt->tg.hit_t[pix1] = win_t.y; }
            }
        }

        // -- local shading E(h0) and the surface's albedo ----------------------------------------------------------
        f2 cr = splat(0.0f), cg = splat(0.0f), cb = splat(0.0f);
        f2 tr = splat(0.0f), tgc = splat(0.0f), tb = splat(0.0f);
        if (__any(any2(obj >= 0))) {
            f2 mr, mg, mb, xr, xg, xb;
            kernarg<WfPrimaryArgs> *const qh = wf_args_again(ka);   // material constants, the texture, the shading records
            const ShadeRec *shade = qh->shade;
            const float4 *tex = qh->tex;
            if (NMAP) shade_mesh_pair<true, false, true>(qh->p, shade, tex, obj, last_shade, best, D, mr, mg, mb, xr, xg, xb);
            else if (qh->p.n_materials > 1u) shade_mesh_pair<true, false>(qh->p, shade, tex, obj, last_shade, best, D, mr, mg, mb, xr, xg, xb);
            else if (n_tested == 1u) shade_mesh_pair<false, true>(qh->p, shade, tex, obj, last_shade, best, D, mr, mg, mb, xr, xg, xb);
            else shade_mesh_pair<false, false>(qh->p, shade, tex, obj, last_shade, best, D, mr, mg, mb, xr, xg, xb);
            const i2 is_mesh = obj >= 0;
            cr = is_mesh ? mr : cr; cg = is_mesh ? mg : cg; cb = is_mesh ? mb : cb;
            tr = is_mesh ? xr : tr; tgc = is_mesh ? xg : tgc; tb = is_mesh ? xb : tb;
        }
        v3 n;  // the surface normal as the reference's HitRecord holds it (exact: it steers the bounce)
        n.x = n.y = splat(0.0f); n.z = splat(1.0f);
        if (__any(any2(obj < -1))) {  // sphere winners (few tiles): one pixel at a time
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int o = k ? obj.y : obj.x;
                if (o < -1) {
                    const f3 Dk = lane3(D, k);
                    const f3 center = ld3(wf_args_again(ka)->p.spheres[-2 - o].center);
                    const f3 P = along(O, k ? win_t.y : win_t.x, Dk);
                    const f3 c = shade_sphere(cnormalize(sub3(P, center)), Dk);
                    const f3 ne = normalize3(sub3(P, center));
                    if (k) { cr.y = c.x; cg.y = c.y; cb.y = c.z; tr.y = 1.0f; tgc.y = 0.0f; tb.y = 0.0f; n.x.y = ne.x; n.y.y = ne.y; n.z.y = ne.z; }
                    else { cr.x = c.x; cg.x = c.y; cb.x = c.z; tr.x = 1.0f; tgc.x = 0.0f; tb.x = 0.0f; n.x.x = ne.x; n.y.x = ne.y; n.z.x = ne.z; }
                }
            }
        }
        const i2 hit = obj != -1;
        f2 lr = splat(0.0f), lg = splat(0.0f), lb = splat(0.0f);   // GLOW: Le(h0) of each pixel's hit
        if (GLOW) {
            kernarg<WfPrimaryArgs> *const qg = wf_args_again(ka);   // the emission table, the shading records
            const WfGlow gl = {qg->glow.table, qg->glow.n_parts, 0u, qg->glow.hits, nullptr, nullptr, nullptr};
            const bool parts = qg->p.n_materials > 1u;
            const ShadeRec *const shade = qg->shade;
            const i2 seen = hit & i2{in0 ? -1 : 0, in1 ? -1 : 0};   // (a pixel off the frame is no hit anyone counts)
            bool lit[2] = {false, false};
#pragma unroll
            for (int k = 0; k < 2; k++) {
                if (k ? seen.y : seen.x) {
                    const float4 g = glow_record(gl, parts, shade, k ? obj.y : obj.x);
                    if (k) { lr.y = g.x; lg.y = g.y; lb.y = g.z; } else { lr.x = g.x; lg.x = g.y; lb.x = g.z; }
                    lit[k] = glows(g);
                }
            }
            cr = cr + lr; cg = cg + lg; cb = cb + lb;   // E'(h0) = E(h0) + Le(h0)
            count_glow_hits(gl.hits, lit[0], lit[1]);
        }
        int32_t dr0 = 0, dg0 = 0, db0 = 0, dr1 = 0, dg1 = 0, db1 = 0;   // SHADOW: fix(E) - fix(ambient part) in the planes' units
        if (SHADOW) {
            // the term is a select between its ambient part and E(h0), decided by the hit's shadow ray: the ambient part is summed
            // here, the difference of the two fixed-point values travels in the record
            constexpr float kScale22 = kWfFixedScale / 16.0f;
            constexpr uint32_t kCap = (kWfE0Cap << 22) - 1u;
            kernarg<WfPrimaryArgs> *const qa = wf_args_again(ka);
            f2 ar = splat(qa->p.ambient[0]), ag = splat(qa->p.ambient[1]), ab = splat(qa->p.ambient[2]);
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int o = k ? obj.y : obj.x;
                f3 am = mk3(k ? ar.y : ar.x, k ? ag.y : ag.x, k ? ab.y : ab.x);
                if (o < -1) am = mk3(0.1f, 0.0f, 0.0f);   // sphere/compute.wgsl: 0.1 * mat_color
                else if (o >= 0 && qa->p.n_materials > 1u) am = ld3(qa->p.materials[qa->shade[o].material].ambient);
                if (o == -1) am = mk3(0.0f, 0.0f, 0.0f);
                if (k) { ar.y = am.x; ag.y = am.y; ab.y = am.z; } else { ar.x = am.x; ag.x = am.y; ab.x = am.z; }
            }
            if (GLOW) { ar = ar + lr; ag = ag + lg; ab = ab + lb; }   // the occluded hit's shading: ambient(h0) + Le(h0)
            const f2 sr = cr * kScale22, sg = cg * kScale22, sb = cb * kScale22;
            const f2 qr = ar * kScale22, qg = ag * kScale22, qb2 = ab * kScale22;
            const uint32_t F[6] = {min((uint32_t)sr.x, kCap), min((uint32_t)sg.x, kCap), min((uint32_t)sb.x, kCap),
                                   min((uint32_t)sr.y, kCap), min((uint32_t)sg.y, kCap), min((uint32_t)sb.y, kCap)};
            const uint32_t A[6] = {min((uint32_t)qr.x, kCap), min((uint32_t)qg.x, kCap), min((uint32_t)qb2.x, kCap),
                                   min((uint32_t)qr.y, kCap), min((uint32_t)qg.y, kCap), min((uint32_t)qb2.y, kCap)};
            fr0 += A[0]; fg0 += A[1]; fb0 += A[2]; fr1 += A[3]; fg1 += A[4]; fb1 += A[5];
            dr0 = ((int32_t)F[0] - (int32_t)A[0]) * 16; dg0 = ((int32_t)F[1] - (int32_t)A[1]) * 16; db0 = ((int32_t)F[2] - (int32_t)A[2]) * 16;
            dr1 = ((int32_t)F[3] - (int32_t)A[3]) * 16; dg1 = ((int32_t)F[4] - (int32_t)A[4]) * 16; db1 = ((int32_t)F[5] - (int32_t)A[5]) * 16;
            hits0 += hit.x ? 1u : 0u; hits1 += hit.y ? 1u : 0u;
        } else
        {   // (cr, cg, cb are 0 where nothing was hit; float -> u32 conversion sends NaN / negatives to 0; alpha is 1 + 1 on a
            // written pixel, :231-234)
            constexpr float kScale22 = kWfFixedScale / 16.0f;
            constexpr uint32_t kCap = (kWfE0Cap << 22) - 1u;
            static_assert((unsigned long long)kWfMaxGroup * (kWfE0Cap << 22) <= (1ull << 32), "a launch group's sum of clamped terms fits 32 bits");
            const f2 sr = cr * kScale22, sg = cg * kScale22, sb = cb * kScale22;
            fr0 += min((uint32_t)sr.x, kCap); fg0 += min((uint32_t)sg.x, kCap); fb0 += min((uint32_t)sb.x, kCap);
            fr1 += min((uint32_t)sr.y, kCap); fg1 += min((uint32_t)sg.y, kCap); fb1 += min((uint32_t)sb.y, kCap);
            hits0 += hit.x ? 1u : 0u; hits1 += hit.y ? 1u : 0u;
        }

        // -- bounce ray of every pixel that hit something ----------------------------------------------------------
        kernarg<WfPrimaryArgs> *const qb = wf_args_again(ka);   // the ray queue
        if (SHADOW || qb->p.bounces != 0u) {
            const bool bounces = !SHADOW || qb->p.bounces != 0u;   // (without SHADOW: what got us here)
            const uint32_t wf_group = qb->wf.group;
            const TriRecord *tris = qb->tris;
            const i2 emit = hit & i2{in0 ? -1 : 0, in1 ? -1 : 0};
            const unsigned long long m0 = __ballot(emit.x != 0), m1 = __ballot(emit.y != 0);
            const uint32_t slot_base = (tile * wf_group + sidx) * kWfTilePixels + wave * 128u;
            if (bounces && lane == 0u) {
                unsigned long long *mk = qb->wf.masks + (size_t)(tile * wf_group + sidx) * 8u + wave * 2u;
                mk[0] = m0; mk[1] = m1;
            }
            if (SHADOW && lane == 0u) {
                unsigned long long *mk = qb->sw.masks + (size_t)(tile * wf_group + sidx) * 8u + wave * 2u;
                mk[0] = m0; mk[1] = m1;
            }
            if (bounces) emitted += (uint32_t)__popcll(m0) + (uint32_t)__popcll(m1);
            if (m0 | m1) {
                // mesh winners: +-normalize(N), prebaked with the shader's own operations (TriRecord::nhat)
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int o = k ? obj.y : obj.x;
                    if (o >= 0) {
                        f3 nh = ld3(tris[o].nhat);
                        if ((k ? best.ndotd.y : best.ndotd.x) > 0.0f) nh = neg3(nh);   // compute.wgsl:140-142
                        if (k) { n.x.y = nh.x; n.y.y = nh.y; n.z.y = nh.z; } else { n.x.x = nh.x; n.y.x = nh.y; n.z.x = nh.z; }
                    }
                }
                const v3 P = along(splat3(O), win_t, D);
                v3 O1 = v3{P.x + n.x * 1e-4f, P.y + n.y * 1e-4f, P.z + n.z * 1e-4f};
                if (SHADOW) {
                    ShadowRec *const recs = wf_args_again(ka)->sw.recs;
                    if (emit.x) {
                        uint4 *dst = reinterpret_cast<uint4 *>(recs + slot_base + lane);
                        const uint32_t fl = (obj.x < -1 ? 1u : 0u) | (dr0 < 0 ? 2u : 0u) | (dg0 < 0 ? 4u : 0u) | (db0 < 0 ? 8u : 0u);
                        dst[0] = make_uint4(__float_as_uint(O1.x.x), __float_as_uint(O1.y.x), __float_as_uint(O1.z.x), fl);
                        dst[1] = make_uint4((uint32_t)dr0, (uint32_t)dg0, (uint32_t)db0, 0u);
                    }
                    if (emit.y) {
                        uint4 *dst = reinterpret_cast<uint4 *>(recs + slot_base + 64u + lane);
                        const uint32_t fl = (obj.y < -1 ? 1u : 0u) | (dr1 < 0 ? 2u : 0u) | (dg1 < 0 ? 4u : 0u) | (db1 < 0 ? 8u : 0u);
                        dst[0] = make_uint4(__float_as_uint(O1.x.y), __float_as_uint(O1.y.y), __float_as_uint(O1.z.y), fl);
                        dst[1] = make_uint4((uint32_t)dr1, (uint32_t)dg1, (uint32_t)db1, 0u);
                    }
                }
                if (bounces) {
                v3 D1;
                i2 lit_from = emit;   // GLOW with light sampling on: the pixels whose ray 1 is a diffuse ray
                if (MIRROR) {
                    // each pixel's surface record (rwr_surface.h surface_record), decoded
                    kernarg<WfPrimaryArgs> *const qv = wf_args_again(ka);
                    const SurfaceRec *const table = qv->surfaces.table;
                    const uint32_t n_parts = qv->surfaces.n_parts;
                    const bool parts = qv->p.n_materials > 1u;
                    const ShadeRec *const shade = qv->shade;
                    i2 mir = i2{0, 0}, gl = i2{0, 0}, gs = i2{0, 0};
                    f2 eta = splat(0.0f);   // GLASS: the index of a pixel's glass hit
                    f2 rho = splat(0.0f);   // GLOSS: the roughness of a pixel's glossy hit (it draws the diffuse direction too)
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        if (k ? emit.y : emit.x) {
                            const float4 m = surface_record(table, n_parts, parts, shade, k ? obj.y : obj.x);
                            const SurfaceDecode sd = decode_surface<SURF>(m.w);
                            if (sd.mirror || sd.glass || sd.gloss) {
                                if (k) { tr.y = m.x; tgc.y = m.y; tb.y = m.z; } else { tr.x = m.x; tgc.x = m.y; tb.x = m.z; }
                                if (sd.glass) {
                                    if (k) { gl.y = -1; eta.y = sd.eta; } else { gl.x = -1; eta.x = sd.eta; }
                                } else if (sd.gloss) {
                                    if (k) { gs.y = -1; rho.y = sd.rho; } else { gs.x = -1; rho.x = sd.rho; }
                                } else {
                                    if (k) mir.y = -1; else mir.x = -1;
                                }
                            }
                        }
                    }
                    const i2 diffuse = emit & ~mir & ~gl;
                    lit_from = diffuse & ~gs;
                    v3 Dd = D, Dm = D;
                    if (__any(any2(diffuse))) Dd = bounce_direction_pair(n, base, diffuse, sample, (wf_args_again(ka)->p.flags & RWR_FLAG_SOBOL) != 0u);
                    if (__any(any2(mir))) {   // D' = D - (2 d) n, d = dot3(n, D) (rwr_device.h reflect_direction, for the pair)
                        const f2 two_d = 2.0f * dot3(n, D);
                        Dm = v3{D.x - two_d * n.x, D.y - two_d * n.y, D.z - two_d * n.z};
                    }
                    D1 = v3{mir ? Dm.x : Dd.x, mir ? Dm.y : Dd.y, mir ? Dm.z : Dd.z};
                    if (GLOSS) {
                        if (__any(any2(gs))) {
                            const v3 S = gloss_direction_pair(n, D, Dd, rho);
                            D1 = v3{gs ? S.x : D1.x, gs ? S.y : D1.y, gs ? S.z : D1.z};
                            count_surface_events<true, false>(wf_args_again(ka)->surfaces.events, gs.x ? kEventGlossy : kEventNone,
                                                              gs.y ? kEventGlossy : kEventNone);
                        }
                    }
                    if (GLASS) {
                        uint32_t ev[2] = {kEventNone, kEventNone};
                        if (__any(any2(gl))) {   // (rwr_device.h refract_or_reflect, one pixel of the pair after the other; dimension 2 of the sample)
#pragma unroll
                            for (int k = 0; k < 2; k++)
                                if (k ? gl.y : gl.x) {
                                    f3 Dg, mg;
                                    ev[k] = refract_or_reflect(lane3(n, k), lane3(D, k), (k ? obj.y : obj.x) >= 0, k ? best.ndotd.y : best.ndotd.x,
                                                               k ? eta.y : eta.x, rng_draw(k ? base.y : base.x, sample, 2u, (wf_args_again(ka)->p.flags & RWR_FLAG_SOBOL) != 0u), Dg, mg);
                                    if (k) { D1.x.y = Dg.x; D1.y.y = Dg.y; D1.z.y = Dg.z; O1.x.y = P.x.y + mg.x * 1e-4f; O1.y.y = P.y.y + mg.y * 1e-4f; O1.z.y = P.z.y + mg.z * 1e-4f; }
                                    else { D1.x.x = Dg.x; D1.y.x = Dg.y; D1.z.x = Dg.z; O1.x.x = P.x.x + mg.x * 1e-4f; O1.y.x = P.y.x + mg.y * 1e-4f; O1.z.x = P.z.x + mg.z * 1e-4f; }
                                }
                            count_surface_events(wf_args_again(ka)->surfaces.events, ev[0], ev[1]);
                        }
                    }
                } else {
                    D1 = bounce_direction_pair(n, base, emit, sample, (wf_args_again(ka)->p.flags & RWR_FLAG_SOBOL) != 0u);
                }
                kernarg<WfPrimaryArgs> *const qq = wf_args_again(ka);   // where the rays go
                float4 *const rays = qq->wf.rays;
                uint16_t *const bins = qq->wf.bins;
                f2 mark = splat(0.0f);   // the records' spare half: 0xffff on a diffuse ray of a frame that samples its lights
                if (GLOW) {
                    const bool light_on = qq->glow.light != 0u;   // (scalar)
                    mark = f2{(light_on && lit_from.x) ? 1.0f : 0.0f, (light_on && lit_from.y) ? 1.0f : 0.0f};
                }
                if (emit.x) {
                    const uint32_t slot = slot_base + lane;
                    rays[2u * slot] = make_float4(O1.x.x, O1.y.x, O1.z.x, wf_pack_unorm16x2(tr.x, tgc.x));
                    rays[2u * slot + 1u] = make_float4(D1.x.x, D1.y.x, D1.z.x, wf_pack_unorm16x2(tb.x, mark.x));
                    bins[slot] = (uint16_t)wf_direction_bin(lane3(D1, 0));
                }
                if (emit.y) {
                    const uint32_t slot = slot_base + 64u + lane;
                    rays[2u * slot] = make_float4(O1.x.y, O1.y.y, O1.z.y, wf_pack_unorm16x2(tr.y, tgc.y));
                    rays[2u * slot + 1u] = make_float4(D1.x.y, D1.y.y, D1.z.y, wf_pack_unorm16x2(tb.y, mark.y));
                    bins[slot] = (uint16_t)wf_direction_bin(lane3(D1, 1));
                }
                if (GLOW) {
                    // light sampling (rwr_surface.h WfGlow::light, a scalar branch), for k_wf_light: the hit's normal goes to the slot of
                    // every marked ray and the slot's bit into the light ballots (cleared ahead of this kernel) - behind the ray
                    // stores, where the directions and origins are dead
                    kernarg<WfPrimaryArgs> *const ql = wf_args_again(ka);
                    if (ql->glow.light) {
                        LightRec *const lrecs = ql->glow.light_recs;
                        const unsigned long long l0 = __ballot(lit_from.x != 0), l1 = __ballot(lit_from.y != 0);
                        if (lane == 0u) {
                            unsigned long long *mk = ql->glow.light_masks + (size_t)(tile * wf_group + sidx) * 8u + wave * 2u;
                            mk[0] = l0; mk[1] = l1;
                        }
                        if (lit_from.x) *reinterpret_cast<float4 *>(lrecs + slot_base + lane) = make_float4(n.x.x, n.y.x, n.z.x, 0.0f);
                        if (lit_from.y) *reinterpret_cast<float4 *>(lrecs + slot_base + 64u + lane) = make_float4(n.x.y, n.y.y, n.z.y, 0.0f);
                    }
                }
                }
            }
        }
    }

    // -- the frame's fixed-point sums: once per group and pixel (plain read-modify-write when this workgroup owns the tile's
    // samples alone, integer atomics when it shares them: the same bits either way) ------------------------------------------
    kernarg<WfPrimaryArgs> *const qf = wf_args_again(ka);   // the frame's planes
    if (in0 && !empty_tile) {
        unsigned long long *const fix = qf->wf.fix;
        const size_t plane = (size_t)qf->p.width * qf->p.height;
        const unsigned long long fa0 = (unsigned long long)hits0 * (unsigned long long)(2.0f * kWfFixedScale);
        const unsigned long long fa1 = (unsigned long long)hits1 * (unsigned long long)(2.0f * kWfFixedScale);
        const unsigned long long r0 = (unsigned long long)fr0 << 4, g0 = (unsigned long long)fg0 << 4, b0 = (unsigned long long)fb0 << 4;
        const unsigned long long r1 = (unsigned long long)fr1 << 4, g1 = (unsigned long long)fg1 << 4, b1 = (unsigned long long)fb1 << 4;
        if (!LIST && z_split == 1u && !qf->wf.shared_planes) {
            fix[pix0] += r0; fix[plane + pix0] += g0; fix[2u * plane + pix0] += b0; fix[3u * plane + pix0] += fa0;
            if (in1) { fix[pix0 + 1u] += r1; fix[plane + pix0 + 1u] += g1; fix[2u * plane + pix0 + 1u] += b1; fix[3u * plane + pix0 + 1u] += fa1; }
        } else {
            if (hits0) { atomicAdd(&fix[pix0], r0); atomicAdd(&fix[plane + pix0], g0); atomicAdd(&fix[2u * plane + pix0], b0); atomicAdd(&fix[3u * plane + pix0], fa0); }
            if (in1 && hits1) { atomicAdd(&fix[pix0 + 1u], r1); atomicAdd(&fix[plane + pix0 + 1u], g1); atomicAdd(&fix[2u * plane + pix0 + 1u], b1); atomicAdd(&fix[3u * plane + pix0 + 1u], fa1); }
        }
    }
    if (lane == 0u && emitted) atomicAdd(qf->wf.wave_total + tile * 4u + wave, emitted);   // (zeroed when the frame starts)
    } while (LIST);
}

// k_wf_primary's forms (rwr_wf_forms.h).  LIST walks the list of the tiles the culling found live: only with CULL.  SHADOW goes
// with every such (CULL, LIST) — (1, 1), (1, 0), (0, 0) — so it adds no condition of its own.
struct PrimaryForms {
    struct Form { bool aux, cull, nmap, list, shadow; int surf; bool glow; };
    static constexpr uint32_t kRange = 32u * 4u * 2u;
    static constexpr uint32_t encode(Form f)
    {
        return f.aux + 2u * f.cull + 4u * f.nmap + 8u * f.list + 16u * f.shadow + 32u * (uint32_t)f.surf + 128u * f.glow;
    }
    static constexpr Form decode(uint32_t i)
    {
        return Form{(i & 1u) != 0, (i & 2u) != 0, (i & 4u) != 0, (i & 8u) != 0, (i & 16u) != 0, (int)((i >> 5) & 3u), (i & 128u) != 0};
    }
    static constexpr bool valid(Form f) { return !f.list || f.cull; }
    using Kernel = decltype(&k_wf_primary<false, false, false>);
    template <uint32_t I> static constexpr Kernel kernel()
    {
        constexpr Form f = decode(I);
        return &k_wf_primary<f.aux, f.cull, f.nmap, f.list, f.shadow, f.surf, f.glow>;
    }
};
static constexpr auto kPrimaryForms = form_table<PrimaryForms>();
// GLOW (rwr_surface.h WfGlow) goes with every form of all three templates — a hit is shaded by the kernels that end a path as by
// those that send a ray on — so it adds no condition to any valid(): each table's count is twice what it was.
static_assert(check_forms<PrimaryForms>(192), "8 plain + 4 LIST + 12 SHADOW forms, times four surface models, with and without GLOW");

hipError_t launch_wf_primary(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const ShadeRec *shade,
                             const FrameTri *ftris, const float4 *tex, const Targets &tg, const WfBuffers &wf,
                             uint32_t sample_begin, uint32_t sample_count, uint32_t z_split, const WfFeatures &ft)
{
    if (fp.row_end <= fp.row_begin || fp.width == 0 || sample_count == 0) return hipSuccess;
    z_split = std::max(1u, std::min(z_split, sample_count));
    const WfPrimaryArgs args{ftris, fp.n_tris, fp.row_begin, fp.bins.enabled, fp.mesh_px[0], fp.mesh_px[1], fp.mesh_px[2], fp.mesh_px[3],
                             sample_begin, sample_count, z_split, fp, tris, shade, tex, tg, wf, ft.shadow, ft.surfaces, ft.glow};
    PrimaryForms::Form f;
    f.aux = (fp.flags & RWR_FLAG_AUX_OUTPUTS) != 0;
    f.cull = (fp.flags & RWR_FLAG_NO_CULL) == 0;
    f.nmap = (fp.flags & RWR_FLAG_NORMAL_MAP) != 0;
    f.list = wf.live_list && f.cull;   // item after item of (live tile) x (share of its samples)
    f.shadow = ft.shadows;
    f.surf = ft.primary_surf(fp);
    f.glow = ft.glows;
    const dim3 tiles((fp.width + kWfTileW - 1u) / kWfTileW, band_strips(fp), z_split);
    const dim3 grid = f.list ? dim3(std::min(tiles.x * tiles.y * z_split, 4096u)) : tiles;
    hipLaunchKernelGGL(kPrimaryForms[PrimaryForms::encode(f)], grid, dim3(256), 0, s, args);
    return hipGetLastError();
}

// Frames that show little (a small mesh on an empty screen): which tiles can anything be seen through?  One workgroup per
// 64x8-pixel tile, its four waves reaching the verdict the primary stage's waves would reach (rwr_wf_cull.h).  Tiles with a
// live wave are listed (any order); a wave that sees nothing gives its pixels the clear values of sample 0's planes here,
// and the resolve step skips its pixels' sums (nothing is ever added to them).
template <bool AUX>
__global__ void __launch_bounds__(256)
k_wf_classify(const FrameTri *__restrict__ ftris, uint32_t n_tris, uint32_t row_begin, uint32_t bins_enabled, int32_t mesh_x0,
              int32_t mesh_y0, int32_t mesh_x1, int32_t mesh_y1, const FrameParams p, const Targets tg, uint32_t tiles_x,
              uint32_t *__restrict__ live_list, uint32_t *__restrict__ live_count, uint32_t *__restrict__ tile_live)
{
    __shared__ uint32_t s_live;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (threadIdx.x == 0u) s_live = 0u;
    __syncthreads();
    const uint32_t blk_x0 = blockIdx.x * kWfTileW, blk_y0 = row_begin + blockIdx.y * p.row_pitch;
    const uint32_t tile_x0 = blk_x0 + (wave & 1u) * 32u, tile_y0 = blk_y0 + (wave >> 1) * 4u;
    const WfWaveCull wc = wf_wave_cull<true>(ftris, n_tris, row_begin, bins_enabled, mesh_x0, mesh_y0, mesh_x1, mesh_y1, p.bins, blk_x0,
                                             blk_y0, wave, lane);
    if (wf_wave_empty<true>(wc, p, (float)tile_x0, (float)tile_y0)) {
        const uint32_t px0 = tile_x0 + 2u * (lane & 15u), py = tile_y0 + (lane >> 4);
        if (py < p.row_end && px0 < p.width) {
            const uint32_t pix0 = py * p.width + px0;
            tg.depth[pix0] = 0.0f;
            if (AUX) { tg.obj_id[pix0] = -1; tg.hit_t[pix0] = 0.0f; }
            if (px0 + 1u < p.width) {
                tg.depth[pix0 + 1u] = 0.0f;
                if (AUX) { tg.obj_id[pix0 + 1u] = -1; tg.hit_t[pix0 + 1u] = 0.0f; }
            }
        }
    } else if (lane == 0u) {
        atomicOr(&s_live, 1u << wave);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t tile = blockIdx.y * tiles_x + blockIdx.x, live = s_live;
        tile_live[tile] = live;
        if (live) live_list[atomicAdd(live_count, 1u)] = tile;
    }
}

hipError_t launch_wf_classify(hipStream_t s, const FrameParams &fp, const FrameTri *ftris, const Targets &tg, uint32_t tiles_x,
                              uint32_t *live_list, uint32_t *live_count, uint32_t *tile_live)
{
    if (fp.row_end <= fp.row_begin || fp.width == 0) return hipSuccess;
    const dim3 grid(tiles_x, band_strips(fp));
    constexpr decltype(&k_wf_classify<false>) forms[2] = {&k_wf_classify<false>, &k_wf_classify<true>};   // [AUX]
    hipLaunchKernelGGL(forms[(fp.flags & RWR_FLAG_AUX_OUTPUTS) != 0], grid, dim3(256), 0, s, ftris, fp.n_tris, fp.row_begin, fp.bins.enabled,
                       fp.mesh_px[0], fp.mesh_px[1], fp.mesh_px[2], fp.mesh_px[3], fp, tg, tiles_x, live_list, live_count, tile_live);
    return hipGetLastError();
}

hipError_t preload_kernels_wf_primary()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>((&k_wf_primary<false, true, false>)));
}

}  // namespace rwr
