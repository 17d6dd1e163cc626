// The surface table of the path tracer (RWR_FLAG_MIRRORS, _GLASS, _GLOSSY): its record, the one statement of what the record's
// `on` field means, the one decode the kernels read it with, its fetch and the event counters.  Host and device share this header;
// the host half compiles without HIP (tests/surface_host.cpp).
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define RWR_HD __host__ __device__
#else
#define RWR_HD
#endif

namespace rwr {

// A surface's record, 16 bytes of WfSurfaces::table: r, g, b and the surface's model in `on`.
struct SurfaceRec { float r, g, b, on; };
static_assert(sizeof(SurfaceRec) == 16, "SurfaceRec is a float4");

// The one statement of SurfaceRec::on.  A surface has one model:
//   kDiffuse  on = 0               neither of the others (r, g, b are zero)
//   kMirror   on = 1               reflectance r, g, b (RWR_FLAG_MIRRORS)
//   kGlass    on = -ior            tint r, g, b; ior in [1, 4] (RWR_FLAG_GLASS)
//   kGloss    on = 1 + roughness   reflectance r, g, b; roughness in [2^-10, 1], a multiple of 2^-23 once stored (RWR_FLAG_GLOSSY)
// Invariant: every record a setter can write (scene.cpp, through the makers below) has on in {0} U {1} U [-4, -1] U [1 + 2^-10, 2].
// So `on == 1` and `on > 0 && !(on > 1)` name the same records, and so do `on > 1` and `on >= 1 + 2^-10`: whichever comparison
// decode_surface uses for a kernel's SURF, it agrees with surface_model (the static_asserts below at the ranges' ends,
// tests/test_surface_decode_host.py on every storable value).
enum class SurfaceModel { kDiffuse, kMirror, kGlass, kGloss };
RWR_HD constexpr SurfaceModel surface_model(const SurfaceRec &m)
{
    return m.on > 1.0f ? SurfaceModel::kGloss : m.on > 0.0f ? SurfaceModel::kMirror : m.on < 0.0f ? SurfaceModel::kGlass : SurfaceModel::kDiffuse;
}
constexpr float kGlassIorMin = 1.0f, kGlassIorMax = 4.0f, kGlossRoughnessMin = 0x1p-10f, kGlossRoughnessMax = 1.0f;
constexpr SurfaceRec kDiffuseRec{0.0f, 0.0f, 0.0f, 0.0f};
// the record makers: rgb in [0, 1] each, ior and roughness in the ranges above (the setters refuse anything else before they call)
inline SurfaceRec mirror_rec(const float rgb[3]) { return SurfaceRec{rgb[0], rgb[1], rgb[2], 1.0f}; }
inline SurfaceRec glass_rec(const float rgb[3], float ior) { return SurfaceRec{rgb[0], rgb[1], rgb[2], -ior}; }
inline SurfaceRec gloss_rec(const float rgb[3], float roughness) { return SurfaceRec{rgb[0], rgb[1], rgb[2], 1.0f + roughness}; }
// ... and what a glass record holds of its ior, a glossy one of its roughness (a diffuse record: 0)
RWR_HD constexpr float surface_param(const SurfaceRec &m) { return m.on < 0.0f ? -m.on : m.on > 1.0f ? m.on - 1.0f : 0.0f; }
// A model's bit in the words that say which models a table holds (WfState::surface_modes): 1 mirrors, 2 glass, 4 glossy
RWR_HD constexpr uint32_t surface_mode(SurfaceModel s)
{
    return s == SurfaceModel::kMirror ? 1u : s == SurfaceModel::kGlass ? 2u : s == SurfaceModel::kGloss ? 4u : 0u;
}
// What a frame's copy of the table holds of a record: a surface whose flag the frame lacks (`modes`: surface_mode bits) is the
// diffuse surface it was.  So no kernel looks at a flag.
RWR_HD constexpr SurfaceRec visible_record(const SurfaceRec &m, uint32_t modes)
{
    return (modes & surface_mode(surface_model(m))) ? m : kDiffuseRec;
}

// The kernels' SURF argument, the surface models of the frame's flags: no table, mirrors alone, mirrors and glass, those and glossy.
// A form decodes only what visible_record leaves of the models it knows.
constexpr int kSurfNone = 0, kSurfMirrors = 1, kSurfGlass = 2, kSurfGloss = 3;

// What a kernel reads of a record's `on`: which model the surface has, a glass surface's index, a glossy one's roughness.
struct SurfaceDecode {
    bool mirror, glass, gloss;
    float eta, rho;   // 0 where the surface is not glass / not glossy
};
template <int SURF>
RWR_HD constexpr SurfaceDecode decode_surface(float on)
{
    const bool gloss = SURF == kSurfGloss && on > 1.0f;   // (1 + roughness, in (1, 2]; the other forms never see one)
    const bool mirror = SURF == kSurfNone || SURF == kSurfMirrors ? on != 0.0f : on > 0.0f && !gloss;
    const bool glass = (SURF == kSurfGlass || SURF == kSurfGloss) && on < 0.0f;
    return SurfaceDecode{mirror, glass, gloss, glass ? -on : 0.0f, gloss ? on - 1.0f : 0.0f};
}
// decode_surface<SURF> names the model and the parameter that surface_model and surface_param do, on a record as a frame of
// `modes` sees it
template <int SURF>
RWR_HD constexpr bool decode_agrees(float on, uint32_t modes)
{
    const SurfaceRec v = visible_record(SurfaceRec{0.0f, 0.0f, 0.0f, on}, modes);
    const SurfaceDecode d = decode_surface<SURF>(v.on);
    const SurfaceModel s = surface_model(v);
    return d.mirror == (s == SurfaceModel::kMirror) && d.glass == (s == SurfaceModel::kGlass) && d.gloss == (s == SurfaceModel::kGloss) &&
           (d.glass ? d.eta : d.gloss ? d.rho : 0.0f) == surface_param(v) && (d.glass || d.eta == 0.0f) && (d.gloss || d.rho == 0.0f);
}
template <int SURF>
RWR_HD constexpr bool decode_agrees_at_ends(uint32_t modes)
{
    return decode_agrees<SURF>(0.0f, modes) && decode_agrees<SURF>(1.0f, modes) && decode_agrees<SURF>(-kGlassIorMin, modes) &&
           decode_agrees<SURF>(-kGlassIorMax, modes) && decode_agrees<SURF>(1.0f + kGlossRoughnessMin, modes) &&
           decode_agrees<SURF>(1.0f + kGlossRoughnessMax, modes);
}
static_assert(decode_agrees_at_ends<kSurfMirrors>(1u), "the mirror forms decode what surface_model states");
static_assert(decode_agrees_at_ends<kSurfGlass>(2u) && decode_agrees_at_ends<kSurfGlass>(3u), "the glass forms decode what surface_model states");
static_assert(decode_agrees_at_ends<kSurfGloss>(4u) && decode_agrees_at_ends<kSurfGloss>(5u) && decode_agrees_at_ends<kSurfGloss>(6u) &&
                  decode_agrees_at_ends<kSurfGloss>(7u),
              "the glossy forms decode what surface_model states");

// What a ray did at a surface that is counted: a glass hit's three outcomes (rwr_device.h refract_or_reflect returns them) and a
// glossy hit's one.  A value is the event's index among the frame's counters, WfSurfaces::events; kEventNone is their number.
enum SurfaceEvent : uint32_t { kEventReflected = 0u, kEventTransmitted = 1u, kEventTotalReflection = 2u, kEventGlossy = 3u, kEventNone = 4u };

// The kernels' argument (the surface forms of k_wf_primary and of the trace kernels' EMIT forms): the table — one record per scene
// part, then one per sphere index (RWR_MAX_SPHERES of them) — as the frame sees it (visible_record).  A kernel argument of its own
// behind the others (cf. WfSky), so that MaterialRec and ShadeRec stay as they are and the kernels without a surface flag keep
// their code.  events: the frame's kEventNone counters, one atomic per wave and event kind; null in the mirror forms, which count
// nothing (all are allocated whenever one is).
struct WfSurfaces {
    const SurfaceRec *table;
    uint32_t n_parts;
    uint32_t pad;
    unsigned long long *events;
};

// Emissive surfaces (RWR_FLAG_EMISSIVE; the GLOW forms of k_wf_primary and of the trace kernels — "glow", since EMIT, emit_next_ray
// and WfEmit already mean "sends a ray on").  A second table of the surface table's shape and order — one record {r, g, b, 0} per
// scene part, then one per sphere index: the radiance Le the surface gives off, zeros where it gives off none — fetched like
// WfSurfaces::table (surface_record below).  Emission stands beside a surface's model: a record here says nothing about `on` there.
// hits: the frame's count of shaded hits with Le != 0, one atomic per wave (count_glow_hits).  A kernel argument of its own behind
// the others (cf. WfSurfaces), so that the forms without GLOW read their arguments where they did.
// Light sampling (RWR_FLAG_LIGHT_SAMPLING; kernels_wf_light.hip) rides on the GLOW forms behind a run-time switch, `light` (wave-
// uniform: a scalar branch; 0 in every frame without the flag, whose GLOW forms then do what they did).  With it on, the kernel
// that sends on a DIFFUSE ray from a hit — the primary stage, emit_next_ray — marks the ray's record (upper 16 bits of its last
// word), leaves the hit's normal at the slot (light_recs, 16 B per queue slot) and sets the slot's bit in the light ballots
// (light_masks: layout of WfBuffers::masks, cleared per generation); and add_glow takes Le as 0 for the hit of a marked ray on an
// emitting sphere seen from outside (the light sample of the ray's origin has that light already) and counts it in
// light_counts[2] ([0], [1]: k_wf_light's rays traced and rays that reached their sphere).
// `light` is two bits: 1 — RWR_FLAG_LIGHT_SAMPLING is effective, the spheres above; 2 — RWR_FLAG_LIGHT_PARTS is effective: the light
// stage aims at the mesh light too (rwr_part_lights.h), and add_glow takes Le as 0 for the hit of a marked ray on a face of an
// emitting part and counts it in light_counts[2] and [5].  Either bit marks rays and stores normals.  light_counts holds six:
// [3], [4], [5] are the mesh light's share of [0], [1], [2].
// A third bit, mask value 4 — RWR_FLAG_LIGHT_MIS is effective (with bit 1 or 2): k_wf_light adds T Le m(g) in place of T Le g, and add_glow gives
// the hits it silenced Le m(g') in place of 0 (mis_weight below; g' from the ray, the hit and the slot's LightRec, which the hit's own
// emit_next_ray has not overwritten yet).  Bits 8-15 hold L, the lights the stage chooses among (M + 1 with the mesh light, else M),
// which g' needs; a part's record of `table` carries the inv_pdf of the part's listed faces in its fourth component (0: none listed).
// A fourth bit, mask value 8 — RWR_FLAG_LIGHT_SKY is effective: the sky's image is the last of the L lights (k_wf_light's SKY forms), the
// trace kernels run the LSKY forms, whose marked misses are silenced or weighted, and light_counts holds nine: [6], [7], [8] are the
// sky's share of [0], [1], [2] ([8]: the suppressed misses).  The table may then hold zeros alone (no RWR_FLAG_EMISSIVE in effect).
struct LightRec { float n[3]; uint32_t pad; };
static_assert(sizeof(LightRec) == 16, "LightRec is 16 B");
struct WfGlow {
    const SurfaceRec *table;
    uint32_t n_parts;
    uint32_t light;
    unsigned long long *hits;
    LightRec *light_recs;
    unsigned long long *light_masks;
    unsigned long long *light_counts;
};
// The emitting spheres in use, s_0 < ... < s_{M-1} (rwr_hip.h RWR_FLAG_LIGHT_SAMPLING): index and radiance; centre and radius are
// FrameParams::spheres[index]'s.  A kernel argument of k_wf_light: scalar registers.
struct WfLights {
    uint32_t m;
    uint32_t index[8];
    float le[8][3];
};
constexpr float kMaxEmission = 64.0f;   // RWR_MAX_EMISSION
// the record of a surface of radiance rgb (each in [0, kMaxEmission]: the setters refuse anything else; -0.0 is stored as +0.0, so
// that "emits" is "a component is not zero" on the bits as well)
inline SurfaceRec glow_rec(const float rgb[3]) { return SurfaceRec{rgb[0] + 0.0f, rgb[1] + 0.0f, rgb[2] + 0.0f, 0.0f}; }
RWR_HD constexpr bool glows(const SurfaceRec &g) { return g.r != 0.0f || g.g != 0.0f || g.b != 0.0f; }

#ifdef __HIPCC__
// The record {r, g, b, on} of the hit `obj` (a face, or -2 - the sphere's index).  Part 0's record sits at the table's start and
// is read at a constant index through the constant address space: a wave-uniform address, one scalar load into scalar registers,
// and all a face of a one-part scene needs (it never looks at ShadeRec::material).  Only a sphere hit (by its index) and a face of
// a scene with several parts (`several_parts`, by ShadeRec::material) read their record per lane, under a branch of their own, so
// that the two reads stay two.  Shade: ShadeRec (rwr_internal.h, which includes this header).
template <typename Shade>
__device__ __forceinline__ float4 surface_record(const SurfaceRec *table, uint32_t n_parts, bool several_parts, const Shade *__restrict__ shade,
                                                 int32_t obj)
{
    const __attribute__((address_space(4))) float *const tab = (const __attribute__((address_space(4))) float *)(table);
    // part 0; the empty asm pins the four values to scalar registers where they are read, or the compiler folds this read into the
    // per-lane one below (one vector load at a selected index)
    float r0 = tab[0], r1 = tab[1], r2 = tab[2], r3 = tab[3];
    asm volatile("" : "+s"(r0), "+s"(r1), "+s"(r2), "+s"(r3));
    float4 m = make_float4(r0, r1, r2, r3);
    if (obj < 0 || several_parts) {
        const uint32_t i = obj < 0 ? n_parts + (uint32_t)(-2 - obj) : shade[obj].material;
        m = make_float4(tab[4u * i], tab[4u * i + 1u], tab[4u * i + 2u], tab[4u * i + 3u]);
    }
    return m;
}

// A wave's events (two per lane: a packet's or a pixel pair's rays) into the frame's counters — ballots and popcounts, added by the
// wave's first active lane, one atomic per event kind the wave saw.  Call where the wave's lanes have come together again.
// GLASS: the three glass events; GLOSS (the glossy forms): the glossy rays too.
template <bool GLOSS = false, bool GLASS = true>
__device__ __forceinline__ void count_surface_events(unsigned long long *__restrict__ events, uint32_t ev0, uint32_t ev1 = kEventNone)
{
    const unsigned long long active = __ballot(true);
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t k = GLASS ? kEventReflected : kEventGlossy; k < (GLOSS ? kEventNone : kEventGlossy); k++) {
        const uint32_t n = (uint32_t)__popcll(__ballot(ev0 == k)) + (uint32_t)__popcll(__ballot(ev1 == k));
        if (n && lane == (uint32_t)__builtin_ctzll(active)) atomicAdd(&events[k], (unsigned long long)n);
    }
}

// GLOW forms: the radiance {r, g, b, 0} of the hit `obj` — surface_record on the emission table: part 0's record by the one scalar
// load, a sphere's or another part's per lane under the same branch.
template <typename Shade>
__device__ __forceinline__ float4 glow_record(const WfGlow &gl, bool several_parts, const Shade *__restrict__ shade, int32_t obj)
{
    return surface_record(gl.table, gl.n_parts, several_parts, shade, obj);
}
__device__ __forceinline__ bool glows(const float4 &g) { return g.x != 0.0f || g.y != 0.0f || g.z != 0.0f; }
// RWR_FLAG_LIGHT_MIS item 3: the balance heuristic's weight of the bounce side, m(g) = g / (1 + g) for g = p_b / p_l, in the form that
// is exact at both ends with no special case — 1 / g is +inf for a denormal g (m = 0) and 0 for g = +inf (m = 1); 0 for g <= 0 and NaN.
__device__ __forceinline__ float mis_weight(float g) { return g > 0.0f ? 1.0f / (1.0f + 1.0f / g) : 0.0f; }
// A wave's shaded hits on emitting surfaces (two per lane: a packet's or a pixel pair's) into the frame's counter, as
// count_surface_events counts: ballots and popcounts, one atomic from the wave's first active lane.  Call where the wave's lanes
// have come together again.
__device__ __forceinline__ void count_glow_hits(unsigned long long *__restrict__ hits, bool lit0, bool lit1 = false)
{
    const unsigned long long active = __ballot(true);
    const uint32_t n = (uint32_t)__popcll(__ballot(lit0)) + (uint32_t)__popcll(__ballot(lit1));
    if (n && (threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(active)) atomicAdd(hits, (unsigned long long)n);
}
#endif

}  // namespace rwr
