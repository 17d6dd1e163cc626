// The context behind the C ABI (include/rwr_hip.h) and what its units share: context.cpp (life cycle, targets, timers),
// scene.cpp, the frame units (rwr_frame.h), diagnostics.cpp, dist.cpp.  The units read the context's members directly.
#pragma once

#include <hip/hip_runtime.h>

#include <utility>
#include <memory>
#include <vector>

#include "rwr_internal.h"

typedef struct ncclComm *ncclComm_t;   // (RCCL's own typedef; the library is known to dist.cpp alone)

namespace rwr {

#define RWR_HIP_CHECK(expr)                                                                          \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return set_error(RWR_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// Device memory that is freed with its owner; moved, never copied.
template <typename T>
struct DeviceBuffer {
    T *ptr = nullptr;
    size_t count = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : ptr(o.ptr), count(o.count) { o.ptr = nullptr; o.count = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { std::swap(ptr, o.ptr); std::swap(count, o.count); return *this; }
    ~DeviceBuffer() { release(); }
    hipError_t ensure(size_t n)
    {
        if (n <= count && ptr) return hipSuccess;
        release();
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&ptr), n * sizeof(T));
        if (e == hipSuccess) count = n;
        else ptr = nullptr;
        return e;
    }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        count = 0;
    }
};

// A stream, event, graph or pinned word that is destroyed with its owner; moved, never copied.  Created through `&x.h`.
template <typename T, hipError_t (*Destroy)(T)>
struct Owned {
    T h = nullptr;
    Owned() = default;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = nullptr; }
    Owned &operator=(Owned &&o) noexcept { std::swap(h, o.h); return *this; }
    ~Owned() { if (h) (void)Destroy(h); }
    operator T() const { return h; }
};
inline hipError_t free_pinned_words(uint32_t *p) { return hipHostFree(p); }
using OwnedStream = Owned<hipStream_t, hipStreamDestroy>;
using OwnedEvent = Owned<hipEvent_t, hipEventDestroy>;
using OwnedGraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;
using PinnedWords = Owned<uint32_t *, free_pinned_words>;
inline hipError_t free_pinned_surface(SurfaceRec *p) { return hipHostFree(p); }
using PinnedSurface = Owned<SurfaceRec *, free_pinned_surface>;   // (the record and what it means: rwr_surface.h)

// Everything one frame in flight owns: its stream, its targets and the per-frame records / tables.
// Frames alternate between slots (rwr_ctx_set_frames_in_flight), so the ramp-up of one frame's kernel
// fills the machine while the previous frame's last waves drain; a slot is reused in stream order.
struct FrameSlot {
    hipStream_t stream = nullptr;   // slot 0: the context's stream (may be the caller's); others: owned
    OwnedStream owned;
    OwnedEvent done;                // rwr_timer_end: joins the slot into the timing stream
    DeviceBuffer<uint8_t> d_color;
    DeviceBuffer<float> d_depth;
    DeviceBuffer<float> d_color_f32;
    DeviceBuffer<int32_t> d_obj_id;
    DeviceBuffer<float> d_hit_t;
    DeviceBuffer<FrameTri> d_ftris;
    DeviceBuffer<float> d_tnum;                  // per frame: plane-distance numerator per face
    DeviceBuffer<float4> d_ray_colp, d_ray_row;  // per frame: ray tables (FrameParams::ray_colp / ray_row)
    DeviceBuffer<uint32_t> d_tile_lists;         // per frame: the two-pixel frame kernel's per-tile face sets (FrameParams::tile_lists)
    DeviceBuffer<uint32_t> d_bin_lists, d_bin_counts, d_bin_offsets, d_bin_total;   // per-frame screen bins (large scenes)
    PinnedWords h_bin_total;   // entries the last binned frame of this slot needed (read a frame late, never waited for)
    bool aux_valid = false;
    // RWR_FLAG_DENOISE, allocated by the slot's first denoised frame: the guide records and the two colour planes the iterations
    // alternate between (kernels_wf_denoise.hip)
    DeviceBuffer<float4> d_dn_guide, d_dn_a, d_dn_b;
    // RWR_FLAG_TONEMAP, allocated by the slot's first tone-mapped frame: the measure's sums and the exposure (kernels_wf_tonemap.hip),
    // zeroed on the stream by every frame that measures
    DeviceBuffer<TonemapRecord> d_tm_record;
    // RWR_FRAME_GRAPH (A/B knob): the reference frame's two launches (k_frame_setup -> k_primary_p2) as a
    // hipGraph of this slot — replayed as it is while camera and parameters stay the same, updated in place when they change
    OwnedGraphExec frame_graph;
    std::vector<unsigned char> frame_graph_key;
    // what the records, tables and face sets above were made from, byte for byte (frame_records.cpp launch_records), while they stand:
    // a frame with the same key on this slot finds them made and launches no k_frame_setup.  Empty: nothing to rely on
    std::vector<unsigned char> records_key;
    uint32_t cover_frames = 0;   // frames with RWR_FLAG_TILE_COVER on this slot since its last k_frame_setup (which zeroes the cover words)
    // The kept plane of ray directions (rwr_internal.h RayPlane; frame_records.cpp ray_plane_step), allocated by the slot's first build:
    // the xy array, then the z array.  ray_plane_key: the plane key (camera, screen, rows, addresses) of the slot's last frame
    // that could use a plane, empty when there is nothing to rely on; ray_plane_built: d_ray_plane holds that key's directions
    DeviceBuffer<float2> d_ray_plane;
    std::vector<unsigned char> ray_plane_key;
    bool ray_plane_built = false;
    void forget_ray_plane() { ray_plane_key.clear(); ray_plane_built = false; }
    // the frame kernel's fused form (one launch per frame): {finished record blocks, "a wait ran out"} on the device, the count
    // the host expects before the next frame, and the block count it is valid for
    DeviceBuffer<uint32_t> d_fused;
    uint32_t fused_count = 0, fused_blocks = 0;
    bool fused_used = false;
    // a slot no longer used gives its memory back: everything but the stream and its event starts over
    void reset()
    {
        FrameSlot fresh;
        fresh.stream = stream;
        fresh.owned = std::move(owned);
        fresh.done = std::move(done);
        *this = std::move(fresh);
    }
};
constexpr uint32_t kMaxFramesInFlight = 3;
constexpr rwr_denoise_params kDenoiseDefaults{5u, 0.04f, 0.95f, 0.05f};   // RWR_FLAG_DENOISE: DESIGN.md §6 says why these
constexpr rwr_reproject_params kReprojectDefaults{32u, 0.95f, 0.05f};   // RWR_FLAG_REPROJECT: the tap tests are the denoiser's
constexpr rwr_tonemap_params kTonemapDefaults = RWR_TONEMAP_DEFAULTS;   // RWR_FLAG_TONEMAP
constexpr rwr_sky_params kSkyDefaults = RWR_SKY_DEFAULTS;   // RWR_FLAG_SKY
constexpr rwr_shadow_params kShadowDefaults = RWR_SHADOW_DEFAULTS;   // RWR_FLAG_SOFT_SHADOWS
constexpr uint32_t kWfMaxQueues = 4;

// The wavefront integrator's device state, one set per frame slot: a frame of the integrator then shares nothing with the
// frames in the other slots (they overlap like reference frames do), and reuses its own set in stream order.
struct WfState {
    // Launch groups alternate between the frame's stream and these, each with its own part of the ray queue: the
    // latency-bound ends of one group (the sort, the last packets) run beside the other group's arithmetic.
    OwnedStream streams[kWfMaxQueues];   // [0] unused: queue 0 runs on the frame's stream
    OwnedEvent fork, join[kWfMaxQueues];
    DeviceBuffer<float4> d_rays;
    bool fix_clean = false;         // the fixed-point planes are all zero (k_wf_resolve leaves them so)
    DeviceBuffer<unsigned long long> d_masks;
    DeviceBuffer<unsigned long long> d_masks_next;   // deeper paths: the ballots of the generation being written (swapped with d_masks)
    DeviceBuffer<uint16_t> d_sorted, d_bins;
    DeviceBuffer<uint32_t> d_wave_total;
    DeviceBuffer<unsigned long long> d_fix;   // the frame's fixed-point sums, 4 planes
    DeviceBuffer<uint8_t> d_pool_info;
    DeviceBuffer<uint32_t> d_live;            // device counters of the bounce stage, a set of four per ray queue
    DeviceBuffer<uint32_t> d_pool_list;       // live pools by class, 2 x tiles
    // RWR_FLAG_SHADOWS, allocated by the first frame that asks for them: a 32-byte record per queue slot (as d_rays), their
    // ballots (as d_masks), the slot's two counters {shadow rays, occluded}
    DeviceBuffer<ShadowRec> d_shadow_recs;
    DeviceBuffer<unsigned long long> d_shadow_masks, d_shadow_counts;
    DeviceBuffer<uint32_t> d_tiles;           // frames that show little: live tile list, per-tile live pieces, the count (k_wf_classify)
    // RWR_FLAG_MIRRORS, _GLASS, _GLOSSY, allocated by the first frame with one of them: this slot's copy of the surface table
    // (WfSurfaces::table), the pinned image it is copied from on the slot's stream, the event behind that copy (the image is not
    // rewritten before it), and the context's surface_version the copy holds (0: none)
    DeviceBuffer<SurfaceRec> d_surface;
    PinnedSurface h_surface;
    size_t h_surface_count = 0;
    OwnedEvent surface_copied;
    uint64_t surface_version = 0;
    uint32_t surface_modes = 0;                // which surfaces that copy holds: 1 mirrors, 2 glass, 4 glossy (surface_mode, rwr_surface.h)
    DeviceBuffer<unsigned long long> d_surface_events;   // RWR_FLAG_GLASS, _GLOSSY: the frame's kEventNone counters by SurfaceEvent (WfSurfaces::events); zeroed per frame
    // RWR_FLAG_EMISSIVE, allocated by the first frame with an emitter: this slot's copy of the emission table (WfGlow::table), kept
    // as the surface table's copy is — pinned image, event behind the copy, the context's glow_version it holds (0: none) — and the
    // frame's count of emitting hits (WfGlow::hits), zeroed per frame
    DeviceBuffer<SurfaceRec> d_glow;
    PinnedSurface h_glow;
    size_t h_glow_count = 0;
    OwnedEvent glow_copied;
    uint64_t glow_version = 0;
    bool glow_dark = false;   // the copy holds zeros: a frame that runs the GLOW forms for RWR_FLAG_LIGHT_SKY without RWR_FLAG_EMISSIVE in effect
    DeviceBuffer<unsigned long long> d_glow_hits;
    // RWR_FLAG_LIGHT_SAMPLING, allocated by the first frame that samples its lights: per ray queue a 16-byte record per slot (the
    // hit's normal, WfGlow::light_recs) and the light ballots (layout of d_masks), kept like the queues; the frame's nine counts
    // {light rays, reached, silenced hits}, the mesh light's share of each and the sky's (WfGlow::light_counts), zeroed per frame
    DeviceBuffer<LightRec> d_light_recs;
    DeviceBuffer<unsigned long long> d_light_masks;
    DeviceBuffer<unsigned long long> d_light_counts;
    std::shared_ptr<DeviceBuffer<float4>> sky_image;   // RWR_FLAG_SKY_IMAGE: the image this slot's last frame under the flag reads, kept until the slot's next
    std::shared_ptr<DeviceBuffer<float>> sky_light;    // RWR_FLAG_LIGHT_SKY: likewise the image's sampling table (rwr_sky_light.h)
};

// Progressive accumulation (RWR_FLAG_ACCUMULATE): ONE accumulation per context.  Its sums and the first frame's sample-0 planes
// are context-wide (global pixel index, whatever the slot), allocated by the first accumulating frame; `key` is everything a
// frame must share with the one before for the accumulation to go on (accum_key), empty when the next frame starts over.
struct Accum {
    DeviceBuffer<unsigned long long> d_hist;   // 4 planes of W*H, 2^-26 fixed point (AccumBuffers::hist)
    DeviceBuffer<float> d_depth;
    DeviceBuffer<int32_t> d_obj_id;
    DeviceBuffer<float> d_hit_t;
    std::vector<unsigned char> key;
    uint64_t samples = 0;              // samples per pixel the history holds
    OwnedEvent done;                   // recorded after every accumulating resolve: the next one waits for it (frames in flight)
    bool done_recorded = false;
    // a new screen size: the history goes, the event and what it has seen stay
    void reset()
    {
        Accum fresh;
        fresh.done = std::move(done);
        fresh.done_recorded = done_recorded;
        *this = std::move(fresh);
    }
};

// Temporal reprojection (RWR_FLAG_REPROJECT): ONE history per context, as the accumulation's.  Two sets alternate — frame k reads
// set (k - 1) & 1 and writes set k & 1 — allocated by the first reprojecting frame; `key` is everything a frame must share with the
// one before for the history to go on (frame_request.cpp reproject_key_of; the camera is not in it), empty when the next frame starts over.
struct Reproject {
    DeviceBuffer<float4> d_colour[2], d_guide[2];   // {r, g, b, n}, {nhat.xyz or zeros, t} (RpHistory)
    DeviceBuffer<int32_t> d_id[2];
    DeviceBuffer<unsigned long long> d_counts;      // {reused, fresh, background} per set
    std::vector<unsigned char> key;
    uint64_t frames = 0;               // frames the history holds
    RpCamera camera{};                 // of the frame that wrote the history last
    OwnedEvent done;                   // recorded after every stage: the next one waits for it (frames in flight)
    bool done_recorded = false;
    // a new screen size: the history goes, the event and what it has seen stay
    void reset()
    {
        Reproject fresh;
        fresh.done = std::move(done);
        fresh.done_recorded = done_recorded;
        *this = std::move(fresh);
    }
};

// One gather set per frame slot (rwr_dist_*): the gather of the frame in one slot shares nothing with the frame rendered next in another
struct GatherSet {
    DeviceBuffer<uint8_t> d_gathered;       // root: the assembled RGBA8 frame
    DeviceBuffer<uint8_t> d_pack, d_recv;   // interleaved partition: this rank's message; root: every rank's, side by side (rwr_strips.h)
    OwnedEvent done;                        // the set's last gather has finished
    bool valid = false;                     // d_gathered holds (or will hold, once `done`) a whole frame
};

}  // namespace rwr

// Members are destroyed last to first: the streams come before everything that was enqueued on them.  rwr_ctx_destroy has
// waited for all of them by then.
struct rwr_context {
    int device = 0;
    rwr::OwnedStream own_stream;
    hipStream_t stream = nullptr;   // == slots[0].stream
    rwr::OwnedEvent ev_begin, ev_end;
    rwr::FrameSlot slots[rwr::kMaxFramesInFlight];
    uint32_t n_slots = 1;           // frames in flight
    uint32_t cur = 0;               // slot of the most recent frame

    // scene
    rwr::DeviceBuffer<rwr_model_vertex_small> d_verts;
    rwr::DeviceBuffer<rwr_model_face_small> d_faces;
    rwr::DeviceBuffer<rwr_instance_raw> d_instances;
    rwr::DeviceBuffer<rwr::TriRecord> d_tris;
    rwr::DeviceBuffer<rwr::ShadeRec> d_shade;
    rwr::DeviceBuffer<rwr::CullRec> d_cull;
    rwr::DeviceBuffer<rwr::TangentRec> d_tangent;            // per-face tangent frames (normal-mapped shading)
    std::vector<rwr::DeviceBuffer<float4>> d_nmaps;          // one optional normal map per scene part (linear texels)
    uint32_t bin_min_faces = 256;                       // tunable: RWR_BIN_MIN_FACES
    uint32_t bin_min_capacity = 65536;                  // tunable: RWR_BIN_CAPACITY (entries the bin lists start with)
    bool force_one_pixel = false;                       // debug: RWR_ONE_PIXEL_PER_LANE=1
    bool frame_graph = false;                           // A/B: RWR_FRAME_GRAPH=1 (hipGraph replay / update of the reference frame's launches)
    bool fused_setup = true;                            // one launch per small reference frame (k_primary_p2<FUSED>); RWR_FUSED_SETUP=0: two
    bool fused_setup_force = false;                     // RWR_FUSED_SETUP=1: wherever the fused form is possible
    bool tile_lists = true;                             // per-tile face sets from k_frame_setup for the two-pixel kernel; RWR_TILE_LISTS=0: it culls itself
    bool setup_cache = true;                            // a slot keeps its records while their inputs stand still (FrameSlot::records_key); RWR_SETUP_CACHE=0: made every frame
    uint64_t setup_launches = 0;                        // k_frame_setup launches put on a stream so far (rwr_frame_setup_launches)
    bool ray_plane = true;                              // a slot keeps its pixels' ray directions while the camera rests (FrameSlot::d_ray_plane); RWR_RAY_PLANE=0: computed every frame
    uint64_t ray_plane_builds = 0, ray_plane_frames = 0;   // k_ray_plane launches / frames that loaded their rays from a plane, so far (rwr_ray_plane_stats)
    bool tile_class = true;                             // the two-pixel kernel takes a tile by the class word k_frame_setup left with its face set; RWR_TILE_CLASS=0: it ignores the words
    struct LastClasses { uint32_t slot = 0, gx = 0, gy = 0; };   // the class words of the frame rendered last: its slot and the frame kernel's grid (gy == 0: it has none)
    LastClasses last_classes;                           // (rwr_debug_tile_classes)
    bool tile_cover = true;                             // a frame served from a slot's kept records learns and uses the tiles' cover words (rwr_internal.h kTileCovered); RWR_TILE_COVER=0: no frame looks at them
    uint64_t tile_cover_frames = 0;                     // frames that ran with RWR_FLAG_TILE_COVER so far (rwr_tile_cover_stats)
    uint32_t last_cover_frames = 0;                     // the frame rendered last: 0 without the flag, else its slot's FrameSlot::cover_frames (1: it learnt, more: it used what was learnt)
    bool lean_rest = true;                              // a resting camera's plain frame runs the frame kernel's lean form (kernels_primary_p2.hip k_primary_p2_lean); RWR_LEAN_REST=0: the cover form
    uint64_t lean_rest_frames = 0;                      // frames launched in the lean form so far (rwr_lean_rest_stats)
    // BVH over the (flattened) world-space faces, for bounce rays
    rwr::DeviceBuffer<rwr::BvhNode4> d_bvh_nodes;
    rwr::DeviceBuffer<uint32_t> d_bvh_leaf_faces;
    uint32_t bvh_n_nodes = 0, bvh_depth = 0;
    float bvh_leaf_extent = 0.0f;
    float wf_packet_extent = 0.5f;   // x mean leaf extent; tunable: RWR_WF_PACKET_EXTENT
    uint32_t wf_min_packet_pools = 64;    // tunable: RWR_WF_MIN_PACKET_POOLS (a quarter share of configs[4]'s frame has about 100 packet pools of 30 000 rays
                                          // and is 5 % faster with them as packets, an eighth share has 50 and is 10 % faster per lane: tools/share_probe.py)
    uint32_t wf_lane_items = 0;           // tunable: RWR_WF_LANE_ITEMS (0: chosen per frame, see the BvhDevice of the wavefront path)
    int32_t wf_wide_lane = -1;            // the per-lane trace kernel as 1 024-thread workgroups: -1 by itself (render_wavefront.cpp wf_schedule), tunable: RWR_WF_WIDE_LANE=0/1
    bool wf_stack16 = true;               // the per-lane kernels' 16-bit stack entries where the scene allows them (rwr_bvh.h lane_lds_plan); RWR_WF_STACK16=0: 32-bit
                                          // entries for every scene — and so no wide form, which needs the 16-bit ones.  It can only switch them off
    rwr::LanePlanRecord last_trace_plan, last_shadow_plan;   // the last wavefront frame's per-lane launches, by stage (rwr_last_traversal_plan)
    uint32_t wf_packet_dense_rays = 16384;   // a pool of at least this many rays (32 samples of a full tile) is traced as packets
                                             // however far apart its rays start; tunable: RWR_WF_PACKET_RAYS (0: never).  Measured
                                             // (tools/packet_rays_sweep.sh): configs[4]'s frame, 64 samples per group, 2.11 -> 1.75
                                             // ms with any threshold from 2 000 to 24 000 (2.30 -> 2.18 one frame at a time at
                                             // 16 000); configs[3], 16 samples (pools of at most 8 192): 0.604 -> 0.71-0.77 ms
                                             // with thresholds up to 8 000, unchanged from 12 000
    float aabb_lo[3] = {0, 0, 0}, aabb_hi[3] = {0, 0, 0};   // of the (flattened) world-space faces
    float auto_bvh_face_px = 150.0f;   // tunable: RWR_AUTO_BVH_FACE_PX (0 = never pick the BVH kernel by itself)
    // wavefront integrator: tunables and what the host remembers of the last frame
    rwr::PinnedWords h_wf_live;     // live pools of the last launch group {packets, per-lane}, read a frame late
    uint32_t wf_z_split = 0;        // tunable: RWR_WF_ZSPLIT (0 = from the previous frame's live pools)
    rwr::DeviceBuffer<unsigned long long> d_wf_dbg;   // RWR_WF_STATS=1: pool classification counters, printed at destroy
    uint64_t wf_launches_before[3] = {0, 0, 0};       // RWR_WF_STATS=1: wf_trace_launch_counts when the context was made
    uint32_t wf_group = 0;          // samples per launch group; tunable: RWR_WF_GROUP (1..64); 0: 32 for a context that renders one
                                    // frame at a time (a 64-spp frame's two groups overlap each other on two queues), 64 with frames in
                                    // flight (larger pools sort into tighter packets; the overlap comes from the other frame): measured
                                    // at configs[2], two slots: 8.55 -> 8.21 ms per frame; one slot: 8.81 -> 8.98
    float wf_packet_fill = 0.25f;   // pools filled at least this much are traced as packets; tunable: RWR_WF_PACKET_FILL (> 1: never)
    uint32_t last_segments = 0;     // tiles of the last wavefront frame
    uint32_t last_wf_state = 0;     // ... and whose accumulators and queues it used
    uint32_t wf_queues = 2;         // tunable: RWR_WF_OVERLAP (1 puts every launch group on the frame's stream; measured at
                                    // configs[2] / [4]: two queues -6.5 % / -9.5 %, three and four less, a staggered start less)
    rwr::WfState wf_state[rwr::kMaxFramesInFlight];
    uint32_t last_spp = 0;
    bool last_had_bounce = false;
    rwr::Accum accum;
    uint64_t accum_max = 1u << 24;         // samples per pixel at most (f32 holds the divisor exactly); RWR_ACCUM_MAX_SAMPLES lowers it
    uint64_t last_accum_samples = 0;       // rwr_accum_samples: of the frame rendered last, 0 when it did not accumulate
    rwr::Reproject reproj;
    rwr_reproject_params reproject = rwr::kReprojectDefaults;   // RWR_FLAG_REPROJECT (rwr_reproject_set_params)
    uint64_t last_reproject_frames = 0;    // rwr_reproject_frames: of the frame rendered last, 0 when it did not reproject
    uint32_t last_reproject_set = 0;       // ... and the history set it wrote (rwr_reproject_readback, rwr_last_reproject_stats)
    rwr_denoise_params denoise = rwr::kDenoiseDefaults;   // RWR_FLAG_DENOISE (rwr_denoise_set_params)
    rwr_tonemap_params tonemap = rwr::kTonemapDefaults;   // RWR_FLAG_TONEMAP (rwr_tonemap_set_params)
    bool last_tonemap = false;                            // the last render call ran the stage, with these parameters (rwr_last_tonemap_stats;
    rwr_tonemap_params last_tonemap_params = rwr::kTonemapDefaults;   // its record is its slot's d_tm_record)
    rwr_sky_params sky = rwr::kSkyDefaults;               // RWR_FLAG_SKY (rwr_sky_set_params)
    // RWR_FLAG_SKY_IMAGE (rwr_sky_set_image): the octahedral map, n x n float4 texels (null: none), and its generation.  A call makes a
    // new buffer; a frame slot holds on to the one its frame was enqueued with (WfState::sky_image), so nothing waits for a frame.
    std::shared_ptr<rwr::DeviceBuffer<float4>> sky_image;
    uint32_t sky_image_n = 0;
    uint64_t sky_image_generation = 0;
    // RWR_FLAG_LIGHT_SKY: the image's texels as the host handed them over (kept: the table is built lazily, by the first frame that asks
    // for the flag after the image changed — scene_sky_light), the table's device copy (null: none, or W = 0) and the image
    // generation it was built for (0: never)
    std::vector<float4> sky_image_host;
    std::shared_ptr<rwr::DeviceBuffer<float>> sky_light;
    uint64_t sky_light_generation = 0;
    rwr_shadow_params shadow = rwr::kShadowDefaults;      // RWR_FLAG_SOFT_SHADOWS (rwr_shadow_set_params)
    uint64_t scene_generation = 0;         // bumped by every change of the scene (an accumulation does not survive one)
    // one decoded texture per scene part (texels decoded to linear f32 at upload, Rgba8UnormSrgb semantics)
    std::vector<rwr::DeviceBuffer<float4>> d_texs;
    std::vector<rwr::DeviceBuffer<uint4>> d_quads;   // the same textures as quad records (rwr_internal.h QuadTex): the frame kernel's
    rwr::DeviceBuffer<const uint4 *> d_mat_quads;    // per material: its d_quads entry
    rwr::DeviceBuffer<float> d_srgb_lut;             // build_srgb_lut's table
    rwr::DeviceBuffer<uint32_t> d_face_mat;      // per face: index of its part's material
    rwr::DeviceBuffer<rwr::MaterialRec> d_materials;
    // host staging of the scene being assembled (rwr_scene_clear / add_mesh / commit)
    std::vector<rwr_model_vertex_small> st_verts;
    std::vector<rwr_model_face_small> st_faces;
    std::vector<uint32_t> st_face_mat;
    std::vector<rwr::MaterialRec> st_materials;
    uint32_t n_verts = 0, n_faces = 0, n_instances = 0, n_tris = 0;
    uint32_t tex_w = 0, tex_h = 0;
    rwr_material_data material{};
    bool have_mesh = false;
    bool tris_dirty = false;
    rwr_sphere_buffer_data spheres[RWR_MAX_SPHERES]{};
    uint32_t n_spheres = 0;
    // RWR_FLAG_MIRRORS (rwr_scene_set_part_mirror / _sphere_mirror): {r, g, b, on} per scene part (one entry per st_materials
    // entry) and per sphere index; surface_version counts their changes, a WfState's table is refreshed when it lags behind
    std::vector<rwr::SurfaceRec> part_surfaces;
    rwr::SurfaceRec sphere_surfaces[RWR_MAX_SPHERES]{};
    uint64_t surface_version = 1;
    // RWR_FLAG_EMISSIVE (rwr_scene_set_part_emission / _sphere_emission): the radiance {r, g, b, 0} per scene part and per sphere
    // index, beside the surface records and with their reset rules; glow_version counts their changes (a WfState's table lags behind)
    std::vector<rwr::SurfaceRec> part_glow;
    rwr::SurfaceRec sphere_glow[RWR_MAX_SPHERES]{};
    uint64_t glow_version = 1;
    // RWR_FLAG_LIGHT_PARTS: the mesh light (rwr_part_lights.h) — the world-space corners rebuild_tris read back (9 floats per world
    // face), the list built from them and the parts' radiances, and its device copy.  part_lights_dirty: the scene's faces or a part's
    // emission changed since the list was built; scene_part_lights (scene.cpp) rebuilds and uploads it for the next frame that asks.
    std::vector<float> world_corners;
    std::vector<rwr::PartLightRec> part_lights;
    rwr::DeviceBuffer<rwr::PartLightRec> d_part_lights;
    bool part_lights_dirty = true;
    std::vector<float> part_inv_pdf;   // RWR_FLAG_LIGHT_MIS: per part, the inv_pdf of its listed faces (0: none listed), as the list built last holds it
    rwr::WfLights lights{};   // RWR_FLAG_LIGHT_SAMPLING: the emitting spheres in use (scene.cpp rebuild_lights: after the emission setters and rwr_scene_set_spheres)
    rwr_triangle_buffer_data triangles[RWR_MAX_TRIANGLES]{};
    uint32_t n_triangles = 0;

    // targets
    rwr_screen screen{0, 0};

    uint64_t last_primary = 0, last_bounce = 0;
    bool last_shadows = false;      // the last render call traced shadow rays (RWR_FLAG_SHADOWS): their counters are in its WfState
    bool last_gloss = false;        // the last render call ran the glossy forms (RWR_FLAG_GLOSSY): their counter is d_surface_events[kEventGlossy]
    bool last_glass = false;        // the last render call ran the glass forms (RWR_FLAG_GLASS): their counters are in its WfState
    bool last_light = false;        // the last render call sampled its lights (RWR_FLAG_LIGHT_SAMPLING, RWR_FLAG_LIGHT_PARTS, RWR_FLAG_LIGHT_SKY): the counts are its WfState's d_light_counts
    bool last_glow = false;         // the last render call ran the GLOW forms (RWR_FLAG_EMISSIVE): their counter is its WfState's d_glow_hits
    // optional per-kernel timing (rwr_ctx_set_kernel_timing)
    uint32_t timing_every = 0;
    uint64_t timing_calls = 0;
    std::vector<rwr::OwnedEvent> timing_events;  // pairs
    uint32_t timing_pairs = 0;
    uint32_t wave_cull_min = 4;  // tunable: RWR_WAVE_CULL_MIN
    // multi-GPU frame (rwr_dist_*): one process per GPU, one RCCL communicator per context
    ncclComm_t comm = nullptr;
    int dist_rank = 0, dist_world = 0;
    rwr::GatherSet gather[rwr::kMaxFramesInFlight];
    uint32_t last_gather = 0;               // the set rwr_dist_frame / rwr_dist_readback refer to
    rwr::OwnedEvent exchange_done;          // orders the RCCL exchanges of consecutive frames (they run on different slots' streams)
    // shader-clock probe (rwr_clock_probe_start / _read): one spinning wave on its own stream
    rwr::OwnedStream probe_stream;
    rwr::DeviceBuffer<ulonglong2> d_probe;
};

namespace rwr {

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Waits for every frame in flight (scene changes, resizes, stream changes and teardown need an idle context).
inline hipError_t sync_all(rwr_context *ctx)
{
    hipError_t first = hipSuccess;
    for (uint32_t i = 0; i < kMaxFramesInFlight; i++) {
        if (!ctx->slots[i].stream) continue;
        const hipError_t e = hipStreamSynchronize(ctx->slots[i].stream);
        if (first == hipSuccess) first = e;
    }
    return first;
}

// faces the kernels see: every face of the mesh once per instance (no instances: once); at most 2^31 - 1 in a scene that was accepted
inline uint64_t instanced_faces(uint64_t n_faces, uint32_t n_instances) { return n_faces * (n_instances ? n_instances : 1u); }

// which surface models the context's parts and its spheres in use hold, as surface_mode bits
inline uint32_t surface_modes(const rwr_context *ctx)
{
    uint32_t modes = 0;
    for (const SurfaceRec &m : ctx->part_surfaces) modes |= surface_mode(surface_model(m));
    for (uint32_t i = 0; i < ctx->n_spheres; i++) modes |= surface_mode(surface_model(ctx->sphere_surfaces[i]));
    return modes;
}
// does a part of the context's scene or one of its spheres in use emit (RWR_FLAG_EMISSIVE)?
inline bool scene_glows(const rwr_context *ctx)
{
    for (const SurfaceRec &g : ctx->part_glow)
        if (glows(g)) return true;
    for (uint32_t i = 0; i < ctx->n_spheres; i++)
        if (glows(ctx->sphere_glow[i])) return true;
    return false;
}
// the emitting spheres in use, in index order (RWR_FLAG_LIGHT_SAMPLING: s_0 < ... < s_{M-1}); scene.cpp keeps ctx->lights equal to it
inline WfLights scene_lights(const rwr_context *ctx) { return ctx->lights; }
// scene.cpp: the mesh light's length, after rebuilding and uploading the list if the scene changed it (RWR_FLAG_LIGHT_PARTS item 1);
// waits for the frames in flight only when it has to upload.  Called for frames that ask for the flag, so no other frame pays.
int scene_part_lights(rwr_context *ctx, uint32_t &n);
// context.cpp: whether the sky's image has a sampling table (RWR_FLAG_LIGHT_SKY item 1: an image, and W > 0), after building and
// uploading it if the image changed since the last one was built.  Called for frames that ask for the flag, so no other frame pays.
int scene_sky_light(rwr_context *ctx, bool &have);

// context.cpp: per-frame buffers of every active slot for the current scene and screen
hipError_t ensure_frame_buffers(rwr_context *ctx);
// scene.cpp: the world-space records and the BVH, when the mesh or its instances have changed
int rebuild_tris(rwr_context *ctx);
// render_reference.cpp: a frame of the fused frame kernel in idle slot `i` is complete
int check_fused_frame(rwr_context *ctx, uint32_t i);

}  // namespace rwr
