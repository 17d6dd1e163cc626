// Internal declarations shared by the HIP kernels and the C-ABI implementation.
// Not part of the public boundary (include/rwr_hip.h is).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rwr_hip.h"
#include "rwr_part_lights.h"
#include "rwr_surface.h"

namespace rwr {

// Internal debug flag (not in the public header): with RWR_FLAG_AUX_OUTPUTS, the
// obj_id plane receives the number of block-level candidate faces and the hit_t
// plane the number of faces the pixel's wave ran the exact test on.  (Bit 20: bit 16, which it had, is the public header's
// RWR_FLAG_LIGHT_SAMPLING now.  Bits 17-20 are the internal ones; the header reserves them and goes on at bit 21.)
constexpr uint32_t RWR_FLAG_DEBUG_COUNTS = 1u << 20;

// Internal: render frames with the one-pixel-per-lane kernel (k_primary) instead of the
// two-pixels-per-lane one (k_primary_p2); both must give identical results.
constexpr uint32_t RWR_FLAG_ONE_PIXEL_PER_LANE = 1u << 17;
// Internal, set by render_reference.cpp alone (a caller's bit is cleared): the frame's per-tile face sets come with class words
// (TileClassIn below) and the two-pixel frame kernel branches on them.  Clear (RWR_TILE_CLASS=0): the kernel never loads one.
constexpr uint32_t RWR_FLAG_TILE_CLASS = 1u << 18;
// Internal, set by render_reference.cpp alone (a caller's bit is cleared), only beside RWR_FLAG_TILE_CLASS and only on a frame that found its
// slot's records made (launch_records: a key hit): the kernel reads the tiles' cover words (kTileCovered below) and writes the ones
// it learns.  Clear (a key miss, RWR_TILE_COVER=0, any other form): the kernel neither reads nor writes them.
constexpr uint32_t RWR_FLAG_TILE_COVER = 1u << 19;
constexpr uint32_t kInternalFlags = RWR_FLAG_DEBUG_COUNTS | RWR_FLAG_ONE_PIXEL_PER_LANE | RWR_FLAG_TILE_CLASS | RWR_FLAG_TILE_COVER;
static_assert(kInternalFlags == RWR_FLAGS_RESERVED && (kInternalFlags & RWR_FLAGS_PUBLIC) == 0u, "no internal bit equals a public one: the internal bits are the ones the header reserves");

// ---------------------------------------------------------------------------
// Device-side scene records (data layout in HBM, see DESIGN.md §"Data layout").
//
// TriRecord: everything triangleRayIntersect (compute.wgsl:82-148) derives from
// the triangle alone, hoisted out of the per-ray loop.  The values are produced
// by k_prebake with exactly the operations the shader writes (no fusion), so
// hoisting does not change a single bit of the per-ray result.
// 128 B = four s_load_dwordx8 when the face index is wave-uniform.
struct alignas(16) TriRecord {
    float p0[3]; float d;      // d = -dot(N, p0)                      compute.wgsl:99
    float p1[3]; float denom;  // denom = dot(N, N)                    compute.wgsl:88
    float p2[3]; float pad0;
    float N[3];  float pad1;   // cross(p1 - p0, p2 - p0)              compute.wgsl:84-87
    float e0[3]; float pad2;   // p1 - p0                              compute.wgsl:115
    float e1[3]; float pad3;   // p2 - p1                              compute.wgsl:123
    float e2[3]; float pad4;   // p0 - p2                              compute.wgsl:132
    float nhat[3]; float pad5; // normalize(N), literal f32 operations (compute.wgsl:142 before the flip of :140):
                               // the extended integrator's bounce rays start from it (normalize(-N) == -normalize(N) exactly)
};
static_assert(sizeof(TriRecord) == 128, "TriRecord is 128 B");

// Per-face shading record (colour path only; 48 B = three dwordx4), made by k_prebake.
// Everything of triangle_list/compute.wgsl:217-234 that depends on the face alone is folded in
// double precision and rounded once: the unit normal, its Lambert term against the fixed
// directional light (:55), and the affine map from the winner's un-normalised edge functions
// (u, v) (:126,135) to texel space,  (x, y) = c0 + u*c1 + v*c2  with  x = tex_w * dot(barycentric,
// tex_coords.x) - 0.5  (:144-147,218-225), y likewise with the 1 - v flip of :224.  (x, y) pairs are
// adjacent so that the map is two v_pk_fma_f32.
struct alignas(16) ShadeRec {
    float n[3];  float ndl0;        // N / |N| (as wound, not flipped), dot(n, -normalize(kLightDir))
    float c0[2], c1[2];
    float c2[2]; uint32_t material; // index into MaterialRec[]
    float pad;
};
static_assert(sizeof(ShadeRec) == 48, "ShadeRec is 48 B");

// Largest texture edge accepted (wgpu's own default limit is 8192): keeps tap byte offsets in 32 bits.
constexpr uint32_t kMaxTextureDim = 16384;

// One material (MaterialData's ambient / specular, triangle_list.rs:24-33) with its decoded diffuse
// texture.  The reference binds materials[0] only (triangle_list.rs:212); more than one is an extension.
struct alignas(16) MaterialRec {
    float ambient[3];  uint32_t tex_w;
    float specular[3]; uint32_t tex_h;
    const float4 *tex;
    float wmax, hmax;               // (float)(tex_w - 1), (float)(tex_h - 1): the ClampToEdge bounds
    const float4 *nmap;             // optional normal map (extension, RWR_FLAG_NORMAL_MAP): linear texels, nullptr = none
    uint32_t nmap_w, nmap_h;
};
static_assert(sizeof(MaterialRec) == 64, "MaterialRec is 64 B");

// The frame kernel's (k_primary_p2) form of the diffuse textures: one 16-byte "quad" record per bilinear footprint, so that
// a pixel's four taps are ONE vector-memory instruction (the texture addresser's cost is per instruction, not per byte).
// Record (px, py), px in [0, w], py in [0, h], row pitch w + 1, holds the texels (cx(px-1), cy(py-1)), (cx(px), cy(py-1)),
// (cx(px-1), cy(py)), (cx(px), cy(py)) with cx / cy ClampToEdge on [0, w-1] / [0, h-1].  A texel is one dword
// r << 2 | g << 12 | b << 22 of its sRGB bytes: each channel's byte offset into the 256-float decode table
// (build_srgb_lut), which the kernel keeps in LDS.  Alpha is not stored: shading never reads it.
struct QuadTex {
    const uint4 *quad0;         // material 0
    const uint4 *const *mats;   // per material (n_materials > 1)
    const float *lut;           // build_srgb_lut's table (device memory; the kernel copies it to LDS)
};
// host (frame_consts.cpp): the (w + 1) * (h + 1) records of a w x h RGBA8 image, 4 dwords each
void build_tex_quads(const uint8_t *rgba8, uint32_t w, uint32_t h, uint32_t *out);
// host (frame_consts.cpp): the 256 floats of the Rgba8UnormSrgb decode
void build_srgb_lut(float *lut);

// Per-face tangent frame for normal-mapped shading (extension; 32 B, made by k_prebake in double and rounded once):
// t = normalize(dP/du - n (n . dP/du)), b = +-cross(n, t) towards -dP/dv' (v' = 1 - v: the sampling space of
// compute.wgsl:224; the map's green axis points up the image); zeros for degenerate texture coordinates.
struct alignas(16) TangentRec {
    float t[3]; float pad0;
    float b[3]; float pad1;
};
static_assert(sizeof(TangentRec) == 32, "TangentRec is 32 B");

// The three corners again, packed (48 B): what the conservative tile/block
// frustum tests read, one record per lane, coalesced.
struct alignas(16) CullRec {
    float p0[3], p1[3], p2[3];
    float pad[3];
};
static_assert(sizeof(CullRec) == 48, "CullRec is 48 B");

struct Targets {
    uint8_t *color;     // W*H*4 rgba8unorm            (screen_texture, lib.rs:503-515)
    float *depth;       // W*H r32float                (depth_texture_output, lib.rs:482-495)
    float *color_f32;   // W*H*4, aux
    int32_t *obj_id;    // W*H, aux
    float *hit_t;       // W*H, aux
};

// The culling margins (rwr_cull.h).  The host evaluates its side in double from these doubles (frame_consts.cpp); the kernels'
// floats are the same numbers rounded once.
constexpr double kCullRelHost = 2e-5;                      // relative margin, folded into CullConsts::corner_margin
constexpr double kCullWorldHost = 12.0 * 5.9604645e-8;     // 12 f32 unit roundoffs of the world magnitude
constexpr float kCullRel = (float)kCullRelHost;
constexpr float kCullWorld = (float)kCullWorldHost;

// Per-frame constants of the conservative culling code (host-computed in double
// from the camera uniform, frame_consts.cpp).  The un-normalised world direction of the
// ray through pixel-space point (fx, fy) is affine:  dir = A + fx*Bx + fy*By
// (compute.wgsl:151-159), so every plane through the origin that contains a
// pixel column x = const or row y = const has the normal  Ux + x*Vx  resp.
// Uy + y*Vy, and a point q = t*dir(x, y) has  Vx.q = t*vxa,  Vy.q = t*vya.
struct CullConsts {
    float A[4], Bx[4], By[4];
    float Ux[4], Vx[4];    // [3]: L1 norm of the xyz part
    float Uy[4], Vy[4];
    float origin[4];
    float vxa, vya;        // Vx.A, Vy.A  (non-zero for a pinhole camera)
    float corner_margin;   // kCullRel * max |dir|_1 over the frame
    uint32_t enabled;      // 0: degenerate camera, cull nothing
};

// Per-frame, per-face culling record written by k_frame_setup (64 B, one
// dwordx4 x4 per lane): the face's conservative pixel-space bounding rectangle
// and, for each of its edges, the affine function  d(x, y) = ea + x*ex + y*ey
// of dot(edge plane normal, dir(x, y)), signed so that the face can only be hit
// where all three are >= -me.
struct alignas(16) FrameTri {
    float bx0, by0, bx1, by1;
    float ea[3]; float me0;
    float ex[3]; float me1;
    float ey[3]; float me2;
};
static_assert(sizeof(FrameTri) == 64, "FrameTri is 64 B");

// Per-frame screen bins (kernels_primary.hip k_bin_faces): for scenes with more faces than one
// 256-wide batch, every 64x32-pixel bin (= 2x4 workgroups of the render kernels) gets the
// ascending list of faces that can be seen through it, so a workgroup walks its bin's list
// instead of the whole scene.  Built once per frame, shared by all sample passes.
constexpr uint32_t kBinW = 64, kBinH = 32;
struct BinGrid {
    const uint32_t *lists;    // the bins' face lists, back to back (sized by a count pass: count -> exclusive scan -> fill)
    const uint32_t *counts;   // bins
    const uint32_t *offsets;  // bins: where a bin's list starts; kBinNoList = "walk the whole scene" (the lists did not
                              // fit this frame's capacity; the context grows it for the next frames)
    uint32_t bins_x, bins_y, capacity, enabled;
};
constexpr uint32_t kBinNoList = 0xffffffffu;
constexpr uint32_t kStripRows = 8;   // rows of a strip = of every render kernel's workgroup tile (RWR_STRIP_ROWS)
// Per-tile face sets (FrameParams::tile_lists): a 256-bit set per 32x4 tile, for scenes of at most kTileListMaxFaces faces
// (made by waves of k_frame_setup that cover kListRegionsPerWave regions of kListRegionWgs x kListRegionWgs workgroups each)
constexpr uint32_t kTileListMaxFaces = 256, kTileListWords = kTileListMaxFaces / 32;
constexpr uint32_t kListRegionWgs = 4, kListRegionsPerWave = 1;
// One class word per tile, a parallel array behind the sets in the same buffer (word 8 * tiles + tile, tiles = 4 * workgroups of
// the frame kernel's grid; tile = 4 * workgroup + wave, as the sets), made by the same lane of k_frame_setup that makes the set
// (rwr_frame_setup.h) from the compares the frame kernel would make itself:
//   bits 0-1   faces: kTileFacesNone / One / More — the set's population, and None for a tile outside the mesh's pixel rectangle
//              (FrameParams::mesh_px, the kernel's `live`)
//   bits 8-15  the face's index when there is exactly one
//   bits 16-23 spheres: bit s set <=> s < n_spheres and the tile's rectangle touches sphere s's (FrameParams::sphere_rect)
// The kernel (kernels_primary_p2.hip) takes one of three ways through a tile by it, once per wave.
constexpr uint32_t kTileFacesNone = 0u, kTileFacesOne = 1u, kTileFacesMore = 2u, kTileFacesMask = 3u;
constexpr uint32_t kTileFaceShift = 8u, kTileSphereShift = 16u, kTileSphereMask = 0xffu << kTileSphereShift;
static_assert(RWR_MAX_SPHERES <= 8 && kTileListMaxFaces <= 256, "a class word has 8 bits for the spheres and 8 for a face index");
// One cover word per tile, a third parallel array behind the class words (word 9 * tiles + tile).  The setup lane that writes a
// tile's class word zeroes it; the frame kernel of a frame served from the slot's kept records (RWR_FLAG_TILE_COVER) sets it to
// kTileCovered when its own hit test found, for a tile of class "one face, no sphere", that every pixel pair of the tile hit the
// face, won the depth test and stayed in the domain of both short forms (division, depth) — a pure function of what RecordsKey
// holds, so it stands exactly as long as the class word beside it — and from the next such frame on takes the tile without the
// tests that could only confirm it.
constexpr uint32_t kTileCovered = 1u;
inline size_t tile_list_words(uint32_t gx, uint32_t gy) { return (size_t)gx * gy * 4u * (kTileListWords + 2u); }   // sets, then class words, then cover words

struct FrameParams {
    rwr_camera_inv_uniform cam;
    BinGrid bins;
    uint32_t width, height;       // full frame
    uint32_t row_begin, row_end;  // band rendered by this launch ...
    uint32_t row_pitch;           // ... in 8-row strips: strip k of the launch starts at row_begin + k * row_pitch (8: every row of the
                                  // band; 8 N: every N-th strip — the interleaved partition of a multi-GPU frame, rwr_render_strips)
    uint32_t n_spheres;
    uint32_t n_tris;
    uint32_t tex_w, tex_h;
    float tex_wmax, tex_hmax;     // (float)(tex_w - 1), (float)(tex_h - 1) of material 0
    uint32_t flags;
    uint32_t wave_cull_min;   // run the per-wave (8x8 tile) cull only for block lists longer than this
    // wavefront integrator (extension): samples per pixel of this frame; the count the jitter rule looks at (jittered when > 1:
    // the frame's spp, at least 2 in an accumulating frame, RWR_FLAG_ACCUMULATE); RNG seed; bounces
    uint32_t spp, jitter_spp, seed, bounces;
    rwr_sphere_buffer_data spheres[RWR_MAX_SPHERES];
    // conservative pixel-space bounds {x0, y0, x1, y1} of each sphere's silhouette
    // (host-computed per frame, frame_consts.cpp); a tile outside them skips the sphere
    float sphere_rect[RWR_MAX_SPHERES][4];
    // conservative pixel-space bounds of the whole mesh's bounding box (+-inf when the camera is in or near it):
    // a tile outside skips the mesh pass
    float mesh_rect[4];
    int32_t mesh_px[4];   // the same, rounded outwards to whole pixels (scalar compares in the frame kernel)
    float ambient[4];
    float specular[4];
    // Per-frame tables written by k_frame_setup (the frame kernel with centre rays reads them; nothing
    // here changes a bit of the ray: the entries are the shader's own operations, hoisted because they
    // depend on the column, the row or the face alone):
    //   ray_colp[x / 2] (x even) = two float4 {c(x).x, c(x+1).x, c(x).y, c(x+1).y}, {c(x).z, c(x+1).z, -, -}
    //   with c(x) = proj_inv[0].xyz * x_nds(x),  x_nds = 2 * (x + 0.5) / width - 1     (compute.wgsl:151-155)
    //   ray_row[y] = {proj_inv[1].xyz * y_nds(y), y_nds}
    //   tnum[face] = -(dot(N, origin) + d)                                              (compute.wgsl:99-102)
    const float4 *ray_colp;
    const float4 *ray_row;
    const float *tnum;
    // multi-material scenes (n_materials > 1): per-face material through ShadeRec::material
    const MaterialRec *materials;
    uint32_t n_materials;
    uint32_t pad_m;
    const TangentRec *tangents;   // per face (RWR_FLAG_NORMAL_MAP)
    // Per-tile face sets of the two-pixel frame kernel, made by k_frame_setup (rwr_frame_setup.h frame_tile_lists_block):
    // kTileListWords words per 32x4 tile, bit f set = face f survives the tile's culling.  Null: the kernel culls itself.
    const uint32_t *tile_lists;
};
// 8-row strips a launch renders (the y extent of every render kernel's grid)
inline uint32_t band_strips(const FrameParams &fp) { return fp.row_end > fp.row_begin ? (fp.row_end - fp.row_begin + fp.row_pitch - 1u) / fp.row_pitch : 0u; }

// Host arithmetic of a frame (frame_consts.cpp; no device needed): what fill_frame_consts reads of the scene and the screen ...
struct FrameScene {
    uint32_t width, height;
    const rwr_sphere_buffer_data *spheres;
    uint32_t n_spheres;
    uint32_t n_tris, tex_w, tex_h;
    const float *aabb_lo, *aabb_hi;   // of the world-space faces
    const rwr_material_data *material;
    const MaterialRec *materials;     // device
    uint32_t n_materials;
    const TangentRec *tangents;       // device
    uint32_t wave_cull_min;
};
// ... and what it makes of them and the camera: the kernels' parameters but the per-frame tables, bins and tile lists (whoever
// enqueues the frame owns those), the culling constants, and the mean projected area of a face in pixels (+inf: unknown)
struct FrameConsts {
    FrameParams fp;
    CullConsts cc;
    double mean_face_px;
};
void fill_frame_consts(const FrameScene &scene, const rwr_camera_inv_uniform &cam, const rwr_render_params &rp, bool accumulate,
                       uint32_t row_begin, uint32_t row_end, uint32_t row_pitch, FrameConsts &out);

// context.cpp: records the calling thread's error message, returns `code`.
int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// kernels_primary.hip
hipError_t launch_prebake(hipStream_t s, const rwr_model_vertex_small *verts, const rwr_model_face_small *faces,
                          const uint32_t *face_material, uint32_t n_faces, const rwr_instance_raw *instances,
                          uint32_t n_instances, const MaterialRec *materials, TriRecord *tris, ShadeRec *shade, CullRec *cull,
                          TangentRec *tangents);
// Wavefront integrator state (kernels_wf_primary.hip / kernels_wf_bounce.hip).  A launch group traces `group`
// samples of every pixel.  A *tile* is the 64x8-pixel block of one workgroup of the primary stage (4 waves of
// 32x4 pixels, two pixels per lane); its *pool* is the bounce rays those samples emit.  Ray queue = SoA in HBM,
// 32 B per bounce ray, at FIXED slots
//     slot = (tile * group + sample_in_group) * 512 + wave * 128 + k * 64 + lane        (k: which pixel of the lane)
// rays[2 slot] = {O.xyz, throughput r | g << 16}, rays[2 slot + 1] = {D.xyz, throughput b}: ONE 32-byte record per ray, because
// the bounce stage reads rays in sorted order, i.e. at random slots, and every separate access costs a whole memory
// sector (three separate arrays measured 4.5x the bytes the rays have); the throughput (the first hit's albedo, in
// [0, 1]) travels as unorm16, which moves a colour by at most 8e-6 of the second hit's radiance.  masks[(tile * group + s) * 8 + wave * 2 + k] = ballot of the
// lanes that emitted.  The bounce stage compacts a pool by those ballots while sorting it by direction.
constexpr uint32_t kWfTileW = 64, kWfTileH = 8, kWfTilePixels = kWfTileW * kWfTileH;
#ifndef RWR_WF_MAX_GROUP
#define RWR_WF_MAX_GROUP 64
#endif
constexpr uint32_t kWfMaxGroup = RWR_WF_MAX_GROUP;   // samples per launch group at most (the sort's LDS: 4 B per ray of a pool = 128 KiB at 64;
                                                     // the primary stage's 32-bit sums: kWfMaxGroup terms of at most kWfE0Cap)
constexpr float kWfFixedScale = 67108864.0f;  // 2^26: a term < 64, thousands of them < 2^64
// The integrator's definition (rwr_hip.h rwr_render_params; oracle render_path_core): a sample's E(h0) is clamped to [0, 16] per
// channel, its albedo * E(h1) to [0, 64] (= what a u32 of 2^-26 units holds: the float -> u32 conversion saturates).  Fixed
// numbers, not tuning parameters.
constexpr uint32_t kWfE0Cap = 16;
#ifndef RWR_WF_CELL_BITS
#define RWR_WF_CELL_BITS 4
#endif
constexpr uint32_t kWfDirCellBits = RWR_WF_CELL_BITS;                 // cells per side of an octant of the octahedral map, log2
constexpr uint32_t kWfDirBins = 8u << (2u * kWfDirCellBits);   // 8 octants x 16x16 cells (8x8: +6 % at configs[2] — coarser packets; the sort keeps its
                                                               // counts and offsets in ONE LDS array, or the finer histogram costs it its occupancy)
struct WfBuffers {
    unsigned long long *fix;       // 4 planes of W*H: the frame's radiance sums as 2^-26 FIXED POINT — red, green, blue of
                                   // E(h0) + albedo(h0) * E(h1) over all samples, and alpha (2 per primary hit).  Integer sums are
                                   // the same bits in whatever order and by whichever workgroups they are added.
    float4 *rays;                  // two float4 per slot: {O.xyz, thr.r | thr.g << 16}, {D.xyz, thr.b} (throughput as unorm16)
    unsigned long long *masks;
    uint16_t *bins;                // per slot: the ray's direction bin (wf_direction_bin; written with the ray, read by the sort)
    uint16_t *sorted;              // per tile: group * 512 pool slots in direction order (scratch of the bounce stage)
    uint32_t *wave_total;          // per tile and wave: bounce rays emitted over all groups of the frame
    uint32_t group;                // samples per launch group this frame
    uint32_t tiles_x;
    unsigned long long *dbg;       // optional (RWR_WF_STATS=1): {packet pools, their rays, per-lane pools, their rays}
    uint32_t *counters;            // this queue's four counters of the bounce stage (kernels_wf_bounce.hip); null without a bounce
    uint32_t shared_planes;        // another launch group may be adding to `fix` at the same time: atomics only
    // frames that show little (k_wf_classify ran): the tiles something can be seen through, how many, and per tile which of its
    // four waves' 32x4-pixel pieces; null otherwise (every tile is looked at)
    const uint32_t *live_list;
    const uint32_t *live_count;
    const uint32_t *tile_live;
};
// Deeper paths (RWR_FLAG_MULTI_BOUNCE; the EMIT forms of the trace kernels, kernels_wf_bounce.hip): the next generation's ballots
// (same layout as WfBuffers::masks, cleared before the generation), the RNG dimension its rays start from (2 + 16 k for ray
// k + 1), and the global sample index of the launch group's first sample (accumulation base + group base).  A kernel argument
// of its own behind the others, so that the kernels which end a path keep their argument layout and their code.
struct WfEmit {
    unsigned long long *masks_out;
    uint32_t next_dim;
    uint32_t sample_base;
};
// Shadow rays (RWR_FLAG_SHADOWS; kernels_wf_shadow.hip).  The kernel that shades a hit adds the term's ambient part to the sums and
// leaves a 32-byte record at the hit's fixed queue slot: where the shadow ray starts, which of the reference's two lights it
// runs towards (flags bit 0: the sphere shader's), and per channel what the light adds to the term — fix(lit) - fix(ambient)
// modulo 2^32, flags bit 1 + c set when channel c's difference is negative — which k_wf_shadow adds when the ray gets through.
// Wrapping 64-bit sums: ambient + (lit - ambient) is the lit term's bits whoever adds what when.
struct alignas(16) ShadowRec {
    float o[3]; uint32_t flags;
    uint32_t d[3]; uint32_t pad;
};
static_assert(sizeof(ShadowRec) == 32, "ShadowRec is 32 B");
// Per ray queue: the records (one per slot, as WfBuffers::rays), their ballots (layout of WfBuffers::masks) and the slot's two
// counters {shadow rays traced, occluded}.  A kernel argument of its own behind the others (cf. WfEmit); recs == nullptr: no shadows.
struct WfShadow {
    ShadowRec *recs;
    unsigned long long *masks;
    unsigned long long *counts;
};
// Soft shadows (RWR_FLAG_SOFT_SHADOWS; the SOFT forms of k_wf_shadow): per light ([0] the mesh shader's, [1] the sphere shader's)
// bounce_direction's basis about the unit vector towards it and its radius; the first of the 16 RNG dimensions this launch's disk
// draws read (130 + 16 k behind generation k: behind every block a path reads) and the global sample index of the launch group's
// first sample.  A kernel argument of its own behind the others (cf. WfEmit), so that the hard forms keep their code.
struct WfSoft {
    float b1[2][3], b2[2][3], radius[2];
    uint32_t dim0, sample_base;
};
// Sky light (RWR_FLAG_SKY; the SKY forms of the trace kernels, kernels_wf_bounce.hip): the context's rwr_sky_params.  A kernel
// argument of its own behind the others (cf. WfEmit), so that the six floats are scalar registers and the kernels without the
// flag keep their code.
struct WfSky {
    float zr, zg, zb, hr, hg, hb;   // zenith, horizon: rwr_sky_params' six floats in its order (plain members, no arrays: they stay registers)
};
static_assert(sizeof(WfSky) == sizeof(rwr_sky_params), "WfSky is rwr_sky_params");
// The sky's image (RWR_FLAG_SKY_IMAGE; the IMG forms of the trace kernels' SKY forms, add_sky_image): the context's octahedral map,
// n x n float4 texels, and n; image == nullptr: the gradient of WfSky, the SKY forms without IMG.  A kernel argument of its own
// behind all others (cf. WfEmit): no other form reads it, and all of them keep their instructions.
// table: RWR_FLAG_LIGHT_SKY in effect — the image's sampling distribution (rwr_sky_light.h), read by k_wf_light's SKY forms and, behind
// WfGlow::light & 8, at the miss sites of the trace kernels' IMG x GLOW forms; null otherwise.  (The last member of the last
// argument: no other argument moves.)
struct WfSkyImage {
    const float4 *image;
    uint32_t n;
    uint32_t pad;
    const float *table;
};
// The mesh light (RWR_FLAG_LIGHT_PARTS; rwr_part_lights.h): the face list, its length, the frame's shading records (a listed face's
// part is ShadeRec::material, its radiance that part's record of WfGlow::table) and L = M + 1, the lights the stage chooses among.
// A kernel argument of k_wf_light behind WfLights: scalar registers.
struct WfPartLights {
    const PartLightRec *list;
    const ShadeRec *shade;
    uint32_t n;
    uint32_t l;
};
// What the kernels of one launch group know: the four argument structs above — all zero where the frame lacks the flag, and that
// is what the kernels then get — and the switches the launchers pick the kernels' forms by.  render_wavefront.cpp fills it once per launch
// group; `emit` and `emits` change per generation (a generation that is not the path's last: the trace kernels' EMIT forms).
struct WfFeatures {
    WfEmit emit{nullptr, 0u, 0u};
    WfShadow shadow{nullptr, nullptr, nullptr};
    WfSky sky{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    WfSkyImage sky_image{nullptr, 0u, 0u, nullptr};   // RWR_FLAG_SKY_IMAGE in effect: the image the IMG forms fetch S(D) from (else null: the gradient)
    WfSurfaces surfaces{nullptr, 0u, 0u, nullptr};   // rwr_surface.h
    WfGlow glow{nullptr, 0u, 0u, nullptr, nullptr, nullptr, nullptr};   // rwr_surface.h
    bool emits = false, shadows = false, sky_on = false;
    bool glows = false;   // RWR_FLAG_EMISSIVE with an emitter in the scene: the GLOW forms of all three kernels, which read `glow`
    bool soft = false;   // RWR_FLAG_SOFT_SHADOWS: k_wf_shadow's SOFT forms (no other kernel looks)
    bool lights_on = false;   // RWR_FLAG_LIGHT_SAMPLING, RWR_FLAG_LIGHT_PARTS or RWR_FLAG_LIGHT_SKY: glow.light is set, k_wf_light runs (kernels_wf_light.hip) with `lights`
    WfLights lights{};        // rwr_surface.h (m = 0 while RWR_FLAG_LIGHT_SAMPLING is not effective)
    WfPartLights part_lights{nullptr, nullptr, 0u, 0u};   // RWR_FLAG_LIGHT_PARTS: the mesh light (n = 0 while the flag is not effective: the forms without PARTS)
    int surf = kSurfNone;   // the surface models of the frame's flags (kSurfGlass: the table may hold glass records; kSurfGloss: glossy ones too)
    // The two rules for SURF.  The surface forms differ where a ray is emitted and nowhere else: the primary stage has one only
    // when the frame bounces at all, a trace kernel only in a generation that emits (a kernel that ends a path has none).
    int primary_surf(const FrameParams &fp) const { return fp.bounces != 0u ? surf : kSurfNone; }
    int trace_surf() const { return emits ? surf : kSurfNone; }
};
struct BvhNode4;
struct BvhDevice {
    const BvhNode4 *nodes;
    const uint32_t *leaf_faces;
    uint32_t n_nodes;
    uint32_t stack_depth;  // 3 * tree depth + 2
    float packet_extent;   // pools whose ray origins span less than this are traced as packets (kernels_wf_bounce.hip)
    uint32_t min_packet_pools;  // fewer packet pools than this in a launch group: the per-lane kernel traces them
    uint32_t lane_items;        // work items the per-lane kernel's launch should have when pools are few (pool_split; tunable)
    uint32_t packet_dense_rays; // a pool of at least this many rays is traced as packets however far apart its rays start (0: never)
    uint32_t wide_lane;         // the per-lane trace kernel may run as 1 024-thread workgroups sharing one LDS copy of the nodelets
    uint32_t no_stack16;        // the per-lane kernels keep 32-bit stack entries whatever the scene's size (RWR_WF_STACK16=0; host only: lane_lds_plan)
};
// What a stage of the last wavefront frame launched per lane, written by the launchers where they encode the form (rwr_last_traversal_plan):
// launches of the per-lane kernel by that stage, and the LaneLdsPlan (rwr_bvh.h) of the last of them — all zero while launches is.
struct LanePlanRecord { uint32_t launches = 0, nodes_in_lds = 0, stack16 = 0, wide = 0; };

// A frame slot's kept plane of ray directions (frame_records.cpp ray_plane_step): the normalised directions of the two-pixel frame
// kernel's pixel pairs, 24 bytes per lane of its grid — xy[i] = {x.x, x.y, y.x, y.y}, z[i] = {z.x, z.y} of the pair whose lane
// is thread i % 256 of workgroup i / 256 (workgroups in the order of their flattened index).  Every lane of the grid has an
// entry, on or off the frame, so neither the kernel that fills it nor the one that loads from it tests a bound.
struct RayPlane {
    float4 *xy;
    float2 *z;
};
constexpr uint32_t kRayPlaneMaxW = 3840, kRayPlaneMaxH = 2160;   // larger frames compute their rays every frame
// entries (lanes of the frame kernel's grid) of the plane of fp's launch
inline size_t ray_plane_entries(const FrameParams &fp) { return (size_t)((fp.width + 63u) / 64u) * band_strips(fp) * 256u; }
// kernels_ray_plane.hip: fills the plane for the launch of fp from the slot's ray tables (fp.ray_colp / ray_row, made for fp.cam)
hipError_t launch_ray_plane(hipStream_t s, const FrameParams &fp, const RayPlane &plane);
hipError_t preload_kernels_ray_plane();

struct FusedSetup;
// plane (may be null): the frame's ray directions are loaded from it instead of computed (the culled frame without normal
// maps, two launches per frame: anything else with a plane is hipErrorInvalidValue)
// lean (may be null): in, whether the lean resting form (k_primary_p2_lean) may be launched where the frame is one of its kind —
// a plane frame with RWR_FLAG_TILE_COVER, tile sets, one material, no extra outputs; out, whether it was
hipError_t launch_primary_p2(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const ShadeRec *shade,
                             const FrameTri *ftris, const QuadTex &tex, const Targets &tg, hipEvent_t ev_start = nullptr,
                             hipEvent_t ev_stop = nullptr, const FusedSetup *fused = nullptr, const RayPlane *plane = nullptr,
                             bool *lean = nullptr);
// grid rows the fused form puts in front of the frame's strips for `n_blocks` record-making workgroups
uint32_t primary_p2_fused_rows(const FrameParams &fp, uint32_t n_blocks);
// ft (WfFeatures): ft.shadows — the SHADOW forms, which read ft.shadow; ft.primary_surf(fp) — SURF, the forms that read ft.surfaces
hipError_t launch_wf_primary(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const ShadeRec *shade,
                             const FrameTri *ftris, const float4 *tex, const Targets &tg,
                             const WfBuffers &wf, uint32_t sample_begin, uint32_t sample_count, uint32_t z_split, const WfFeatures &ft);
// once per frame, ahead of the primary stage, when the frame is expected to show little: fills live_list / live_count / tile_live
hipError_t launch_wf_classify(hipStream_t s, const FrameParams &fp, const FrameTri *ftris, const Targets &tg, uint32_t tiles_x,
                              uint32_t *live_list, uint32_t *live_count, uint32_t *tile_live);
// One generation of rays: the sort, then the trace kernels in the forms of ft (WfFeatures) — ft.emits: a generation of a deeper
// path that is not its last, the EMIT forms write every hit's next ray back into its slot; else the kernels that end the path.
// ft.shadows: the SHADOW forms; ft.sky_on: the SKY forms, a ray that hits nothing adds the sky's term; ft.trace_surf(): SURF.
// plan (may be null): receives the per-lane launch and its LaneLdsPlan.
hipError_t launch_wf_bounce(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const ShadeRec *shade,
                            const BvhDevice &bvh, const float4 *tex, const WfBuffers &wf,
                            uint32_t n_tiles, uint32_t sample_count, uint32_t packet_min_rays, void *pool_info, uint32_t *pool_list,
                            const WfFeatures &ft, LanePlanRecord *plan = nullptr);
// RWR_FLAG_SHADOWS: traces the shadow records the kernels of one stage left in the queue (the primary stage's, or one generation's
// trace kernels') and adds the light's part of every term whose ray got through.  light_mesh / light_sphere: the unit directions
// towards the reference's two lights; expected_tiles: how many tiles are expected to hold records (sizes the work items only).
// soft (may be null: point lights, the hard forms): the lights' radii, RWR_FLAG_SOFT_SHADOWS — the SOFT forms, which key their disk
// draws by gen (0 behind the primary stage, k behind generation k) and sample_base (the launch group's first global sample).
// plan (may be null): as launch_wf_bounce's.
hipError_t launch_wf_shadow(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const BvhDevice &bvh, const WfBuffers &wf,
                            const WfShadow &shadow, uint32_t n_tiles, uint32_t expected_tiles, uint32_t sample_count, const float light_mesh[3],
                            const float light_sphere[3], uint32_t gen, uint32_t sample_base, const rwr_shadow_params *soft,
                            LanePlanRecord *plan = nullptr);
// kernels_wf_light.hip (RWR_FLAG_LIGHT_SAMPLING, RWR_FLAG_LIGHT_PARTS): the light samples of the hits whose diffuse rays generation
// `gen` emitted (0: the primary stage), from glow's records and ballots, added to wf's sums; the rays traced and reached into
// glow.light_counts.  parts.n != 0: the PARTS forms, which aim at the mesh light too.  sky.table != null (RWR_FLAG_LIGHT_SKY): the
// SKY forms, which aim at the sky's image too.
hipError_t launch_wf_light(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const BvhDevice &bvh, const WfBuffers &wf,
                           const WfGlow &glow, const WfLights &lights, const WfPartLights &parts, const WfSkyImage &sky, uint32_t n_tiles,
                           uint32_t expected_tiles, uint32_t sample_count, uint32_t gen, uint32_t sample_base);
size_t wf_pool_info_bytes();
// RWR_WF_STATS=1: trace launches of this process so far {packet kernel, per-lane kernel, its 1 024-thread form}
void wf_trace_launch_counts(uint64_t out[3]);
hipError_t launch_primary_bvh(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const ShadeRec *shade,
                              const BvhDevice &bvh, const float4 *tex, const Targets &tg);
// live_counters / host_live: the last launch group's counters (kernels_wf_bounce.hip) and the pinned words the host reads them from
hipError_t launch_wf_resolve(hipStream_t s, const FrameParams &fp, const Targets &tg, const WfBuffers &wf, const uint32_t *live_counters = nullptr,
                             uint32_t *host_live = nullptr);
// Progressive accumulation (RWR_FLAG_ACCUMULATE): the context's sums over every frame of the accumulation so far, 4 planes of
// W*H u64 in the 2^-26 units of WfBuffers::fix (global pixel index), and the first frame's sample-0 planes (aux: id and t too).
struct AccumBuffers {
    unsigned long long *hist;
    float *depth;
    int32_t *obj_id;
    float *hit_t;
};
// How a frame's resolve treats the history: the first frame of an accumulation stores its sums and copies its sample-0 planes
// out; a later frame adds its sums and copies the planes back in; a frame past the cap traced nothing and only shows the history.
enum class AccumMode { kFirst, kAdd, kShow };
// k_wf_resolve for an accumulating frame: the slot's sums (left zeroed) go into the history, colour = history / total_samples
hipError_t launch_wf_resolve_accum(hipStream_t s, const FrameParams &fp, const Targets &tg, const WfBuffers &wf, const AccumBuffers &ac,
                                   AccumMode mode, uint32_t total_samples, const uint32_t *live_counters = nullptr,
                                   uint32_t *host_live = nullptr);

// RWR_FLAG_DENOISE (kernels_wf_denoise.hip): the guide pre-pass and dp.iterations filter launches behind the frame's resolve.  tg holds
// the resolved frame with its aux planes; guide, plane_a and plane_b are width * height records each (the slot's scratch).
hipError_t launch_wf_denoise(hipStream_t s, uint32_t width, uint32_t height, const TriRecord *tris, const Targets &tg,
                             const rwr_denoise_params &dp, float4 *guide, float4 *plane_a, float4 *plane_b);

// RWR_FLAG_REPROJECT (kernels_wf_reproject.hip).  RpCamera: what the history keeps of a frame's camera (rwr_hip.h item 3), made on
// the host in the oracle's f32 operations (frame_request.cpp reproject_camera); nc0 = dot3(nrm, c0), nn = dot3(nrm, nrm).
struct RpCamera {
    float o[3], c0[3], cx[3], cy[3], nrm[3];
    float nc0, nn;
};
// One history set, width * height records each: {r, g, b, n}, {nhat.xyz of the face or zeros, t}, the object id
struct RpHistory {
    float4 *colour;
    float4 *guide;
    int32_t *id;
};
// The stage behind the frame's resolve: tg holds the resolved frame with its aux planes; prev = nullptr: frame 0 of a history
// (`from` is not read); counts: {reused, fresh, background}, zeroed by the caller.
hipError_t launch_wf_reproject(hipStream_t s, uint32_t width, uint32_t height, const TriRecord *tris, const Targets &tg,
                               const rwr_camera_inv_uniform &cam, const RpCamera *prev, const rwr_reproject_params &rp,
                               const RpHistory &from, const RpHistory &to, unsigned long long *counts);

// RWR_FLAG_TONEMAP (kernels_wf_tonemap.hip).  The frame slot's record: the measure's two sums, added atomically, and the exposure
// k_tm_exposure makes of them (rwr_tonemap.h tonemap_exposure).
struct TonemapRecord {
    long long log_sum;
    uint32_t count;
    float exposure;
};
static_assert(sizeof(TonemapRecord) == 16, "the slot's record is 16 bytes");
// The stage, behind everything else of the frame: tg holds the frame with its colour_f32 plane, whose rgba8 plane it rewrites.  rec
// is zeroed here, on the stream, and used with tp.auto_exposure alone (manual mode: one launch, E = tp.exposure).
hipError_t launch_wf_tonemap(hipStream_t s, uint32_t width, uint32_t height, const Targets &tg, const rwr_tonemap_params &tp, TonemapRecord *rec);

// per-frame records and tables (kernels_primary.hip): FrameTri + tnum per face, ray tables per column pair / row
struct FrameSetupOut {
    FrameTri *ftris;   // n_tris
    float *tnum;       // n_tris
    float4 *ray_colp;  // 2 * ray_pairs
    float4 *ray_row;   // ray_rows
    uint32_t ray_pairs, ray_rows;
    // words the frame wants zeroed before its first kernel (the wavefront integrator's per-tile ray counts and live-tile count):
    // done here instead of by memset commands of their own on the stream (4-5 us each on a frame of a few hundred)
    uint32_t *zero_a, *zero_b;
    uint32_t n_zero_a, n_zero_b;
    // the two-pixel frame kernel's per-tile face sets (FrameParams::tile_lists; null: none this frame), for the kernel's grid of
    // list_gx x list_gy workgroups at row_begin + by * row_pitch; list_blocks blocks of the launch make them
    uint32_t *tile_lists;
    uint32_t list_gx, list_gy, list_row_begin, list_row_pitch, list_blocks;
};
// What the blocks that make the face sets need on top for the tiles' class words (kTileFaces* above): where the words go (null:
// no sets this frame) and the frame kernel's own operands of the compares they record — FrameParams::mesh_px, n_spheres and
// sphere_rect.  An argument of k_frame_setup of its own, so that FusedSetup (which holds a FrameSetupOut) and with it the fused
// frame kernel's arguments stay what they were.
struct TileClassIn {
    uint32_t *classes;
    uint32_t *cover;   // the tiles' cover words (kTileCovered above), zeroed with every class word written
    int32_t mesh_px[4];
    uint32_t n_spheres, pad;
    float sphere_rect[RWR_MAX_SPHERES][4];
};
static_assert(sizeof(TileClassIn) == 8 + 8 + 16 + 8 + RWR_MAX_SPHERES * 16, "TileClassIn has no padding");
// The frame kernel's FUSED form (one launch per frame, kernels_primary_p2.hip): the grid's first rows are workgroups that make
// the frame's records and tables (the work of k_frame_setup), the others wait until all of them have finished.
struct FusedSetup {
    CullConsts cc;
    const CullRec *cull;
    FrameSetupOut out;
    uint32_t n_blocks;     // record-making workgroups: blocks of k_frame_setup's grid
    uint32_t nb_tris;      // ... of which make face records
    uint32_t extra_rows;   // grid rows in front of the frame's own strips: ceil(n_blocks / grid.x)
    uint32_t flag_base;    // flag[0] before this frame (it counts finished record blocks: + n_blocks per frame, modulo 2^32)
    uint32_t *flag;        // [0] finished record blocks, [1] != 0: a wait ran out (the frame is incomplete; rwr_synchronize says so)
};

// kernels_dormant.hip: frames with single-triangle passes or orthographic rays (brute force, one pixel per lane)
struct SingleTriangles {  // the single-triangle passes of a frame (kept out of FrameParams: only this kernel reads them)
    uint32_t n;
    uint32_t pad[3];
    rwr_triangle_buffer_data t[RWR_MAX_TRIANGLES];
};
hipError_t launch_primary_dormant(hipStream_t s, const FrameParams &fp, const SingleTriangles &st, const TriRecord *tris,
                                  const ShadeRec *shade, const float4 *tex, const Targets &tg);

// kernels_*.hip: resolve one kernel of each translation unit (HIP loads a code object on first use)
hipError_t preload_kernels();
hipError_t preload_kernels_primary();
hipError_t preload_kernels_primary_p2();
hipError_t preload_kernels_wavefront();
hipError_t preload_kernels_wf_primary();
hipError_t preload_kernels_wf_bounce();
hipError_t preload_kernels_wf_shadow();
hipError_t preload_kernels_wf_light();
hipError_t preload_kernels_dist();

// kernels_dist.hip: the interleaved partition's gather (layout: rwr_strips.h) — every rank packs its strips into one message,
// the root deals the received messages out into the frame; one launch each.  The _host forms move host memory the same way.
struct StripLayout;
hipError_t launch_strips_pack(hipStream_t s, const StripLayout &L, uint32_t rank, uint32_t row_bytes, const uint8_t *frame, uint8_t *message);
hipError_t launch_strips_deal(hipStream_t s, const StripLayout &L, uint32_t row_bytes, const uint8_t *recv, uint8_t *frame);
void strips_pack_host(const StripLayout &L, uint32_t rank, size_t row_bytes, const uint8_t *frame, uint8_t *message);
void strips_deal_host(const StripLayout &L, size_t row_bytes, const uint8_t *recv, uint8_t *frame);

// kernels_selftest.hip: out[0..3] += depth inputs compared, mismatches, normalize inputs compared, mismatches
hipError_t launch_selftest_exact_math(hipStream_t s, unsigned long long *d_out4, uint32_t normalize_count, uint32_t seed);
hipError_t launch_selftest_exact_div(hipStream_t s, unsigned long long *d_out4, uint32_t count, uint32_t seed);
// kernels_selftest.hip: d_out[i] = rng_sobol(d_in[i], d_in[n + i], d_in[2 n + i], d_in[3 n + i]) (RWR_FLAG_SOBOL's word)
hipError_t launch_selftest_sobol(hipStream_t s, const uint32_t *d_in, uint32_t n, uint32_t *d_out);
// kernels_selftest.hip: d_out[3 i ...] = sky_image_radiance(si, d_dirs[3 i ...]) (RWR_FLAG_SKY_IMAGE's S_img), count directions
hipError_t launch_selftest_sky_image(hipStream_t s, const WfSkyImage &si, const float *d_dirs, uint32_t count, float *d_out);
// d_out[8 i ...] = {w.x, w.y, w.z, texel column, texel row (as uint32 bits), P, g, -} of sky_light_draw and sky_light_g (RWR_FLAG_LIGHT_SKY)
// for the four uniforms d_u4[4 i ...], the normal nrm and L lights, count tuples
hipError_t launch_selftest_sky_light(hipStream_t s, const WfSkyImage &si, const float *d_u4, uint32_t count, const float nrm[3], uint32_t n_lights, float *d_out);

// kernels_selftest.hip: d_out[wave] = {shader cycles, 100 MHz ticks} around iters * 8 v_fma_f32 (mode 0) / v_pk_fma_f32 (mode 1)
hipError_t launch_clock_probe(hipStream_t s, ulonglong2 *d_out, uint32_t ticks_100mhz);
hipError_t launch_measure_valu(hipStream_t s, int mode, ulonglong2 *d_out, uint32_t n_workgroups, uint32_t iters);

hipError_t launch_frame_setup(hipStream_t s, const CullConsts &cc, const rwr_camera_inv_uniform &cam, uint32_t width,
                              uint32_t height, const CullRec *cull, const TriRecord *tris, uint32_t n_tris,
                              const FrameSetupOut &out, const TileClassIn &tc);
// count -> scan -> fill; *total_out (device) receives the entries the frame's lists need
hipError_t launch_bin_faces(hipStream_t s, const FrameTri *ftris, uint32_t n_tris, uint32_t row_begin, uint32_t *lists,
                            uint32_t *counts, uint32_t *offsets, uint32_t *total_out, uint32_t bins_x, uint32_t bins_y, uint32_t capacity,
                            const int32_t mesh_px[4], uint32_t *total_host);
hipError_t launch_primary(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const ShadeRec *shade,
                          const FrameTri *ftris, const float4 *tex, const Targets &tg);

}  // namespace rwr
