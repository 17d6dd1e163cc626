// What both frame kinds put ahead of their kernels: the per-frame records and tables, the kept plane of ray directions, the bins.
#include <algorithm>
#include <cstring>

#include "rwr_frame.h"

namespace rwr {

// Per-frame records and tables (k_frame_setup): they depend on the camera, the screen, the launch's rows and the scene, and
// on nothing else — not on the frame's number — so a slot keeps them while those stand still (launch_records below) and
// makes them again, on the render stream just ahead of the render kernel, when one of them changes.  (Running this small
// kernel on a side stream, double-buffered so that it overlaps the previous frame, was
// measured 4-10 us SLOWER per frame than the 3 us it hides: cross-stream event waits cost
// more than the kernel.)  Here: where they go.
int frame_tables(rwr_context *ctx, FrameSlot &sl, FrameParams &fp, FrameSetupOut &so)
{
    so.ray_pairs = ((ctx->screen.width + 63u) / 64u) * 32u;  // whole 64-pixel workgroup columns
    so.ray_rows = ctx->screen.height + 8u;                   // whole 8-row tiles below any band
    RWR_HIP_CHECK(sl.d_ray_colp.ensure(2u * (size_t)so.ray_pairs));
    RWR_HIP_CHECK(sl.d_ray_row.ensure(so.ray_rows));
    so.ftris = sl.d_ftris.ptr; so.tnum = sl.d_tnum.ptr;
    so.ray_colp = sl.d_ray_colp.ptr; so.ray_row = sl.d_ray_row.ptr;
    fp.ray_colp = so.ray_colp; fp.ray_row = so.ray_row; fp.tnum = so.tnum;
    return RWR_OK;
}

namespace {

// Everything k_frame_setup reads, and everything that decides where and what it writes: two launches with equal keys write the
// same bytes to the same addresses.  Field by field (no padding bytes); the buffers' addresses are part of it, so a buffer that
// moved between two frames is a different key.
struct RecordsKey {
    rwr_camera_inv_uniform cam;
    CullConsts cc;
    uint64_t scene_generation;
    const void *cull, *tris, *ftris, *tnum, *ray_colp, *ray_row, *zero_a, *zero_b, *tile_lists;
    uint32_t width, height, n_tris, ray_pairs, ray_rows, n_zero_a, n_zero_b, list_gx, list_gy, list_row_begin, list_row_pitch, list_blocks;
    uint32_t row_begin, row_end, row_pitch, pad;   // the launch's rows, with or without face sets: a change of rows is a change of key
    TileClassIn tc;   // the tiles' class words: where they go, and the mesh rectangle, sphere count and sphere rectangles they record
};
static_assert(sizeof(RecordsKey) == sizeof(rwr_camera_inv_uniform) + sizeof(CullConsts) + 8 + 9 * sizeof(void *) + 16 * 4 + sizeof(TileClassIn),
              "RecordsKey has no padding");
static_assert(sizeof(FrameSetupOut) == 96, "a new member of FrameSetupOut belongs in RecordsKey");
static_assert(sizeof(TileClassIn) == 168, "a new member of TileClassIn is a new input of k_frame_setup: RecordsKey holds the whole struct");

// What a slot's plane of ray directions (rwr_internal.h RayPlane) is a function of, and where it lies: the camera uniform, the
// screen, the launch's rows (they place the grid's workgroups) and the addresses of the two ray tables it is made from and of
// the plane itself.  No scene generation and no culling constants: the directions survive other spheres, instances or meshes.
// Field by field (no padding bytes).
struct RayPlaneKey {
    rwr_camera_inv_uniform cam;
    const void *ray_colp, *ray_row, *plane;
    uint32_t width, height, row_begin, row_end, row_pitch, pad;
};
static_assert(sizeof(RayPlaneKey) == sizeof(rwr_camera_inv_uniform) + 3 * sizeof(void *) + 6 * 4, "RayPlaneKey has no padding");

// The class words' inputs for a launch whose sets go to so.tile_lists (rwr_internal.h: the words lie behind the sets); all zero
// for a launch without sets.
TileClassIn tile_class_in(const FrameParams &fp, const FrameSetupOut &so)
{
    TileClassIn tc{};
    if (!so.tile_lists) return tc;
    tc.classes = so.tile_lists + (size_t)so.list_gx * so.list_gy * 4u * kTileListWords;
    tc.cover = tc.classes + (size_t)so.list_gx * so.list_gy * 4u;
    for (int k = 0; k < 4; k++) tc.mesh_px[k] = fp.mesh_px[k];
    tc.n_spheres = fp.n_spheres;
    std::memcpy(tc.sphere_rect, fp.sphere_rect, sizeof tc.sphere_rect);
    return tc;
}

}  // namespace

// Every k_frame_setup goes through here.  The slot's records are a pure function of the launch's key, so a launch whose key is
// the one the slot's records were made from is not made: camera, screen, rows and scene stand still on most frames of a redraw
// loop (and on all of a progressive accumulation).  Not pure are the words the wavefront integrator wants zeroed (zero_a /
// zero_b: its kernels count in them, every frame from zero), so a launch that carries such words is always made; the records
// it leaves are those of its key all the same.  `captured`: the launch is being recorded into a graph whose replays rewrite the
// records whenever they run — made, not counted (launch_frame_graph counts replays), and it leaves no key.
// This is the only place that leaves a key behind; whatever else writes the slot's records clears it (launch_frame_graph,
// launch_fused_frame, and ensure_frame_buffers when a buffer moves outside a frame).
// *kept (may be null): the launch was not made, the slot's records — and the tiles' class and cover words among them — are the
// ones an earlier launch with this key left.
hipError_t launch_records(rwr_context *ctx, FrameSlot &sl, const FrameConsts &fc, const FrameSetupOut &so, bool captured, bool *kept)
{
    if (kept) *kept = false;
    const FrameParams &fp = fc.fp;
    const RecordsKey key{fp.cam, fc.cc, ctx->scene_generation, ctx->d_cull.ptr, ctx->d_tris.ptr, so.ftris, so.tnum, so.ray_colp, so.ray_row,
                         so.zero_a, so.zero_b, so.tile_lists, fp.width, fp.height, ctx->n_tris, so.ray_pairs, so.ray_rows, so.n_zero_a,
                         so.n_zero_b, so.list_gx, so.list_gy, so.list_row_begin, so.list_row_pitch, so.list_blocks,
                         fp.row_begin, fp.row_end, fp.row_pitch, 0u, tile_class_in(fp, so)};
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(&key);
    const bool pure = so.n_zero_a == 0u && so.n_zero_b == 0u;
    if (!captured && pure && sl.records_key.size() == sizeof key && std::memcmp(sl.records_key.data(), bytes, sizeof key) == 0) {
        if (kept) *kept = true;
        return hipSuccess;
    }
    sl.records_key.clear();
    sl.cover_frames = 0;   // (the launch zeroes the cover words it reaches: what the frames since the last one learnt is forgotten)
    const hipError_t e = launch_frame_setup(sl.stream, fc.cc, fp.cam, fp.width, fp.height, ctx->d_cull.ptr, ctx->d_tris.ptr, ctx->n_tris, so, key.tc);
    if (e != hipSuccess || captured) return e;
    ctx->setup_launches++;
    if (ctx->setup_cache) sl.records_key.assign(bytes, bytes + sizeof key);   // (RWR_SETUP_CACHE=0: never a key, never a hit)
    return hipSuccess;
}

// The two-pixel frame kernel's rays for a camera at rest.  A fifth of the kernel's instructions turn the ray tables into the
// normalised directions of its pixel pairs, the same ones every frame while camera, screen and rows stand still — in a redraw
// loop that is most frames, the camera moves only while a key is held.  Per slot, for a frame with key K behind launch_records
// on the slot's stream:
//   the slot's plane was built for K:        the frame kernel loads its directions from it            (returns true)
//   else the slot's frame before had key K:  k_ray_plane fills the plane once, then the same          (returns true)
//   else:                                    K is remembered and the frame computes its rays, as ever (returns false)
// so a moving camera never pays for a plane it would not use, and a camera that comes to rest computes one more frame per
// slot, builds on the next and loads from then on.  Frames that cannot use a plane (another kernel or form, RWR_RAY_PLANE=0, a
// frame beyond kRayPlaneMaxW x kRayPlaneMaxH) pass the slot's key and plane by.  A plane that cannot be allocated is no
// error: the frame computes its rays.  The key is cleared by whatever moves the tables outside a frame (ensure_frame_buffers)
// and by rwr_resize.
bool ray_plane_step(rwr_context *ctx, FrameSlot &sl, const FrameParams &fp, RayPlane &plane)
{
    if (!ctx->ray_plane || fp.width > kRayPlaneMaxW || fp.height > kRayPlaneMaxH || fp.row_end <= fp.row_begin) return false;
    const size_t n = ray_plane_entries(fp);
    auto key_of = [&]() {
        const RayPlaneKey k{fp.cam, fp.ray_colp, fp.ray_row, sl.d_ray_plane.ptr, fp.width, fp.height, fp.row_begin, fp.row_end, fp.row_pitch, 0u};
        const unsigned char *b = reinterpret_cast<const unsigned char *>(&k);
        return std::vector<unsigned char>(b, b + sizeof k);
    };
    std::vector<unsigned char> key = key_of();
    if (key != sl.ray_plane_key) {
        sl.ray_plane_key.swap(key);
        sl.ray_plane_built = false;
        return false;
    }
    if (!sl.ray_plane_built) {
        if (sl.d_ray_plane.count < 3u * n) {   // (a larger plane than the slot has held: the old one goes, and with it the key's address)
            if (sl.d_ray_plane.ensure(3u * n) != hipSuccess) {
                (void)hipGetLastError();
                sl.forget_ray_plane();
                return false;
            }
            sl.ray_plane_key = key_of();
        }
        plane = RayPlane{reinterpret_cast<float4 *>(sl.d_ray_plane.ptr), sl.d_ray_plane.ptr + 2u * n};
        if (launch_ray_plane(sl.stream, fp, plane) != hipSuccess) {
            (void)hipGetLastError();
            sl.forget_ray_plane();
            return false;
        }
        sl.ray_plane_built = true;
        ctx->ray_plane_builds++;
    }
    plane = RayPlane{reinterpret_cast<float4 *>(sl.d_ray_plane.ptr), sl.d_ray_plane.ptr + 2u * n};
    ctx->ray_plane_frames++;
    return true;
}

// k_frame_setup, the screen bins of a large scene, and the start of the frame's timing pair.
int enqueue_records(rwr_context *ctx, FrameSlot &sl, FrameKernel kernel, FrameConsts &fc, const FrameSetupOut &so, FrameTiming &timing,
                    bool *kept)
{
    FrameParams &fp = fc.fp;
    const hipStream_t stream = sl.stream;
    RWR_HIP_CHECK(launch_records(ctx, sl, fc, so, false, kept));
    if (ctx->n_tris > ctx->bin_min_faces && !(fp.flags & RWR_FLAG_NO_CULL)) {
        // more faces than one 256-wide batch: bin them per 64x32-pixel screen region, once per frame.  The lists
        // are sized by a count pass on the device; the buffer keeps what the previous frames needed (read back a
        // frame late through pinned memory, never waited for) with headroom, and a frame whose lists do not fit
        // walks the whole scene instead — the same pixels — while the buffer grows for the next one.
        const uint32_t bins_x = (fp.width + kBinW - 1) / kBinW, bins_y = (fp.row_end - fp.row_begin + kBinH - 1) / kBinH;
        const size_t n_bins = (size_t)bins_x * bins_y;
        if (!sl.h_bin_total) {
            RWR_HIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&sl.h_bin_total.h), sizeof(uint32_t), hipHostMallocCoherent | hipHostMallocMapped));   // fine-grained: kernels store to it, the host reads it without a synchronisation
            *sl.h_bin_total = 0u;
        }
        const uint64_t needed = *sl.h_bin_total;
        uint64_t capacity = std::max<uint64_t>(sl.d_bin_lists.count, std::max<uint64_t>(ctx->bin_min_capacity, ctx->bin_min_capacity >= 65536u ? 8ull * ctx->n_tris : 0ull));
        if (needed > capacity || needed + needed / 4u > capacity) capacity = std::max<uint64_t>(capacity, needed + needed / 2u);
        capacity = std::min<uint64_t>(capacity, 0xfffffff0ull);
        if (capacity > sl.d_bin_lists.count) RWR_HIP_CHECK(hipStreamSynchronize(stream));   // the old buffer may still be read
        RWR_HIP_CHECK(sl.d_bin_lists.ensure((size_t)capacity));
        RWR_HIP_CHECK(sl.d_bin_counts.ensure(5u * (size_t)n_bins));   // four wave counts per bin, then the bins' own counts (launch_bin_faces)
        RWR_HIP_CHECK(sl.d_bin_offsets.ensure(n_bins));
        RWR_HIP_CHECK(sl.d_bin_total.ensure(1));
        RWR_HIP_CHECK(launch_bin_faces(stream, sl.d_ftris.ptr, ctx->n_tris, fp.row_begin, sl.d_bin_lists.ptr, sl.d_bin_counts.ptr,
                                       sl.d_bin_offsets.ptr, sl.d_bin_total.ptr, bins_x, bins_y, (uint32_t)sl.d_bin_lists.count, fp.mesh_px,
                                       sl.h_bin_total));   // (the scan writes the total to the pinned word itself: no copy command)
        fp.bins = BinGrid{sl.d_bin_lists.ptr, sl.d_bin_counts.ptr + 4u * (size_t)n_bins, sl.d_bin_offsets.ptr, bins_x, bins_y, (uint32_t)sl.d_bin_lists.count, 1u};
    }
    timing.on = ctx->timing_every && (ctx->timing_calls++ % ctx->timing_every == 0) && ctx->timing_pairs < 256;
    timing.dispatch = timing.on && kernel == FrameKernel::kTwoPixel;
    if (timing.on) {
        while (ctx->timing_events.size() < 2u * (ctx->timing_pairs + 1u)) {
            ctx->timing_events.emplace_back();
            RWR_HIP_CHECK(hipEventCreate(&ctx->timing_events.back().h));
        }
        if (!timing.dispatch) RWR_HIP_CHECK(hipEventRecord(ctx->timing_events[2 * ctx->timing_pairs], stream));
    }
    return RWR_OK;
}

}  // namespace rwr
