// Fused frame kernel, two pixels per lane (see rwr_device_p2.h for why): ONE launch replaces the
// reference's three clears, two sphere passes, two depth copies and the mesh pass
// (/root/reference/src/lib.rs:1024-1184).  Same results as kernels_primary.hip's k_primary, which stays
// as the one-pixel-per-lane form (RWR_FLAG_ONE_PIXEL_PER_LANE and the wavefront integrator's first stage).
//   wave64 = 32x4 pixel tile, lane l owns pixels (2*(l&15), l>>4) and (2*(l&15)+1, l>>4);
//   workgroup (4 waves, 2x2 tiles) = 64x8 pixels = one screen-bin column (kBinW).
//   The workgroup loads the per-frame culling records of k_frame_setup for its (bin's) face list once,
//   256 at a time, into LDS; each wave culls them for its own tile, 64 at a time, one per lane, and runs
//   the exact test on the survivors in ascending face order with the face record in scalar registers.
//   The diffuse texture is read as one quad record per pixel (rwr_internal.h QuadTex) decoded through an
//   LDS copy of the sRGB table: one vector-memory instruction per pixel instead of four.
#include <hip/hip_ext.h>

#include "rwr_frame_setup.h"
#include "rwr_p2_tile.h"   // RWR_P2_TILE_32x4: a wave's tile, 32x4 pixels (default) or 16x8
#include "rwr_primary.h"
#include "rwr_shade_p2.h"

namespace rwr {

#ifndef RWR_P2_OCC
#define RWR_P2_OCC 7  // 72 VGPRs: the shading step needs 66; at 8 waves (64) it spills and is slower (measured)
#endif
// NMAP: normal-mapped shading (extension, RWR_FLAG_NORMAL_MAP) — its own instantiation, so that the reference's frame keeps
// its registers.
// FUSED: ONE launch per frame (the reference submits a frame once, lib.rs:1226).  The grid's first rows are workgroups that
// make the frame's records and tables — the work of k_frame_setup, rwr_frame_setup.h — and count themselves off in
// FusedSetup::flag; every other workgroup waits for that count before it touches a record (workgroups are dispatched in
// order of their flattened index, so the record makers are running before a waiting one exists; the wait is BOUNDED all the
// same: a wave whose wait runs out flags the frame as incomplete and leaves, it never hangs).  Saves the host one of its two
// launches per frame and the device the boundary between them.
// PLANE: the camera rests (frame_records.cpp ray_plane_step) — the pairs' ray directions are loaded from the slot's kept plane
// (rwr_internal.h RayPlane, filled by k_ray_plane from the same function) instead of computed from the ray tables.  The form has
// no use for the tables, and the plane's two arrays arrive in the tables' arguments (ray_colp: RayPlane::xy, ray_row:
// RayPlane::z), so that the kernel's arguments, and with them the code of every other form, stay what they were.
// Tile classes (the forms that walk per-tile face sets: CULL, not FUSED; RWR_FLAG_TILE_CLASS): the setup leaves a class word
// with every tile's set (rwr_internal.h kTileFaces*), and a wave takes one of three ways through its tile by it — clear values
// for a tile nothing can show in, a straight path for exactly one face and no sphere, the whole kernel otherwise.  The ways
// meet again at the stores: one tail, so that the form's registers are those of the general path alone.
// COVER: a frame served from the slot's kept records (RWR_FLAG_TILE_COVER, render_reference.cpp) — the straight path reads and learns the
// tiles' cover words (rwr_internal.h kTileCovered).  An instantiation of its own, so that every other frame runs the code it ran.
// LISTS: the face sets, class words and cover words are there and looked at — a compile-time fact of the lean resting form
// (k_primary_p2_lean below), the frame of a resting camera: PLANE and COVER, no AUX, one material, RWR_FLAG_TILE_CLASS and
// RWR_FLAG_TILE_COVER set, p.tile_lists not null (launch_primary_p2 launches it for nothing else).  The form walks sets only, so it
// has no culling records in LDS, no bin lookup and no culling rounds; every wave copies the whole sRGB table (all four to the
// same 1 KB, the same values) and waits for its own copy, so no wave meets a workgroup barrier on any way through a tile.  The
// arithmetic is the other forms': the same functions in the same order.
// The kernels' statements are rwr_primary_p2_body.h, included by both entry points: each is a kernel with arguments of its own
// (a function called from both changed the code of every form: its pointer arguments lose what a kernel argument tells the
// compiler about aliasing).
template <bool AUX, bool CULL, bool NMAP, bool FUSED = false, bool PLANE = false, bool COVER = false>
__global__ void __launch_bounds__(256, (AUX || NMAP) ? 4 : RWR_P2_OCC)
// (the first eleven arguments repeat FrameParams fields: they are what a wave needs first, and the Makefile
// has their 14 dwords preloaded into SGPRs)
k_primary_p2(const FrameTri *__restrict__ ftris, const float4 *__restrict__ ray_colp, const float4 *__restrict__ ray_row,
             uint32_t n_tris, uint32_t row_begin, uint32_t bins_enabled, uint32_t row_pitch,
             int32_t mesh_x0, int32_t mesh_y0, int32_t mesh_x1, int32_t mesh_y1,
             const FrameParams p, const TriRecord *__restrict__ tris, const ShadeRec *__restrict__ shade,
             const QuadTex tex, const Targets tg, const FusedSetup fs)
{
    constexpr bool LISTS = false;
    const auto tl = [&]() { return p.tile_lists; };   // the tiles' sets, class words and cover words (read where the body asks)
    const float *const lut_src = tex.lut;
    // the tile arrays' strides and the numerators, read where the body asks (the grid from the dispatch packet's copy)
    const auto grid_x = [&]() { return gridDim.x; };
    const auto grid_tiles = [&]() { return gridDim.x * gridDim.y * 4u; };
    const auto tnum_ptr = [&]() { return p.tnum; };
#include "rwr_primary_p2_body.h"
}

// The lean resting form (LISTS above): an entry point of its own, so that its register budget is its own.  A CU admits eight
// workgroups of 256 threads only up to 80 scalar registers a wave (.sgpr_count; 82-96: seven — measured,
// profiles/r12_residency_census.txt).  The allocator knows that rule, but per declared wave count: k_primary_p2 declares
// RWR_P2_OCC = 7 waves per SIMD and is given 96, this form declares 8 and is held to 80 (amdgpu_num_sgpr(82) on top of it changes
// no instruction).  Its first fourteen argument dwords — the plane, the tiles' words, the table, the band, the numerators and the
// tile arrays' strides — are preloaded like k_primary_p2's.
// tnum (FrameParams::tnum), tiles_x, n_tiles (the launch's gridDim.x and gridDim.x * gridDim.y * 4, from launch_primary_p2): what a
// wave needs to ask for its tile's words arrives in registers, so that no load stands between the dispatch and that request
// (gridDim itself is a load from the hidden arguments, FrameParams::tnum one from the argument block).
__global__ void __launch_bounds__(256, 8)
k_primary_p2_lean(const float4 *__restrict__ ray_colp, const float4 *__restrict__ ray_row, const uint32_t *__restrict__ tile_lists,
                  const float *__restrict__ lut_src, uint32_t row_begin, uint32_t row_pitch,
                  const float *__restrict__ tnum, uint32_t tiles_x, uint32_t n_tiles,
                  const FrameParams p, const TriRecord *__restrict__ tris, const ShadeRec *__restrict__ shade,
                  const QuadTex tex, const Targets tg)
{
    constexpr bool AUX = false, CULL = true, NMAP = false, FUSED = false, PLANE = true, COVER = true, LISTS = true;
    // what the body names and this form never reads (k_primary_p2's other arguments)
    const FrameTri *ftris = nullptr;
    const uint32_t n_tris = 0u, bins_enabled = 0u;
    const int32_t mesh_x0 = 0, mesh_y0 = 0, mesh_x1 = 0, mesh_y1 = 0;
    const FusedSetup fs{};
    const auto tl = [&]() { return tile_lists; };
    const auto grid_x = [&]() { return tiles_x; };
    const auto grid_tiles = [&]() { return n_tiles; };
    const auto tnum_ptr = [&]() { return tnum; };
#include "rwr_primary_p2_body.h"
}

uint32_t primary_p2_fused_rows(const FrameParams &fp, uint32_t n_blocks)
{
    const uint32_t gx = (fp.width + 63u) / 64u;
    return gx ? (n_blocks + gx - 1u) / gx : 0u;
}

hipError_t launch_primary_p2(hipStream_t s, const FrameParams &fp, const TriRecord *tris, const ShadeRec *shade,
                             const FrameTri *ftris, const QuadTex &tex, const Targets &tg, hipEvent_t ev_start,
                             hipEvent_t ev_stop, const FusedSetup *fused, const RayPlane *plane, bool *lean)
{
    const bool lean_allowed = lean && *lean;
    if (lean) *lean = false;
    if (fp.row_end <= fp.row_begin || fp.width == 0) return hipSuccess;
    if (fp.row_pitch % kStripRows != 0u) return hipErrorInvalidValue;   // a workgroup's four tiles must share a screen bin
    if (!tex.lut) return hipErrorInvalidValue;
    const dim3 grid((fp.width + 63u) / 64u, band_strips(fp) + (fused ? fused->extra_rows : 0u));
    const dim3 block(256);
    const bool aux = (fp.flags & RWR_FLAG_AUX_OUTPUTS) != 0;
    const bool do_cull = (fp.flags & RWR_FLAG_NO_CULL) == 0;
    // ev_start / ev_stop (may be null): timestamps of this dispatch itself (hipExtLaunchKernelGGL), i.e. the
    // kernel's own duration as a profiler reports it, without the gap to the preceding kernel
    const bool nmap = (fp.flags & RWR_FLAG_NORMAL_MAP) != 0 && fp.tangents != nullptr;
    const FusedSetup fs = fused ? *fused : FusedSetup{};
#define RWR_P2_LAUNCH(A, C, N, F) hipExtLaunchKernelGGL((k_primary_p2<A, C, N, F>), grid, block, 0, s, ev_start, ev_stop, 0, ftris, fp.ray_colp, fp.ray_row, \
    fp.n_tris, fp.row_begin, fp.bins.enabled, fp.row_pitch, fp.mesh_px[0], fp.mesh_px[1], fp.mesh_px[2], fp.mesh_px[3], fp, tris, shade, tex, tg, fs)
    if (plane) {   // (a resting camera's frame: frame_records.cpp ray_plane_step)
        if (fused || nmap || !do_cull || !plane->xy || !plane->z) return hipErrorInvalidValue;
        const bool cover = (fp.flags & RWR_FLAG_TILE_COVER) != 0u;
        const float4 *const pxy = plane->xy, *const pz = reinterpret_cast<const float4 *>(plane->z);   // in the ray tables' arguments
#define RWR_P2_LAUNCH_PLANE(A, V) hipExtLaunchKernelGGL((k_primary_p2<A, true, false, false, true, V>), grid, block, 0, s, ev_start, ev_stop, 0, ftris, pxy, pz, \
    fp.n_tris, fp.row_begin, fp.bins.enabled, fp.row_pitch, fp.mesh_px[0], fp.mesh_px[1], fp.mesh_px[2], fp.mesh_px[3], fp, tris, shade, tex, tg, fs)
        // the lean resting form: everything it takes for granted holds (it reads the tiles' words without a null test)
        if (lean_allowed && cover && !aux && fp.tile_lists && (fp.flags & RWR_FLAG_TILE_CLASS) != 0u && fp.n_materials <= 1u) {
            hipExtLaunchKernelGGL(k_primary_p2_lean, grid, block, 0, s, ev_start, ev_stop, 0, pxy, pz, fp.tile_lists, tex.lut, fp.row_begin, fp.row_pitch,
                                  fp.tnum, grid.x, grid.x * grid.y * 4u, fp, tris, shade, tex, tg);
            *lean = true;
        } else if (aux && cover) RWR_P2_LAUNCH_PLANE(true, true);
        else if (aux) RWR_P2_LAUNCH_PLANE(true, false);
        else if (cover) RWR_P2_LAUNCH_PLANE(false, true);
        else RWR_P2_LAUNCH_PLANE(false, false);
#undef RWR_P2_LAUNCH_PLANE
    } else if (fused) {   // (the plain reference frame only: context.cpp)
        RWR_P2_LAUNCH(false, true, false, true);
    } else if (nmap) {
        if (aux && do_cull) RWR_P2_LAUNCH(true, true, true, false);
        else if (aux) RWR_P2_LAUNCH(true, false, true, false);
        else if (do_cull) RWR_P2_LAUNCH(false, true, true, false);
        else RWR_P2_LAUNCH(false, false, true, false);
    } else if ((fp.flags & RWR_FLAG_TILE_COVER) != 0u) {   // (a resting camera's frame without a plane: RWR_RAY_PLANE=0, a frame too large for one)
        if (!do_cull) return hipErrorInvalidValue;
#define RWR_P2_LAUNCH_COVER(A) hipExtLaunchKernelGGL((k_primary_p2<A, true, false, false, false, true>), grid, block, 0, s, ev_start, ev_stop, 0, ftris, fp.ray_colp, fp.ray_row, \
    fp.n_tris, fp.row_begin, fp.bins.enabled, fp.row_pitch, fp.mesh_px[0], fp.mesh_px[1], fp.mesh_px[2], fp.mesh_px[3], fp, tris, shade, tex, tg, fs)
        if (aux) RWR_P2_LAUNCH_COVER(true);
        else RWR_P2_LAUNCH_COVER(false);
#undef RWR_P2_LAUNCH_COVER
    } else {
        if (aux && do_cull) RWR_P2_LAUNCH(true, true, false, false);
        else if (aux) RWR_P2_LAUNCH(true, false, false, false);
        else if (do_cull) RWR_P2_LAUNCH(false, true, false, false);
        else RWR_P2_LAUNCH(false, false, false, false);
    }
#undef RWR_P2_LAUNCH
    return hipGetLastError();
}

hipError_t preload_kernels_primary_p2()
{
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>((&k_primary_p2<false, true, false>)));
}

}  // namespace rwr
