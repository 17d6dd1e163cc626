// The reference frame (one sample per pixel, no bounce) on the slot's stream.
#include <algorithm>
#include <cstring>

#include "rwr_frame.h"

namespace rwr {

namespace {

// A/B (RWR_FRAME_GRAPH=1): the plain reference frame — records + frame kernel, nothing else on the stream — as one graph launch
int launch_frame_graph(rwr_context *ctx, FrameSlot &sl, const FrameConsts &fc, const FrameSetupOut &so, const QuadTex &quad_tex, const Targets &tg)
{
    const FrameParams &fp = fc.fp;
    const hipStream_t stream = sl.stream;
    sl.records_key.clear();   // the graph's k_frame_setup writes the slot's records
    std::vector<unsigned char> key(sizeof(FrameParams) + sizeof(CullConsts));
    std::memcpy(key.data(), &fp, sizeof fp);
    std::memcpy(key.data() + sizeof fp, &fc.cc, sizeof fc.cc);
    if (!sl.frame_graph || key != sl.frame_graph_key) {
        hipGraph_t g = nullptr;
        RWR_HIP_CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        hipError_t e = launch_records(ctx, sl, fc, so, true);
        if (e == hipSuccess) e = launch_primary_p2(stream, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, sl.d_ftris.ptr, quad_tex, tg);
        const hipError_t e2 = hipStreamEndCapture(stream, &g);
        RWR_HIP_CHECK(e);
        RWR_HIP_CHECK(e2);
        bool updated = false;
        if (sl.frame_graph) {
            hipGraphNode_t bad = nullptr;
            hipGraphExecUpdateResult res;
            updated = hipGraphExecUpdate(sl.frame_graph, g, &bad, &res) == hipSuccess;
            if (!updated) { (void)hipGetLastError(); sl.frame_graph = OwnedGraphExec{}; }
        }
        if (!updated) {
            const hipError_t e3 = hipGraphInstantiate(&sl.frame_graph.h, g, nullptr, nullptr, 0);
            if (e3 != hipSuccess) { (void)hipGraphDestroy(g); RWR_HIP_CHECK(e3); }
        }
        (void)hipGraphDestroy(g);
        sl.frame_graph_key.swap(key);
    }
    RWR_HIP_CHECK(hipGraphLaunch(sl.frame_graph, stream));
    ctx->setup_launches++;
    return RWR_OK;
}

// The plain reference frame — records + frame kernel, nothing else — as ONE launch: the frame kernel's first workgroups
// make the records (kernels_primary_p2.hip, FUSED).
// Where it pays (A/B in one box, tools/fused_ab.py, profiles/r03_fused_ab.txt): SMALL frames with frames in flight, which
// are bound by the host's launches — one rank's share of a multi-GPU 1080p frame: 9.8 -> 6.9 us per frame (1/8), 10.4 -> 8.2
// (1/4), the host's enqueue time 9.8 -> 5.2 us.  A whole 1080p frame is VALU-bound and LOSES (15.0 -> 17.4 us with two slots:
// the next frame's waiting workgroups hold slots the running frame could use; 22.7 -> 23.8 us alone), so it keeps its two
// launches.  RWR_FUSED_SETUP=1 forces the fused form wherever it is possible (tests), 0 switches it off.
bool fused_pays(const rwr_context *ctx, const FrameParams &fp)
{
    const uint32_t render_groups = ((fp.width + 63u) / 64u) * ((fp.row_end - fp.row_begin + fp.row_pitch - 1u) / std::max(1u, fp.row_pitch));
    return ctx->fused_setup_force || (ctx->n_slots > 1u && render_groups <= 1200u);
}

int launch_fused_frame(rwr_context *ctx, FrameSlot &sl, const FrameConsts &fc, const FrameSetupOut &so, const QuadTex &quad_tex, const Targets &tg)
{
    const hipStream_t stream = sl.stream;
    sl.records_key.clear();   // the launch's record makers write the slot's records (and no tile lists)
    FusedSetup fs{};
    fs.cc = fc.cc;
    fs.cull = ctx->d_cull.ptr;
    fs.out = so;
    fs.nb_tris = (ctx->n_tris + 255u) / 256u;
    fs.n_blocks = fs.nb_tris + (so.ray_pairs + so.ray_rows + 255u) / 256u;
    fs.extra_rows = primary_p2_fused_rows(fc.fp, fs.n_blocks);
    if (!sl.d_fused.ptr || sl.fused_blocks != fs.n_blocks) {   // first use, or another scene / frame size: the count starts over
        RWR_HIP_CHECK(hipStreamSynchronize(stream));
        RWR_HIP_CHECK(sl.d_fused.ensure(2));
        RWR_HIP_CHECK(hipMemsetAsync(sl.d_fused.ptr, 0, 2 * sizeof(uint32_t), stream));
        sl.fused_count = 0;
        sl.fused_blocks = fs.n_blocks;
    }
    fs.flag = sl.d_fused.ptr;
    fs.flag_base = sl.fused_count;
    sl.fused_count += fs.n_blocks;   // (modulo 2^32, like the device's count)
    sl.fused_used = true;
    RWR_HIP_CHECK(launch_primary_p2(stream, fc.fp, ctx->d_tris.ptr, ctx->d_shade.ptr, sl.d_ftris.ptr, quad_tex, tg, nullptr, nullptr, &fs));
    return RWR_OK;
}

}  // namespace

// The reference frame (one sample per pixel, no bounce): records, bins, the chosen kernel — or, for the plain frame of a small
// scene, the graph or the fused launch in their place.
int enqueue_reference(rwr_context *ctx, FrameSlot &sl, const FrameRequest &rq, FrameKernel kernel, FrameConsts &fc, const Targets &tg,
                      FrameTiming &timing)
{
    FrameParams &fp = fc.fp;
    const hipStream_t stream = sl.stream;
    FrameSetupOut so{};
    int rc = frame_tables(ctx, sl, fp, so);
    if (rc != RWR_OK) return rc;
    const bool small_culled = small_culled_frame(ctx, rq, kernel), band = fp.row_end > fp.row_begin;
    // Unbinned scenes in the two-pixel frame kernel with culling: k_frame_setup's last blocks make every tile's face set
    // (rwr_frame_setup.h frame_tile_lists_block), one wave per region of 4x4 of the kernel's workgroups (recomputing the faces'
    // records per block is the blocks' fixed cost; one region per wave keeps the launch short: it delays this slot's frame kernel).
    // (The fused form ignores them: its record makers run in the frame kernel's own launch.)
    if (small_culled && ctx->tile_lists && ctx->n_tris <= kTileListMaxFaces && band) {
        so.list_gx = (fp.width + 63u) / 64u;
        so.list_gy = band_strips(fp);
        so.list_row_begin = fp.row_begin;
        so.list_row_pitch = fp.row_pitch;
        const uint32_t regions = ((so.list_gx + kListRegionWgs - 1u) / kListRegionWgs) * ((so.list_gy + kListRegionWgs - 1u) / kListRegionWgs);
        so.list_blocks = (regions + 4u * kListRegionsPerWave - 1u) / (4u * kListRegionsPerWave);
        RWR_HIP_CHECK(sl.d_tile_lists.ensure(tile_list_words(so.list_gx, so.list_gy)));   // (the sets, then the tiles' class words)
        so.tile_lists = sl.d_tile_lists.ptr;
        fp.tile_lists = so.tile_lists;
    }
    // the frame kernel takes a tile by its class word (RWR_TILE_CLASS=0: it looks at none; the setup writes them all the same)
    fp.flags &= ~(RWR_FLAG_TILE_CLASS | RWR_FLAG_TILE_COVER);
    if (so.tile_lists && ctx->tile_class) fp.flags |= RWR_FLAG_TILE_CLASS;
    ctx->last_classes = rwr_context::LastClasses{so.tile_lists ? ctx->cur : 0u, so.list_gx, so.tile_lists ? so.list_gy : 0u};
    ctx->last_cover_frames = 0;   // (set below, by the one form that looks at cover words)
    const QuadTex quad_tex{ctx->d_quads.empty() ? nullptr : ctx->d_quads[0].ptr, ctx->d_mat_quads.ptr, ctx->d_srgb_lut.ptr};
    const bool plain = small_culled && !rq.aux && !ctx->timing_every;   // nothing but records + frame kernel on the stream
    if (plain && ctx->frame_graph) return launch_frame_graph(ctx, sl, fc, so, quad_tex, tg);   // (an empty band too: captured as it is)
    if (plain && ctx->fused_setup && fused_pays(ctx, fp) && !(fp.flags & RWR_FLAG_NORMAL_MAP) && band) {
        ctx->last_classes = rwr_context::LastClasses{};   // (the fused form makes no sets)
        return launch_fused_frame(ctx, sl, fc, so, quad_tex, tg);
    }
    bool kept = false;
    if ((rc = enqueue_records(ctx, sl, kernel, fc, so, timing, &kept)) != RWR_OK) return rc;
    switch (kernel) {
    case FrameKernel::kDormant: {
        SingleTriangles st{};
        st.n = ctx->n_triangles;
        for (uint32_t i = 0; i < ctx->n_triangles; i++) st.t[i] = ctx->triangles[i];
        RWR_HIP_CHECK(launch_primary_dormant(stream, fp, st, ctx->d_tris.ptr, ctx->d_shade.ptr, tex0_of(ctx), tg));
        break;
    }
    case FrameKernel::kBvh: {
        const BvhDevice bvh_p{ctx->d_bvh_nodes.ptr, ctx->d_bvh_leaf_faces.ptr, ctx->bvh_n_nodes, 3u * ctx->bvh_depth + 2u, 0.0f, 0u, 0u, 0u, 0u, 0u};
        RWR_HIP_CHECK(launch_primary_bvh(stream, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, bvh_p, tex0_of(ctx), tg));
        break;
    }
    case FrameKernel::kOnePixel:
        RWR_HIP_CHECK(launch_primary(stream, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, sl.d_ftris.ptr, tex0_of(ctx), tg));
        break;
    default: {
        // (the forms with a loading twin: culled, no normal maps — launch_primary_p2's own rule for RWR_FLAG_NORMAL_MAP)
        RayPlane plane{};
        const bool can_load = !(fp.flags & RWR_FLAG_NO_CULL) && !((fp.flags & RWR_FLAG_NORMAL_MAP) && fp.tangents);
        const bool load = can_load && ray_plane_step(ctx, sl, fp, plane);
        // Cover words (rwr_internal.h kTileCovered): only a frame served from the slot's kept records looks at them — the first
        // such frame learns them with the straight path's own tests, the frames after it skip those tests on the tiles learnt —
        // so a frame that made its records (a moving camera, RWR_SETUP_CACHE=0) neither reads nor writes one.  RWR_TILE_COVER=0:
        // no frame does.
        // (can_load: no normal maps; one material — the frames whose one-face tiles take the straight path at all)
        if (kept && (fp.flags & RWR_FLAG_TILE_CLASS) && ctx->tile_cover && can_load && fp.n_materials <= 1u) {
            fp.flags |= RWR_FLAG_TILE_COVER;
            ctx->tile_cover_frames++;
            ctx->last_cover_frames = ++sl.cover_frames;
        }
        // (the lean resting form where the frame is one of its kind — launch_primary_p2's rule; RWR_LEAN_REST=0: never)
        bool lean = ctx->lean_rest;
        RWR_HIP_CHECK(launch_primary_p2(stream, fp, ctx->d_tris.ptr, ctx->d_shade.ptr, sl.d_ftris.ptr, quad_tex, tg,
                                        timing.dispatch ? ctx->timing_events[2 * ctx->timing_pairs].h : nullptr,
                                        timing.dispatch ? ctx->timing_events[2 * ctx->timing_pairs + 1].h : nullptr, nullptr,
                                        load ? &plane : nullptr, &lean));
        if (lean) ctx->lean_rest_frames++;
    }
    }
    return RWR_OK;
}

// A frame rendered by the fused frame kernel is complete unless one of its waves waited in vain for the records (the wait is
// bounded; it has never been seen to run out): slot `i` is idle when this is called.
int check_fused_frame(rwr_context *ctx, uint32_t i)
{
    FrameSlot &sl = ctx->slots[i];
    if (!sl.fused_used || !sl.d_fused.ptr) return RWR_OK;
    uint32_t timed_out = 0;
    RWR_HIP_CHECK(hipMemcpy(&timed_out, sl.d_fused.ptr + 1, sizeof timed_out, hipMemcpyDeviceToHost));
    if (timed_out) {
        sl.fused_blocks = 0;   // the count is no longer what the host expects: start over with the next frame
        return set_error(RWR_ERR_HIP, "a frame is incomplete: workgroups of the fused frame kernel waited in vain for the frame's records "
                         "(RWR_FUSED_SETUP=0 renders with two launches per frame)");
    }
    return RWR_OK;
}

}  // namespace rwr
