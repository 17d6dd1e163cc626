// The statements of the two-pixel frame kernel (kernels_primary_p2.hip), included into the body of each of its entry points,
// k_primary_p2<...> and k_primary_p2_lean: no include guard, nothing at file scope.  It names the entry point's arguments
// (k_primary_p2's list), the form's compile-time facts AUX, CULL, NMAP, FUSED, PLANE, COVER, LISTS, and two pointers the entry point
// makes: tl() (the tiles' sets, class words and cover words: FrameParams::tile_lists) and lut_src (QuadTex::lut); and three facts of the
// launch it reads through the entry point: grid_x() and grid_tiles() (workgroups per row of the grid, tiles of the grid: the strides
// of the tile arrays) and tnum_ptr() (FrameParams::tnum).
    static_assert(!LISTS || (PLANE && COVER && !AUX), "the lean form is the resting frame's: rays from the plane, cover words, no extra outputs");
    static_assert(!PLANE || (CULL && !NMAP && !FUSED), "the loading form exists for the culled two-launch frame without normal maps");
    static_assert(!COVER || (CULL && !NMAP && !FUSED), "cover words lie beside the face sets of the culled two-launch frame; normal maps take the general path");
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t by = blockIdx.y;
    const_ptr<TriRecord> tris_c = nullptr;
    const_ptr<ShadeRec> shade_c = nullptr;
    const_ptr<float> tnum_c = nullptr;
    if (FUSED) {
        if (blockIdx.y < fs.extra_rows) {   // a record-making workgroup (or a spare one of the last extra row)
            const uint32_t f = blockIdx.y * gridDim.x + blockIdx.x;
            if (f < fs.n_blocks) {
                frame_setup_block(f, fs.n_blocks, fs.cc, p.cam, p.width, p.height, fs.cull, tris, n_tris, fs.nb_tris, fs.out);
                __threadfence();      // the records are visible to the device ...
                __syncthreads();
                if (threadIdx.x == 0u) atomicAdd(fs.flag, 1u);   // ... before the block counts itself off
            }
            return;
        }
        by -= fs.extra_rows;
        // One wave per workgroup watches the count (thousands of waves polling one word swamp its L2 channel: measured, a
        // frame took 125 us), the others wait for it at a barrier.
        __shared__ uint32_t s_ready;
        if (wave == 0u) {
            uint32_t spins = 0;
            bool ok = true;
            while (__hip_atomic_load(fs.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - fs.flag_base < fs.n_blocks) {   // (wave-uniform)
                __builtin_amdgcn_s_sleep(16);
                if (++spins > (1u << 15)) { ok = false; break; }   // ~15 ms: never in practice — and never a hang
            }
            if (lane == 0u) {
                s_ready = ok ? 1u : 0u;
                if (!ok) atomicOr(fs.flag + 1, 1u);
            }
        }
        __syncthreads();
        if (s_ready == 0u) return;   // the frame is flagged incomplete (rwr_synchronize / rwr_readback report it)
        // No cache invalidation here on purpose: the kernel's launch invalidated this CU's caches, and no wave reads a line of
        // the records before this point (they are allocations of their own), so no stale line can be resident; what is needed
        // is that the loads below are ISSUED after the count was seen, which the pointers re-made here guarantee.
        // everything the record makers wrote is read through pointers made HERE, behind the wait
        asm volatile("" : "+s"(ftris), "+s"(ray_colp), "+s"(ray_row));
        const float *tn = p.tnum;
        asm volatile("" : "+s"(tn));
        tnum_c = to_const_space(tn);
        tris_c = to_const_space(tris);
        shade_c = to_const_space(shade);
    }
    const uint32_t blk_x0 = blockIdx.x * 64u;
#if RWR_P2_TILE_32x4
    const uint32_t tile_x0 = blk_x0 + (wave & 1u) * 32u;
    const uint32_t tile_y0 = row_begin + by * row_pitch + (wave >> 1) * 4u;
    const uint32_t px0 = tile_x0 + 2u * (lane & 15u), py = tile_y0 + (lane >> 4);
    constexpr float kTileWf = 32.0f, kTileHf = 4.0f;
#else
    const uint32_t tile_x0 = blk_x0 + wave * 16u;
    const uint32_t tile_y0 = p.row_begin + by * row_pitch;
    const uint32_t px0 = tile_x0 + 2u * (lane & 7u), py = tile_y0 + (lane >> 3);
    constexpr float kTileWf = 16.0f, kTileHf = 8.0f;
#endif

    // -- candidate faces of the workgroup: its bin's list (binned scenes) or the whole scene.  The four tiles lie in one
    // bin (a workgroup's 8 rows start on a multiple of 8 rows from row_begin: launch_primary_p2 checks row_pitch), so
    // the list is the same for all four waves, and its culling records are loaded once per workgroup: wave w
    // requests entries [64 w, 64 w + 64) of each round of 256 before anything else, so that their latency hides
    // behind the ray generation, and puts them in LDS, where every wave reads the ones it culls against ------------
    const uint32_t wu = __builtin_amdgcn_readfirstlane(wave);
    uint32_t n_list = n_tris;
    const uint32_t *__restrict__ src = nullptr;
    bool live = true;   // (wave-uniform) this wave's tile overlaps the screen rectangle of the whole mesh
    if (CULL && !LISTS) {
        if (bins_enabled) {
            const uint32_t bin = ((by * row_pitch) / kBinH) * p.bins.bins_x + blk_x0 / kBinW;
            const uint32_t off = p.bins.offsets[bin];
            if (off != kBinNoList) {   // (kBinNoList: this frame's lists did not fit; walk the whole scene)
                n_list = p.bins.counts[bin];
                src = p.bins.lists + off;
            }
        }
        // scalar integer compares against the mesh rectangle: the wave's tile, and the workgroup's (no wave has work
        // when the workgroup's rectangle is outside, and then no record is loaded)
        const int32_t bx0 = (int32_t)blk_x0, by0 = (int32_t)(row_begin + by * row_pitch);
#if RWR_P2_TILE_32x4
        const int32_t sx0 = bx0 + (int32_t)(wu & 1u) * 32, sy0 = by0 + (int32_t)(wu >> 1) * 4;
        const int32_t sx1 = sx0 + 32, sy1 = sy0 + 4;
#else
        const int32_t sx0 = bx0 + (int32_t)wu * 16, sy0 = by0;
        const int32_t sx1 = sx0 + 16, sy1 = sy0 + 8;
#endif
        if (sx1 < mesh_x0 || sx0 > mesh_x1 || sy1 < mesh_y0 || sy0 > mesh_y1) live = false;
        if (bx0 + 64 < mesh_x0 || bx0 > mesh_x1 || by0 + 8 < mesh_y0 || by0 > mesh_y1) n_list = 0u;
    }
    n_list = __builtin_amdgcn_readfirstlane(n_list);
    // Unbinned scenes of at most kTileListMaxFaces faces come with this frame's per-tile face sets (k_frame_setup,
    // rwr_frame_setup.h): the wave loads its tile's set with scalar loads now, behind the ray generation, and walks it instead
    // of culling the records itself (no record copy to LDS, no culling batch).
    // (LISTS: the set is requested on the one way through a tile that walks it, so that its eight scalar registers are not held
    // across the others)
    const bool lists = LISTS || (CULL && !FUSED && tl() != nullptr);   // (uniform)
    uint32_t set[kTileListWords] = {};
    if (lists) {
        if constexpr (!LISTS) {
            const const_ptr<uint32_t> rec = to_const_space(tl()) + ((by * grid_x() + blockIdx.x) * 4u + wu) * kTileListWords;
#pragma unroll
            for (uint32_t k = 0; k < kTileListWords; k++) set[k] = rec[k];
        }
        n_list = 0u;
    }
    // ... and, requested with it, the tile's class word (rwr_internal.h kTileFaces*; a parallel array behind the grid's sets): what
    // the compares below and the set's population would tell, found out by the setup.  RWR_TILE_CLASS=0: never looked at.
    const bool classed = LISTS || (lists && (p.flags & RWR_FLAG_TILE_CLASS) != 0u);   // (uniform)
    uint32_t cls = 0u;
    if (classed) cls = to_const_space(tl())[grid_tiles() * kTileListWords + (by * grid_x() + blockIdx.x) * 4u + wu];
    // (LISTS: the tile's cover word leaves with the class word — its address needs the same indices and nothing of the class — so
    // that the straight path below finds it there instead of asking for it a round trip later.  A tile of another class has read a
    // word it does not use; the array holds one for every tile of the grid.)
    auto cover_at = [&](uint32_t w) { return grid_tiles() * (kTileListWords + 1u) + (by * grid_x() + blockIdx.x) * 4u + w; };
    uint32_t cov_entry = 0u;
    if constexpr (LISTS) cov_entry = to_const_space(tl())[cover_at(wu)];
    // (LISTS: the setup made `live`'s compares and put their outcome in the word — a tile outside the mesh's rectangle has class
    // "no face", rwr_frame_setup.h frame_tile_lists_block — and a tile with a face in its class lies inside)
    if constexpr (LISTS) live = (cls & kTileFacesMask) != kTileFacesNone;
    constexpr bool kRounds = CULL && !LISTS;   // the form may cull rounds of records itself
    __shared__ float4 s_rec[kRounds ? 4 : 1][kRounds ? 256 : 1];   // round's culling records, one plane per 16 B of FrameTri
    __shared__ uint32_t s_face[kRounds ? 256 : 1];                 // ... and their face indices
    __shared__ float s_lut[256];                                   // sRGB decode table of the quad texels (rwr_internal.h QuadTex)
    // The records and the table go from memory to LDS without passing through registers (LDS DMA: lane l of wave w
    // writes 16 / 4 bytes at M0 + 16 l / 4 l); rwait() waits for them before the barrier that publishes them.
    const uint32_t slot = 64u * wu + lane;
    auto load_round = [&](uint32_t base) {   // wave w: entries [base + 64 w, base + 64 w + 64) of the list
        const uint32_t e = base + slot;
        if (e < n_list) {
            const uint32_t f = src ? src[e] : e;
            s_face[slot] = f;
            const char *r = reinterpret_cast<const char *>(ftris + f);
#pragma unroll
            for (int k = 0; k < 4; k++)
                __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)(r + 16 * k),
                                                 (__attribute__((address_space(3))) void *)&s_rec[k][64u * wu], 16, 0, 0);
        }
    };
    auto rwait = []() { __builtin_amdgcn_s_waitcnt(0xF70); };   // vmcnt(0)
    if (kRounds && !lists) load_round(0u);
    if constexpr (LISTS) {
        // Every wave copies the WHOLE table, all four to the same 1 KB: one DMA of 16 B per lane (four of 4 B for a table that is
        // not 16-byte aligned).  The wave's vmcnt(0) orders its reads behind its own DMA, after which every word holds its value;
        // what another wave's DMA writes there later is the same value again, so no barrier is needed and no read can see
        // anything else.  (A copy per wave at s_lut[256 w] was measured first: its base is not a constant, and the 24 table
        // reads of a lane's two pixels cost 18 more VALU instructions per wave, 265 -> 283, profiles/r12_pmc_cfg2.txt.)
        if ((reinterpret_cast<uintptr_t>(lut_src) & 15u) == 0u) {   // (uniform)
            __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)(lut_src + 4u * lane),
                                             (__attribute__((address_space(3))) void *)&s_lut[0], 16, 0, 0);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
                __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)(lut_src + 64u * k + lane),
                                                 (__attribute__((address_space(3))) void *)&s_lut[64u * k], 4, 0, 0);
        }
    } else {
        __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)(lut_src + threadIdx.x),
                                         (__attribute__((address_space(3))) void *)&s_lut[64u * wu], 4, 0, 0);
    }
    // the table's wait, and the barrier that publishes it (LISTS: the wave's own DMA covers the table, no barrier)
    auto lut_ready = [&]() {
        rwait();
        if constexpr (LISTS) asm volatile("" ::: "memory");   // (the table's reads stay behind the wait)
        else __syncthreads();
    };

    const f3 O = ld3(p.cam.origin);
    v3 D;
    if constexpr (PLANE) {   // requested where the table loads are: ahead of the LDS table's wait, behind the same work
        const uint32_t i = (by * grid_x() + blockIdx.x) * 256u + threadIdx.x;   // this lane's entry (k_ray_plane's index)
        const float4 dxy = ray_colp[i];
        const float2 dz = reinterpret_cast<const float2 *>(ray_row)[i];
        D = v3{f2{dxy.x, dxy.y}, f2{dxy.z, dxy.w}, f2{dz.x, dz.y}};
    } else {
        D = pixel_pair_ray_dir_tab(p.cam, ray_colp, ray_row, px0, py);
    }

    // where the pair's results go, and the stores (every way through a tile ends in them)
    struct PairSlot { bool in_frame, both, pair_store; uint32_t o; };
    auto pair_slot = [&](uint32_t px0, uint32_t py) {
        PairSlot ps;
        ps.in_frame = py < p.row_end && px0 < p.width;
        ps.o = py * p.width + px0;  // < 2^30 pixels (rwr_resize)
        ps.both = px0 + 1u < p.width;
        ps.pair_store = ps.both && (ps.o & 1u) == 0u;
        return ps;
    };
    // depth plane first (nothing behind it needs it): 8-byte aligned pair whenever the width is even
    auto store_depth = [&](const PairSlot &ps, f2 depth_tex) {
        if (ps.in_frame) {
            if (ps.pair_store) {
                // streaming stores: the targets are written once and never read here; they must not push the
                // texture and the face records out of the L2 (3.7 % of the frame rate)
                __builtin_nontemporal_store(depth_tex, reinterpret_cast<f2 *>(tg.depth + ps.o));
            } else {
                tg.depth[ps.o] = depth_tex.x;
                if (ps.both) tg.depth[ps.o + 1] = depth_tex.y;
            }
        }
    };
    auto store_colour = [&](const PairSlot &ps, const uint32_t (&rgba)[2], const float4 (&cf)[2], i2 obj, f2 win_t, uint32_t dbg_listed,
                            uint32_t dbg_tested) {
        if (ps.in_frame) {
            const uint32_t o = ps.o;
            if (ps.pair_store) {
                __builtin_nontemporal_store(u2{rgba[0], rgba[1]}, reinterpret_cast<u2 *>(reinterpret_cast<uint32_t *>(tg.color) + o));
            } else {
                reinterpret_cast<uint32_t *>(tg.color)[o] = rgba[0];
                if (ps.both) reinterpret_cast<uint32_t *>(tg.color)[o + 1] = rgba[1];
            }
            if (AUX) {
                const bool dbg = (p.flags & RWR_FLAG_DEBUG_COUNTS) != 0;
                reinterpret_cast<float4 *>(tg.color_f32)[o] = cf[0];
                tg.obj_id[o] = dbg ? (int32_t)dbg_listed : obj.x;
                tg.hit_t[o] = dbg ? (float)dbg_tested : win_t.x;
                if (ps.both) {
                    reinterpret_cast<float4 *>(tg.color_f32)[o + 1] = cf[1];
                    tg.obj_id[o + 1] = dbg ? (int32_t)dbg_listed : obj.y;
                    tg.hit_t[o + 1] = dbg ? (float)dbg_tested : win_t.y;
                }
            }
        }
    };
    // the mesh winners' colours as rgba8unorm (rwr_device.h; alpha 2.0 -> 255) over what the pair holds
    auto pack_mesh = [&](i2 obj, f2 cr, f2 cg, f2 cb, uint32_t (&rgba)[2], float4 (&cf)[2]) {
        const f2 sr = cr * 255.0f, sg = cg * 255.0f, sb = cb * 255.0f;
        const uint32_t m0 = pack_rgba8_scaled(sr.x, sg.x, sb.x, 0xff000000u);
        const uint32_t m1 = pack_rgba8_scaled(sr.y, sg.y, sb.y, 0xff000000u);
        rgba[0] = obj.x >= 0 ? m0 : rgba[0];
        rgba[1] = obj.y >= 0 ? m1 : rgba[1];
        if (AUX) {
            if (obj.x >= 0) cf[0] = make_float4(cr.x, cg.x, cb.x, 2.0f);
            if (obj.y >= 0) cf[1] = make_float4(cr.y, cg.y, cb.y, 2.0f);
        }
    };

    // -- the tile's class, known to the setup: three ways through the tile, chosen once per wave (uniform), which meet again where
    // the pair's results are stored ----------------------------------------------------------------------------------------------
    constexpr uint32_t kWayNone = 0u, kWayOne = 1u, kWayAll = 2u;
    const uint32_t tile_class = cls & (kTileFacesMask | kTileSphereMask);
    const uint32_t way = !classed ? kWayAll
                         : tile_class == kTileFacesNone ? kWayNone
                         : (tile_class == kTileFacesOne && !NMAP && (LISTS || !(p.n_materials > 1u))) ? kWayOne : kWayAll;
    // framebuffer state of the two pixels, as the reference's cleared textures hold it
    f2 depth_tex = splat(0.0f), win_t = splat(0.0f);
    i2 obj = i2{-1, -1};
    MeshHit2 best;
    best.have = i2{0, 0};
    best.t = best.u = best.v = best.ndotd = splat(0.0f);
    best.idx = u2{0u, 0u};
    uint32_t dbg_listed = 0, dbg_tested = 0;
    uint32_t n_tested = 0;  // wave-uniform
    uint32_t last_idx = 0;  // (wave-uniform) the face tested last: a wave that tested exactly one face loads its shading
                            // record for the shading step, into scalar registers (carried through the loop, the record's
                            // 11 dwords lived in vector registers)
    ShadeRec one_shade = {};   // (kWayOne: that record, requested with the face's other records)
    if (way == kWayNone) {
        // no face and no sphere can show: the cleared frame.  No sphere pass, no mesh pass, no shading, no use for the ray; the
        // wave still meets its workgroup at the table's barrier (LISTS: it waits for its own DMA, which must not land in LDS
        // that another workgroup holds by then).
        lut_ready();
    } else if (way == kWayOne) {
        // exactly one face and no sphere: the straight path.  The face's index is in the class word, so its records — the hit
        // test's, the numerator and the shading's — are requested at once, ahead of the table's barrier; there is no state of an
        // earlier pass to composite with: the framebuffer holds the clear values, the first hit is the nearest.  The arithmetic is
        // the general path's own functions, which therefore give its bits.
        const uint32_t idx = (cls >> kTileFaceShift) & 0xffu;
        const TriRecord T = tris[idx];
        const float tnum = to_const_space(tnum_ptr())[idx];
        one_shade = shade[idx];
        // ... and with them, on a frame served from the slot's kept records (RWR_FLAG_TILE_COVER, render_reference.cpp), the tile's cover word
        // (rwr_internal.h kTileCovered; the third parallel array): what the tests below said about the tile on an earlier frame
        // with these records.  Without the flag the word is neither read nor written.
        // (cov: the word, or kTileNotCovering without the flag — one scalar register carries both facts across the test)
        constexpr uint32_t kTileNotCovering = 2u;
        uint32_t cov = kTileNotCovering;
        if constexpr (COVER) {
            if constexpr (LISTS) cov = cov_entry;   // (requested at entry)
            else if ((p.flags & RWR_FLAG_TILE_COVER) != 0u) cov = to_const_space(tl())[cover_at(wu)];
        }
        rwait();   // (the table's barrier)
        // (p0 and e0 are read by one of the two branches below alone; left to itself the compiler moves their loads into that
        // branch, behind the barrier, where nothing hides them: keep the whole record requested ahead of it)
        if constexpr (COVER && !LISTS) asm volatile("" ::"s"(T.p0[0]), "s"(T.p0[1]), "s"(T.p0[2]), "s"(T.e0[0]), "s"(T.e0[1]), "s"(T.e0[2]));
        if constexpr (LISTS) asm volatile("" ::: "memory");   // (the wave's own DMA: no barrier)
        else __syncthreads();
        best.idx = u2{idx, idx};
        last_idx = idx;
        n_tested = 1u;
        if (AUX) dbg_listed = dbg_tested = 1u;
        if (COVER && cov == kTileCovered) {
            // ... and the cover word says what the lines of the other branch found on an earlier frame with these very records and
            // rays: every pair hits, wins, and both short forms are in their domain.  What feeds colour and depth is computed as
            // there; what could only confirm the word is not.
            triangle_covered(T, tnum, O, D, best.t, best.u, best.v, best.ndotd);
            best.have = i2{-1, -1};
            depth_tex = 1.0f - to_non_linear_depth_fast(best.t);
            obj = i2{(int)idx, (int)idx};
            win_t = best.t;
        } else {
            f2 u, v;
            best.have = triangle_hit(T, tnum, O, D, best.t, u, v, best.ndotd);
            best.u = best.have ? u : splat(0.0f);   // (a pair without a hit shades texel (0, 0) and drops the result, as ever)
            best.v = best.have ? v : splat(0.0f);
            // the depth test against the cleared plane: current_depth = 1 - 0 (compute.wgsl:210)
            const bool fast = !__any(any2(best.have & ~depth_fast_domain(best.t)));
            const f2 depth = fast ? to_non_linear_depth_fast(best.t) : to_non_linear_depth(best.t);
            const i2 win = best.have & ~(depth >= 1.0f);
            depth_tex = win ? (1.0f - depth) : splat(0.0f);
            obj = win ? i2{(int)idx, (int)idx} : i2{-1, -1};
            win_t = win ? best.t : splat(0.0f);
            if (COVER && cov != kTileNotCovering) {
                // learn the word: the masks these lines decided, compared once per wave (hit_t's own two domain tests again, the
                // same expressions).  One lane stores, with a plain vector store; the slot's stream orders it against the slot's
                // next launch, and no other wave reads this word.
                const bool all = fast && hit_div_num_domain(tnum) && hit_div_lanes_in_domain(abs2(best.ndotd)) &&
                                 __builtin_amdgcn_ballot_w64((win.x & win.y) != 0) == __builtin_amdgcn_read_exec();
                uint32_t w = wu;
                asm volatile("" : "+s"(w));   // (the address is formed again here, once per tile and key, not carried through the test)
                if constexpr (LISTS) {
                    // (the strides again from the dispatch's own grid, a load on this way alone — a tile learns once per key —
                    // instead of two argument registers held across the test on every way)
                    if (all && lane == 0u)
                        const_cast<uint32_t *>(tl())[gridDim.x * gridDim.y * 4u * (kTileListWords + 1u) + (by * gridDim.x + blockIdx.x) * 4u + w] = kTileCovered;
                } else if (all && lane == 0u) const_cast<uint32_t *>(tl())[cover_at(w)] = kTileCovered;
            }
        }
    } else {
    // -- every other tile ---------------------------------------------------------------------------------------------------
    if constexpr (LISTS) {   // (the tile's set: requested on this way alone, ahead of the sphere passes and the table's wait)
        const const_ptr<uint32_t> rec = to_const_space(tl()) + ((by * grid_x() + blockIdx.x) * 4u + wu) * kTileListWords;
#pragma unroll
        for (uint32_t k = 0; k < kTileListWords; k++) set[k] = rec[k];
    }

    // -- analytic sphere passes, in order (lib.rs:1106-1173) -----------------
    // (classed: the setup made the rectangle compares, bit s of the word's sphere field says "not outside"; a tile that touches
    // no sphere does not enter the loop, nor what the compiler hoists out of it)
    const float tx0 = (float)tile_x0, ty0 = (float)tile_y0;
    const uint32_t sph = classed ? (cls >> kTileSphereShift) & 0xffu : 0xffu;
    for (uint32_t s = 0; sph != 0u && s < p.n_spheres; s++) {
        if (classed ? ((sph >> s) & 1u) == 0u
                    : (CULL && ((tx0 + kTileWf < p.sphere_rect[s][0]) || (tx0 > p.sphere_rect[s][2]) ||
                                (ty0 + kTileHf < p.sphere_rect[s][1]) || (ty0 > p.sphere_rect[s][3]))))
            continue;
        f2 t = splat(0.0f);
        const i2 hit = sphere_ray_intersect_t(ld3(p.spheres[s].center), p.spheres[s].radius, O, D, t);
        if (any2(hit)) {
            const f2 current_depth = 1.0f - depth_tex;  // sphere/compute.wgsl:130
            const f2 depth = to_non_linear_depth(t);
            const i2 win = hit & ~(depth >= current_depth);
            depth_tex = win ? (1.0f - depth) : depth_tex;
            obj = win ? i2{-2 - (int)s, -2 - (int)s} : obj;
            win_t = win ? t : win_t;
        }
    }

    // -- mesh pass (lib.rs:1174-1184) -----------------------------------------
    if constexpr (CULL) {
        // Each wave culls the round's records for its own tile, 64 at a time, one per lane (rwr_cull.h), and walks the
        // survivors in ascending face order.  Every wave reaches every barrier: n_list is the workgroup's (a wave
        // outside the mesh rectangle loads its share and keeps no face).
        const TileRect tile_rect = {tx0, ty0, tx0 + kTileWf, ty0 + kTileHf};
        if (lists) {   // the tile's set, 64 faces at a time, ascending
            lut_ready();   // (the table's barrier)
#pragma unroll
            for (uint32_t k = 0; k < kTileListWords / 2u; k++) {
                unsigned long long m = live ? ((unsigned long long)set[2u * k + 1u] << 32 | set[2u * k]) : 0ull;
                if (AUX) dbg_listed += (uint32_t)__popcll(m);
                while (m) {
                    const uint32_t idx = 64u * k + (uint32_t)__builtin_ctzll(m);
                    m &= m - 1ull;
                    intersect_and_select(tris[idx], to_const_space(tnum_ptr())[idx], idx, O, D, best);
                    last_idx = idx;
                    n_tested++;
                    if (AUX) dbg_tested++;
                }
            }
        }
        if constexpr (kRounds) {
        for (uint32_t base = 0; base < n_list; base += 256u) {
            if (base) {   // lists of more than 256 faces: every wave is done with the previous round
                __syncthreads();
                load_round(base);
            }
            rwait();
            __syncthreads();
            const uint32_t n_round = min(n_list - base, 256u);
            for (uint32_t b = 0; b < n_round; b += 64u) {
                // every lane reads and culls its slot (i < 256: inside the arrays), the slots past the round's end are
                // dropped by the ballot: no branch, and the lane mask comes straight from the compares
                const uint32_t i = b + lane;
                const float4 q0 = s_rec[0][i], q1 = s_rec[1][i], q2 = s_rec[2][i], q3 = s_rec[3][i];
                const FrameTri rec = {q0.x, q0.y, q0.z, q0.w, {q1.x, q1.y, q1.z}, q1.w,
                                      {q2.x, q2.y, q2.z}, q2.w, {q3.x, q3.y, q3.z}, q3.w};
                const uint32_t my_face = s_face[i];
                unsigned long long m = live ? __builtin_amdgcn_ballot_w64(i < n_round && !rect_culls(rec, tile_rect)) : 0ull;
                if (AUX) dbg_listed += (uint32_t)__popcll(m);
                while (m) {
                    const uint32_t bit = (uint32_t)__builtin_ctzll(m);
                    m &= m - 1ull;
                    // wave-uniform face index: the record comes in through scalar loads
                    const uint32_t idx = (uint32_t)__builtin_amdgcn_readlane((int)my_face, (int)bit);
                    if (FUSED) intersect_and_select(load_tri_record(tris_c + idx), tnum_c[idx], idx, O, D, best);
                    else intersect_and_select(tris[idx], to_const_space(tnum_ptr())[idx], idx, O, D, best);
                    last_idx = idx;
                    n_tested++;
                    if (AUX) dbg_tested++;
                }
            }
        }
        if (n_list == 0u && !lists) {   // (the table's barrier when no round ran)
            rwait();
            __syncthreads();
        }
        }   // (kRounds)
    } else {
        rwait();   // (the table's)
        __syncthreads();
        // no culling: every face, in ascending order
        for (uint32_t base = 0; base < n_list; base += 64u) {
            unsigned long long m = __ballot(base + lane < n_list);
            if (AUX) dbg_listed += (uint32_t)__popcll(m);
            while (m) {
                const uint32_t idx = base + (uint32_t)__builtin_ctzll(m);
                m &= m - 1ull;
                intersect_and_select(tris[idx], to_const_space(tnum_ptr())[idx], idx, O, D, best);
                last_idx = idx;
                n_tested++;
                if (AUX) dbg_tested++;
            }
        }
    }
    if (any2(best.have)) {
        const f2 current_depth = 1.0f - depth_tex;  // compute.wgsl:210
        // same bits either way; the short form covers every distance a scene produces (rwr_device.h)
        const bool fast = !__any(any2(best.have & ~depth_fast_domain(best.t)));
        const f2 depth = fast ? to_non_linear_depth_fast(best.t) : to_non_linear_depth(best.t);
        const i2 win = best.have & ~(depth >= current_depth);
        depth_tex = win ? (1.0f - depth) : depth_tex;
        obj = win ? i2{(int)best.idx.x, (int)best.idx.y} : obj;
        win_t = win ? best.t : win_t;
    }
    }   // (kWayAll)

    const PairSlot ps = pair_slot(px0, py);
    // (the store counts in the wave's vector-memory counter, so the shading's first texel wait covers it.  The lean form with the
    // store at the end, beside the colour's, measured the same frame time with four more vector registers:
    // profiles/r13_lean_chain_ab.txt)
    store_depth(ps, depth_tex);

    // -- shade the winners and store --------------------------------------------
    // Sphere winners first (few tiles; one pixel at a time), straight to their packed form, so that the
    // ray direction is dead before the mesh shading starts.  Untouched pixels keep the clear value.
    uint32_t rgba[2] = {0u, 0u};
    float4 cf[2];
    if (AUX) cf[0] = cf[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (any2(obj < -1)) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int o = k ? obj.y : obj.x;
            if (o < -1) {
                const f3 Dk = lane3(D, k);
                const f3 center = ld3(p.spheres[-2 - o].center);
                float t = 0.0f;  // the winner's distance again (same function, same bits) rather than a live register pair
                (void)sphere_ray_intersect_t(center, p.spheres[-2 - o].radius, O, Dk, t);
                const f3 c = shade_sphere(cnormalize(sub3(along(O, t, Dk), center)), Dk);
                rgba[k] = pack_rgba8(c.x, c.y, c.z, 2.0f);
                if (AUX) cf[k] = make_float4(c.x, c.y, c.z, 2.0f);
            }
        }
    }
    if (__any(any2(obj >= 0))) {  // wave-uniform; lanes without a mesh winner shade face 0 and drop the result
        f2 cr, cg, cb;
        QuadTex qt = tex;
        qt.lut = s_lut;   // the decode table in LDS (filled above, behind the barriers of the mesh pass)
        const ShadeRec unused = {};   // (the per-pixel paths load their records themselves)
        if (NMAP) shade_mesh_pair<true, false, true, FrameParams, QuadTex>(p, shade, qt, obj, unused, best, D, cr, cg, cb);   // (per-face material path)
        else if (!LISTS && p.n_materials > 1u) shade_mesh_pair<true, false, false, FrameParams, QuadTex>(p, shade, qt, obj, unused, best, D, cr, cg, cb);
        else if (n_tested == 1u) {
            // the one face the wave tested (so the scene has faces and the record array exists): every mesh winner shows it
            const ShadeRec last_shade = way == kWayOne ? one_shade : FUSED ? load_shade_record(shade_c + last_idx) : shade[last_idx];
            if constexpr (LISTS) {   // (both quad records requested before the first is decoded)
                f2 tr, tgr, tb;
                shade_mesh_pair<false, true, false, FrameParams, QuadTex, true>(p, shade, qt, obj, last_shade, best, D, cr, cg, cb, tr, tgr, tb);
            } else shade_mesh_pair<false, true, false, FrameParams, QuadTex>(p, shade, qt, obj, last_shade, best, D, cr, cg, cb);
        } else if constexpr (LISTS) {
            f2 tr, tgr, tb;
            shade_mesh_pair<false, false, false, FrameParams, QuadTex, true>(p, shade, qt, obj, unused, best, D, cr, cg, cb, tr, tgr, tb);
        } else shade_mesh_pair<false, false, false, FrameParams, QuadTex>(p, shade, qt, obj, unused, best, D, cr, cg, cb);
        pack_mesh(obj, cr, cg, cb, rgba, cf);
    }
    store_colour(ps, rgba, cf, obj, win_t, dbg_listed, dbg_tested);
