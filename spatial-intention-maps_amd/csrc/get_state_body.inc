// The body of get_state_kernel and get_state_mixed_kernel (simaps.hip), included into both with
// GS_MIXED 0 / 1: with GS_MIXED the workgroup's configuration, its map slot's offset and its stack's
// offset come from the launch's tables (simaps_get_state_mixed) instead of the launch-wide arguments.
// (A textual include rather than a template: get_state_kernel's source, and so its code, stay
// exactly those of the single-configuration kernel.)  With SIMAPS_STATE16 (simaps_state16.inc) state
// is the 16-bit stack and RenderCtx converts at the store; nothing else differs.  With GS_INTO
// (simaps_store.inc, GS_MIXED 0) the stack goes to row into_row of the caller's store and faults are
// posted under SIMAPS_K_GET_STATE_INTO (or under GS_INTO_KID where the includer defines it:
// simaps_spec_store.inc, whose 16-bit kernels serve simaps_get_state_as too).
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    Shared &sh = *reinterpret_cast<Shared *>(smem);
    float *dist = reinterpret_cast<float *>(smem + OFF_DIST);
    SsspScratch &S = *reinterpret_cast<SsspScratch *>(smem + OFF_UNION);
    float *tile = reinterpret_cast<float *>(smem + OFF_UNION);

    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    const int H = cfg.H, W = cfg.W;
    if (tid == 0) STAMP_NB(77);  // kernel entry (dispatch skew)
    simaps_agent ag = agents[n];
    // Sources of the shortest-path maps (envs.py:2071-2113 order): receptacle, then the robot.
    const int nsrc = (cfg.use_shortest_path_to_receptacle_map ? 1 : 0) + (cfg.use_shortest_path_map ? 1 : 0);
    // Two tracks run concurrently from the start: waves [0, cs_waves) build the cspace, snap the
    // sources and sweep the distance arrays (4 waves per source); the other waves compute the robot
    // parameters and stamp tiles and render every channel that does not need distances.
    const int cs_waves = nsrc > 0 ? 4 * nsrc : (dbg.cspace ? 4 : 0);
    // Small rooms (every small_* BASELINE config): the crop's robot-code map fits in the tail of
    // distance array 1, outside the raster tile, and the sweep track zeroes the tile when it
    // releases its scratch (early_tile).  Otherwise the code map lies in the union after the sweep
    // scratch and the render track zeroes the tile after a barrier.
    const bool early_tile =
        nsrc > 0 && (cfg.room_h + 2) * sssp_pitch(cfg.room_w) * 4 <= DIST_FLOATS * 4 - CMAP_BYTES;
    uint8_t *cmap = reinterpret_cast<uint8_t *>(smem) + (early_tile ? OFF_UNION - CMAP_BYTES : OFF_CMAP);
    const bool tail_cells = early_tile && !cfg.use_distance_to_receptacle_map &&
                            tail_cells_off(cfg.room_h, cfg.room_w) + LW * LW * 2 <= DIST_FLOATS * 4;
    if (tid < 16) (&sh.bar[0][0])[tid] = 0u;
    if (tid == 16) sh.scratch_free = cs_waves == 0;
#if defined(GS_SPEC) && !GS_MIXED  // GS_SPEC_EARLY_OCC
    // (simaps_spec.hip: the sweep waves' occupancy loads need the agent record only, so they are
    // issued here, ahead of the env record and the entry barrier, and handed to sweep_track)
    OccLoad4<512> pre8;
    OccLoad4<256> pre4;
    const bool pre_occ = (tid >> 6) < cs_waves && nsrc > 0 && occ4_ok(H, W, cfg.room_j0);
    if (pre_occ) {
        const uint8_t *occ_slot = occupancy + (size_t)ag.map_slot * H * W;
        if (cs_waves == 8) cspace_load4<512>(pre8, occ_slot, H, W, cfg.room_i0, cfg.room_j0, cfg.room_h, tid);
        else cspace_load4<256>(pre4, occ_slot, H, W, cfg.room_i0, cfg.room_j0, cfg.room_h, tid);
    }
#endif
#ifdef GS_CACHED  // (simaps_spec_cached.hip: the map slot's cache record -- none for a slot beyond the cache -- whose key
                  // and window words the sweep waves load beside their occupancy; sc_join: a sweep wave of a hit
                  // that has left the sweep track for the render track)
    char *const sc_rec = (unsigned)ag.map_slot < (unsigned)cache_records
                             ? cache + (size_t)ag.map_slot * simaps_state_cache::record_bytes(GS_ROOM_H, GS_ROOM_W)
                             : nullptr;
    CachePre sc_pre;
    if (pre_occ) cache_preload<GS_ROOM_H, GS_ROOM_W>(sc_pre, sc_rec, tid);
    bool sc_join = false;
#endif
    simaps_env ev = envs[ag.env];
    // descriptors come through the C ABI unchecked: clamp what would index past the LDS tables
    // (robot records, segment slots) and report it (SIMAPS_FAULT_DESCRIPTOR)
    // With intention channels C holds 1 (spatial) or 2 (nonspatial) channels per other robot of the
    // configuration's robot count (simaps_num_channels): an env with more robots would write past
    // the agent's stack, so its count is clamped to that and reported too.
    int nr_cap = SIMAPS_MAX_ROBOTS;
    if (cfg.use_intention_channels)
        nr_cap = (C - 1 - !!cfg.use_robot_map - !!cfg.use_distance_to_receptacle_map -
                  !!cfg.use_shortest_path_to_receptacle_map - !!cfg.use_shortest_path_map - !!cfg.use_history_map -
                  !!cfg.use_intention_map) / (cfg.intention_channel_spatial ? 1 : 2) + 1;
    const bool bad_desc = (unsigned)(ev.num_robots - 1) >= (unsigned)SIMAPS_MAX_ROBOTS ||
                          (unsigned)ag.robot >= (unsigned)ev.num_robots ||
                          (cfg.use_intention_channels && ev.num_robots != nr_cap);
    ev.num_robots = min(max(ev.num_robots, 1), min(nr_cap, SIMAPS_MAX_ROBOTS));
    if ((unsigned)ag.robot >= (unsigned)ev.num_robots) ag.robot = 0;
    lds_barrier();  // the group barriers are zeroed
    if (tid == 0 && bad_desc) sh.bar[0][3] = 1u;
    if (tid == 0) STAMP_NB(0);
#if GS_MIXED && defined(SIMAPS_STATE16)  // (simaps_store.inc: the mixed launch's 16-bit stack, out_off in elements)
    uint16_t *out = state + (size_t)out_off[n];
#elif GS_MIXED
    float *out = state + (size_t)out_off[n];
#elif defined(GS_INTO)  // (simaps_store.inc: row into_row of the caller's store, a 64-bit offset onto the base)
    auto *out = state + (size_t)into_row * LW * LW * C;
#elif defined(SIMAPS_STATE16)
    uint16_t *out = state + (size_t)n * LW * LW * C;
#else
    float *out = state + (size_t)n * LW * LW * C;
#endif
    const RenderCtx rc{cfg, sh, out, C, n};
    if ((tid >> 6) < cs_waves) {
        const Group g{tid, 64 * cs_waves, sh.bar[0], cs_waves};
#if GS_MIXED
        // (sweep_track addresses the slot as occupancy + map_slot * H * W: rebase the pointer so that
        // this lands on the slot's own offset)
        const uint8_t *occ_base = occupancy + ((int64_t)map_off[ag.map_slot] - (int64_t)ag.map_slot * H * W);
        if (cs_waves == 8) sweep_track<512>(sh, S, dist, cfg, geo, ag, ev, robots, occ_base, nsrc, dbg, n, g, early_tile);
        else sweep_track<256>(sh, S, dist, cfg, geo, ag, ev, robots, occ_base, nsrc, dbg, n, g, early_tile);
#elif defined(GS_CACHED)  // (two sources, a room class, the dword loads: the launcher saw to it)
        sc_join = sweep_track_cached<GS_ROOM_H, GS_ROOM_W>(sh, S, dist, cfg, geo, ag, ev, robots, sc_rec, pre8, sc_pre, g);
#elif defined(GS_SPEC)  // GS_SPEC_ROOM (simaps_spec.hip: GS_ROOM_H x GS_ROOM_W the instance's compile-time room, 0 in
                       // S1 / S2) and GS_SPEC_EARLY_OCC (a sweep wave: pre_occ is sweep_track's own use4, so the
                       // loads are there when it wants them)
        if (cs_waves == 8)
            sweep_track<512, GS_ROOM_H, GS_ROOM_W>(sh, S, dist, cfg, geo, ag, ev, robots, occupancy, nsrc, dbg, n, g,
                                                   early_tile, &pre8);
        else
            sweep_track<256, GS_ROOM_H, GS_ROOM_W>(sh, S, dist, cfg, geo, ag, ev, robots, occupancy, nsrc, dbg, n, g,
                                                   early_tile, &pre4);
#else
        if (cs_waves == 8) sweep_track<512>(sh, S, dist, cfg, geo, ag, ev, robots, occupancy, nsrc, dbg, n, g, early_tile);
        else sweep_track<256>(sh, S, dist, cfg, geo, ag, ev, robots, occupancy, nsrc, dbg, n, g, early_tile);
#endif
#ifdef GS_CACHED
        if (!sc_join) STAMP_NB(7);
    }
    if ((tid >> 6) >= cs_waves || sc_join) {
        // The render group is waves 8-15 until the barrier after the parameters, where a hit's waves 4-7
        // join it: from there it is waves 4-15 in the one-source instance's thread mapping (nw 12).  A
        // joining wave has no parameter work: its t lies beyond every parameter thread's until then.
        int nw = NT / 64 - cs_waves;
        Group g{tid - 64 * cs_waves, 64 * nw, sh.bar[1], nw};
        int t = sc_join ? SC_NO_PARAM_THREAD : g.t;
#else
        STAMP_NB(7);
    } else {
        const int nw = NT / 64 - cs_waves;
        const Group g{tid - 64 * cs_waves, 64 * nw, cs_waves ? sh.bar[1] : nullptr, nw};
        const int t = g.t;
#endif
        const simaps_robot *rb = robots + ev.robot_off;
        // ---- parameters (one lane per robot; the agent's own local rotation on another wave)
        if (t == 0) {
            sh.nr = ev.num_robots;
            sh.me = ag.robot;
            sh.env = ag.env;
            sh.has_rec = ev.has_receptacle;
        }
        if (t == 64) {
            const simaps_robot &me = rb[ag.robot];
            sh.rot = rot_params(CROP, 90.0 - me.heading * RAD_TO_DEG, cfg.rotate_rounding == SIMAPS_ROT_PLAIN);
            pos_to_pix(me.x, me.y, H, W, sh.pi, sh.pj);
            STAMP_NB(72);
        }
        if (t >= 128 && t < 128 + ev.num_robots) {
            const int k = t - 128;
            const simaps_robot &r = rb[k];
            RobotP &P = sh.rob[k];
            if ((cfg.use_intention_map && r.intention_len > SIMAPS_MAX_PATH) ||
                (cfg.use_history_map && r.history_len > SIMAPS_MAX_PATH))  // cut to SIMAPS_MAX_PATH points
                __hip_atomic_store(&sh.bar[0][3], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            robot_params(P, r, cfg, geo, H, W);
            if (k == 0) STAMP_NB(73);
        }
        {   // the crop's robot-code map starts empty; with 8 render waves the zeroing goes to the
            // waves without parameter work (3, 4, 6, 7), so the robot and segment waves reach the
            // barrier sooner
            const int w8 = t >> 6;
            const bool z8 = g.n == 512;
            const int zt = z8 ? (w8 == 3 || w8 == 4 ? t - 192 : (w8 >= 6 ? t - 256 : -1)) : t;
            const int zn = z8 ? 256 : g.n;
            if (zt >= 0) {
                uint4 *cz = reinterpret_cast<uint4 *>(cmap);
                for (int k = zt; k < CMAP_BYTES / 16; k += zn) cz[k] = uint4{0u, 0u, 0u, 0u};
                if (early_tile) {  // the raster tile beyond the cspace scratch (the sweep track zeroes the rest)
                    uint4 *tz = reinterpret_cast<uint4 *>(tile);
                    for (int k = SCRATCH_Q + zt; k < TILE * TILE / 4; k += zn) tz[k] = uint4{0u, 0u, 0u, 0u};
                }
            }
        }
        // the first history / intention pass's segment table, one lane per robot (raster_lines)
        const bool segs = (cfg.use_history_map || cfg.use_intention_map) && t >= 320 &&
                          t < 320 + ev.num_robots * SEG_PER_ROBOT;
        if (segs) {
            seg_geom(sh, cfg, rb, paths, cfg.use_history_map ? 4 : cfg.intention_map_encoding, t - 320, ag.robot);
            if (t == 320) STAMP_NB(74);
        }
        // the 5 host-computed robot mask windows (stamp tiles below)
        if (t < 5 * 24) sh.mwin[t] = geo.mbits[t / 24][t % 24];
        if (t >= 192 && t < 192 + 20) {
            const int q = t - 192, m = q >> 2, f = q & 3;
            sh.mwin[120 + q] = f == 0 ? geo.mrow0[m] : f == 1 ? geo.mcol0[m] : f == 2 ? geo.mnrows[m] : geo.mncols[m];
        }
        if (t == 0) STAMP_NB(75);
#ifdef GS_CACHED  // (the sweep group's verdict, waited for if need be: 8 or 12 waves meet at this barrier)
        if (sc_join || cache_verdict_hit(sh)) {
            nw = 12;
            g = Group{tid - 256, 768, sh.bar[1], 12};
        }
#endif
        g.sync();
        if (t == 0) STAMP_NB(9);
        if (segs) seg_ramp(sh, t - 320);  // (the segment table is read at raster time, many barriers later)
        if (cfg.use_intention_channels && t == 256) intention_channel_order(sh, cfg, rb);
#ifdef GS_CACHED
        t = g.t;
#endif

        if (t == 0) STAMP_NB(51);
        // ---- rotated robot stamps (Mapper._create_global_robot_map, envs.py:2251-2276): each robot's
        // scipy-rotated mask, evaluated once per workgroup over its <= 32 x 32 global box; the set
        // pixels inside the crop OR their code into the crop's robot-code map (bit g = seg value
        // (g + 5) / 8 of SEG_VALUES robot_group_{g+1}, bit 4 = 0.5, bit 5 = 1.0 lifted-cube mask)
        uint32_t *cmap32 = reinterpret_cast<uint32_t *>(cmap);
        const int ci0 = sh.pi - HALF_CROP, cj0 = sh.pj - HALF_CROP;
        // Waves own robots (nw / nr waves per robot, interleaved over its box rows); per wave-item 2
        // box rows (lane -> row 2 rp + lane / 32, column lane % 32).  The robot's parameters and mask
        // window bounds are loaded once per wave; source positions exactly in fp64 (rot_src).
        const int ln = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
        const int nrb = ev.num_robots, wpr = nrb <= nw ? nw / nrb : 1;
        for (int kk = wv; kk < nrb * wpr; kk += nw) {
            const int k = kk % nrb, sub = kk / nrb;
            const RobotP &P = sh.rob[k];
            const int bi0 = __builtin_amdgcn_readfirstlane(P.bi0), bi1 = __builtin_amdgcn_readfirstlane(P.bi1);
            const int bj0 = P.bj0, bj1 = P.bj1, st_i = P.st_i, st_j = P.st_j;
            const int type = P.type;
            const bool cube = type == SIMAPS_LIFTING && P.lifting;
            const unsigned code0 = P.code0;
            const Rot R{P.c, P.s, P.f0, P.f1, P.S0, P.S1};
            const int *mt = reinterpret_cast<const int *>(sh.mwin + 120 + 4 * type);
            const int *mc = reinterpret_cast<const int *>(sh.mwin + 120 + 4 * 4);
            const int mt0 = mt[0], mt1 = mt[1], mt2 = mt[2], mt3 = mt[3];
            const int mc0 = mc[0], mc1 = mc[1], mc2 = mc[2], mc3 = mc[3];
            // (two box-row pairs per iteration, their fp64 chains interleaved, measured slower: the
            // stamps phase 3.8 -> 4.4 us, round 4)
            for (int rp = sub; 2 * rp <= bi1 - bi0; rp += wpr) {
                const int gi = bi0 + 2 * rp + (ln >> 5), gj = bj0 + (ln & 31);
                unsigned code = 0;
                if (gi <= bi1 && gj <= bj1) {
                    int m0, m1;
                    const bool in = rot_src(R, LW, gi - st_i, gj - st_j, m0, m1);
                    if (in) {
                        const int r = m0 - mt0, cc = m1 - mt1;
                        if ((unsigned)r < (unsigned)mt2 && (unsigned)cc < (unsigned)mt3 && ((sh.mwin[type * 24 + r] >> cc) & 1u))
                            code = code0;
                        const int r2 = m0 - mc0, c2 = m1 - mc1;
                        if (cube && (unsigned)r2 < (unsigned)mc2 && (unsigned)c2 < (unsigned)mc3 && ((sh.mwin[4 * 24 + r2] >> c2) & 1u))
                            code |= 1u << 5;
                    }
                }
                const int ca = gi - ci0, cb = gj - cj0;
                if (code && (unsigned)ca < (unsigned)CROP && (unsigned)cb < (unsigned)CROP) {
                    const int pos = ca * CROP + cb;
                    atomicOr(&cmap32[pos >> 2], code << (8 * (pos & 3)));
                }
            }
        }
#ifdef GS_SPEC  // GS_SPEC_EARLY_ZERO (with GS_SPEC_RENDER_ZERO)
        // (simaps_spec.hip, two sources: the sweep track has usually released its scratch by now, so
        // each render wave zeroes its share of the tile's first SCRATCH_Q words ahead of the barrier
        // below, which the stamps need anyway, and the first raster pass starts without one of its
        // own; a wave that finds the scratch still held raises the late flag bar[1][3] instead and
        // render_maps zeroes after its wait, as before)
        if (early_tile && cfg.use_shortest_path_to_receptacle_map && cfg.use_shortest_path_map)
            zero_scratch_early(sh, tile, g);
#endif
#if defined(GS_CACHED) && !defined(SIMAPS_DIAG_ARRAY_LATE)  // (a hit's waves 4-7: the receptacle's array, in flight since
        // the verdict, is in LDS before they arrive)
        if (sc_join) sc_retire_array();
#endif
        g.sync();
        if (t == 0) STAMP_NB(1);
#if GS_MIXED
        const float *ovh = overhead + (size_t)map_off[ag.map_slot];
#else
        const float *ovh = overhead + (size_t)ag.map_slot * H * W;
#endif
        if (nw == 8) render_maps<18>(rc, g, geo, ovh, rb, paths, tile, cmap, early_tile, tail_cells, dist);
        else if (nw == 12) render_maps<12>(rc, g, geo, ovh, rb, paths, tile, cmap, early_tile, tail_cells, dist);
        else render_maps<9>(rc, g, geo, ovh, rb, paths, tile, cmap, early_tile, tail_cells, dist);
        if (t == 0) STAMP_NB(8);
    }
#if defined(GS_CACHED) && defined(SIMAPS_DIAG_ARRAY_LATE)  // (a diagnostic build for tests/test_gpu_state_cache_prologue.py,
    // never the product: a hit's waves 4-7 fetch the receptacle's array only here, with no work of their own
    // left to hide it, so that their wait and the barrier below are all that stands between the fetch and
    // the distance phase's reads -- without the wait those reads find the array unwritten)
    if (sc_join) {
        hit_array_dma<GS_ROOM_H, GS_ROOM_W>(dist, sc_rec, tid - 256);
        sc_retire_array();
    }
#endif
    lds_barrier();
    STAMP(4);

    // ---- all waves: distance channels (need the converged sweeps)
    STAMP(5);
    render_distance_channels(rc, ev, dist, nsrc, reinterpret_cast<const uint16_t *>(tile),
                             tail_cells ? reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(dist) +
                                                                          tail_cells_off(cfg.room_h, cfg.room_w))
                                        : reinterpret_cast<const uint16_t *>(tile) + LW * LW);
    STAMP(6);

    // ---- debug outputs
    if (nsrc > 0) {
        if (dbg.sources && tid < 2) {
            int32_t *o = dbg.sources + ((size_t)n * 2 + tid) * 4;
            const int s = sh.sp_slot[tid];
            if (s >= 0) { o[0] = sh.src_q[s][0]; o[1] = sh.src_q[s][1]; o[2] = sh.src_s[s][0]; o[3] = sh.src_s[s][1]; }
            else { o[0] = o[1] = o[2] = o[3] = -1; }
        }
    }
    if (tid == 0) {
        const unsigned f = group_faults(sh.bar, sh.rounds, nsrc);
#if defined(GS_INTO) && defined(GS_INTO_KID)  // (simaps_spec_store.inc: one kernel for the store launch and the plain 16-bit one)
        post_faults(fault, f, GS_INTO_KID, n);
#elif defined(GS_INTO)
        post_faults(fault, f, SIMAPS_K_GET_STATE_INTO, n);
#else
        post_faults(fault, f, GS_MIXED ? SIMAPS_K_GET_STATE_MIXED : SIMAPS_K_GET_STATE, n);
#endif
        if (dbg.status) {
            int st = (f & SIMAPS_FAULT_ROUNDS ? 2 : 0) | (f & SIMAPS_FAULT_TIMEOUT ? 4 : 0) |
                     (f & SIMAPS_FAULT_DESCRIPTOR ? 8 : 0);
            for (int s = 0; s < nsrc; s++) st |= sh.src_ok[s] ? 0 : 1;
            dbg.status[n] = st | ((nsrc > 0 ? sh.rounds & 0xfffff : 0) << 8);
        }
    }
#ifdef SIMAPS_PHASE_STAMPS
    if (tid == 0 && blockIdx.x < MAX_STAMP_WG) g_stamps[blockIdx.x * NSTAMP + 10] = (unsigned long long)sh.rounds;
#endif
