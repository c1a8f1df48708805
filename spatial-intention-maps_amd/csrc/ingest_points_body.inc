// The point pass of the observation ingest: the body of ingest_points_kernel (simaps.hip) and of
// ingest_points_seq_kernel (simaps_ingest_seq.hip), included as text inside the kernel, whose
// parameters it names (cfg, cam, agents, seg_ids, cam_params, depth, seg_raw, occupancy, keys, boxes;
// WCS) together with `tag`, the top byte of the frame's keys: the launch epoch, or the launch's base
// tag plus the frame's seq.
    __shared__ unsigned long long win[INGEST_WIN];
    // per chunk: A[c][j] = right[c] * pixel_x(j) + principal[c] (column j), Bt[c][i] = up[c] * pixel_y(i)
    // (row row0 + i): a point's ray t[c] = A[c][j] + Bt[c][i], the same float32 operations in the same
    // order as per point (capture_image, envs.py:1946-1950)
    // (A holds INGEST_PPT wrapped columns past Wc: A[c][Wc + t] = A[c][t], so a lane's 8 columns are
    // consecutive table entries even where its pixels wrap to the next row; segT: seg * 8 of body
    // ids -1 .. 254 at segT[id + 1])
    __shared__ float A[3][WCS + INGEST_PPT], Bt[3][INGEST_MAX_ROWS], Fs[3];
    __shared__ uint8_t segT[256];
    __shared__ int box[4];  // min i, -max i, min j, -max j of the chunk's map pixels
    const int n = blockIdx.y, tid = threadIdx.x;
    const int H = cfg.H, W = cfg.W, Hc = cam.height_px, Wc = cam.width_px, NP = Hc * Wc;
    const float *db = depth + (size_t)n * NP;
    const int32_t *raw = seg_raw + (size_t)n * NP;
    const int k0 = blockIdx.x * INGEST_PTS + tid * INGEST_PPT;
    float dv[INGEST_PPT];
    int rv[INGEST_PPT];
    // issue the chunk's loads first: the per-chunk tables below hide their latency
    ingest_load(db, raw, k0, NP, dv, rv);
    const simaps_agent ag = agents[n];
    const simaps_seg_ids ids = seg_ids[ag.env];
    const float c1 = (float)(cam.far_m * cam.near_m), cfar = (float)cam.far_m, cfn = (float)(cam.far_m - cam.near_m);
    const float cx2 = (float)cam.cx2, cy2 = (float)cam.cy2;
    // seg * 8 per body id (the reference's float sum of 1/8 multiples < 2 is exact: its integer sum)
    auto seg8_of = [&](int r) {
        int v = r == 0 ? 1 : 0;
        v += (r >= ids.min_obstacle && r <= ids.max_obstacle) ? 2 : 0;
        v += (ids.has_receptacle && r == ids.receptacle) ? 3 : 0;
        v += (r >= ids.min_cube && r <= ids.max_cube) ? 4 : 0;
        return v;
    };
    // per chunk once, by wave 0 alone (the pass is VALU-issue bound: the other waves' issue slots
    // go to other chunks): the camera frame and the column and row tables (envs.py:1932-1947; the
    // float32 divisions and products every point of a column / row would repeat)
    const int row0 = (blockIdx.x * INGEST_PTS) / Wc;
    if (tid < 64) {
        float F[12];
        camera_frame(cam_params + 9 * (size_t)n, F);
#pragma unroll
        for (int c = 0; c < 12; c++) F[c] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(F[c])));
        for (int j = tid; j < Wc + INGEST_PPT; j += 64) {
            const int jj = j < Wc ? j : j - Wc;
            const float px = cx2 * ((float)jj / (float)Wc - 0.5f);
#pragma unroll
            for (int c = 0; c < 3; c++) A[c][j] = F[3 + c] + px * F[9 + c];
        }
#pragma unroll
        for (int e = tid; e < 256; e += 64) segT[e] = (uint8_t)seg8_of(e - 1);
        if (tid < INGEST_MAX_ROWS) {
            const float py = cy2 * (0.5f - ((float)(row0 + tid) + 1.0f) / (float)Hc);
#pragma unroll
            for (int c = 0; c < 3; c++) Bt[c][tid] = py * F[6 + c];
        }
        if (tid < 3) Fs[tid] = F[tid];
        if (tid < 4) box[tid] = INT32_MAX;
    }
    const float h2 = (float)((double)H / 2), w2 = (float)((double)W / 2);
    const size_t base = (size_t)ag.map_slot * H * W;
    uint8_t *const occ = occupancy + base;
    {
        __syncthreads();
        float F[3];
#pragma unroll
        for (int c = 0; c < 3; c++) F[c] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(Fs[c])));
        // Per point, branch-free: cell[q] = map row << 16 | map column, or -1 (no point); key[q] as
        // below.  A lane whose 8 pixels all lie in the frame (every lane but the frame's last few)
        // takes the TAIL = false instance: no validity selects.  (A point past the end computes on
        // zero inputs and is dropped.)  No per-point branch, so the unrolled arrays are never copied
        // at branch joins.
        int cell[INGEST_PPT];
        unsigned long long key[INGEST_PPT];
        int cmin = -1, cmax = 0;  // the lane's (row, column) box, packed like cell: u16 halves
        // body ids all in the seg table's range -1 .. 254 (wave-uniform): a table look-up per point
        unsigned idor = 0;
#pragma unroll
        for (int q = 0; q < INGEST_PPT; q++) idor |= (unsigned)(rv[q] + 1);
        const bool ids_ok = __builtin_amdgcn_ballot_w64(idor >= 256u) == 0;
        auto points = [&](auto tail) {
            constexpr bool TAIL = decltype(tail)::value;
            const int i0 = k0 / Wc, j0 = k0 - i0 * Wc, ir0 = i0 - row0;  // (rows past the frame stay inside the table)
            // a full lane's 8 columns are the consecutive table entries j0 .. j0 + 7 (wrapped copies
            // past Wc); its points from q = Wc - j0 on lie in the next row
            float B0[3], B1[3];
#pragma unroll
            for (int c = 0; c < 3; c++) B0[c] = Bt[c][ir0], B1[c] = Bt[c][min(ir0 + 1, INGEST_MAX_ROWS - 1)];  // (B1 only matters below the last row)
            int i = i0, j = j0;
#pragma unroll
            for (int q = 0; q < INGEST_PPT; q++, j = (j + 1 == Wc) ? (i++, 0) : j + 1) {
                const int k = k0 + q;
                const bool valid = !TAIL || k < NP;
                const float dep = c1 / (cfar - cfn * dv[q]);
                float p[3];
                if constexpr (TAIL) {
#pragma unroll
                    for (int c = 0; c < 3; c++) p[c] = F[c] + dep * (A[c][j] + Bt[c][i - row0]);
                } else {
                    const bool nxt = q >= Wc - j0;
#pragma unroll
                    for (int c = 0; c < 3; c++) p[c] = F[c] + dep * (A[c][j0 + q] + (nxt ? B1[c] : B0[c]));
                }
                int s8;
                if (ids_ok) s8 = segT[rv[q] + 1];
                else s8 = seg8_of(rv[q]);
                int pi = ingest_clip(floorf(h2 - p[1] * 96.0f), H), pj = ingest_clip(floorf(w2 + p[0] * 96.0f), W);
                const int cq = (pi << 16) | pj;
                cell[q] = valid ? cq : -1;
                cmin = valid ? pk_min_u16(cmin, cq) : cmin, cmax = valid ? pk_max_u16(cmax, cq) : cmax;
                if (valid && s8 == 2) occ[(unsigned)__umul24(pi, W) + pj] = 1;  // np.isclose(seg, obstacle) (exact values)
                // np.argsort order by z: float bits made unsigned-monotone, NaN last; equal z -> later pixel
                const unsigned zb = __float_as_uint(p[2]);
                const unsigned zk = p[2] != p[2] ? 0xffffffffu : ((zb & 0x80000000u) ? ~zb : (zb | 0x80000000u));
                key[q] = ((unsigned long long)tag << 56) | ((unsigned long long)zk << 24) | (((unsigned)(k + 1) << 4) | (unsigned)s8);
            }
            // runs of one map pixel inside the lane: the run's last entry carries the run's max key
#pragma unroll
            for (int q = 1; q < INGEST_PPT; q++) {
                const bool run = cell[q] == cell[q - 1] && (!TAIL || cell[q] >= 0);
                key[q] = run && key[q - 1] > key[q] ? key[q - 1] : key[q];
                cell[q - 1] = run ? -1 : cell[q - 1];
            }
        };
        if (k0 + INGEST_PPT <= NP) points(std::false_type{});
        else points(std::true_type{});
        // the chunk's box of map pixels
        cmin = wave_reduce_dpp(cmin, pk_min_u16), cmax = wave_reduce_dpp(cmax, pk_max_u16);
        const int imin = (unsigned)cmin >> 16, jmin = cmin & 0xffff, imax = (unsigned)cmax >> 16, jmax = cmax & 0xffff;
        if ((tid & 63) == 0 && imin <= imax)  // (a wave without points keeps cmin = 0xffff'ffff, cmax = 0)
            atomicMin(&box[0], imin), atomicMin(&box[1], -imax), atomicMin(&box[2], jmin), atomicMin(&box[3], -jmax);
        __syncthreads();
        const int bi = box[0], bj = box[2], bh = -box[1] - bi + 1, bw = -box[3] - bj + 1;
        const int area = bh * bw;  // block-uniform (a chunk holds >= 1 point)
        if (tid == 0)  // the chunk's box of map pixels [i0, i1) x [j0, j1), for the resolve sweep
            reinterpret_cast<uint4 *>(boxes)[(size_t)n * gridDim.x + blockIdx.x] =
                make_uint4((unsigned)bi, (unsigned)(bi + bh), (unsigned)bj, (unsigned)(bj + bw));
        if (area > INGEST_WIN) {
            // box past the window (a forward camera's far rows: ~2-3 points per pixel, spread wide;
            // global atomics per run instead measured 3 us more per 256 frames):
            // a direct-mapped table of HS (cell tag, key) slots in the window's LDS.
            // Each cell's tag is written by its points (any one wins); points whose cell owns the
            // slot max-reduce there, the others (collisions) go straight to the global key map;
            // then one global atomic per used slot.
            constexpr int HS = INGEST_WIN * 2 / 3;  // keys (8 B) + tags (4 B) in the window's LDS
            unsigned long long *hk = win;
            int *ht = reinterpret_cast<int *>(win + HS);
            // slot: the cell's index in the box (row-major) mod HS -- neighbouring cells of a row
            // take neighbouring slots (the packed cell itself mod HS would fold rows 16 columns apart
            // onto one slot)
            auto slot = [&](int c) { return (unsigned)(((c >> 16) - bi) * bw + ((c & 0xffff) - bj)) % HS; };
            for (int e = tid; e < HS; e += INGEST_WG) hk[e] = 0ull, ht[e] = -1;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < INGEST_PPT; q++)
                if (cell[q] >= 0) ht[slot(cell[q])] = cell[q];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < INGEST_PPT; q++)
                if (cell[q] >= 0) {
                    const int h = slot(cell[q]);
                    if (ht[h] == cell[q]) atomicMax(&hk[h], key[q]);
                    else atomicMax(&keys[base + (cell[q] >> 16) * W + (cell[q] & 0xffff)], key[q]);
                }
            __syncthreads();
            for (int e = tid; e < HS; e += INGEST_WG) {
                const unsigned long long v = hk[e];
                if (v) atomicMax(&keys[base + (ht[e] >> 16) * W + (ht[e] & 0xffff)], v);
            }
            return;
        }
        for (int e = tid; e < area; e += INGEST_WG) win[e] = 0ull;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < INGEST_PPT; q++)
            if (cell[q] >= 0) atomicMax(&win[((cell[q] >> 16) - bi) * bw + ((cell[q] & 0xffff) - bj)], key[q]);
        __syncthreads();
        // the window's entries e = tid + m * INGEST_WG as (row, column) of the box, stepped without
        // a division per entry
        const int qs = INGEST_WG / bw, rs = INGEST_WG - qs * bw;
        int di = tid / bw, dj = tid - di * bw;
        for (int e = tid; e < area; e += INGEST_WG) {
            const unsigned long long v = win[e];
            if (v) atomicMax(&keys[base + (size_t)((bi + di) * W + bj + dj)], v);
            di += qs, dj += rs;
            if (dj >= bw) dj -= bw, di++;
        }
    }
