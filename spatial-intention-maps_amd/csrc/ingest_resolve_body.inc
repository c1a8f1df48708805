// The resolve pass of the observation ingest: the body of ingest_resolve_kernel (simaps.hip,
// INGEST_RESOLVE_SEQ 0) and of ingest_resolve_seq_kernel (simaps_ingest_seq.hip, INGEST_RESOLVE_SEQ 1),
// included as text inside the kernel, whose parameters it names (cfg, agents, overhead, keys, boxes,
// nch, epoch; ZERO).
// In the ordered launch two frames of one slot sweep overlapping boxes, so two workgroups may visit
// one pixel.  That is benign: the point pass has ended before this kernel starts (stream order), so
// each reads either the pixel's final key -- and writes the one value that key carries -- or, in the
// zeroing mode, the 0 another workgroup has already left there, and then writes nothing; whoever
// zeroes a key writes the same 0.  A key is one aligned 8-byte word, read and written whole.
    const int n = blockIdx.y, lane = threadIdx.x & 63, W = cfg.W;
    const int gw = blockIdx.x * (INGEST_RES_WG / 64) + (threadIdx.x >> 6), nw = INGEST_RES_G * (INGEST_RES_WG / 64);
    const uint4 *bx = reinterpret_cast<const uint4 *>(boxes) + (size_t)n * nch;
    // lane c < 64 holds box c (an empty box for c >= nch); more than 64 boxes (cameras over 131 k
    // pixels) are re-read per row below
    uint4 b0 = lane < nch ? bx[lane] : make_uint4(0x7fffffffu, 0u, 0x7fffffffu, 0u);
    const int fi0 = wave_reduce_dpp((int)b0.x, true), fi1 = wave_reduce_dpp((int)b0.y, false);
    int ri0 = fi0, ri1 = fi1;
    for (int c = 64 + lane; c < nch; c += 64) ri0 = min(ri0, (int)bx[c].x), ri1 = max(ri1, (int)bx[c].y);
    if (nch > 64) ri0 = wave_reduce_dpp(ri0, true), ri1 = wave_reduce_dpp(ri1, false);
    // the interval [lo, hi) of row r: the hull of the boxes containing r
    auto extent = [&](int r, int &lo, int &hi) {
        const bool in = (int)b0.x <= r && r < (int)b0.y;
        int a = in ? (int)b0.z : INT32_MAX, z = in ? (int)b0.w : 0;
        for (int c = 64 + lane; c < nch; c += 64) {
            const uint4 q = bx[c];
            if ((int)q.x <= r && r < (int)q.y) a = min(a, (int)q.z), z = max(z, (int)q.w);
        }
        lo = wave_reduce_dpp(a, true), hi = wave_reduce_dpp(z, false);
        if (hi <= lo) lo = hi = 0;  // no box holds the row
    };
    const size_t base = (size_t)agents[n].map_slot * cfg.H * W;
    constexpr int R = INGEST_RES_ROWS, U = 2;  // rows in flight; columns per lane and row in flight
    for (int r = ri0 + gw; r < ri1; r += R * nw) {
        int lo[R], hi[R], wmax = 0;
#pragma unroll
        for (int t = 0; t < R; t++) {
            lo[t] = hi[t] = 0;
            if (r + t * nw < ri1) extent(r + t * nw, lo[t], hi[t]);
            wmax = max(wmax, hi[t] - lo[t]);
        }
        for (int c0 = 0; c0 < wmax; c0 += 64 * U) {
            size_t idx[R * U];
            unsigned long long kv[R * U];
#pragma unroll
            for (int u = 0; u < R * U; u++) {
                const int t = u / U, c = lo[t] + c0 + (u % U) * 64 + lane;
                idx[u] = base + (size_t)(r + t * nw) * W + c;
                kv[u] = c < hi[t] ? keys[idx[u]] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < R * U; u++) {
                const unsigned tag = (unsigned)(kv[u] >> 56);
                if (INGEST_RESOLVE_SEQ ? tag >= epoch : tag == epoch) overhead[idx[u]] = (float)(kv[u] & 15ull) * 0.125f;
                if (ZERO && kv[u]) keys[idx[u]] = 0ull;
            }
        }
    }
