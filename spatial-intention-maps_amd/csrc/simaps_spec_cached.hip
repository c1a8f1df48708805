// The get_state instance that reuses an unchanged map's cspace and receptacle distances
// (include/simaps_state_cache.h, state_cache.h): a twin of simaps_spec.hip's S1 small-room float32
// instance, get_state_spec_kernel<1, 184, 232, 44, 92>, in a unit of its own so that every other kernel
// keeps its code.  The body is get_state_body.inc's with GS_SPEC and GS_CACHED; what differs from the
// twin is the sweep track (sweep_track_cached below) and who renders on a hit.
//
// Waves: the robot's source (distance array 1) sweeps on waves 0-3 and the receptacle's (array 0) on
// waves 4-7 -- the twin's assignment swapped, so that on a hit the idle sweep waves are 4-7 and, with
// the render waves 8-15, form waves 4-15: the one-source instance's render group (render_maps<12>).
//
// The verdict.  The sweep waves load the record's window words beside their early occupancy loads (wave 0
// also the key), build the window words as the twin does and compare them bit for bit as they store
// them; a thread that sees a difference (thread 0: in the key) ORs into the LDS word sc_diff before the
// sweep group's first barrier, so every sweep wave reads the same verdict after it.  Thread 0 then
// publishes it in sc_verdict (1 miss, 2 hit) behind a local release fence.
//   miss: the twin's sweep track, which also rewrites the record: window words and free bits after the
//         dilation, the receptacle's array by its own four waves when their rounds end (rec_export),
//         key, results and the miss counter by thread 0 at the track's end.  A record is valid only
//         with its key's magic, written last and only if no round cap was hit.
//   hit:  waves 0-3 take the free bits from the record, initialise array 1 from them with the robot's
//         snapped cell at 0, and sweep the robot's source alone; no dilation, no receptacle rounds.
//         Waves 4-7 start the copy of the record's array into array 0 (LDS-DMA, hit_array_dma) and leave
//         for the render track with it in flight.
//         The free bits, which the sweep track needs at once, are loaded on speculation with the key,
//         after the verdict's own loads, so that a hit does not wait a second memory latency (a miss
//         drops them: 0.7 KB).  The array, which nothing reads before the distance phase, is fetched
//         after the verdict and by a hit only.
//
// The 8-or-12 barrier.  The render waves 8-15 run the parameter phase as in the twin and read
// sc_verdict before the barrier that ends it, waiting (bounded, as wait_scratch) while it is 0.  The
// word is written once, so all eight read the same value, which is the value waves 4-7 acted on: the
// barrier has 12 participants on a hit (each arrives counting to 12) and 8 on a miss, where waves 4-7
// never touch the render group's barrier words.  A wave of 4-7 may arrive first: arrivals only count,
// and the last one, whichever it is, opens the barrier.  From there the group is Group{tid - 256, 768}.
//
// Bounds: a record is record_bytes(RH, RW) bytes at cache + map_slot * that, for map_slot below
// cache_records only; every access to it goes through offsets below record_bytes (static_asserts).
#define GS_SPEC
#define GS_CACHED
#define GS_ROOM_H RH
#define GS_ROOM_W RW
#define SIMAPS_DEVICE_ONLY
#include "simaps.hip"
#include "get_state_instance.h"
#include "spec.h"
#include "state_cache.h"

namespace {
using namespace simaps_state_cache;
static_assert(WIN_PAD == RMAX && WIN_ROW_U32 * 4 == (int)sizeof(uint64_t) * WIN_WORDS, "the record's window rows are SsspScratch::win's");
static_assert(sizeof(B128) == 16, "a row of free bits");

constexpr int SC_NO_PARAM_THREAD = 1 << 20;  // a joining wave's t in the parameter phase: no parameter thread's
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// LDS words of the verdict: source 1's sweep-wave barrier words, which the round words replaced
// (GS_SPEC_ROUND_WORD; bar[3][2] stays its timeout flag); zero since the kernel's entry
__device__ __forceinline__ unsigned &sc_diff(Shared &sh) { return sh.bar[3][0]; }
__device__ __forceinline__ unsigned &sc_verdict(Shared &sh) { return sh.bar[3][3]; }

// what a sweep thread holds of its record from the kernel's start (8 sweep waves, G = 512)
struct CachePre {
    u32x4 key[4];                       // simaps_state_cache_header's key (3 words) and results: wave 0 only
    uint32_t w[OccLoad4<512>::NQ], w2;  // the window words this thread builds (win_from_dwords' mapping)
    // what a hit will take from the record, loaded on speculation (a miss drops it): waves 0-3 the free
    // bits of their array rows (hit_rows)
    u32x4 pf[3];
};
// a hit's work split: array row (t >> 4) + 16 k of thread t < 256, k < ROWS; the receptacle's array by
// waves 4-7 as PIECES whole 1 KiB pieces (one LDS-DMA wave-instruction each, piece p on wave 4 + p % 4)
// and its last REST dwords by the first REST lanes of one wave
template <int RH, int RW>
struct HitSplit {
    static constexpr int cells = (RH + 2) * ((RW + 2) | 1);
    static constexpr int ROWS = (RH + 2 + 15) / 16, PIECES = cells * 4 / 1024, REST = cells - 256 * PIECES;
    static_assert(ROWS <= 3 && REST >= 0 && REST <= 64, "CachePre::pf holds a thread's rows; one wave-instruction for the rest");
};

// The record's buffer descriptor, for the builtin loads and, as its four words, for the written-out
// LDS-DMA: base, stride 0, the record's length in bytes (0 for a missing record: every load reads 0
// and touches no memory), raw 32-bit data format.  One place, so the two forms cannot disagree.
template <int RH, int RW>
struct RecordRsrc {
    static constexpr unsigned FLAGS = 0x00020000u;
    __device__ static __forceinline__ int len(const char *rec) { return rec ? record_bytes(RH, RW) : 0; }
    __device__ static __forceinline__ __amdgpu_buffer_rsrc_t builtin(const char *rec)
    {
        return __builtin_amdgcn_make_buffer_rsrc((void *)rec, (short)0, len(rec), (int)FLAGS);
    }
    __device__ static __forceinline__ u32x4 words(const char *rec)  // (wave-uniform: scalar registers)
    {
        auto u = [](unsigned x) { return (unsigned)__builtin_amdgcn_readfirstlane((int)x); };
        const uint64_t base = (uint64_t)(uintptr_t)rec;
        return u32x4{u((unsigned)base), u((unsigned)(base >> 32) & 0xffffu), u((unsigned)len(rec)), FLAGS};
    }
};

// Range-checked loads (offset -1 and a missing record read 0, as cspace_load4's): all in flight at once.
// Only what is used: the key by wave 0, a window word where the wave has a window row, the free bits
// by waves 0-3; a condition that is the same for a whole wave is a branch, not an offset -1.
template <int RH, int RW>
__device__ __forceinline__ void cache_preload(CachePre &P, const char *rec, int t)
{
    const __amdgpu_buffer_rsrc_t rs = RecordRsrc<RH, RW>::builtin(rec);
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    constexpr int whM = RH + 2 * RMAX;
    static_assert(whM % 2 == 0, "a wave's two window rows are in or out together");
#pragma unroll
    for (int k = 0; k < 4; k++) {
        P.key[k] = u32x4{0u, 0u, 0u, 0u};
        if (wave == 0) P.key[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * k, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < OccLoad4<512>::NQ; q++) {
        const int rr = 2 * (wave + 8 * q) + (lane >> 5);
        P.w[q] = 0u;
        if (2 * (wave + 8 * q) < whM)
            P.w[q] = __builtin_amdgcn_raw_buffer_load_b32(rs, OFF_WIN + (rr * WIN_ROW_U32 + ((lane >> 3) & 3)) * 4, 0, 0);
    }
    const int rr = t >> 2;
    P.w2 = 0u;
    if (16 * wave < whM)
        P.w2 = __builtin_amdgcn_raw_buffer_load_b32(rs, rr < whM ? OFF_WIN + (rr * WIN_ROW_U32 + 4) * 4 : -1, 0, 0);
    // (last: the verdict's loads above come back first)
    using HS = HitSplit<RH, RW>;
#pragma unroll
    for (int k = 0; k < HS::ROWS; k++) {
        const int r = (t >> 4) + 16 * k;
        P.pf[k] = u32x4{0u, 0u, 0u, 0u};
        if (wave < 4) P.pf[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, r >= 1 && r <= RH ? off_free(RH) + (r - 1) * 16 : -1, 0, 0);
    }
}

// A hit's waves 4-7 (t2 = t - 256), after the verdict: the record's array straight into distance array 0
// by LDS-DMA, nothing through registers.  Record and LDS image are both contiguous, so piece p is the
// record's bytes [1024 p, 1024 p + 1024) of the array to the wave-uniform LDS base array + 1024 p, lane
// l's 16 bytes at + 16 l.  The array's last REST dwords go as one 4-byte DMA of REST lanes: an inactive
// lane writes nothing, so the DMA ends with the array and the render track's cell table behind it
// (tail_cells_off: the next 16-byte boundary) is not written.  That bound rests on the arithmetic below
// (static_assert), not on a test: the render track writes the table after the DMA has landed, so an
// overrun would be overwritten unseen.  The loads are range-checked against the record like every
// other (buffer loads through the record's descriptor).
// Nothing reads array 0 before the distance phase; the issuing wave retires its DMA (sc_retire_array)
// before a barrier that every reader passes.  The instruction is written out because the compiler
// retires an LDS-DMA that it knows of at the wave's next LDS fence or read -- here the 12-wave barrier,
// where a joining wave would make the render group wait for its DMA; it restores M0, which is the
// compiler's.  vmcnt counts in order, so a wait the compiler places for a later load is only stricter.
template <int BYTES>
__device__ __forceinline__ void sc_dma_piece(u32x4 rs, unsigned lds_base, int voffset)
{
    static_assert(BYTES == 16 || BYTES == 4, "");
    unsigned keep;
    if (BYTES == 16)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(voffset), "s"(rs), "s"(lds_base)
                     : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(voffset), "s"(rs), "s"(lds_base)
                     : "memory");
}
template <int RH, int RW>
__device__ __forceinline__ void hit_array_dma(float *dist, const char *rec, int t2)
{
    using HS = HitSplit<RH, RW>;
    constexpr int arr = off_rec(RH) + REC_HDR;
    static_assert(arr % 16 == 0 && OFF_DIST % 16 == 0, "16-byte pieces");
    static_assert(arr + 1024 * HS::PIECES + 4 * HS::REST == arr + 4 * HS::cells && arr + 4 * HS::cells <= record_bytes(RH, RW),
                  "the DMA covers the array and stays inside the record");
    auto u = [](unsigned x) { return (unsigned)__builtin_amdgcn_readfirstlane((int)x); };
    const u32x4 rs = RecordRsrc<RH, RW>::words(rec);
    const int lane = t2 & 63, wave = __builtin_amdgcn_readfirstlane(t2 >> 6);
    const unsigned d = u((unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)reinterpret_cast<char *>(dist));
#pragma unroll
    for (int k = 0; k < (HS::PIECES + 3) / 4; k++) {
        const int p = wave + 4 * k;
        if (p < HS::PIECES) sc_dma_piece<16>(rs, d + 1024 * p, arr + 1024 * p + 16 * lane);
    }
    if (HS::REST > 0 && wave == (HS::PIECES & 3) && lane < HS::REST)
        sc_dma_piece<4>(rs, d + 1024 * HS::PIECES, arr + 1024 * HS::PIECES + 4 * lane);
}
// The issuing wave's wait for hit_array_dma.  The product calls it on a joining wave between the 12-wave
// barrier and the stamps' barrier, earlier than it must (any barrier up to the workgroup barrier ahead of
// the distance phase would do): there the wave has issued next to nothing else (in the product nothing;
// a stamp build's stamp stores, and intention_channel_order's loads where a configuration has them), so
// vmcnt(0) is the DMA's count or at most stricter, and about 4 us of the wave's own work lie between
// issue and wait.  Later, behind render_maps' stores, the same wait would expose their latency.
__device__ __forceinline__ void sc_retire_array() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// win_from_dwords<512> with each stored word compared with the record's: true if one of this
// thread's differs
__device__ __forceinline__ bool win_from_dwords_cmp(SsspScratch &S, const OccLoad4<512> &L, const CachePre &P, int whM, int t)
{
    static_assert(OccLoad4<512>::NU == 1, "one tail dword per thread");
    const int lane = t & 63, wave = t >> 6;
    uint32_t *win32 = reinterpret_cast<uint32_t *>(&S.win[0][0]);
    bool diff = false;
#pragma unroll
    for (int q = 0; q < OccLoad4<512>::NQ; q++) {
        unsigned x = nib4(L.v[q]) << (4 * (lane & 7));
        x |= (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x111, 0xf, 0xf, true);  // row_shr:1
        x |= (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x112, 0xf, 0xf, true);  // row_shr:2
        x |= (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x114, 0xf, 0xf, true);  // row_shr:4
        const int rr = 2 * (wave + 8 * q) + (lane >> 5);
        if ((lane & 7) == 7 && rr < whM) {
            win32[rr * 6 + ((lane >> 3) & 3)] = x;
            diff |= x != P.w[q];
        }
    }
    {
        const int rr = t >> 2;
        unsigned x = nib4(L.v2[0]) << (4 * (t & 3));
        x |= (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x111, 0xf, 0xf, true);
        x |= (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0x112, 0xf, 0xf, true);
        if ((t & 3) == 3 && rr < whM) {
            win32[rr * 6 + 4] = x;
            diff |= x != P.w2;
        }
    }
    return diff;
}

// A render wave, before the barrier that ends the parameter phase: the sweep group's verdict, true for
// a hit.  Lane 0 polls while it is undecided, bounded as wait_scratch is (then: the timeout flag, and a
// miss).
__device__ __forceinline__ bool cache_verdict_hit(Shared &sh)
{
    unsigned v = 0;
    if ((threadIdx.x & 63) == 0) {
        unsigned spins = 0;
        while (!(v = __hip_atomic_load(&sc_verdict(sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (1u << 22)) {  // never in a correct run (SIMAPS_FAULT_TIMEOUT)
                __hip_atomic_store(&sh.bar[1][2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                break;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    return (unsigned)__builtin_amdgcn_readfirstlane((int)v) == 2u;
}

// source 1's rounds on waves 0-3, source 0's on waves 4-7 (sssp_rounds_room with the sources swapped)
template <int RH, int RW>
__device__ __forceinline__ void sssp_rounds_swapped(Shared &sh, float *dist)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    switch ((wave + 2 * ((wave >> 2) ^ 1)) & 3) {  // sssp_rounds_word's own dir
    case 0: sssp_rounds_word<0, RH, RW, 1>(sh, dist); break;
    case 1: sssp_rounds_word<1, RH, RW, 1>(sh, dist); break;
    case 2: sssp_rounds_word<2, RH, RW, 1>(sh, dist); break;
    default: sssp_rounds_word<3, RH, RW, 1>(sh, dist); break;
    }
}

// The sweep track of the cached instance (group g: waves 0-7; see the head of this file).  rec: the map
// slot's record, nullptr for a slot beyond the cache (always a miss, nothing written).  Returns true
// in a hit's waves 4-7, which go on to the render track.
template <int RH, int RW>
__device__ __forceinline__ bool sweep_track_cached(Shared &sh, SsspScratch &S, float *dist, const simaps_config &cfg,
                                                   const Geometry &geo, const simaps_agent &ag, const simaps_env &ev,
                                                   const simaps_robot *__restrict__ robots, char *rec,
                                                   const OccLoad4<512> &occ4, const CachePre &P, const Group &g)
{
    constexpr int h = RH, w = RW, pw = (RW + 2) | 1, cells = (h + 2) * pw, whM = h + 2 * RMAX;
    static_assert(OFF_WIN + whM * WIN_ROW_U32 * 4 <= off_free(h) && off_rec(h) + REC_HDR + cells * 4 <= record_bytes(h, w),
                  "the record's parts");
    static_assert(REC_HDR == 16 && off_rec(h) % 16 == 0 && off_free(h) % 16 == 0, "16-byte aligned parts");
    const int t = g.t, H = cfg.H, W = cfg.W;
#ifdef SIMAPS_PHASE_STAMPS
    if (t == 0 && ag.map_slot >= 0) STAMP_NB(43);
#endif
    const simaps_robot *rb = robots + ev.robot_off;
    const int radius = geo.cspace_r[rb[ag.robot].type];
    int rq0 = 0, rq1 = 0;  // (thread 0: the receptacle's query pixel)
    if (t == 0) {  // (as sweep_track)
        sh.h = h;
        sh.w = w;
        sh.i0 = cfg.room_i0;
        sh.j0 = cfg.room_j0;
        pos_to_pix(ev.receptacle_x, ev.receptacle_y, H, W, rq0, rq1);
        sh.src_q[0][0] = rq0;
        sh.src_q[0][1] = rq1;
        pos_to_pix(rb[ag.robot].x, rb[ag.robot].y, H, W, sh.src_q[1][0], sh.src_q[1][1]);
        sh.sp_slot[0] = 0;
        sh.sp_slot[1] = 1;
        sh.nsrc = 2;
    }
    const u32x4 key0 = {(unsigned)SIMAPS_STATE_CACHE_MAGIC, (unsigned)H, (unsigned)W, (unsigned)cfg.room_i0};
    const u32x4 key1 = {(unsigned)cfg.room_j0, (unsigned)h, (unsigned)w, (unsigned)radius};
    const u32x4 key2 = {(unsigned)ev.has_receptacle, (unsigned)rq0, (unsigned)rq1, 0u};
    bool diff = win_from_dwords_cmp(S, occ4, P, whM, t);
    if (t == 0) {  // (P.key[3]: the results, no part of the key)
        const u32x4 d = (P.key[0] ^ key0) | (P.key[1] ^ key1) | (P.key[2] ^ key2);
        diff |= (d.x | d.y | d.z | d.w) != 0u;
    }
    if (__ballot(diff) && (t & 63) == 0)
        __hip_atomic_fetch_or(&sc_diff(sh), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    g.sync();  // S.win, sh's fields above and sc_diff are the group's
    if (t == 0) STAMP_NB(15);
    const bool hit = __builtin_amdgcn_readfirstlane(
                         (int)__hip_atomic_load(&sc_diff(sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == 0;
    if (t == 0) {
#ifdef SIMAPS_DIAG_VERDICT_LATE  // (a diagnostic build for tests/test_gpu_state_cache.py, never the product: every
        // render wave finds the verdict undecided and takes cache_verdict_hit's wait)
        for (int k = 0; k < 8; k++) __builtin_amdgcn_s_sleep(127);
#endif
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __hip_atomic_store(&sc_verdict(sh), hit ? 2u : 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    const float scale = (float)cfg.shortest_path_map_scale;
    if (hit) {
        using HS = HitSplit<RH, RW>;
        static_assert(HS::cells == cells, "the same array");
        if (t >= 256) {  // waves 4-7: the record's array -> distance array 0 (in flight when they join the render track)
#ifndef SIMAPS_DIAG_ARRAY_LATE  // (the diagnostic build issues it at the last moment instead: get_state_body.inc, at the
                                // workgroup barrier ahead of the distance phase)
            hit_array_dma<RH, RW>(dist, rec, t - 256);
#endif
            return true;
        }
        // waves 0-3: 16 lanes per array row as build_cspace writes it (free +inf, blocked / border -inf).
        // snap_init_sources' fast path in the same pass: the thread that writes the cell of the robot's
        // query pixel knows whether it is free, writes 0 there if so and publishes the source and its
        // dirty lines (thread 0 for a pixel outside the rect); every thread reads src_ok after the barrier.
        const Group g4{t, 256, sh.bar[0], 4};
        const int qr = sh.src_q[1][0] - cfg.room_i0, qc = sh.src_q[1][1] - cfg.room_j0;
        const bool q_in = (unsigned)qr < (unsigned)h && (unsigned)qc < (unsigned)w;
        auto publish = [&](bool fr) {
            sh.src_ok[1] = fr;
            sh.src_s[1][0] = sh.src_q[1][0];
            sh.src_s[1][1] = sh.src_q[1][1];
#pragma unroll
            for (int q = 0; q < 8; q++) {  // only the source's row / column is dirty (snap_init_sources)
                const int d2 = (q >> 1) & 3, word = q & 1, bit = fr ? (d2 < 2 ? qr : qc) : -1;
                sh.dirty[1][d2][word] = bit >= 0 && (bit >> 6) == word ? 1ull << (bit & 63) : 0ull;
            }
        };
        const int l16 = t & 15;
        float *D1 = dist + DIST_FLOATS;
        bool own = false, own_free = false;  // this thread writes the query pixel's cell / and it is free
#pragma unroll
        for (int k = 0; k < HS::ROWS; k++) {
            const int r = (t >> 4) + 16 * k;
            if (r < h + 2) {  // (P.pf[k]: rect row r - 1's free bits, 0 for the border rows)
                const B128 f = {P.pf[k].x | ((uint64_t)P.pf[k].y << 32), P.pf[k].z | ((uint64_t)P.pf[k].w << 32)};
                if (l16 == 0 && r >= 1 && r <= h) S.freeb[r - 1] = f;
                const bool qrow = q_in && r == qr + 1;
#pragma unroll
                for (int i = 0; i < (pw + 15) / 16; i++) {
                    const int c = l16 + 16 * i;  // array column c = rect column c - 1
                    if (c < pw) {
                        const bool fc = c >= 1 && c <= w && b_test(f, c - 1);
                        const bool src = qrow && c == qc + 1;
                        own |= src;
                        own_free |= src && fc;
                        D1[r * pw + c] = src && fc ? 0.0f : (fc ? INFINITY : -INFINITY);
                    }
                }
            }
        }
        if (own || (t == 0 && !q_in)) publish(own_free);
        if (t == 0) {
            const u32x4 res = P.key[3];
            sh.src_s[0][0] = (int)res.x;  // the receptacle's: the record's
            sh.src_s[0][1] = (int)res.y;
            sh.src_ok[0] = (int)res.z;
            sh.dmax[0] = __uint_as_float(res.w);
            sh.unreach[0] = (__uint_as_float(res.w) / 96.0f) * scale;  // (sssp_max_final's expression)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned *>(rec + offsetof(simaps_state_cache_header, hits)), 1u,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (t < 6) (&sh.changed[0][0])[t] = 0;
        if (t == 6) sh.rounds = 0;
        g4.sync();
        if (t == 0) STAMP_NB(2);
        if (!sh.src_ok[1]) {  // (uniform: read behind the barrier) the EDT snap on one wave
            if (t < 64)
                snap_wave(S.freeb, h, w, cfg.room_i0, cfg.room_j0, sh.src_q[1][0], sh.src_q[1][1], [&](int si, int sj) {
                    const int sr = si - cfg.room_i0, sc = sj - cfg.room_j0;
                    if (t == 0) {
                        sh.src_s[1][0] = si;
                        sh.src_s[1][1] = sj;
                        sh.src_ok[1] = 1;
                        D1[(sr + 1) * pw + sc + 1] = 0.0f;
                    }
                    if (t < 8) {
                        const int d2 = (t >> 1) & 3, word = t & 1, bit = d2 < 2 ? sr : sc;
                        sh.dirty[1][d2][word] = (bit >> 6) == word ? 1ull << (bit & 63) : 0ull;
                    }
                });
            g4.sync();
        }
        if (t == 0) {  // every read of the scratch is done: the render group may take it (as sweep_track)
            STAMP_NB(48);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            __hip_atomic_store(&sh.scratch_free, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            STAMP_NB(3);
        }
        sssp_rounds_swapped<RH, RW>(sh, dist);
        const float m = max_finite_part(D1, cells, t, 256);
        if ((t & 63) == 0) sh.red[1][t >> 6] = m;
        g4.sync();
        if (t == 0) STAMP_NB(49);
        if (t == 1) {  // (sssp_max_final for source 1)
            float mm = sh.red[1][0];
            for (int k = 1; k < 4; k++) mm = fmaxf(mm, sh.red[1][k]);
            sh.dmax[1] = mm;
            sh.unreach[1] = (mm / 96.0f) * scale;
        }
        if (t == 0) STAMP_NB(50);
        return false;
    }
    // ---- a miss: the twin's sweep track, and the record rewritten
    build_cspace<512>(S, nullptr, h, w, radius, g, dist, 2, &occ4, nullptr, H, W, cfg.room_i0, cfg.room_j0, true);
    if (t == 0) STAMP_NB(2);
    if (rec) {
        const uint32_t *win32 = reinterpret_cast<const uint32_t *>(&S.win[0][0]);
        uint32_t *rw = reinterpret_cast<uint32_t *>(rec + OFF_WIN);
        for (int k = t; k < whM * WIN_ROW_U32; k += 512)
            if (k % WIN_ROW_U32 != 5) rw[k] = win32[k];  // (word 5 of a row is never built)
        if (t < h) reinterpret_cast<B128 *>(rec + off_free(h))[t] = S.freeb[t];
    }
    snap_init_sources(sh, S, dist, 2, g);
    if (t == 0) {
        STAMP_NB(48);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __hip_atomic_store(&sh.scratch_free, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        STAMP_NB(3);
    }
    sssp_rounds_swapped<RH, RW>(sh, dist);
    {   // each source's four waves take its maximum as soon as its own rounds end; the receptacle's
        // also write its array to the record
        const int s = (t >> 8) ^ 1;
        if (rec && s == 0) rec_export(rec + off_rec(h), dist, h, w, sh.src_ok[0], nullptr, t & 255, 256);
        const float m = max_finite_part(dist + s * DIST_FLOATS, cells, t & 255, 256);
        if ((t & 63) == 0) sh.red[s][(t >> 6) & 3] = m;
    }
    g.sync();
    if (t == 0) STAMP_NB(49);
    sssp_max_final(sh, 2, 4, scale, t);
    if (rec && t == 0) {  // the key last; a run that hit the round cap leaves no valid record
        const bool good = sh.rounds < (1 << 20);
        u32x4 *hd = reinterpret_cast<u32x4 *>(rec);
        hd[0] = u32x4{good ? key0[0] : 0u, key0[1], key0[2], key0[3]};
        hd[1] = key1;
        hd[2] = key2;
        const bool ok0 = sh.src_ok[0] != 0;  // (no free cell: no snapped cell either)
        hd[3] = u32x4{ok0 ? (unsigned)sh.src_s[0][0] : ~0u, ok0 ? (unsigned)sh.src_s[0][1] : ~0u, ok0 ? 1u : 0u,
                      __float_as_uint(sh.dmax[0])};
        __hip_atomic_fetch_add(reinterpret_cast<unsigned *>(rec + offsetof(simaps_state_cache_header, misses)), 1u,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (t == 0) STAMP_NB(50);
    return false;
}

#ifndef GS_CACHED_DEVICE  // (simaps_spec_cached_store.inc includes this file for the device code above only and
                          // brings its own kernel and launcher: the store and 16-bit twins of the ones below)
// MH x MW / RH x RW: the room class's map shape and room (simaps_spec.hip's GS_SPEC_ROOM arguments)
template <int MH, int MW, int RH, int RW>
__global__ void __launch_bounds__(NT) get_state_cached_kernel(
    simaps_config cfg_in, Geometry geo, const simaps_agent *__restrict__ agents, const simaps_env *__restrict__ envs,
    const simaps_robot *__restrict__ robots, const double *__restrict__ paths, const uint8_t *__restrict__ occupancy,
    const float *__restrict__ overhead, float *__restrict__ state, int C, unsigned *fault, char *cache, int cache_records)
{
    simaps_config cfg = cfg_in;
    fix_instance_fields<1, MH, MW, RH, RW>(cfg);  // (instance S1 in the room class, as simaps_spec.hip's twin)
    const simaps_debug dbg = {};
#define GS_MIXED 0
#include "get_state_body.inc"
#undef GS_MIXED
}
#endif  // GS_CACHED_DEVICE
}  // namespace

#ifndef GS_CACHED_DEVICE
namespace simaps_state_cache {
void launch_get_state(const simaps::GetStateLaunch &L)
{
    constexpr int MH = SIMAPS_ROOM_SMALL_H, MW = SIMAPS_ROOM_SMALL_W, RH = SIMAPS_ROOM_SMALL_RH, RW = SIMAPS_ROOM_SMALL_RW;
    hipLaunchKernelGGL((get_state_cached_kernel<MH, MW, RH, RW>), dim3(L.N), dim3(NT), 0, L.stream, *L.cfg, *L.geo,
                       L.agents, L.envs, L.robots, L.paths, L.occupancy, L.overhead, (float *)L.state, L.C, L.fault,
                       (char *)L.cache, L.cache_records);
}

#if defined(SIMAPS_PHASE_STAMPS) || defined(SIMAPS_LIGHT_STAMPS)
int read_stamps(unsigned long long *host_out)
{
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), sizeof(g_stamps)) == hipSuccess ? 0 : SIMAPS_EHIP;
}
#endif
}  // namespace simaps_state_cache
#endif  // GS_CACHED_DEVICE
