// The per-map-slot state cache of get_state (include/simaps_state_cache.h): the record's layout, which
// calls use it, and the launcher of the one kernel that does (simaps_spec_cached.hip, a unit of its
// own so that it cannot change the code of any other kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "get_state_launch.h"
#include "simaps_state_cache.h"
#include "spec.h"

namespace simaps_state_cache {
// byte offsets inside a record of a room h x w; every part 16-byte aligned
constexpr int WIN_PAD = 7;     // RMAX (simaps.hip): the window's margin around the rect
constexpr int WIN_ROW_U32 = 6;  // SsspScratch::win's row, as 32-bit words
constexpr int OFF_WIN = (int)sizeof(simaps_state_cache_header);
static_assert(OFF_WIN == 80 && offsetof(simaps_state_cache_header, snap_i) == 48 &&
                  offsetof(simaps_state_cache_header, hits) == 64,
              "header: three 16-byte key words, one of results, one of counters");
__host__ __device__ constexpr int align16(int x) { return (x + 15) & ~15; }
__host__ __device__ constexpr int off_free(int h) { return align16(OFF_WIN + (h + 2 * WIN_PAD) * WIN_ROW_U32 * 4); }
__host__ __device__ constexpr int off_rec(int h) { return off_free(h) + h * 16; }
__host__ __device__ constexpr int record_bytes(int h, int w)
{
    return (off_rec(h) + 16 + (h + 2) * ((w + 2) | 1) * 4 + 255) & ~255;
}

// the calls that use a cache they are given (the header's rule); any_debug as spec.h's
inline bool uses_cache(const simaps_config &c, bool any_debug)
{
    const int a0 = (c.room_j0 - WIN_PAD) & ~3;
    return simaps_spec::instance_of(c, any_debug) == SIMAPS_SPEC_S1 && simaps_spec::room_class_of(c) == SIMAPS_ROOM_SMALL &&
           c.room_j0 - WIN_PAD >= 0 && a0 + 144 <= c.W;  // (occ4_ok: W % 4 == 0 in the class)
}

// float32, no store; L.cache and L.cache_records are set (get_state_launch.h)
void launch_get_state(const simaps::GetStateLaunch &L);
#if defined(SIMAPS_PHASE_STAMPS) || defined(SIMAPS_LIGHT_STAMPS)
int read_stamps(unsigned long long *host_out);  // (as simaps_spec::read_stamps: this unit's table)
#endif
}  // namespace simaps_state_cache
