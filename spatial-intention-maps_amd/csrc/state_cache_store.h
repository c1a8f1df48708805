// The state cache for the store launches and the 16-bit launches (include/simaps_state_cache_store.h):
// which of them use a cache they are given, and the launchers of the three kernels that do
// (simaps_spec_cached_store_f32.hip, _bf16.hip, _f16.hip, all simaps_spec_cached_store.inc: units of
// their own, so that they cannot change the code of any other kernel).  The record, its layout and the
// hit / miss rule are state_cache.h's, unchanged: any cached kernel may hit on any other's record.
#pragma once
#include <hip/hip_runtime.h>
#include "get_state_launch.h"
#include "simaps_state_cache_store.h"
#include "spec_store.h"
#include "state_cache.h"

namespace simaps_state_cache_store {
// the calls that use a cache they are given (the header's rule); any_debug as spec.h's.  float32 without
// a store is simaps_get_state_cached's own rule.
inline bool applies(const simaps_config &c, int state_dtype, bool into, bool any_debug)
{
    if (state_dtype == SIMAPS_STATE_F32 && !into) return simaps_state_cache::uses_cache(c, any_debug);
    const int a0 = (c.room_j0 - simaps_state_cache::WIN_PAD) & ~3;
    return simaps_spec_store::instance_as(c, state_dtype, into, any_debug) == SIMAPS_SPEC_S1 &&
           simaps_spec::room_class_of(c) == SIMAPS_ROOM_SMALL && !any_debug &&
           c.room_j0 - simaps_state_cache::WIN_PAD >= 0 && a0 + 144 <= c.W;
}

// simaps_spec_store's launchers (spec_store.h) for instance S1 in the small room class, with L.cache and
// L.cache_records set.  Only the 16-bit ones take L.dest == nullptr (simaps_get_state_as_cached).
void launch_f32(const simaps::GetStateLaunch &L);
void launch_bf16(const simaps::GetStateLaunch &L);
void launch_f16(const simaps::GetStateLaunch &L);
inline void launch(const simaps::GetStateLaunch &L)
{
    (L.state_dtype == SIMAPS_STATE_F32 ? launch_f32 : L.state_dtype == SIMAPS_STATE_BF16 ? launch_bf16 : launch_f16)(L);
}
}  // namespace simaps_state_cache_store
