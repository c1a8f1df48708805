// The state cache for the store launches and the 16-bit launches (include/simaps_state_cache_store.h):
// which of them use a cache they are given, and the launchers of the three kernels that do
// (simaps_spec_cached_store_f32.hip, _bf16.hip, _f16.hip, all simaps_spec_cached_store.inc: units of
// their own, so that they cannot change the code of any other kernel).  The record, its layout and the
// hit / miss rule are state_cache.h's, unchanged: any cached kernel may hit on any other's record.
#pragma once
#include <hip/hip_runtime.h>
#include "geom.h"
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

// simaps_spec_store's launchers (spec_store.h) for instance S1 in the small room class, and the cache.
// The 16-bit launchers take dest == nullptr for simaps_get_state_as_cached: stack n goes to row n of
// `store` (capacity unused) and faults are posted under SIMAPS_K_GET_STATE.
void launch_f32(const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                const simaps_env *envs, const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                const float *overhead, float *store, int64_t capacity, const int64_t *dest, int C, unsigned *fault,
                void *cache, int cache_records, hipStream_t stream);
void launch_bf16(const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                 const simaps_env *envs, const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                 const float *overhead, uint16_t *store, int64_t capacity, const int64_t *dest, int C, unsigned *fault,
                 void *cache, int cache_records, hipStream_t stream);
void launch_f16(const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                const simaps_env *envs, const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                const float *overhead, uint16_t *store, int64_t capacity, const int64_t *dest, int C, unsigned *fault,
                void *cache, int cache_records, hipStream_t stream);
}  // namespace simaps_state_cache_store
