// One get_state launch as get_state_impl (simaps.hip) has checked it: every launcher of a get_state
// family (spec.h, spec_store.h, store.h, state16.h, state_cache.h, state_cache_store.h) takes this
// descriptor and unpacks it at its one hipLaunchKernelGGL, so that an argument is named where it is
// set and where it is used and nowhere in between.  Host only; the kernels' own parameters are theirs.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "geom.h"
#include "simaps.h"

namespace simaps {
struct GetStateLaunch {
    const simaps_config *cfg;  // has passed check_cfg
    const Geometry *geo;
    int N;  // > 0: workgroups, one per agent
    const simaps_agent *agents;
    const simaps_env *envs;
    const simaps_robot *robots;
    const double *paths;
    const uint8_t *occupancy;
    const float *overhead;
    // state: [N, C, 96, 96] (chw) or [N, 96, 96, C] elements of state_dtype (SIMAPS_STATE_*: float32 as
    // float *, bf16 / fp16 as uint16_t *).  With dest it is the caller's store, [capacity, ...] in the
    // same layout, and dest[n] (DEVICE [N]) is agent n's row: -1 skips the agent, a row outside
    // [0, capacity) is reported as SIMAPS_FAULT_DESCRIPTOR and nothing is written.  dest == nullptr:
    // stack n goes to row n (capacity unused) and faults are posted under SIMAPS_K_GET_STATE.
    void *state;
    int state_dtype;
    int64_t capacity;
    const int64_t *dest;
    int C;             // simaps_num_channels of cfg
    simaps_debug dbg;  // the call's, all NULL without one; the instances take none
    unsigned *fault;   // the context's fault word
    // the state cache (state_cache.h): cache_records records, or nullptr / 0; read only by the cached
    // launchers, which get_state_impl calls only with both set
    void *cache;
    int cache_records;
    hipStream_t stream;
};
}  // namespace simaps
