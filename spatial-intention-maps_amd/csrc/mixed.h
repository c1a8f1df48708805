// simaps_get_state_mixed: the launch-wide table of configurations (at most SIMAPS_MAX_MIXED) that
// travels in the kernel arguments, and the launcher of get_state_mixed_kernel.  The kernel lives in
// its own translation unit (simaps_mixed.hip), so that adding it cannot change the code the
// compiler makes of the single-configuration kernels in simaps.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "geom.h"
#include "simaps.h"

namespace simaps_mixed {
struct MixedCfgs {
    simaps_config cfg[SIMAPS_MAX_MIXED];
    int C[SIMAPS_MAX_MIXED];  // simaps_num_channels of each configuration
    int n;                    // configurations in use
};
// One mixed launch as get_state_mixed_impl (simaps.hip) has checked it, for the float32 launcher here
// and the 16-bit ones of store.h (as simaps::GetStateLaunch, get_state_launch.h, for the other families)
struct MixedLaunch {
    const MixedCfgs *mx;
    const simaps::Geometry *geo;
    int N;  // > 0: workgroups, one per agent
    const simaps_agent *agents;
    const int32_t *agent_cfg;  // DEVICE [N]: agent n's configuration, an index into mx
    const simaps_env *envs;
    const simaps_robot *robots;
    const double *paths;
    const uint8_t *occupancy;
    const int64_t *map_off;  // DEVICE: each map slot's offset into occupancy / overhead
    const float *overhead;
    void *state;  // elements of state_dtype (SIMAPS_STATE_*: float32 as float *, bf16 / fp16 as uint16_t *)
    int state_dtype;
    const int64_t *out_off;  // DEVICE [N]: agent n's stack's offset into state, in elements
    unsigned *fault;         // the context's fault word
    hipStream_t stream;
};
void launch_get_state_mixed(const MixedLaunch &L);  // float32
}  // namespace simaps_mixed
