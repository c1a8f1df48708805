// simaps_get_state_as (include/simaps_state16.h): the launchers of the bf16 / fp16 instantiations of
// get_state_kernel.  Each lives in its own translation unit (simaps_state_bf16.hip,
// simaps_state_f16.hip, both simaps_state16.inc), so that adding them cannot change the code the
// compiler makes of the float32 kernels in simaps.hip and simaps_mixed.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "geom.h"
#include "simaps.h"

namespace simaps_state16 {
// state: [N, C, 96, 96] (chw) or [N, 96, 96, C] 16-bit elements; the arguments of get_state_kernel
void launch_get_state_bf16(const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                           const simaps_env *envs, const simaps_robot *robots, const double *paths,
                           const uint8_t *occupancy, const float *overhead, uint16_t *state, int C,
                           const simaps_debug &dbg, unsigned *fault, hipStream_t stream);
void launch_get_state_f16(const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                          const simaps_env *envs, const simaps_robot *robots, const double *paths,
                          const uint8_t *occupancy, const float *overhead, uint16_t *state, int C,
                          const simaps_debug &dbg, unsigned *fault, hipStream_t stream);
}  // namespace simaps_state16
