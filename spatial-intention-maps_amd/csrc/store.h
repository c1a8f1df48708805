// simaps_get_state_into / simaps_get_state_mixed_as (include/simaps_store.h): the launchers of
// get_state_into_kernel in float32, bf16 and fp16 and of get_state_mixed_kernel in bf16 and fp16.
// One translation unit per element type (simaps_store_f32.hip, simaps_store_bf16.hip,
// simaps_store_f16.hip, all simaps_store.inc), so that adding them cannot change the code the
// compiler makes of the kernels in simaps.hip, simaps_mixed.hip and the simaps_state16 units.
#pragma once
#include <hip/hip_runtime.h>
#include "geom.h"
#include "mixed.h"
#include "simaps.h"

namespace simaps_store {
// store: [capacity, C, 96, 96] (chw) or [capacity, 96, 96, C] elements; dest: DEVICE [N], -1 = skip;
// the other arguments are get_state_kernel's
void launch_get_state_into_f32(const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                               const simaps_env *envs, const simaps_robot *robots, const double *paths,
                               const uint8_t *occupancy, const float *overhead, float *store, int64_t capacity,
                               const int64_t *dest, int C, const simaps_debug &dbg, unsigned *fault,
                               hipStream_t stream);
void launch_get_state_into_bf16(const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                                const simaps_env *envs, const simaps_robot *robots, const double *paths,
                                const uint8_t *occupancy, const float *overhead, uint16_t *store, int64_t capacity,
                                const int64_t *dest, int C, const simaps_debug &dbg, unsigned *fault,
                                hipStream_t stream);
void launch_get_state_into_f16(const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                               const simaps_env *envs, const simaps_robot *robots, const double *paths,
                               const uint8_t *occupancy, const float *overhead, uint16_t *store, int64_t capacity,
                               const int64_t *dest, int C, const simaps_debug &dbg, unsigned *fault,
                               hipStream_t stream);
// the arguments of simaps_mixed::launch_get_state_mixed, state in 16-bit elements (out_off in elements)
void launch_get_state_mixed_bf16(const simaps_mixed::MixedCfgs &mx, const simaps::Geometry &geo, int N,
                                 const simaps_agent *agents, const int32_t *agent_cfg, const simaps_env *envs,
                                 const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                                 const int64_t *map_off, const float *overhead, uint16_t *state, const int64_t *out_off,
                                 unsigned *fault, hipStream_t stream);
void launch_get_state_mixed_f16(const simaps_mixed::MixedCfgs &mx, const simaps::Geometry &geo, int N,
                                const simaps_agent *agents, const int32_t *agent_cfg, const simaps_env *envs,
                                const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                                const int64_t *map_off, const float *overhead, uint16_t *state, const int64_t *out_off,
                                unsigned *fault, hipStream_t stream);
}  // namespace simaps_store
