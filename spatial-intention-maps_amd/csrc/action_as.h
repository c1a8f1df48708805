// simaps_store_new_action_as (include/simaps_action_as.h): the launchers of its decode kernel (float32,
// bf16 and fp16 Q maps, the exploration draw), its finish kernel and the kernel that advances the rng
// state.  They live in their own translation unit (simaps_action_as.hip), so that adding them cannot
// change the code the compiler makes of the kernels in simaps.hip; the path launch between them is
// simaps.hip's own.
#pragma once
#include <hip/hip_runtime.h>
#include "simaps_action_as.h"

namespace simaps_action_as {
// q_dtype: SIMAPS_STATE_*, checked by the caller.  eps and rng: both NULL, or rng given.
void launch_decode(int q_dtype, int N, const simaps_agent *agents, const simaps_env *envs, const simaps_robot *robots,
                   const void *q, const int64_t *q_off, const int32_t *actions_in, const float *eps,
                   const uint64_t *rng, int flags, int max_points, int32_t *out_action, double *out_source,
                   double *out_target, double *out_xy, int32_t *out_count, uint8_t *out_explored, unsigned *fault,
                   hipStream_t stream);
// ee[t]: END_EFFECTOR_LOCATION + CUBE_WIDTH / 2 of robot class t.  With an rng, the advance kernel follows.
void launch_finish(int N, const simaps_agent *agents, const simaps_env *envs, simaps_robot *robots, double *paths,
                   const int32_t *actions_in, const float *eps, uint64_t *rng, bool have_q, int flags, int max_points,
                   const double ee[4], const double *out_target, double *out_xy, double *out_heading,
                   int32_t *out_count, hipStream_t stream);
}  // namespace simaps_action_as
