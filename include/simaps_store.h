/* simaps_store.h -- states rendered into a caller-owned store at slots chosen on the device, and the
 * mixed-configuration launch in bf16 / fp16.
 *
 * simaps_get_state and simaps_get_state_as write agent n's stack to row n of a dense [N, ...] batch.
 * What outlives the step (a replay store, a ring of recent observations) then needs a copy pass, and
 * rendering only the agents that act needs a new agent list from the host.  simaps_get_state_into
 * takes both decisions from a DEVICE array instead: dest[n] is the row of `store` that agent n's
 * stack goes to, or -1 for "do not render agent n".  It is one launch of the fused kernel and nothing
 * else -- no pass over dest, no synchronisation -- so a captured graph serves every step, whichever
 * agents the device-side dest names that step.
 *
 * Per agent n (one workgroup), with dest[n] read once on the device:
 *   -1                 the workgroup returns at once: it writes nothing, posts nothing, and leaves its
 *                      rows of the debug outputs and its receptacle cache record untouched;
 *   in [0, capacity)   agent n is rendered exactly as simaps_get_state_as renders it (values, layout,
 *                      debug outputs indexed by n, receptacle cache, descriptor clamping); its stack
 *                      goes to store + dest[n] * 96 * 96 * C elements (a 64-bit offset: the store may
 *                      be larger than 4 GiB);
 *   anything else      SIMAPS_FAULT_DESCRIPTOR is posted for unit n, and the workgroup writes nothing.
 * Every fault of this launch is posted under kernel id SIMAPS_K_GET_STATE_INTO (simaps_ctx.h).
 *
 * Contract: the non-negative values of dest must be distinct.  Two agents with the same destination
 * race for the row (each element holds one of the two stacks' values); this is not detected.
 *
 * simaps_get_state_mixed_as is simaps_get_state_mixed (simaps.h) with the element type of `state`
 * chosen as in simaps_get_state_as (simaps_state16.h): the same launch, out_off still in elements,
 * each value the round-to-nearest-even conversion of the float32 one, faults under
 * SIMAPS_K_GET_STATE_MIXED.  It has no skip value.
 */
#ifndef SIMAPS_STORE_H
#define SIMAPS_STORE_H

#include "simaps_state16.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAPS_STORE_ABI_VERSION 1

int simaps_store_abi_version(void);

/* `store` is a DEVICE pointer to [capacity, C, 96, 96] (cfg.layout_chw) or [capacity, 96, 96, C]
 * elements of state_dtype (SIMAPS_STATE_*), aligned to 16 bytes; `dest` is a DEVICE pointer to N
 * int64 values, read by the kernel (it may be written by earlier work on the same stream, a captured
 * graph's replays included).  Every other argument is simaps_get_state's; dbg->rec_cache is honoured
 * as there, and a skipped or refused agent's record is not written.
 *
 * SIMAPS_EINVAL before any device use: an unknown state_dtype; capacity < 0; with N > 0, a NULL dest,
 * and with capacity > 0 too a NULL store or one not aligned to 16 bytes; and everything
 * simaps_get_state refuses.  N == 0 returns 0 without a launch.  With capacity == 0 every dest[n]
 * other than -1 is out of range. */
int simaps_get_state_into(const simaps_config *cfg, int N, const simaps_agent *agents, const simaps_env *envs,
                          const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                          const float *overhead, void *store, int state_dtype, int64_t capacity, const int64_t *dest,
                          int num_robots_per_env, const simaps_debug *dbg, void *stream);

/* The same through a context (simaps_ctx.h): its fault record and device. */
int simaps_ctx_get_state_into(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                              const simaps_env *envs, const simaps_robot *robots, const double *paths,
                              const uint8_t *occupancy, const float *overhead, void *store, int state_dtype,
                              int64_t capacity, const int64_t *dest, int num_robots_per_env, const simaps_debug *dbg,
                              void *stream);

/* simaps_get_state_mixed with `state` a DEVICE pointer to elements of state_dtype, aligned to 16
 * bytes; SIMAPS_STATE_F32 launches simaps_get_state_mixed's own kernel.
 *
 * SIMAPS_EINVAL before any device use: an unknown state_dtype, with N > 0 a NULL state or one not
 * aligned to 16 bytes, and everything simaps_get_state_mixed refuses. */
int simaps_get_state_mixed_as(const simaps_config *cfgs, const int32_t *num_robots_per_env, int n_cfgs, int N,
                              const simaps_agent *agents, const int32_t *agent_cfg, const simaps_env *envs,
                              const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                              const int64_t *map_off, const float *overhead, void *state, const int64_t *out_off,
                              int state_dtype, void *stream);
int simaps_ctx_get_state_mixed_as(simaps_ctx *ctx, const simaps_config *cfgs, const int32_t *num_robots_per_env,
                                  int n_cfgs, int N, const simaps_agent *agents, const int32_t *agent_cfg,
                                  const simaps_env *envs, const simaps_robot *robots, const double *paths,
                                  const uint8_t *occupancy, const int64_t *map_off, const float *overhead, void *state,
                                  const int64_t *out_off, int state_dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_STORE_H */
