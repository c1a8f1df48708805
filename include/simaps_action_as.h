/* simaps_action_as.h -- the action call of simaps_action.h, simaps_store_new_action, for a policy
 * under autocast and for a captured training step: the Q maps may be bfloat16 or float16 as well as float32, and the
 * epsilon-greedy exploration draw (policies.py:61-62) may be taken on the device.
 *
 * Everything simaps_action.h says of simaps_store_new_action holds here unless stated otherwise:
 * the descriptor errors, the write-back, max_points, the decode / path / finish launches on the
 * caller's stream, the capture rules and the fault kernel id SIMAPS_K_ACTION.  A call with an rng
 * state adds one more launch after the finish kernel: a one-thread kernel that advances the state.
 *
 * The device draw does NOT reproduce Python's `random` stream.  A run that has to follow the
 * reference's draws takes them on the host (simaps.policy_output.select_actions) and passes them as
 * actions_in; the device draw is for a step that stays on the device -- Q maps, actions, descriptors
 * and next states in one stream or one captured graph, with fresh exploration at every replay.
 */
#ifndef SIMAPS_ACTION_AS_H
#define SIMAPS_ACTION_AS_H

#include "simaps_action.h"
#include "simaps_state16.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAPS_ACTION_AS_ABI_VERSION 1

int simaps_action_as_abi_version(void);

/* simaps_store_new_action with these arguments added or changed (every array a DEVICE pointer):
 *   q, q_dtype           agent n's [K_n, 96, 96] block in the element type q_dtype names: SIMAPS_STATE_F32,
 *                        SIMAPS_STATE_BF16 or SIMAPS_STATE_F16 (simaps_state16.h); anything else is
 *                        SIMAPS_EINVAL.  q_off[n] counts ELEMENTS of that type.  A block whose first
 *                        byte is 16-byte aligned is read with 16-byte loads (8 elements of a 16-bit
 *                        type), any other with element-sized loads: same result.  Every value is
 *                        widened exactly to float32 and compared as simaps_store_new_action compares:
 *                        a NaN counts as the greatest value, -0.0 equals +0.0, the lowest index wins
 *                        among equals (which 16-bit outputs have far more often than float32 ones).
 *   eps      [N] float32 may be NULL: no exploration; rng may then be NULL too, and with q_dtype
 *                        SIMAPS_STATE_F32 the call equals simaps_store_new_action bit for bit.
 *                        eps[n] is agent n's exploration probability.  A NaN, a negative value or a
 *                        value above 1 is a descriptor error of agent n, reported as a bad action is:
 *                        out_count 0, SIMAPS_FAULT_DESCRIPTOR, kernel id SIMAPS_K_ACTION, unit n.
 *                        eps without rng is SIMAPS_EINVAL.
 *   rng      uint64_t[2] {seed, step} in device memory, read by the kernels of the call.  Every call
 *                        that launches (N > 0) with an rng advances step by exactly 1, in a kernel of its
 *                        own behind the finish kernel in stream order -- never from the host, so a
 *                        replayed graph advances it too.  N == 0 launches nothing and leaves it alone.
 *   out_explored [N] uint8   may be NULL; 1 where the agent's action came from the draw, else 0.
 *
 * Precedence per agent: actions_in[n] >= 0 is used as given and no draw counts for that agent;
 * otherwise the draw decides; otherwise the arg-max is taken.  An agent whose action is given or
 * drawn does not read its Q block.  q may be NULL only if actions_in is given, as before; an agent
 * with actions_in[n] == -1 that is not drawn and has no q is a bad action.
 *
 * The draw.  Philox4x32-10 (Salmon et al., SC'11) with key (seed & 0xffffffff, seed >> 32) and
 * counter (n, 0, step & 0xffffffff, step >> 32), step as read at the launch, n the agent's index
 * in THIS call; output words w0..w3.  Agent n explores iff (float)(w0 >> 8) * 2^-24 < eps[n],
 * compared in float32: eps == 1 always explores, eps == 0 never does.  Its action is then
 * (uint64_t)w1 * total >> 32 with total = K_n * 9216: multiply-shift without rejection, so a
 * value's probability differs from 1 / total by at most total / 2^32 relative (4.3e-6 for K = 2).
 * The draw is per agent and counter-based: it does not depend on which other agents the launch
 * holds or on their order, only on (seed, step, n, eps[n], K_n).
 *
 * SIMAPS_EINVAL before any device use: an unknown q_dtype, eps without rng, and everything
 * simaps_store_new_action refuses. */
int simaps_store_new_action_as(const simaps_config *cfg, int N, const simaps_agent *agents, const simaps_env *envs,
                               simaps_robot *robots, double *paths, const uint8_t *occupancy, const void *q,
                               int q_dtype, const int64_t *q_off, const int32_t *actions_in, const float *eps,
                               uint64_t *rng, int flags, int max_points, int32_t *out_action, double *out_source,
                               double *out_target, double *out_xy, double *out_heading, int32_t *out_count,
                               uint8_t *out_explored, void *stream);

/* The same through a context (simaps_ctx.h): its fault record, path mode and pool; the plain form is
 * this on the default context. */
int simaps_ctx_store_new_action_as(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                                   const simaps_env *envs, simaps_robot *robots, double *paths,
                                   const uint8_t *occupancy, const void *q, int q_dtype, const int64_t *q_off,
                                   const int32_t *actions_in, const float *eps, uint64_t *rng, int flags,
                                   int max_points, int32_t *out_action, double *out_source, double *out_target,
                                   double *out_xy, double *out_heading, int32_t *out_count, uint8_t *out_explored,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_ACTION_AS_H */
