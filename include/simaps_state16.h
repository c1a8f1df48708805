/* simaps_state16.h -- the state stack rendered directly as bf16 or fp16.
 *
 * simaps_get_state (simaps.h) writes float32.  A policy under bf16 / fp16 autocast and a 16-bit
 * device-resident replay store want the narrow format; instead of a cast pass over the float32
 * batch, simaps_get_state_as has the fused kernel convert each value where it stores it.  The
 * launch, its shapes, its layout (cfg.layout_chw), its debug outputs, the receptacle cache it fills
 * and the faults it posts (kernel id SIMAPS_K_GET_STATE) are those of simaps_get_state; only the
 * element type of `state` differs.
 *
 * Value rule: every element is the IEEE round-to-nearest-even conversion of the float32 value
 * simaps_get_state writes -- fp16 subnormals are kept, overflow goes to +-inf, -0.0 keeps its sign,
 * a float32 subnormal converts like any other value: bit for bit tensor.to(torch.bfloat16 /
 * torch.float16) of the float32 stack.  NaN inputs are unspecified (states contain none).
 *
 * Not covered here: simaps_get_state_mixed stays float32; its 16-bit form is simaps_get_state_mixed_as
 * (simaps_store.h).
 */
#ifndef SIMAPS_STATE16_H
#define SIMAPS_STATE16_H

#include "simaps_ctx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAPS_STATE16_ABI_VERSION 1

/* state_dtype */
#define SIMAPS_STATE_F32 0  /* float32: launches simaps_get_state's kernel */
#define SIMAPS_STATE_BF16 1 /* bfloat16 */
#define SIMAPS_STATE_F16 2  /* IEEE binary16 */

int simaps_state16_abi_version(void);

/* simaps_get_state with the stack's element type chosen by state_dtype (SIMAPS_STATE_*): `state` is a
 * DEVICE pointer to [N, C, 96, 96] (cfg.layout_chw) or [N, 96, 96, C] elements of that type, aligned
 * to 16 bytes; every other argument is simaps_get_state's.
 *
 * SIMAPS_EINVAL before any device use: an unknown state_dtype, a NULL state with N > 0, a state not
 * aligned to 16 bytes, and everything simaps_get_state refuses. */
int simaps_get_state_as(const simaps_config *cfg, int N, const simaps_agent *agents, const simaps_env *envs,
                        const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                        const float *overhead, void *state, int state_dtype, int num_robots_per_env,
                        const simaps_debug *dbg, void *stream);

/* The same through a context (simaps_ctx.h): its fault record and device; the plain form is this on
 * the default context. */
int simaps_ctx_get_state_as(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                            const simaps_env *envs, const simaps_robot *robots, const double *paths,
                            const uint8_t *occupancy, const float *overhead, void *state, int state_dtype,
                            int num_robots_per_env, const simaps_debug *dbg, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_STATE16_H */
