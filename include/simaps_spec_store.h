/* simaps_spec_store.h -- which get_state kernel a store launch or a 16-bit launch takes.
 *
 * simaps_spec.h / simaps_spec_room.h say which compile-time instance (S1 / S2, and its room-class
 * twin) a float32 simaps_get_state call launches.  The same instances exist for the other entry
 * points of the single-configuration kernel:
 *
 *   simaps_get_state_into / simaps_ctx_get_state_into   float32, bf16, fp16     (simaps_store.h)
 *   simaps_get_state_as / simaps_ctx_get_state_as       bf16, fp16              (simaps_state16.h)
 *
 * by the rule of simaps_spec.h: the instance whose fixed fields match the call's simaps_config, when
 * the call asks for no simaps_debug output (dbg NULL, or every pointer of it NULL, rec_cache
 * included), and its room-class twin where H, W, room_h and room_w equal a class's exactly; any other
 * call takes the entry point's generic kernel.  Results, the store rows touched, faults (fault word,
 * kernel id and unit) and errors are those of the generic kernel of the entry point bit for bit; only
 * the launch time differs.  The mixed launches always take their own generic kernels.
 *
 * The queries below name an entry point by its element type and by whether it writes into a store.
 * They are host-only: they launch nothing and need no GPU.
 */
#ifndef SIMAPS_SPEC_STORE_H
#define SIMAPS_SPEC_STORE_H

#include "simaps_spec.h"
#include "simaps_spec_room.h"
#include "simaps_state16.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAPS_SPEC_STORE_ABI_VERSION 1

int simaps_spec_store_abi_version(void);

/* The id (SIMAPS_SPEC_*) of the kernel that a call with this configuration would launch through the
 * entry point of element type state_dtype (SIMAPS_STATE_F32 / _BF16 / _F16): simaps_get_state_into
 * where into != 0, simaps_get_state (float32) or simaps_get_state_as (16-bit) where into == 0.
 * has_debug as in simaps_get_state_instance.  For SIMAPS_STATE_F32 with into == 0 the answer is
 * simaps_get_state_instance's.  SIMAPS_EINVAL for a NULL cfg or an unknown state_dtype. */
int simaps_get_state_instance_as(const simaps_config *cfg, int state_dtype, int into, int has_debug);

/* The room class (SIMAPS_ROOM_*) of that kernel: SIMAPS_ROOM_NONE whenever
 * simaps_get_state_instance_as gives SIMAPS_SPEC_GENERIC.  For SIMAPS_STATE_F32 with into == 0 the
 * answer is simaps_get_state_room_class's.  SIMAPS_EINVAL as above. */
int simaps_get_state_room_class_as(const simaps_config *cfg, int state_dtype, int into, int has_debug);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_SPEC_STORE_H */
