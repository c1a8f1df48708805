/* simaps_spec.h -- which get_state kernel a call takes.
 *
 * simaps_get_state's kernel reads the configuration's feature flags and layout at run time.  For the
 * standard stacks libsimaps.so also carries instances of the same kernel body compiled with those
 * fields fixed: simaps_get_state and simaps_ctx_get_state launch the instance
 * whose fixed fields match the call's simaps_config, by truthiness as the device code tests them,
 * when the call asks for no simaps_debug output (dbg NULL, or every pointer of it NULL, rec_cache
 * included); any other call takes the generic kernel.  Room rect, H / W, line thickness, encodings,
 * scales and rotate_rounding do not enter this choice.  Results, faults and errors are those of the
 * generic kernel bit for bit; only the launch time differs.
 *
 * Which configuration takes which kernel (the ids below; the room class: simaps_spec_room.h):
 *   flags and layout of S1, H x W 184 x 232, room 44 x 92 (every small_* room)   S1, room class small
 *   flags and layout of S1, any other shape (the 92 x 92 large rooms, ...)        S1
 *   the same two rows without the shortest-path-to-receptacle map                 S2, room class small / S2
 *   any other flags or layout, or a simaps_debug output                           generic
 * A call of S1 / S2 whose H, W, room_h and room_w equal the small room's exactly launches that
 * instance's twin with those four fixed as well; the id reported here stays S1 / S2.
 *
 * simaps_get_state_as (16-bit stacks) and simaps_get_state_into take instances of their own by the
 * same rule (simaps_spec_store.h has their queries); the mixed launches always take their own
 * generic kernels.
 *
 * The query below is host-only: it launches nothing and needs no GPU.
 */
#ifndef SIMAPS_SPEC_H
#define SIMAPS_SPEC_H

#include "simaps.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAPS_SPEC_ABI_VERSION 1

/* instance ids */
#define SIMAPS_SPEC_GENERIC 0 /* the generic kernel */
#define SIMAPS_SPEC_S1 1      /* robot map, both shortest-path maps, intention map; no history map, no
                                 intention channels, no distance-to-receptacle map; CHW */
#define SIMAPS_SPEC_S2 2      /* S1 without the shortest-path-to-receptacle map */
#define SIMAPS_SPEC_COUNT 3

int simaps_spec_abi_version(void);

/* The id of the kernel a float32 simaps_get_state call with this configuration would launch;
 * has_debug != 0 says that the call passes a simaps_debug with some pointer set.  SIMAPS_EINVAL for a
 * NULL cfg.  The configuration is not validated otherwise (simaps_get_state does that). */
int simaps_get_state_instance(const simaps_config *cfg, int has_debug);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_SPEC_H */
