/* simaps_spec_room.h -- the room class of the get_state instance a call takes.
 *
 * Beside the instances S1 / S2 of simaps_spec.h, which fix a configuration's feature flags and layout,
 * libsimaps.so carries twins of both with the map shape (H x W) and the room's size (room_h x room_w)
 * fixed at compile time as well, for the rooms that training runs in launch after launch (DESIGN.md
 * section 5).  A float32 simaps_get_state / simaps_ctx_get_state call takes such a
 * twin when simaps_get_state_instance gives S1 or S2 for it AND its H, W, room_h and room_w equal a
 * class's exactly; a configuration that differs in any of them, by one cell even, takes S1 / S2 as
 * before, and a call with a simaps_debug output the generic kernel.  The room's origin
 * (room_i0 / room_j0), rotate_rounding, line thickness, encodings and scales stay run-time values in
 * every instance.
 * simaps_get_state_instance keeps reporting S1 / S2 for these calls: the room class is reported here.
 * Results, faults and errors are those of the generic kernel bit for bit; only the launch time differs.
 *
 *   class               H x W      room_h x room_w   configurations
 *   SIMAPS_ROOM_SMALL   184 x 232  44 x 92           every small_* room (lifting_4-small_divider,
 *                                                    rescue_4-small_empty, ...)
 *   SIMAPS_ROOM_NONE    any other shape (the 92 x 92 large rooms included): S1 / S2 / generic
 *
 * The query is host-only: it launches nothing and needs no GPU.
 */
#ifndef SIMAPS_SPEC_ROOM_H
#define SIMAPS_SPEC_ROOM_H

#include "simaps_spec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAPS_SPEC_ROOM_ABI_VERSION 1

/* room classes */
#define SIMAPS_ROOM_NONE 0  /* no room-class instance: S1 / S2 / the generic kernel as simaps_spec.h says */
#define SIMAPS_ROOM_SMALL 1 /* the small room */
#define SIMAPS_ROOM_COUNT 2

/* the small room's shape, as simaps_config carries it */
#define SIMAPS_ROOM_SMALL_H 184
#define SIMAPS_ROOM_SMALL_W 232
#define SIMAPS_ROOM_SMALL_RH 44
#define SIMAPS_ROOM_SMALL_RW 92

int simaps_spec_room_abi_version(void);

/* The room class (SIMAPS_ROOM_*) of the instance a float32 simaps_get_state call with this
 * configuration would launch; has_debug as in simaps_get_state_instance.  SIMAPS_ROOM_NONE whenever
 * simaps_get_state_instance gives SIMAPS_SPEC_GENERIC.  SIMAPS_EINVAL for a NULL cfg. */
int simaps_get_state_room_class(const simaps_config *cfg, int has_debug);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_SPEC_ROOM_H */
