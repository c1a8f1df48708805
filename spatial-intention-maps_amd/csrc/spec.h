// Compile-time instances of get_state_kernel (include/simaps_spec.h): which instance a call takes,
// and their launcher.  The kernels live in their own translation unit (simaps_spec.hip), so that
// adding them cannot change the code the compiler makes of the generic kernel in simaps.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "get_state_launch.h"
#include "simaps_spec.h"
#include "simaps_spec_room.h"

namespace simaps_spec {
// The instance whose fixed fields match cfg, by truthiness as the device code tests them
// (SIMAPS_SPEC_*); SIMAPS_SPEC_GENERIC when none does or the call asks for a simaps_debug output.
inline int instance_of(const simaps_config &c, bool has_debug)
{
    if (has_debug || !c.use_robot_map || c.use_distance_to_receptacle_map || !c.use_shortest_path_map ||
        !c.use_intention_map || c.use_history_map || c.use_intention_channels || !c.layout_chw)
        return SIMAPS_SPEC_GENERIC;
    return c.use_shortest_path_to_receptacle_map ? SIMAPS_SPEC_S1 : SIMAPS_SPEC_S2;
}

// The room class (include/simaps_spec_room.h) whose map shape and room equal cfg's exactly; the
// caller has found instance_of(cfg, ...) to be S1 or S2.
inline int room_class_of(const simaps_config &c)
{
    if (c.H == SIMAPS_ROOM_SMALL_H && c.W == SIMAPS_ROOM_SMALL_W && c.room_h == SIMAPS_ROOM_SMALL_RH &&
        c.room_w == SIMAPS_ROOM_SMALL_RW)
        return SIMAPS_ROOM_SMALL;
    return SIMAPS_ROOM_NONE;
}

inline bool any_debug(const simaps_debug &d)
{
    return d.cspace || d.sources || d.dist || d.status || d.rec_cache;
}

// id: SIMAPS_SPEC_S1 / SIMAPS_SPEC_S2, as instance_of(cfg, false) gave it; float32, no store
void launch_get_state(int id, const simaps::GetStateLaunch &L);
#if defined(SIMAPS_PHASE_STAMPS) || defined(SIMAPS_LIGHT_STAMPS)
// diagnostic builds: the instances' stamp table (simaps_debug_read_stamps reads the table of the
// kernel that the last get_state launch took)
int read_stamps(unsigned long long *host_out);
#endif
}  // namespace simaps_spec
