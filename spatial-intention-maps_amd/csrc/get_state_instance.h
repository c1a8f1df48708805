// What the kernels around get_state_body.inc share ahead of it: the fixed fields of a compile-time
// instance, and the store row of a launch into a store.  Included after simaps.hip (SIMAPS_DEVICE_ONLY)
// by the units that build such kernels.  The forms are the ones that leave each kernel's code as it
// was with the text pasted in (tools/isa_sha.py; DESIGN.md section 5 lists those that do not).
#pragma once

namespace {
// The fixed fields of the standard stack: instance S1 (REC 1) / S2 (REC 0), REC being
// use_shortest_path_to_receptacle_map, and with RH != 0 (GS_SPEC_ROOM) the room class's map shape
// MH x MW and room RH x RW; RH == 0 leaves the shape at its run-time values.  The kernel keeps its own
// `simaps_config cfg = cfg_in;` and hands the local in: the constants fold through every helper.
template <int REC, int MH, int MW, int RH, int RW>
__device__ __forceinline__ void fix_instance_fields(simaps_config &cfg)
{
    cfg.use_robot_map = 1;
    cfg.use_distance_to_receptacle_map = 0;
    cfg.use_shortest_path_to_receptacle_map = REC;
    cfg.use_shortest_path_map = 1;
    cfg.use_intention_map = 1;
    cfg.use_history_map = 0;
    cfg.use_intention_channels = 0;
    cfg.layout_chw = 1;
    if (RH) {
        cfg.H = MH;
        cfg.W = MW;
        cfg.room_h = RH;
        cfg.room_w = RW;
    }
}

// The workgroup's row of the caller's store, dest[blockIdx.x]: one value per workgroup, read before
// anything else.  false: the workgroup returns at once, having touched nothing -- -1 is "not this
// agent" (nothing written, nothing posted), a row outside [0, capacity) is reported as
// SIMAPS_FAULT_DESCRIPTOR under SIMAPS_K_GET_STATE_INTO.  dest is not NULL: a kernel that also serves
// launches without a store tests that itself (`if (dest && !store_row(...)) return;`).
__device__ __forceinline__ bool store_row(const int64_t *__restrict__ dest, int64_t capacity, unsigned *fault,
                                          int64_t &row)
{
    row = dest[blockIdx.x];
    if (row == -1) return false;
    if ((uint64_t)row >= (uint64_t)capacity) {
        if (threadIdx.x == 0) post_faults(fault, SIMAPS_FAULT_DESCRIPTOR, SIMAPS_K_GET_STATE_INTO, blockIdx.x);
        return false;
    }
    return true;
}
}  // namespace
