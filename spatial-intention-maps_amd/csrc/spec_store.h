// Compile-time instances of get_state_kernel for the store launches and the 16-bit launches
// (include/simaps_spec_store.h): which launches take one, and their launchers.  The kernels live in
// one translation unit per element type (simaps_spec_store_f32.hip, simaps_spec_store_bf16.hip,
// simaps_spec_store_f16.hip, all simaps_spec_store.inc), so that adding them cannot change the code
// the compiler makes of any other kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "get_state_launch.h"
#include "simaps_spec_store.h"
#include "spec.h"

namespace simaps_spec_store {
// The instance (SIMAPS_SPEC_*) that a launch of element type state_dtype takes, `into` a store or
// not.  Both families of launches -- simaps_get_state_into (float32, bf16, fp16) and simaps_get_state_as
// (bf16, fp16) -- are dispatched to instances as a whole (DESIGN.md section 5 has the timings that
// decided it), and float32 without a store is simaps_get_state's own choice (spec.h): the same
// instance in every case.
inline int instance_as(const simaps_config &c, int /*state_dtype*/, bool /*into*/, bool has_debug)
{
    return simaps_spec::instance_of(c, has_debug);
}

// id: SIMAPS_SPEC_S1 / SIMAPS_SPEC_S2, as instance_as gave it; the room-class twin is chosen inside
// (spec.h room_class_of).  One function per element type's unit; only the 16-bit ones take
// L.dest == nullptr (simaps_get_state_as).
void launch_f32(int id, const simaps::GetStateLaunch &L);
void launch_bf16(int id, const simaps::GetStateLaunch &L);
void launch_f16(int id, const simaps::GetStateLaunch &L);
inline void launch(int id, const simaps::GetStateLaunch &L)
{
    (L.state_dtype == SIMAPS_STATE_F32 ? launch_f32 : L.state_dtype == SIMAPS_STATE_BF16 ? launch_bf16 : launch_f16)(id, L);
}
}  // namespace simaps_spec_store
