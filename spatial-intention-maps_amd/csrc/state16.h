// simaps_get_state_as (include/simaps_state16.h): the launchers of the bf16 / fp16 instantiations of
// get_state_kernel.  Each lives in its own translation unit (simaps_state_bf16.hip,
// simaps_state_f16.hip, both simaps_state16.inc), so that adding them cannot change the code the
// compiler makes of the float32 kernels in simaps.hip and simaps_mixed.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "get_state_launch.h"
#include "simaps.h"

namespace simaps_state16 {
// one function per element type's unit; L.state_dtype is bf16 or fp16 and L.dest unused (get_state_launch.h)
void launch_get_state_bf16(const simaps::GetStateLaunch &L);
void launch_get_state_f16(const simaps::GetStateLaunch &L);
inline void launch_get_state(const simaps::GetStateLaunch &L)
{
    (L.state_dtype == SIMAPS_STATE_BF16 ? launch_get_state_bf16 : launch_get_state_f16)(L);
}
}  // namespace simaps_state16
