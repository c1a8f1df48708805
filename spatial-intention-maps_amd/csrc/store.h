// simaps_get_state_into / simaps_get_state_mixed_as (include/simaps_store.h): the launchers of
// get_state_into_kernel in float32, bf16 and fp16 and of get_state_mixed_kernel in bf16 and fp16.
// One translation unit per element type (simaps_store_f32.hip, simaps_store_bf16.hip,
// simaps_store_f16.hip, all simaps_store.inc), so that adding them cannot change the code the
// compiler makes of the kernels in simaps.hip, simaps_mixed.hip and the simaps_state16 units.
#pragma once
#include <hip/hip_runtime.h>
#include "get_state_launch.h"
#include "mixed.h"
#include "simaps.h"

namespace simaps_store {
// one function per element type's unit; L.dest is set (get_state_launch.h)
void launch_get_state_into_f32(const simaps::GetStateLaunch &L);
void launch_get_state_into_bf16(const simaps::GetStateLaunch &L);
void launch_get_state_into_f16(const simaps::GetStateLaunch &L);
inline void launch_get_state_into(const simaps::GetStateLaunch &L)
{
    (L.state_dtype == SIMAPS_STATE_F32    ? launch_get_state_into_f32
     : L.state_dtype == SIMAPS_STATE_BF16 ? launch_get_state_into_bf16
                                          : launch_get_state_into_f16)(L);
}
// simaps_mixed::launch_get_state_mixed with the state in 16-bit elements: L.state_dtype is bf16 or fp16
void launch_get_state_mixed_bf16(const simaps_mixed::MixedLaunch &L);
void launch_get_state_mixed_f16(const simaps_mixed::MixedLaunch &L);
inline void launch_get_state_mixed16(const simaps_mixed::MixedLaunch &L)
{
    (L.state_dtype == SIMAPS_STATE_BF16 ? launch_get_state_mixed_bf16 : launch_get_state_mixed_f16)(L);
}
}  // namespace simaps_store
