// Compile-time instances of get_state_kernel for the store launches and the 16-bit launches
// (include/simaps_spec_store.h): which launches take one, and their launchers.  The kernels live in
// one translation unit per element type (simaps_spec_store_f32.hip, simaps_spec_store_bf16.hip,
// simaps_spec_store_f16.hip, all simaps_spec_store.inc), so that adding them cannot change the code
// the compiler makes of any other kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "geom.h"
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
// (spec.h room_class_of).  store / capacity / dest: get_state_into_kernel's.  The 16-bit launchers
// take dest == nullptr for simaps_get_state_as: stack n goes to row n of `store` (capacity unused)
// and faults are posted under SIMAPS_K_GET_STATE.
void launch_f32(int id, const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                const simaps_env *envs, const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                const float *overhead, float *store, int64_t capacity, const int64_t *dest, int C, unsigned *fault,
                hipStream_t stream);
void launch_bf16(int id, const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                 const simaps_env *envs, const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                 const float *overhead, uint16_t *store, int64_t capacity, const int64_t *dest, int C, unsigned *fault,
                 hipStream_t stream);
void launch_f16(int id, const simaps_config &cfg, const simaps::Geometry &geo, int N, const simaps_agent *agents,
                const simaps_env *envs, const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                const float *overhead, uint16_t *store, int64_t capacity, const int64_t *dest, int C, unsigned *fault,
                hipStream_t stream);
}  // namespace simaps_spec_store
