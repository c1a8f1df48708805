// get_state_bf16_kernel / get_state_f16_kernel (simaps_get_state_as, include/simaps_state16.h):
// get_state_kernel writing its stack as bf16 or fp16.  The body is get_state_kernel's
// (get_state_body.inc with GS_MIXED 0); SIMAPS_STATE16 (1 = bf16, 2 = fp16, set by the including
// simaps_state_bf16.hip / simaps_state_f16.hip) makes RenderCtx::put / put4 round each float32 value
// to nearest-even at the store, and nothing else: debug outputs, the receptacle cache and faults
// (kernel id SIMAPS_K_GET_STATE) are the float32 kernel's.  Built into libsimaps.so beside
// simaps.hip, whose device helpers it includes (SIMAPS_DEVICE_ONLY: no other kernel, no C ABI).
#if SIMAPS_STATE16 != 1 && SIMAPS_STATE16 != 2
#error "SIMAPS_STATE16 must be 1 (bf16) or 2 (fp16)"
#endif
#define SIMAPS_DEVICE_ONLY
#include "simaps.hip"
#include "state16.h"

#if SIMAPS_STATE16 == 1
#define GS16_KERNEL get_state_bf16_kernel
#define GS16_LAUNCH launch_get_state_bf16
#else
#define GS16_KERNEL get_state_f16_kernel
#define GS16_LAUNCH launch_get_state_f16
#endif

namespace {
__global__ void __launch_bounds__(NT) GS16_KERNEL(
    simaps_config cfg, Geometry geo, const simaps_agent *__restrict__ agents, const simaps_env *__restrict__ envs,
    const simaps_robot *__restrict__ robots, const double *__restrict__ paths, const uint8_t *__restrict__ occupancy,
    const float *__restrict__ overhead, uint16_t *__restrict__ state, int C, simaps_debug dbg, unsigned *fault)
{
#define GS_MIXED 0
#include "get_state_body.inc"
#undef GS_MIXED
}
}  // namespace

namespace simaps_state16 {
void GS16_LAUNCH(const simaps::GetStateLaunch &L)
{
    hipLaunchKernelGGL(GS16_KERNEL, dim3(L.N), dim3(NT), 0, L.stream, *L.cfg, *L.geo, L.agents, L.envs, L.robots,
                       L.paths, L.occupancy, L.overhead, (uint16_t *)L.state, L.C, L.dbg, L.fault);
}
}  // namespace simaps_state16
