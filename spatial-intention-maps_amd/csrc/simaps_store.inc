// The kernels of include/simaps_store.h, one element type per including translation unit
// (SIMAPS_STORE_DTYPE 0 = float32: simaps_store_f32.hip; 1 = bf16: simaps_store_bf16.hip; 2 = fp16:
// simaps_store_f16.hip -- RenderCtx has one element type per unit, chosen by SIMAPS_STATE16).
//
// get_state_into_{f32,bf16,f16}_kernel (simaps_get_state_into): get_state_kernel with its stack's row
// of the caller's store read from dest[blockIdx.x] on the device.  -1 skips the agent (the workgroup
// returns before it touches anything), a row outside [0, capacity) is reported as
// SIMAPS_FAULT_DESCRIPTOR and nothing is written.  The body is get_state_kernel's
// (get_state_body.inc with GS_MIXED 0 and GS_INTO): the row's 64-bit offset goes onto the base
// pointer, the body's own 32-bit offsets stay per stack; its faults go under SIMAPS_K_GET_STATE_INTO.
//
// get_state_mixed_{bf16,f16}_kernel (simaps_get_state_mixed_as; the 16-bit units only):
// get_state_mixed_kernel (simaps_mixed.hip) with the 16-bit stack, GS_MIXED 1 and SIMAPS_STATE16.
//
// Built into libsimaps.so beside simaps.hip, whose device helpers it includes (SIMAPS_DEVICE_ONLY: no
// other kernel, no C ABI).
#if SIMAPS_STORE_DTYPE != 0 && SIMAPS_STORE_DTYPE != 1 && SIMAPS_STORE_DTYPE != 2
#error "SIMAPS_STORE_DTYPE must be 0 (float32), 1 (bf16) or 2 (fp16)"
#endif
#if SIMAPS_STORE_DTYPE != 0
#define SIMAPS_STATE16 SIMAPS_STORE_DTYPE
#endif
#define SIMAPS_DEVICE_ONLY
#include "simaps.hip"
#include "get_state_instance.h"
#include "store.h"

#if SIMAPS_STORE_DTYPE == 0
#define GSI_ELEM float
#define GSI_KERNEL get_state_into_f32_kernel
#define GSI_LAUNCH launch_get_state_into_f32
#elif SIMAPS_STORE_DTYPE == 1
#define GSI_ELEM uint16_t
#define GSI_KERNEL get_state_into_bf16_kernel
#define GSI_LAUNCH launch_get_state_into_bf16
#define GSM_KERNEL get_state_mixed_bf16_kernel
#define GSM_LAUNCH launch_get_state_mixed_bf16
#else
#define GSI_ELEM uint16_t
#define GSI_KERNEL get_state_into_f16_kernel
#define GSI_LAUNCH launch_get_state_into_f16
#define GSM_KERNEL get_state_mixed_f16_kernel
#define GSM_LAUNCH launch_get_state_mixed_f16
#endif

namespace {
__global__ void __launch_bounds__(NT) GSI_KERNEL(
    simaps_config cfg, Geometry geo, const simaps_agent *__restrict__ agents, const simaps_env *__restrict__ envs,
    const simaps_robot *__restrict__ robots, const double *__restrict__ paths, const uint8_t *__restrict__ occupancy,
    const float *__restrict__ overhead, GSI_ELEM *__restrict__ state, int64_t capacity,
    const int64_t *__restrict__ dest, int C, simaps_debug dbg, unsigned *fault)
{
    // the workgroup's row of the store, read before anything else (store_row: get_state_instance.h)
    int64_t into_row;
    if (!store_row(dest, capacity, fault, into_row)) return;
#define GS_MIXED 0
#define GS_INTO 1
#include "get_state_body.inc"
#undef GS_INTO
#undef GS_MIXED
}

#ifdef GSM_KERNEL
__global__ void __launch_bounds__(NT) GSM_KERNEL(
    simaps_mixed::MixedCfgs mx, Geometry geo, const simaps_agent *__restrict__ agents,
    const int32_t *__restrict__ agent_cfg, const simaps_env *__restrict__ envs, const simaps_robot *__restrict__ robots,
    const double *__restrict__ paths, const uint8_t *__restrict__ occupancy, const int64_t *__restrict__ map_off,
    const float *__restrict__ overhead, uint16_t *__restrict__ state, const int64_t *__restrict__ out_off,
    unsigned *fault)
{
    const int k = __builtin_amdgcn_readfirstlane(agent_cfg[blockIdx.x]);
    if ((unsigned)k >= (unsigned)mx.n) {
        // a configuration index past the table: reported, and the workgroup writes nothing (as
        // get_state_mixed_kernel)
        if (threadIdx.x == 0) post_faults(fault, SIMAPS_FAULT_DESCRIPTOR, SIMAPS_K_GET_STATE_MIXED, blockIdx.x);
        return;
    }
    const simaps_config cfg = mx.cfg[k];
    const int C = mx.C[k];
    const simaps_debug dbg = {};
#define GS_MIXED 1
#include "get_state_body.inc"
#undef GS_MIXED
}
#endif
}  // namespace

namespace simaps_store {
void GSI_LAUNCH(const simaps::GetStateLaunch &L)
{
    hipLaunchKernelGGL(GSI_KERNEL, dim3(L.N), dim3(NT), 0, L.stream, *L.cfg, *L.geo, L.agents, L.envs, L.robots, L.paths,
                       L.occupancy, L.overhead, (GSI_ELEM *)L.state, L.capacity, L.dest, L.C, L.dbg, L.fault);
}

#ifdef GSM_KERNEL
void GSM_LAUNCH(const simaps_mixed::MixedLaunch &L)
{
    hipLaunchKernelGGL(GSM_KERNEL, dim3(L.N), dim3(NT), 0, L.stream, *L.mx, *L.geo, L.agents, L.agent_cfg, L.envs, L.robots,
                       L.paths, L.occupancy, L.map_off, L.overhead, (uint16_t *)L.state, L.out_off, L.fault);
}
#endif
}  // namespace simaps_store
