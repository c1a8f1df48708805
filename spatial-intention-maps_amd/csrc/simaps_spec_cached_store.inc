// The cached get_state instance for the store launches and the 16-bit launches
// (include/simaps_state_cache_store.h, state_cache_store.h), one element type per including translation
// unit (SIMAPS_STORE_DTYPE 0 = float32: simaps_spec_cached_store_f32.hip; 1 = bf16: _bf16.hip; 2 = fp16:
// _f16.hip -- RenderCtx has one element type per unit, chosen by SIMAPS_STATE16).
//
// Each unit holds one kernel: the twin of simaps_spec_store.inc's S1 small-room instance
// GSS_KERNEL<1, 184, 232, 44, 92> with the state cache.  Its body is get_state_body.inc with
//   - GS_SPEC and GS_CACHED: simaps_spec_cached.hip's sweep track, verdict, 8-or-12 barrier and LDS-DMA,
//     which this file includes as they are (GS_CACHED_DEVICE: the device code without that unit's kernel
//     and launcher), so the record's bytes and the hit / miss rule are that kernel's;
//   - GS_INTO 1 for the store row, and SIMAPS_STATE16 for the element type, as in simaps_spec_store.inc.
// The render waves' stores are narrower in the 16-bit units, nothing else: sc_retire_array still sits
// ahead of render_maps' stores (get_state_body.inc), where the joining wave has issued nothing but its DMA.
//
// Order inside a workgroup: dest[blockIdx.x] is read first.  A workgroup with -1, or with a row outside
// [0, capacity), returns before the body -- so before cache_preload: it loads nothing from its record,
// bumps no counter and rewrites nothing (the row outside the store posts SIMAPS_FAULT_DESCRIPTOR under
// SIMAPS_K_GET_STATE_INTO first).  The 16-bit kernels also serve simaps_get_state_as_cached: dest == NULL,
// stack n at row n, faults under SIMAPS_K_GET_STATE (GS_INTO_KID).  The float32 kernel serves the store
// launch only (float32 without a store is simaps_spec_cached.hip's).
#if SIMAPS_STORE_DTYPE != 0 && SIMAPS_STORE_DTYPE != 1 && SIMAPS_STORE_DTYPE != 2
#error "SIMAPS_STORE_DTYPE must be 0 (float32), 1 (bf16) or 2 (fp16)"
#endif
#if SIMAPS_STORE_DTYPE != 0
#define SIMAPS_STATE16 SIMAPS_STORE_DTYPE
#endif
#define GS_CACHED_DEVICE
#include "simaps_spec_cached.hip"
#include "state_cache_store.h"

#if SIMAPS_STORE_DTYPE == 0
#define GSC_ELEM float
#define GSC_KERNEL get_state_cached_into_f32_kernel
#define GSC_LAUNCH launch_f32
#elif SIMAPS_STORE_DTYPE == 1
#define GSC_ELEM uint16_t
#define GSC_KERNEL get_state_cached_into_bf16_kernel
#define GSC_LAUNCH launch_bf16
#define GSC_PLAIN
#else
#define GSC_ELEM uint16_t
#define GSC_KERNEL get_state_cached_into_f16_kernel
#define GSC_LAUNCH launch_f16
#define GSC_PLAIN
#endif

namespace {
// MH x MW / RH x RW: get_state_cached_kernel's (simaps_spec_cached.hip)
template <int MH, int MW, int RH, int RW>
__global__ void __launch_bounds__(NT) GSC_KERNEL(
    simaps_config cfg_in, Geometry geo, const simaps_agent *__restrict__ agents, const simaps_env *__restrict__ envs,
    const simaps_robot *__restrict__ robots, const double *__restrict__ paths, const uint8_t *__restrict__ occupancy,
    const float *__restrict__ overhead, GSC_ELEM *__restrict__ state, int64_t capacity,
    const int64_t *__restrict__ dest, int C, unsigned *fault, char *cache, int cache_records)
{
    // the workgroup's row of the store, read before anything else, the record included (store_row:
    // get_state_instance.h; a workgroup that returns here leaves its record untouched)
#ifdef GSC_PLAIN
    int64_t into_row = blockIdx.x;  // (simaps_get_state_as_cached: no dest, stack n at row n)
    if (dest && !store_row(dest, capacity, fault, into_row)) return;
#else
    int64_t into_row;
    if (!store_row(dest, capacity, fault, into_row)) return;
#endif
    simaps_config cfg = cfg_in;
    fix_instance_fields<1, MH, MW, RH, RW>(cfg);  // (instance S1 in the room class, as get_state_cached_kernel)
    const simaps_debug dbg = {};
#define GS_MIXED 0
#define GS_INTO 1
#ifdef GSC_PLAIN
#define GS_INTO_KID (dest ? SIMAPS_K_GET_STATE_INTO : SIMAPS_K_GET_STATE)
#endif
#include "get_state_body.inc"
#undef GS_INTO_KID
#undef GS_INTO
#undef GS_MIXED
}
}  // namespace

namespace simaps_state_cache_store {
void GSC_LAUNCH(const simaps::GetStateLaunch &L)
{
    constexpr int MH = SIMAPS_ROOM_SMALL_H, MW = SIMAPS_ROOM_SMALL_W, RH = SIMAPS_ROOM_SMALL_RH, RW = SIMAPS_ROOM_SMALL_RW;
    hipLaunchKernelGGL((GSC_KERNEL<MH, MW, RH, RW>), dim3(L.N), dim3(NT), 0, L.stream, *L.cfg, *L.geo, L.agents, L.envs,
                       L.robots, L.paths, L.occupancy, L.overhead, (GSC_ELEM *)L.state, L.capacity, L.dest, L.C, L.fault,
                       (char *)L.cache, L.cache_records);
}
}  // namespace simaps_state_cache_store
