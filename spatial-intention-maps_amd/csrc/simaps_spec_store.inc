// Compile-time instances of get_state_kernel for the store launches and the 16-bit launches
// (include/simaps_spec_store.h, spec_store.h), one element type per including translation unit
// (SIMAPS_STORE_DTYPE 0 = float32: simaps_spec_store_f32.hip; 1 = bf16: simaps_spec_store_bf16.hip;
// 2 = fp16: simaps_spec_store_f16.hip -- RenderCtx has one element type per unit, chosen by
// SIMAPS_STATE16).
//
// The body is get_state_kernel's (get_state_body.inc with GS_MIXED 0) with three things at once:
//   - the fixed fields of S1 / S2 and of their room-class twins, exactly as get_state_spec_kernel
//     (simaps_spec.hip) fixes them, with the same levers (GS_SPEC);
//   - SIMAPS_STATE16 for the element type;
//   - GS_INTO for the store row: get_state_into_kernel's contract (simaps_store.inc), which is store_row's
//     (get_state_instance.h); the row's 64-bit offset goes onto the base pointer once.
// The 16-bit kernels also serve simaps_get_state_as: launched with dest == NULL, stack n goes to row
// n and every fault is posted under SIMAPS_K_GET_STATE, as get_state_bf16_kernel / get_state_f16_kernel
// post it (one kernel for both launches: half the instances to build; the branch is on a kernel
// argument, wave-uniform).  The float32 kernels serve simaps_get_state_into only (float32 without a
// store is simaps_spec.hip's).
//
// Built into libsimaps.so beside simaps.hip, whose device helpers it includes (SIMAPS_DEVICE_ONLY).
#if SIMAPS_STORE_DTYPE != 0 && SIMAPS_STORE_DTYPE != 1 && SIMAPS_STORE_DTYPE != 2
#error "SIMAPS_STORE_DTYPE must be 0 (float32), 1 (bf16) or 2 (fp16)"
#endif
#if SIMAPS_STORE_DTYPE != 0
#define SIMAPS_STATE16 SIMAPS_STORE_DTYPE
#endif
#define GS_SPEC  // this unit builds instances: the levers of simaps_spec.hip, which documents each
#define GS_ROOM_H RH
#define GS_ROOM_W RW
#define SIMAPS_DEVICE_ONLY
#include "simaps.hip"
#include "get_state_instance.h"
#include "spec_store.h"

#if SIMAPS_STORE_DTYPE == 0
#define GSS_ELEM float
#define GSS_KERNEL get_state_spec_into_f32_kernel
#define GSS_LAUNCH launch_f32
#elif SIMAPS_STORE_DTYPE == 1
#define GSS_ELEM uint16_t
#define GSS_KERNEL get_state_spec_into_bf16_kernel
#define GSS_LAUNCH launch_bf16
#define GSS_PLAIN
#else
#define GSS_ELEM uint16_t
#define GSS_KERNEL get_state_spec_into_f16_kernel
#define GSS_LAUNCH launch_f16
#define GSS_PLAIN
#endif

namespace {
// REC, MH x MW / RH x RW: get_state_spec_kernel's (simaps_spec.hip)
template <int REC, int MH = 0, int MW = 0, int RH = 0, int RW = 0>
__global__ void __launch_bounds__(NT) GSS_KERNEL(
    simaps_config cfg_in, Geometry geo, const simaps_agent *__restrict__ agents, const simaps_env *__restrict__ envs,
    const simaps_robot *__restrict__ robots, const double *__restrict__ paths, const uint8_t *__restrict__ occupancy,
    const float *__restrict__ overhead, GSS_ELEM *__restrict__ state, int64_t capacity,
    const int64_t *__restrict__ dest, int C, unsigned *fault)
{
    // the workgroup's row of the store, read before anything else (store_row: get_state_instance.h)
#ifdef GSS_PLAIN
    int64_t into_row = blockIdx.x;  // (simaps_get_state_as: no dest, stack n at row n)
    if (dest && !store_row(dest, capacity, fault, into_row)) return;
#else
    int64_t into_row;
    if (!store_row(dest, capacity, fault, into_row)) return;
#endif
    simaps_config cfg = cfg_in;
    fix_instance_fields<REC, MH, MW, RH, RW>(cfg);  // (RH != 0: GS_SPEC_ROOM)
    const simaps_debug dbg = {};
#define GS_MIXED 0
#define GS_INTO 1
#ifdef GSS_PLAIN
#define GS_INTO_KID (dest ? SIMAPS_K_GET_STATE_INTO : SIMAPS_K_GET_STATE)
#endif
#include "get_state_body.inc"
#undef GS_INTO_KID
#undef GS_INTO
#undef GS_MIXED
}

using spec_store_kernel_t = void (*)(simaps_config, Geometry, const simaps_agent *, const simaps_env *,
                                     const simaps_robot *, const double *, const uint8_t *, const float *, GSS_ELEM *,
                                     int64_t, const int64_t *, int, unsigned *);
}  // namespace

namespace simaps_spec_store {
void GSS_LAUNCH(int id, const simaps::GetStateLaunch &L)
{
    spec_store_kernel_t k = id == SIMAPS_SPEC_S1 ? GSS_KERNEL<1> : GSS_KERNEL<0>;
    // the room-class twin of S1 / S2 where cfg's shape matches a class exactly (spec.h)
    if (simaps_spec::room_class_of(*L.cfg) == SIMAPS_ROOM_SMALL) {
        constexpr int MH = SIMAPS_ROOM_SMALL_H, MW = SIMAPS_ROOM_SMALL_W, RH = SIMAPS_ROOM_SMALL_RH, RW = SIMAPS_ROOM_SMALL_RW;
        k = id == SIMAPS_SPEC_S1 ? GSS_KERNEL<1, MH, MW, RH, RW> : GSS_KERNEL<0, MH, MW, RH, RW>;
    }
    hipLaunchKernelGGL(k, dim3(L.N), dim3(NT), 0, L.stream, *L.cfg, *L.geo, L.agents, L.envs, L.robots, L.paths,
                       L.occupancy, L.overhead, (GSS_ELEM *)L.state, L.capacity, L.dest, L.C, L.fault);
}
}  // namespace simaps_spec_store

#if SIMAPS_STORE_DTYPE == 0
// the queries of include/simaps_spec_store.h
extern "C" {
int simaps_spec_store_abi_version(void) { return SIMAPS_SPEC_STORE_ABI_VERSION; }

static bool spec_store_dtype_ok(int state_dtype)
{
    return state_dtype == SIMAPS_STATE_F32 || state_dtype == SIMAPS_STATE_BF16 || state_dtype == SIMAPS_STATE_F16;
}

int simaps_get_state_instance_as(const simaps_config *cfg, int state_dtype, int into, int has_debug)
{
    if (!cfg || !spec_store_dtype_ok(state_dtype)) return SIMAPS_EINVAL;
    return simaps_spec_store::instance_as(*cfg, state_dtype, into != 0, has_debug != 0);
}

int simaps_get_state_room_class_as(const simaps_config *cfg, int state_dtype, int into, int has_debug)
{
    if (!cfg || !spec_store_dtype_ok(state_dtype)) return SIMAPS_EINVAL;
    if (state_dtype == SIMAPS_STATE_F32 && !into) return simaps_get_state_room_class(cfg, has_debug);
    if (simaps_spec_store::instance_as(*cfg, state_dtype, into != 0, has_debug != 0) == SIMAPS_SPEC_GENERIC)
        return SIMAPS_ROOM_NONE;
    return simaps_spec::room_class_of(*cfg);
}
}
#endif
