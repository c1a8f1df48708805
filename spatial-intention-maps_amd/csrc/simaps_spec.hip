// Compile-time instances of get_state_kernel (include/simaps_spec.h, spec.h): the body is
// get_state_kernel's (get_state_body.inc with GS_MIXED 0), compiled with the configuration's feature
// flags and layout fixed and no simaps_debug output.  The kernel takes the call's simaps_config under
// another name and gives the body a local `cfg` whose fixed fields are constants: every helper is
// __forceinline__ and takes cfg by reference, so the constants fold through render_maps,
// render_distance_channels, RenderCtx::put, sweep_track and the nsrc / cs_waves / nw decisions.
// Room rect, H / W, thickness, encodings, scales and rotate_rounding stay run-time values in S1 / S2;
// their room-class twins (GS_SPEC_ROOM below) fix H / W and the room's size too.  Built
// into libsimaps.so beside simaps.hip, whose device helpers it includes (SIMAPS_DEVICE_ONLY).
//
// With the flags fixed the render track ends about 3 us before the sweep track,
// so the instances also move work off the sweep track that the generic kernel keeps there.  Each lever
// below was once a build switch of its own, timed against the generic schedule (DESIGN.md section 5,
// HISTORY.md) and decided for; they are now one condition, GS_SPEC: "this unit builds instances".
// The names stay in the comments at the sites they gate in simaps.hip and get_state_body.inc:
//   GS_SPEC_FUSED_SNAP   one group barrier for snap + SSSP start (snap_init_sources)
//   GS_SPEC_RENDER_ZERO  with two sources (8 sweep + 8 render waves) the render waves zero the released
//                        cspace scratch (sweep_track, render_maps); with one source the 12 render waves
//                        are the longer track and the sweep track keeps it
// and they cut serial overheads the sweep track carries beside its line steps:
//   GS_SPEC_ROUND_WORD   one LDS word per source and round instead of a change flag plus a 4-wave
//                        barrier (sssp_rounds_word); h / w / pitch / src_ok uniform once, not per round
//   GS_SPEC_FLAT_MARKS   a sweep's marks as unconditional non-returning ORs of wave-uniform,
//                        possibly-zero operands instead of lane-0 diamonds (sweep)
//   GS_SPEC_EARLY_OCC    the sweep waves' occupancy loads issued as soon as the agent record has
//                        landed, ahead of the env record and the entry barrier (get_state_body.inc)
// and, on the render track, so that it does not bind in their place:
//   GS_SPEC_EARLY_ZERO   (with GS_SPEC_RENDER_ZERO) the render waves zero the released scratch ahead
//                        of the barrier after the robot stamps, and the first raster pass starts
//                        without a barrier of its own (zero_scratch_early; late release: as before)
// Room-class instances (GS_SPEC_ROOM; spec.h room_class_of): S1 / S2 with the map shape H x W and the
// room's h x w fixed as well, for the small room of the BASELINE small_* configurations.  Everything
// derived from them folds: the pitch, len / span / cells per lane of each sweep direction, the cspace
// row blocks, early_tile / tail_cells and the crop's range checks against the room.  The room's origin
// and rotate_rounding stay run-time values (a twin per rounding was measured within noise of this and
// removed: HISTORY.md Appendix I).
//   GS_SPEC_DIR_ROUNDS   (with GS_SPEC_ROOM) each sweep wave branches once on its direction into a
//                        rounds loop instantiated for it (sssp_rounds_room / sssp_rounds_word<DIR>)
// They take the early occupancy loads and the round words as given.
#define GS_SPEC  // (GS_ROOM_H x GS_ROOM_W: the kernel's room-class template arguments, for get_state_body.inc)
#define GS_ROOM_H RH
#define GS_ROOM_W RW
#define SIMAPS_DEVICE_ONLY
#include "simaps.hip"
#include "get_state_instance.h"
#include "spec.h"

namespace {
// REC: use_shortest_path_to_receptacle_map (S1: 1, S2: 0)
// MH x MW / RH x RW: the room class's map shape and room, 0 for S1 / S2 themselves (run-time values)
template <int REC, int MH = 0, int MW = 0, int RH = 0, int RW = 0>
__global__ void __launch_bounds__(NT) get_state_spec_kernel(
    simaps_config cfg_in, Geometry geo, const simaps_agent *__restrict__ agents, const simaps_env *__restrict__ envs,
    const simaps_robot *__restrict__ robots, const double *__restrict__ paths, const uint8_t *__restrict__ occupancy,
    const float *__restrict__ overhead, float *__restrict__ state, int C, unsigned *fault)
{
    simaps_config cfg = cfg_in;
    fix_instance_fields<REC, MH, MW, RH, RW>(cfg);  // (RH != 0: GS_SPEC_ROOM)
    const simaps_debug dbg = {};
#define GS_MIXED 0
#include "get_state_body.inc"
#undef GS_MIXED
}

using spec_kernel_t = void (*)(simaps_config, Geometry, const simaps_agent *, const simaps_env *, const simaps_robot *,
                               const double *, const uint8_t *, const float *, float *, int, unsigned *);
}  // namespace

namespace simaps_spec {
void launch_get_state(int id, const simaps::GetStateLaunch &L)
{
    spec_kernel_t k = id == SIMAPS_SPEC_S1 ? get_state_spec_kernel<1> : get_state_spec_kernel<0>;
    // the room-class twin of S1 / S2 where cfg's shape matches a class exactly (spec.h)
    if (room_class_of(*L.cfg) == SIMAPS_ROOM_SMALL) {
        constexpr int MH = SIMAPS_ROOM_SMALL_H, MW = SIMAPS_ROOM_SMALL_W, RH = SIMAPS_ROOM_SMALL_RH, RW = SIMAPS_ROOM_SMALL_RW;
        k = id == SIMAPS_SPEC_S1 ? get_state_spec_kernel<1, MH, MW, RH, RW> : get_state_spec_kernel<0, MH, MW, RH, RW>;
    }
    hipLaunchKernelGGL(k, dim3(L.N), dim3(NT), 0, L.stream, *L.cfg, *L.geo, L.agents, L.envs, L.robots, L.paths,
                       L.occupancy, L.overhead, (float *)L.state, L.C, L.fault);
}

#if defined(SIMAPS_PHASE_STAMPS) || defined(SIMAPS_LIGHT_STAMPS)
int read_stamps(unsigned long long *host_out)
{
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), sizeof(g_stamps)) == hipSuccess ? 0 : SIMAPS_EHIP;
}
#endif
}  // namespace simaps_spec

extern "C" {
int simaps_spec_room_abi_version(void) { return SIMAPS_SPEC_ROOM_ABI_VERSION; }

int simaps_get_state_room_class(const simaps_config *cfg, int has_debug)
{
    if (!cfg) return SIMAPS_EINVAL;
    if (simaps_spec::instance_of(*cfg, has_debug != 0) == SIMAPS_SPEC_GENERIC) return SIMAPS_ROOM_NONE;
    return simaps_spec::room_class_of(*cfg);
}
}
