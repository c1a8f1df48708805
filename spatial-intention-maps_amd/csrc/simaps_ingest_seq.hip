// The kernels of simaps_ingest_seq (include/simaps_ingest_seq.h, ingest_seq.h): several camera frames
// per map slot in one launch, applied in the order of their seq.  The bodies are simaps_ingest's
// (ingest_points_body.inc, ingest_resolve_body.inc; simaps.hip is included for the device helpers they
// use: SIMAPS_DEVICE_ONLY); what differs is the top byte of a
// frame's keys -- base + seq[n] instead of the launch epoch -- and the resolve pass's test for "a key
// of this launch" (tag >= base).  The per-pixel atomicMax of the key map then keeps, per pixel, the
// latest frame that touched it, the highest z inside that frame and the later camera pixel among
// equal z: what successive Mapper.update calls leave (envs.py:2056-2062).  Occupancy bytes are only
// ever set to 1 (envs.py:2450) and need no order.
#define SIMAPS_DEVICE_ONLY
#include "simaps.hip"
#include "ingest_seq.h"

namespace {
template <int WCS>
__global__ void __launch_bounds__(INGEST_WG) ingest_points_seq_kernel(
    simaps_config cfg, simaps_camera cam, const simaps_agent *__restrict__ agents,
    const simaps_seg_ids *__restrict__ seg_ids, const double *__restrict__ cam_params,
    const float *__restrict__ depth, const int32_t *__restrict__ seg_raw, const int32_t *__restrict__ seq, int num_seq,
    uint8_t *__restrict__ occupancy, unsigned long long *__restrict__ keys, unsigned *__restrict__ boxes, unsigned tag0)
{
    // the frame's tag (block-uniform); a seq outside [0, num_seq) is clamped, so no tag leaves the
    // launch's range tag0 .. tag0 + num_seq - 1 <= 255 (checked on the host)
    const unsigned tag = tag0 + (unsigned)min(max(seq[blockIdx.y], 0), num_seq - 1);
#include "ingest_points_body.inc"
}

template <bool ZERO>
__global__ void __launch_bounds__(INGEST_RES_WG) ingest_resolve_seq_kernel(
    simaps_config cfg, const simaps_agent *__restrict__ agents, float *__restrict__ overhead,
    unsigned long long *__restrict__ keys, const unsigned *__restrict__ boxes, int nch, unsigned epoch)
{
    // (epoch: the launch's base tag, the name the shared body reads it by)
#define INGEST_RESOLVE_SEQ 1
#include "ingest_resolve_body.inc"
#undef INGEST_RESOLVE_SEQ
}
}  // namespace

namespace simaps_iseq {
void launch(const simaps_config &cfg, const simaps_camera &cam, int N, const simaps_agent *agents,
            const simaps_seg_ids *seg_ids, const double *cam_params, const float *depth, const int32_t *seg_raw,
            const int32_t *seq, int num_seq, float *overhead, uint8_t *occupancy, unsigned long long *keys,
            unsigned *boxes, int nch, unsigned base, bool zero, hipStream_t stream)
{
    if (cam.width_px + INGEST_PPT <= 320)
        hipLaunchKernelGGL(ingest_points_seq_kernel<320>, dim3(nch, N), dim3(INGEST_WG), 0, stream, cfg, cam, agents,
                           seg_ids, cam_params, depth, seg_raw, seq, num_seq, occupancy, keys, boxes, base);
    else
        hipLaunchKernelGGL(ingest_points_seq_kernel<INGEST_MAX_WC>, dim3(nch, N), dim3(INGEST_WG), 0, stream, cfg, cam,
                           agents, seg_ids, cam_params, depth, seg_raw, seq, num_seq, occupancy, keys, boxes, base);
    if (zero)
        hipLaunchKernelGGL(ingest_resolve_seq_kernel<true>, dim3(INGEST_RES_G, N), dim3(INGEST_RES_WG), 0, stream, cfg,
                           agents, overhead, keys, boxes, nch, base);
    else
        hipLaunchKernelGGL(ingest_resolve_seq_kernel<false>, dim3(INGEST_RES_G, N), dim3(INGEST_RES_WG), 0, stream, cfg,
                           agents, overhead, keys, boxes, nch, base);
}
}  // namespace simaps_iseq
