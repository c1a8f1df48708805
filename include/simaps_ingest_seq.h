/* simaps_ingest_seq.h -- ordered multi-frame ingest: several camera frames per map slot in one launch.
 *
 * simaps_ingest (simaps.h) takes one frame per map slot and launch.  A host that re-maps a moving
 * robot several times between two readers of its maps (RobotController.step's periodic
 * Robot.update_map, envs.py:1401-1403) can instead keep the frames and hand them over together:
 * frame n carries seq[n], its position among the frames of its own map slot in this launch (0 the
 * oldest), and each slot's overhead and occupancy maps come out as if simaps_ingest had been called
 * once per frame in ascending seq.
 *
 * How: frame n writes its keys with the tag base + seq[n] where simaps_ingest writes the launch
 * epoch, so the per-pixel maximum of the key map is the latest frame that touched the pixel, then
 * the highest z inside that frame, then the later camera pixel (the z-tie rule of simaps_ingest).
 * Occupancy bytes are only ever set, in any order.
 *
 * Tags: epoch >= 1 uses the tags epoch .. epoch + num_seq - 1 of the key map; the next launch on
 * that key map (of either entry point) must pass an epoch above the last of them.  epoch == 0 is
 * the zeroing mode: tags 1 .. num_seq on a key map that is all zero on entry, all zero again on
 * exit -- the only mode allowed under stream capture, as for simaps_ingest.
 *
 * seq values: the device clamps seq[n] into [0, num_seq).  Two frames of one slot with the same seq
 * are the caller's error and are not detected: they merge like one frame, as two frames of one slot
 * do in simaps_ingest.  The kernels post no device faults.
 */
#ifndef SIMAPS_INGEST_SEQ_H
#define SIMAPS_INGEST_SEQ_H

#include "simaps_ctx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAPS_INGEST_SEQ_ABI_VERSION 1

int simaps_ingest_seq_abi_version(void);

/* Every argument but seq and num_seq is simaps_ingest's.  The frames of one slot may sit anywhere in
 * the arrays, in any order; cam_params[n] is frame n's own camera pose.
 *   seq      DEVICE [N] int32: frame n's position among the frames of its map slot in this launch.
 *            NULL is allowed with num_seq == 1 only: the call is then exactly simaps_ingest.
 *   num_seq  host int, 1 + the largest position, in [1, 255].
 * SIMAPS_EINVAL, before any device use: num_seq outside [1, 255]; epoch >= 1 with
 * epoch + num_seq - 1 > 255; a NULL seq with num_seq > 1; and everything simaps_ingest refuses, with
 * its codes. */
int simaps_ingest_seq(const simaps_config *cfg, const simaps_camera *cam, int N, const simaps_agent *agents,
                      const simaps_seg_ids *seg_ids, const double *cam_params, const float *depth,
                      const int32_t *seg_raw, const int32_t *seq, int num_seq, float *overhead, uint8_t *occupancy,
                      uint64_t *keys, uint32_t *boxes, int epoch, void *stream);
int simaps_ctx_ingest_seq(simaps_ctx *ctx, const simaps_config *cfg, const simaps_camera *cam, int N,
                          const simaps_agent *agents, const simaps_seg_ids *seg_ids, const double *cam_params,
                          const float *depth, const int32_t *seg_raw, const int32_t *seq, int num_seq,
                          float *overhead, uint8_t *occupancy, uint64_t *keys, uint32_t *boxes, int epoch,
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_INGEST_SEQ_H */
