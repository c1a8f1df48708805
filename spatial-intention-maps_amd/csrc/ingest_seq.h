// Ordered multi-frame ingest (include/simaps_ingest_seq.h): the launcher of its two kernels.  They
// live in their own translation unit (simaps_ingest_seq.hip) and share the bodies of simaps_ingest's
// kernels as text (ingest_points_body.inc, ingest_resolve_body.inc), so that adding them cannot change
// the code the compiler makes of ingest_points_kernel and ingest_resolve_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "simaps_ingest_seq.h"

namespace simaps_iseq {
// The point pass with per-frame tags base + clamp(seq[n], 0, num_seq - 1), then the resolve pass over
// the tags >= base; zero: the zeroing mode (base 1 on an all-zero key map, all zero again on exit).
// The arguments were checked by the caller (ingest_impl, simaps.hip); nch = ingest_chunks(camera).
void launch(const simaps_config &cfg, const simaps_camera &cam, int N, const simaps_agent *agents,
            const simaps_seg_ids *seg_ids, const double *cam_params, const float *depth, const int32_t *seg_raw,
            const int32_t *seq, int num_seq, float *overhead, uint8_t *occupancy, unsigned long long *keys,
            unsigned *boxes, int nch, unsigned base, bool zero, hipStream_t stream);
}  // namespace simaps_iseq
