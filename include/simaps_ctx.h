/* simaps_ctx.h -- the context-scoped form of the C ABI of libsimaps.so (simaps.h).
 *
 * A context owns the three pieces of state that simaps.h keeps per process: the device fault
 * record (SIMAPS_FAULT_* bits and where they were posted), the path mode, and the private memory
 * pool of the path / large-window scratch.  A host that drives several GPUs from one process, or
 * several collectors from several threads, gives each its own context: a bad descriptor in one
 * caller's launch then fails that caller's next call and nobody else's.
 *
 * Every entry point of simaps.h that launches a kernel has a twin here, named with a `ctx_` after
 * the `simaps_` prefix: the context first, then the unchanged argument list, the same results bit
 * for bit.  The entry points of simaps.h are these twins on the process-wide DEFAULT context, which
 * has no device of its own (it launches on the calling thread's current device), one fault record
 * that all devices share, and one pool per device.  A NULL context means the default context in
 * every function here except create and destroy.
 *
 * Device binding: a created context is bound to one device.  A call through it made while another
 * device is current switches the calling thread to the context's device for the duration of the
 * call and restores the previous device before it returns, on every return path.  The stream and
 * every buffer passed to the call must belong to the context's device: that is the caller's duty
 * and is not checked.
 *
 * Thread safety: different contexts may be used concurrently from different threads with no
 * coordination.  One context may also be used from several threads at once: its launches are
 * independent and its path mode is atomic; but all those threads share ONE fault record, so a
 * fault posted by one thread's launch can fail another thread's next call through that context.
 * Handles are checked against a registry of live contexts: a handle that was never created, or
 * was already destroyed, gives SIMAPS_EINVAL, not a crash.  Destroying a context while another
 * thread is inside a call through it is the caller's error, like free() of memory in use.
 */
#ifndef SIMAPS_CTX_H
#define SIMAPS_CTX_H

#include "simaps.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct simaps_ctx simaps_ctx; /* opaque */

/* Kernel ids of the fault record's `where` word (word 3: (kernel id << 24) | min(unit, 0xFFFFFF)):
 * one per kernel that posts SIMAPS_FAULT_* bits; ids start at 1, so a posted word is never 0.
 * `unit` is the index along the call's batch dimension, which the caller can map back to their
 * inputs: the agent n of agents[], the query b, the frame n -- not a raw block id. */
#define SIMAPS_K_GET_STATE 1       /* get_state twin: agent n */
#define SIMAPS_K_GET_STATE_MIXED 2 /* get_state_mixed twin: agent n */
#define SIMAPS_K_SP_DISTANCE 3     /* sp_distance twin: agent n */
#define SIMAPS_K_PATH 4            /* shortest_path twin: agent n */
#define SIMAPS_K_SSSP_GRID 5       /* sssp_grid twin, LDS-resident window: grid b */
#define SIMAPS_K_GRID_PATH 6       /* grid_path twin, LDS-resident window: query b */
#define SIMAPS_K_GL_SSSP 7         /* sssp_grid / grid_path twins, large window, whole-window sweeps: grid b */
#define SIMAPS_K_GL_TILE 8         /* sssp_grid / grid_path twins, large window, tiled fixpoint: grid b */
#define SIMAPS_K_GL_PATH 9         /* grid_path twin, large window, the SPFA replay: query b */
#define SIMAPS_K_OCCUPANCY_MAP 10  /* build_cspace / snap_sources twins: agent n */
#define SIMAPS_K_GLOBAL_MAPS 11    /* global_maps twin: agent n */
#define SIMAPS_K_ACTION 12         /* store_new_action twin (simaps_action.h), the decode kernel: agent n */
#define SIMAPS_K_GET_STATE_INTO 13  /* get_state_into twin (simaps_store.h): agent n */
#define SIMAPS_K_COUNT 13

/* A new context on device `device` (>= 0: that ordinal; -1: the calling thread's current device),
 * with its own 64-byte host-mapped fault record, path mode 0 and (on first use) its own memory pool.
 * SIMAPS_EINVAL: out is NULL, device < -1 or device >= the device count; SIMAPS_EHIP: no usable
 * GPU (a host without one included), or the record could not be allocated.  *out is NULL on every
 * failure. */
int simaps_ctx_create(int device, simaps_ctx **out);

/* Removes the handle from the registry, synchronises the context's device (so that no launch can
 * still post into the record), then frees the record and the pool.  SIMAPS_EINVAL for NULL, for a
 * handle that is not live, and so for a second destroy of the same handle. */
int simaps_ctx_destroy(simaps_ctx *ctx);

/* The context's device ordinal; -1 for the default context (NULL); SIMAPS_EINVAL for a dead handle
 * (device ordinals are >= 0 and the default is -1 == SIMAPS_EINVAL: tell them apart by passing NULL
 * only when the default is meant). */
int simaps_ctx_device(const simaps_ctx *ctx);

/* The context's SIMAPS_FAULT_* bits as of the launches through it that have completed (synchronise
 * the stream first to cover a given launch); clear != 0 resets the record.  Bits (>= 0), or a
 * negative error. */
int simaps_ctx_fault_status(simaps_ctx *ctx, int clear);

/* As above, and where a fault was posted: *kernel = SIMAPS_K_*, *unit = the batch index, of one
 * faulting workgroup (if several faulted, any one of them); both -1 when no `where` word was seen.
 * Either pointer may be NULL. */
int simaps_ctx_fault_info(simaps_ctx *ctx, int clear, int *kernel, int *unit);

/* This context's path mode (0-3, as the path mode of simaps.h, which is the default context's);
 * returns the context's previous mode. */
int simaps_ctx_path_mode(simaps_ctx *ctx, int mode);

/* ---- compute twins: arguments, results and errors of the entry point of the same name in simaps.h.
 * The launch's kernels post into ctx's fault record; only ctx's next compute call returns
 * SIMAPS_EDEVICE for it (once, clearing the record), with a message that ends " in <kernel>, unit <u>"
 * when the `where` word is known (a created context only: the default context's message is that of
 * simaps.h). */
int simaps_ctx_get_state(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                         const simaps_env *envs, const simaps_robot *robots, const double *paths,
                         const uint8_t *occupancy, const float *overhead, float *state, int num_robots_per_env,
                         const simaps_debug *dbg, void *stream);
int simaps_ctx_get_state_mixed(simaps_ctx *ctx, const simaps_config *cfgs, const int32_t *num_robots_per_env, int n_cfgs,
                               int N, const simaps_agent *agents, const int32_t *agent_cfg, const simaps_env *envs,
                               const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                               const int64_t *map_off, const float *overhead, float *state, const int64_t *out_off,
                               void *stream);
int simaps_ctx_sp_distance(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                           const simaps_env *envs, const simaps_robot *robots, const uint8_t *occupancy,
                           const double *sources, const double *targets, int Q, double *out, void *rec_cache,
                           void *stream);
int simaps_ctx_sp_lookup(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                         const void *rec_cache, const double *targets, int Q, double *out, void *stream);
int simaps_ctx_shortest_path(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                             const simaps_env *envs, const simaps_robot *robots, const uint8_t *occupancy,
                             const double *sources, const double *targets, int max_points, double *out_xy,
                             int32_t *out_count, void *stream);
int simaps_ctx_ingest(simaps_ctx *ctx, const simaps_config *cfg, const simaps_camera *cam, int N,
                      const simaps_agent *agents, const simaps_seg_ids *seg_ids, const double *cam_params,
                      const float *depth, const int32_t *seg_raw, float *overhead, uint8_t *occupancy, uint64_t *keys,
                      uint32_t *boxes, int epoch, void *stream);
int simaps_ctx_sssp_grid(simaps_ctx *ctx, int B, int H, int W, const uint8_t *grids, const int32_t *sources,
                         float *dists, int wi0, int wj0, int wh, int ww, void *stream);
int simaps_ctx_grid_path(simaps_ctx *ctx, int B, int H, int W, const uint8_t *grids, const int32_t *sources,
                         const int32_t *targets, int wi0, int wj0, int wh, int ww, int max_points, int32_t *out_ij,
                         int32_t *out_count, void *stream);
int simaps_ctx_occupancy_scatter(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                                 const float *points, const float *seg, int P, double obstacle_seg_value,
                                 uint8_t *occupancy, void *stream);
int simaps_ctx_build_cspace(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                            const simaps_env *envs, const simaps_robot *robots, const uint8_t *occupancy,
                            uint8_t *cspace, uint8_t *cspace_thin, void *stream);
int simaps_ctx_snap_sources(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                            const simaps_env *envs, const simaps_robot *robots, const uint8_t *occupancy,
                            const int32_t *pixels, int Q, int32_t *out, void *stream);
int simaps_ctx_global_maps(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                           const simaps_env *envs, const simaps_robot *robots, const double *paths,
                           const float *overhead, float *overhead_map, float *robot_map, float *history_map,
                           float *intention_map, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_CTX_H */
