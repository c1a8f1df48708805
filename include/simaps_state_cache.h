/* simaps_state_cache.h -- get_state with a per-map-slot record of what an unchanged map makes.
 *
 * A two-source stack (instance S1, simaps_spec.h) builds the agent's configuration space from its
 * occupancy window and runs a full shortest-path sweep from the receptacle on every call.  Both are
 * functions of the slot's occupancy window, the agent's cspace radius, the room rectangle and the
 * receptacle's pixel only -- none of which depends on a robot's pose, and all of which stay the same
 * for most calls of a training run (the reference only ever sets occupancy cells, envs.py:2447-2450;
 * the receptacle does not move within an episode).
 *
 * simaps_get_state_cached is simaps_get_state with a caller-owned array of records, one per map slot.
 * A workgroup whose record matches its inputs (a hit) takes the free bits and the receptacle's
 * converged array from the record and sweeps from the robot only; any other workgroup (a miss)
 * computes everything as simaps_get_state does and rewrites its record.  Results, faults and errors
 * are those of simaps_get_state bit for bit either way.
 *
 * The match is decided on the device and is exact: the workgroup compares the record's key with its
 * own inputs and the record's occupancy window with the window it has just loaded, bit for bit.
 * There is no hash and no host-side version: a caller that writes the occupancy tensor directly gets
 * a miss and a correct result.
 *
 * Which calls use the cache: a float32 call that would take instance S1 in room class
 * SIMAPS_ROOM_SMALL (simaps_spec_room.h), whose occupancy rows allow the kernel's 4-byte window loads
 * (room_j0 >= 7 and ((room_j0 - 7) & ~3) + 144 <= W), with no simaps_debug output.  Every other call
 * through these entry points ignores the cache and is simaps_get_state; so is a call with cache NULL
 * or cache_records 0.  A workgroup whose agents[n].map_slot is not below cache_records computes
 * everything and leaves the cache alone.
 *
 * Contract:
 *   - The caller zeroes the cache once (a zero record matches nothing) and never writes it again.
 *   - A launch names each map_slot at most once: two workgroups of one launch must not share a record.
 *   - Launches that share a cache are ordered by the caller (one stream, or events between streams).
 *   - The cache is passed per call and bound to no context: the default context is shared.
 *
 * One record (simaps_state_cache_bytes(cfg) bytes, a multiple of 256; every part 16-byte aligned):
 *
 *   simaps_state_cache_header   the key, the receptacle source's results, the counters (80 bytes)
 *   window words                (room_h + 14) rows x 6 uint32: the occupancy window's bit rows as the
 *                               sweep waves assemble them (bit k of a row = window column k - sub,
 *                               sub = (room_j0 - 7) & 3; words 0..4 used)
 *   free bits                   room_h rows x 16 bytes: the rect's free cells (bit c of row r)
 *   receptacle array            a simaps_rec_cache_bytes record: 16-byte header {1, src_ok, room_h,
 *                               room_w}, then (room_h + 2) x ((room_w + 2) | 1) float32, border and
 *                               blocked cells -inf, free unreachable cells +inf
 */
#ifndef SIMAPS_STATE_CACHE_H
#define SIMAPS_STATE_CACHE_H

#include "simaps.h"
#include "simaps_ctx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAPS_STATE_CACHE_ABI_VERSION 1

/* layout magic of a valid record (0: never matches) */
#define SIMAPS_STATE_CACHE_MAGIC 0x53433031 /* "SC01" */

typedef struct simaps_state_cache_header {
    /* key: what the cached parts are functions of, beside the occupancy window itself */
    int32_t magic;                                /* SIMAPS_STATE_CACHE_MAGIC */
    int32_t H, W;                                 /* the map's shape */
    int32_t room_i0, room_j0, room_h, room_w;     /* the room rectangle */
    int32_t cspace_radius;                        /* the agent's robot class's dilation radius, pixels */
    int32_t has_receptacle;                       /* simaps_env.has_receptacle */
    int32_t rec_i, rec_j;                         /* the receptacle's query pixel */
    int32_t reserved0;
    /* the receptacle source's results */
    int32_t snap_i, snap_j;                       /* the query pixel snapped to a free cell; -1 if src_ok is 0 */
    int32_t src_ok;                               /* 0: the rect has no free cell */
    float dist_max;                               /* the array's maximum finite value, -1 if none */
    /* for tests and diagnostics: launches that matched this record / rewrote it */
    uint32_t hits, misses;
    uint32_t reserved1[2];
} simaps_state_cache_header;

int simaps_state_cache_abi_version(void);

/* Bytes of one record for this configuration (> 0), or SIMAPS_EINVAL for a NULL or invalid cfg. */
int simaps_state_cache_bytes(const simaps_config *cfg);

/* simaps_get_state with a cache of cache_records records (device memory, 16-byte aligned, record k
 * for map slot k).  SIMAPS_EINVAL for a misaligned cache or cache_records < 0; everything else as
 * simaps_get_state. */
int simaps_get_state_cached(const simaps_config *cfg, int N, const simaps_agent *agents, const simaps_env *envs,
                            const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                            const float *overhead, float *state, int num_robots_per_env, const simaps_debug *dbg,
                            void *stream, void *cache, int cache_records);
int simaps_ctx_get_state_cached(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                                const simaps_env *envs, const simaps_robot *robots, const double *paths,
                                const uint8_t *occupancy, const float *overhead, float *state,
                                int num_robots_per_env, const simaps_debug *dbg, void *stream, void *cache,
                                int cache_records);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_STATE_CACHE_H */
