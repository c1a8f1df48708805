/* simaps_state_cache_store.h -- the state cache for the store launches and the 16-bit launches.
 *
 * simaps_state_cache.h gives a float32 simaps_get_state a caller-owned array of records, one per map
 * slot, from which a workgroup whose map is unchanged takes its configuration space and the
 * receptacle's distances.  The entry points below give the same records to the other launches of the
 * single-configuration kernel:
 *
 *   simaps_get_state_into_cached   simaps_get_state_into (float32, bf16, fp16; simaps_store.h)
 *   simaps_get_state_as_cached     simaps_get_state_as   (bf16, fp16; float32 is simaps_get_state_cached)
 *
 * Everything simaps_state_cache.h says of a record holds unchanged: its layout and size
 * (simaps_state_cache_bytes), the exact match decided on the device against the occupancy window
 * itself, what a hit takes and what a miss rewrites.  A record holds float32 distances and bit words
 * only, whatever the stack's element type: records written through any cached entry point are the same
 * bytes for the same inputs (the hits / misses counters aside), and any of them may hit on a record
 * that another wrote.  Results, the store rows touched, faults (fault word, kernel id and unit) and
 * errors are those of the uncached entry point bit for bit, hit or miss.
 *
 * Because the match is made on the device, the cache stays correct under a `dest` that only the device
 * knows: an agent with dest[n] == -1, or with a row outside [0, capacity), returns before it touches
 * its record -- nothing is loaded from it, no counter moves, nothing is rewritten (the row outside the
 * store still posts SIMAPS_FAULT_DESCRIPTOR under SIMAPS_K_GET_STATE_INTO).
 *
 * Which calls use the cache (simaps_state_cache_applies): a call that would take instance S1 in room
 * class SIMAPS_ROOM_SMALL (simaps_spec_store.h), whose occupancy rows allow the kernel's 4-byte window
 * loads (room_j0 >= 7 and ((room_j0 - 7) & ~3) + 144 <= W), with no simaps_debug output.  Every other
 * call through these entry points ignores the cache -- it is neither read nor written -- and is the
 * uncached entry point; so is a call with cache NULL or cache_records 0.  A workgroup whose
 * agents[n].map_slot is not below cache_records computes everything and leaves the cache alone.
 *
 * Contract (simaps_state_cache.h's): the caller zeroes the cache once (a zero record matches nothing)
 * and never writes it again; a launch names each map_slot at most once; launches that share a cache are
 * ordered by the caller; the cache is passed per call and bound to no context.
 */
#ifndef SIMAPS_STATE_CACHE_STORE_H
#define SIMAPS_STATE_CACHE_STORE_H

#include "simaps_state_cache.h"
#include "simaps_spec_store.h"
#include "simaps_store.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAPS_STATE_CACHE_STORE_ABI_VERSION 1

int simaps_state_cache_store_abi_version(void);

/* Whether a call with this configuration through the entry point of element type state_dtype
 * (SIMAPS_STATE_F32 / _BF16 / _F16; into != 0: into a store) uses a cache it is given: 1 or 0.
 * has_debug as in simaps_get_state_instance_as.  For SIMAPS_STATE_F32 with into == 0 the answer is
 * simaps_get_state_cached's rule.  Host only.  SIMAPS_EINVAL for a NULL cfg or an unknown state_dtype. */
int simaps_state_cache_applies(const simaps_config *cfg, int state_dtype, int into, int has_debug);

/* simaps_get_state_into with a cache of cache_records records (device memory, 16-byte aligned, record k
 * for map slot k).  SIMAPS_EINVAL for a misaligned cache or cache_records < 0, before any device use;
 * everything else as simaps_get_state_into. */
int simaps_get_state_into_cached(const simaps_config *cfg, int N, const simaps_agent *agents, const simaps_env *envs,
                                 const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                                 const float *overhead, void *store, int state_dtype, int64_t capacity,
                                 const int64_t *dest, int num_robots_per_env, const simaps_debug *dbg, void *stream,
                                 void *cache, int cache_records);
int simaps_ctx_get_state_into_cached(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                                     const simaps_env *envs, const simaps_robot *robots, const double *paths,
                                     const uint8_t *occupancy, const float *overhead, void *store, int state_dtype,
                                     int64_t capacity, const int64_t *dest, int num_robots_per_env,
                                     const simaps_debug *dbg, void *stream, void *cache, int cache_records);

/* simaps_get_state_as with the same cache.  With SIMAPS_STATE_F32 it is simaps_get_state_cached. */
int simaps_get_state_as_cached(const simaps_config *cfg, int N, const simaps_agent *agents, const simaps_env *envs,
                               const simaps_robot *robots, const double *paths, const uint8_t *occupancy,
                               const float *overhead, void *state, int state_dtype, int num_robots_per_env,
                               const simaps_debug *dbg, void *stream, void *cache, int cache_records);
int simaps_ctx_get_state_as_cached(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                                   const simaps_env *envs, const simaps_robot *robots, const double *paths,
                                   const uint8_t *occupancy, const float *overhead, void *state, int state_dtype,
                                   int num_robots_per_env, const simaps_debug *dbg, void *stream, void *cache,
                                   int cache_records);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_STATE_CACHE_STORE_H */
