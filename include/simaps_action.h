/* simaps_action.h -- the step back from the policy: Q maps (or given action indices) to actions,
 * end-effector targets, movement waypoints and waypoint headings, on the device.
 *
 * Reference: DQNPolicy.step takes the arg-max of each robot's Q map (policies.py:61-65);
 * Robot.store_new_action (envs.py:857-903, the base-class method) turns that index into the
 * (channel, row, col) action, target_end_effector_position, waypoint_positions (the movement path
 * with its final waypoint moved from the end effector's position to the robot's, and the "avoid
 * backing up" fix) and waypoint_headings.  The subclass overrides (envs.py:1186, 1291, 1351) add a
 * simulator ray test afterwards, which is not part of this.
 *
 * One call is three stream-ordered launches on the caller's stream: the decode kernel, the path
 * kernels of simaps_shortest_path -- unchanged, in the context's path mode, from the robot's current
 * position to the new target -- and a finish kernel.  Nothing synchronises.  Stream capture and the
 * path scratch follow the rules of simaps_shortest_path.
 */
#ifndef SIMAPS_ACTION_H
#define SIMAPS_ACTION_H

#include "simaps_ctx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIMAPS_ACTION_ABI_VERSION 1

/* flags */
#define SIMAPS_ACTION_SHORTEST_PATH 1 /* bit 0: env.use_shortest_path_movement; off: waypoints = [position, target] (envs.py:878) */
#define SIMAPS_ACTION_WRITE_BACK 2    /* bit 1: store the action into robots[] / paths[] for the next get_state */

int simaps_action_abi_version(void);

/* Robot.NUM_OUTPUT_CHANNELS of a robot class (envs.py:810, 1091): 1 for SIMAPS_PUSHING, 2 for the
 * classes with hooks (lifting, throwing, rescue); SIMAPS_EINVAL for any other value. */
int simaps_num_output_channels(int type);

/* Batched Robot.store_new_action behind the policy's arg-max, for agents[N] (robot agents[n].robot of
 * env agents[n].env, on the occupancy map of slot agents[n].map_slot).  Every array is a DEVICE pointer:
 *   q           float32       agent n's policy output: a [K_n, 96, 96] block (CHW, as the FCN emits it)
 *                             at float offset q_off[n]; K_n = simaps_num_output_channels of its robot's
 *                             class.  A block that starts on a 16-byte boundary is read with 16-byte
 *                             loads, any other with 4-byte loads: same result.  The offsets are the
 *                             caller's and are not range-checked.
 *   q_off       [N] int64     with q: both given or both NULL
 *   actions_in  [N] int32     may be NULL (every agent takes the arg-max); >= 0: the action index to use
 *                             for that agent (the host's epsilon-greedy draw, policies.py:61-62), whose
 *                             Q block is then not read; -1: the arg-max.  q may be NULL only if
 *                             actions_in is given.
 *   flags                     SIMAPS_ACTION_* bits
 *   out_action  [N] int32     the chosen index a; the reference's action tuple is np.unravel_index(a,
 *                             (K_n, 96, 96)) = (a / 9216, a % 9216 / 96, a % 96)
 *   out_source  [N][2] fp64   the robot's current position, the path's source
 *   out_target  [N][2] fp64   target_end_effector_position[:2]
 *   out_xy      [N][max_points][2] fp64   waypoint_positions[:, :2], after the final waypoint's offset
 *                             and the back-up fix
 *   out_heading [N][max_points] fp64      waypoint_headings
 *   out_count   [N] int32     number of waypoints; -needed if max_points is too small (then out_xy and
 *                             out_heading of that agent are not valid and nothing is written back)
 * occupancy may be NULL when bit 0 of flags is off; paths may be NULL when bit 1 is off.
 *
 * Arg-max: the lowest index among the maxima of the flattened block (np.argmax); a NaN counts as the
 * greatest value and the lowest-index NaN wins (numpy and torch agree); -0.0 equals +0.0.
 * Geometry, all fp64 (envs.py:866-869, 2400-2403): dx, dy = pixel_indices_to_position(row, col),
 * dist = sqrt(dx^2 + dy^2), theta = heading + atan2(-dx, dy), target = position + dist (cos, sin) theta.
 * Headings (881-885): [heading] + restrict_heading_range(atan2(dy, dx)) of each segment.  Final
 * waypoint (889-896): wp[-2] + signed_dist (cos, sin) headings[-1], signed_dist = |wp[-1] - wp[-2]| -
 * (END_EFFECTOR_LOCATION of the class + CUBE_WIDTH / 2).  Back-up fix (899-903): with more than two
 * waypoints and signed_dist < 0, wp[-2] = wp[-1] and headings[-2] recomputed.
 *
 * A bad action -- an explicit index outside [0, K_n * 9216) other than -1, or -1 with no q -- or an
 * agent whose env / robot indices are out of range is a descriptor error: that agent gets out_count 0
 * and no action, waypoints or headings (its out_source and out_target hold the robot's position, so
 * that the path launch has a query to run), nothing of it is written back, and
 * SIMAPS_FAULT_DESCRIPTOR is posted to the context's fault record with kernel id SIMAPS_K_ACTION and
 * the agent index n.  The other agents of the launch are unaffected.
 *
 * Write-back (SIMAPS_ACTION_WRITE_BACK): robot r = envs[agent.env].robot_off + agent.robot gets
 * target_x / target_y = the new target, idle = 0, its intention path = [position] + wp[1:-1] +
 * [target] (RobotController.get_intention_path with waypoint_index 1, as after controller.reset(),
 * envs.py:1386, 1475-1476, on the adjusted waypoints), intention_len = count, and its reversed history
 * path = [position, wp[0]] (envs.py:1478-1479, 2318), history_len = 2; no other field changes.
 * PRECONDITION: robots[] / paths[] have the layout simaps_pack_robots makes, SIMAPS_MAX_PATH points
 * reserved at each robot's intention_off and history_off (a tightly packed paths[] would be written
 * past a robot's own points).  A count above SIMAPS_MAX_PATH stores the true length and only the first
 * SIMAPS_MAX_PATH points; the next get_state reports such a length as SIMAPS_FAULT_DESCRIPTOR.  Two
 * agents of one launch must not name the same robot.
 *
 * SIMAPS_EINVAL before any device use: a NULL output or descriptor, max_points < 2, N < 0, unknown
 * flag bits, q without q_off or q_off without q, neither q nor actions_in. */
int simaps_store_new_action(const simaps_config *cfg, int N, const simaps_agent *agents, const simaps_env *envs,
                            simaps_robot *robots, double *paths, const uint8_t *occupancy, const float *q,
                            const int64_t *q_off, const int32_t *actions_in, int flags, int max_points,
                            int32_t *out_action, double *out_source, double *out_target, double *out_xy,
                            double *out_heading, int32_t *out_count, void *stream);

/* The same through a context (simaps_ctx.h): its fault record, path mode and pool; the plain form is
 * this on the default context. */
int simaps_ctx_store_new_action(simaps_ctx *ctx, const simaps_config *cfg, int N, const simaps_agent *agents,
                                const simaps_env *envs, simaps_robot *robots, double *paths,
                                const uint8_t *occupancy, const float *q, const int64_t *q_off,
                                const int32_t *actions_in, int flags, int max_points, int32_t *out_action,
                                double *out_source, double *out_target, double *out_xy, double *out_heading,
                                int32_t *out_count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIMAPS_ACTION_H */
