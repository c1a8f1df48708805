// What one thread of a decode workgroup writes once the agent's action is known (action_decode_kernel,
// action.h, and its twin in simaps_action_as.hip, as text): a bad action's count 0 and fault, or the
// action index, the fp64 target geometry and, without shortest-path movement, the two waypoints.  Reads
// n, r, bad, action, flags, max_pts, robots, fault and the out_* pointers of the including kernel.
    const simaps_robot rb = robots[r];
    if (bad) {
        // no action to decode: count 0, and a source and target the path launch can run on harmlessly
        out_count[n] = 0;
        out_source[2 * n] = out_target[2 * n] = rb.x;
        out_source[2 * n + 1] = out_target[2 * n + 1] = rb.y;
        post_faults(fault, SIMAPS_FAULT_DESCRIPTOR, SIMAPS_K_ACTION, n);
        return;
    }
    // np.unravel_index over (K, 96, 96), then envs.py:866-869 in fp64
    const int rem = action % ACT_PLANE, row = rem / LW, col = rem % LW;
    const double dx = ((col + 0.5) - (double)LW / 2) / PPM, dy = ((double)LW / 2 - (row + 0.5)) / PPM;
    const double dist = sqrt(dx * dx + dy * dy);
    const double theta = rb.heading + atan2(-dx, dy);
    const double tx = rb.x + dist * cos(theta), ty = rb.y + dist * sin(theta);
    out_action[n] = action;
    out_source[2 * n] = rb.x;
    out_source[2 * n + 1] = rb.y;
    out_target[2 * n] = tx;
    out_target[2 * n + 1] = ty;
    if (!(flags & SIMAPS_ACTION_SHORTEST_PATH)) {  // [current_position, target] (envs.py:878)
        double *o = out_xy + (size_t)n * max_pts * 2;
        o[0] = rb.x; o[1] = rb.y; o[2] = tx; o[3] = ty;
        out_count[n] = 2;
    }
