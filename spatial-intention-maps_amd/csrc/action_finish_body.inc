// The finish step of one agent whose action was decoded (action_finish_kernel, action.h, and its twin in
// simaps_action_as.hip, as text): waypoint headings, the final waypoint's offset, the "avoid backing up"
// fix and the write-back.  Reads n, r, type, flags, max_pts, offsets, paths, robots, out_target, out_xy,
// out_heading and out_count of the including kernel.
    const int cnt = out_count[n];
    if (cnt < 2 || cnt > max_pts) return;  // -needed: max_points too small, nothing to finish
    const simaps_robot rb = robots[r];
    double *w = out_xy + (size_t)n * max_pts * 2, *hd = out_heading + (size_t)n * max_pts;
    // waypoint headings (envs.py:881-885)
    hd[0] = rb.heading;
    for (int i = 1; i < cnt; i++) hd[i] = restrict_heading(atan2(w[2 * i + 1] - w[2 * i - 1], w[2 * i] - w[2 * i - 2]));
    // the final waypoint: from the end effector's position to the robot's (envs.py:889-896)
    const int l = cnt - 1;
    const double ex = w[2 * l] - w[2 * l - 2], ey = w[2 * l + 1] - w[2 * l - 1];
    const double signed_dist = sqrt(ex * ex + ey * ey) - offsets.ee[type];
    w[2 * l] = w[2 * l - 2] + signed_dist * cos(hd[l]);
    w[2 * l + 1] = w[2 * l - 1] + signed_dist * sin(hd[l]);
    // avoid awkward backing up to reach the last waypoint (envs.py:899-903)
    if (cnt > 2 && signed_dist < 0) {
        w[2 * l - 2] = w[2 * l];
        w[2 * l - 1] = w[2 * l + 1];
        hd[l - 1] = restrict_heading(atan2(w[2 * l - 1] - w[2 * l - 3], w[2 * l - 2] - w[2 * l - 4]));
    }
    if (!(flags & SIMAPS_ACTION_WRITE_BACK)) return;
    // The robot as the next get_state reads it, after controller.reset() (waypoint_index 1, envs.py:1386):
    // intention path [position] + waypoints[1:-1] + [target] (envs.py:1475-1476), reversed history
    // [position, waypoints[0]] (1478-1479, 2318), at the offsets simaps_pack_robots laid out
    // (SIMAPS_MAX_PATH points reserved for each).
    const double tx = out_target[2 * n], ty = out_target[2 * n + 1];
    simaps_robot &o = robots[r];
    o.target_x = tx;
    o.target_y = ty;
    o.idle = 0;
    double *ip = paths + (size_t)2 * rb.intention_off, *hp = paths + (size_t)2 * rb.history_off;
    for (int k = 0; k < cnt && k < SIMAPS_MAX_PATH; k++) {
        const bool first = k == 0, last = k == cnt - 1;
        ip[2 * k] = first ? rb.x : last ? tx : w[2 * k];
        ip[2 * k + 1] = first ? rb.y : last ? ty : w[2 * k + 1];
    }
    o.intention_len = cnt;  // beyond SIMAPS_MAX_PATH: the true length, which get_state reports
    hp[0] = rb.x;
    hp[1] = rb.y;
    hp[2] = w[0];
    hp[3] = w[1];
    o.history_len = 2;
