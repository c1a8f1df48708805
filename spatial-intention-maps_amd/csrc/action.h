// Robot.store_new_action (envs.py:857-903) behind DQNPolicy.step's arg-max (policies.py:61-65), on the
// device (include/simaps_action.h): three launches on the caller's stream,
//   action_decode_kernel  one workgroup per agent: the first-index arg-max of its [K, 96, 96] Q block
//                         (or the given action index), np.unravel_index, the fp64 target geometry;
//   path_kernel           the movement path from the current position to that target, unchanged;
//   action_finish_kernel  one thread per agent: waypoint headings, the final waypoint's offset, the
//                         "avoid backing up" fix, and (flag bit 1) the robot descriptor write-back.
// Included by simaps.hip inside its device namespace.

constexpr int ACT_NT = 768;                 // decode: threads per workgroup (12 waves): 3 float4 groups per thread and channel
constexpr int ACT_PLANE = LW * LW;          // one output channel, 9,216 floats
static_assert(ACT_PLANE / 4 == 3 * ACT_NT, "the decode loop reads three float4 groups per thread and channel");
constexpr int ACT_FIN_NT = 64;              // finish: agents per workgroup

// END_EFFECTOR_LOCATION + CUBE_WIDTH / 2 per robot class (envs.py:889), from the host's Geometry
struct ActionOffsets {
    double ee[4];
};

// Robot.NUM_OUTPUT_CHANNELS (envs.py:810, 1091): 1 for the pushing robot, 2 for the robots with hooks
SIMAPS_HD int action_channels(int type) { return type == SIMAPS_PUSHING ? 1 : 2; }

// The robot an agent acts for, and whether this agent's action can be decoded at all: its descriptor
// in range (as agent_robot_type), and its explicit action, if any, inside [0, K * 9216) -- with no Q
// block to fall back on, -1 is out of range too.  Both kernels decide it from the same inputs.
__device__ __forceinline__ int action_robot(const simaps_agent &ag, const simaps_env *envs, const simaps_robot *robots,
                                            const int32_t *actions_in, int n, bool have_q, int &type, int &given,
                                            bool &bad)
{
    const simaps_env ev = envs[ag.env];
    bad = (unsigned)(ev.num_robots - 1) >= (unsigned)SIMAPS_MAX_ROBOTS || (unsigned)ag.robot >= (unsigned)ev.num_robots;
    const int nr = min(max(ev.num_robots, 1), SIMAPS_MAX_ROBOTS);
    const int r = ev.robot_off + ((unsigned)ag.robot < (unsigned)nr ? ag.robot : 0);
    type = robots[r].type;
    if ((unsigned)type > 3u) { bad = true; type = 0; }
    given = actions_in ? actions_in[n] : -1;
    if (given >= action_channels(type) * ACT_PLANE || given < -1 || (given == -1 && !have_q)) bad = true;
    return r;
}

// np.argmax order on floats: a NaN is the greatest value (numpy and torch propagate the first one),
// -0.0 == +0.0; among equals the lower index wins, whichever thread or wave holds it.
__device__ __forceinline__ bool act_better(float v, int i, float bv, int bi)
{
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (!vn && v != bv) return v > bv;
    return i < bi;
}

__global__ void __launch_bounds__(ACT_NT) action_decode_kernel(
    const simaps_agent *__restrict__ agents, const simaps_env *__restrict__ envs, const simaps_robot *__restrict__ robots,
    const float *__restrict__ q, const int64_t *__restrict__ q_off, const int32_t *__restrict__ actions_in, int flags,
    int max_pts, int32_t *__restrict__ out_action, double *__restrict__ out_source, double *__restrict__ out_target,
    double *__restrict__ out_xy, int32_t *__restrict__ out_count, unsigned *fault)
{
    __shared__ float wv[ACT_NT / 64];
    __shared__ int wi[ACT_NT / 64];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const simaps_agent ag = agents[n];
    int type, given;
    bool bad;
    const int r = action_robot(ag, envs, robots, actions_in, n, q != nullptr, type, given, bad);
    int action = given;
    if (!bad && given < 0) {  // (workgroup-uniform) the arg-max of the flattened block
        const int total = action_channels(type) * ACT_PLANE;
        const float *blk = q + q_off[n];
        float bv = 0.f;
        int bi = 0x7fffffff;  // no candidate yet: any element is better
        bool have = false;
        auto take = [&](float v, int i) {
            if (!have || act_better(v, i, bv, bi)) { bv = v; bi = i; have = true; }
        };
        if ((reinterpret_cast<uintptr_t>(blk) & 15) == 0) {
            // 16-byte loads, group g = tid + 768 j: a wave reads 1 KiB contiguous per instruction;
            // 3 (K = 1) or 6 (K = 2) groups per thread, one channel's three in flight at a time
            const float4 *b4 = reinterpret_cast<const float4 *>(blk);
            const int groups = total / 4;  // 2,304 = 3 ACT_NT per channel
            for (int g0 = tid; g0 < groups; g0 += 3 * ACT_NT) {
                float4 v[3];
#pragma unroll
                for (int u = 0; u < 3; u++) v[u] = b4[g0 + u * ACT_NT];  // (in range: groups is a multiple of 3 ACT_NT)
#pragma unroll
                for (int u = 0; u < 3; u++) {
                    const int i = 4 * (g0 + u * ACT_NT);
                    take(v[u].x, i);
                    take(v[u].y, i + 1);
                    take(v[u].z, i + 2);
                    take(v[u].w, i + 3);
                }
            }
        } else {  // a block that is not 16-byte aligned: the same, one float at a time
            for (int i = tid; i < total; i += ACT_NT) take(blk[i], i);
        }
        // every thread has at least one element (total >= 9,216 > ACT_NT), so `have` holds everywhere
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (act_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < ACT_NT / 64; w++)
                if (act_better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
            action = bi;
        }
    }
    if (tid != 0) return;
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
}

// restrict_heading_range (envs.py:2567-2568): (h + pi) % (2 pi) - pi with Python's floored %
__device__ __forceinline__ double restrict_heading(double h)
{
    const double PI = 3.141592653589793, TWO_PI = 2 * 3.141592653589793;
    double m = fmod(h + PI, TWO_PI);
    if (m < 0) m += TWO_PI;
    return m - PI;
}

__global__ void __launch_bounds__(ACT_FIN_NT) action_finish_kernel(
    int N, const simaps_agent *__restrict__ agents, const simaps_env *__restrict__ envs, simaps_robot *robots,
    double *paths, const int32_t *__restrict__ actions_in, int have_q, int flags, int max_pts, ActionOffsets offsets,
    const double *__restrict__ out_target, double *__restrict__ out_xy, double *__restrict__ out_heading,
    int32_t *__restrict__ out_count)
{
    const int n = blockIdx.x * ACT_FIN_NT + threadIdx.x;
    if (n >= N) return;
    const simaps_agent ag = agents[n];
    int type, given;
    bool bad;
    const int r = action_robot(ag, envs, robots, actions_in, n, have_q != 0, type, given, bad);
    if (bad) {  // (the decode kernel posted the fault; the path launch has since written a count)
        out_count[n] = 0;
        return;
    }
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
}
