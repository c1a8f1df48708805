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

#ifndef SIMAPS_ACTION_HELPERS_ONLY  // (simaps_action_as.hip has kernels of its own)
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
#include "action_decode_body.inc"
}

#endif

// restrict_heading_range (envs.py:2567-2568): (h + pi) % (2 pi) - pi with Python's floored %
__device__ __forceinline__ double restrict_heading(double h)
{
    const double PI = 3.141592653589793, TWO_PI = 2 * 3.141592653589793;
    double m = fmod(h + PI, TWO_PI);
    if (m < 0) m += TWO_PI;
    return m - PI;
}

#ifndef SIMAPS_ACTION_HELPERS_ONLY
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
#include "action_finish_body.inc"
}
#endif
