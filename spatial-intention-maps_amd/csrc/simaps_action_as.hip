// The kernels of simaps_store_new_action_as (include/simaps_action_as.h, action_as.h): the decode
// kernel of action.h for float32, bf16 and fp16 Q maps with the exploration draw in front of it, the
// finish kernel with the same decision, and the kernel that advances the rng state.  The helpers are
// action.h's and the two write-out bodies are shared with its kernels as text
// (action_decode_body.inc, action_finish_body.inc); simaps.hip is included for post_faults and the
// descriptor types only (SIMAPS_DEVICE_ONLY), none of its kernel bodies is instantiated here.
//
// Workgroup shapes.  A channel is 9,216 elements: 2,304 16-byte groups of float32, 1,152 of a 16-bit
// type.  float32 keeps action_decode_kernel's shape and loop: 768 threads, a channel's three groups
// per thread in flight, one round of loads per channel.  The 16-bit kernels keep the 768 threads and
// read the WHOLE block in one round: K = 2 is 2,304 groups, three per thread; K = 1 is 1,152, one per
// thread and a second one for the lower half of the workgroup.  Fewer, wider rounds win here
// (DESIGN.md section 5); measured against shapes with a round per channel (576 threads x 2 groups,
// 384 x 3) and against 576 threads x 4 in one round, this is the only one at which the 16-bit decode
// costs what the float32 decode does (profiles/action_as_shapes.jsonl).
#define SIMAPS_DEVICE_ONLY
#include "simaps.hip"
#include "action_as.h"
#include "philox.h"

namespace {
#define SIMAPS_ACTION_HELPERS_ONLY
#include "action.h"
#undef SIMAPS_ACTION_HELPERS_ONLY

// Element types: how many make a 16-byte group, and the exact widening to float32.
struct QF32 {
    typedef float elem;
    static constexpr int NT = ACT_NT, EPG = 4;
    static __device__ __forceinline__ float widen(float v) { return v; }
    static __device__ __forceinline__ void unpack(const uint4 &g, float (&f)[4])
    {
        f[0] = __uint_as_float(g.x); f[1] = __uint_as_float(g.y); f[2] = __uint_as_float(g.z); f[3] = __uint_as_float(g.w);
    }
};
struct QBF16 {
    typedef uint16_t elem;
    static constexpr int NT = ACT_NT, EPG = 8;
    static __device__ __forceinline__ float widen(uint16_t v) { return __uint_as_float((unsigned)v << 16); }
    static __device__ __forceinline__ void unpack(const uint4 &g, float (&f)[8])
    {
        const unsigned w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {  // little-endian: the low half is the earlier element
            f[2 * j] = __uint_as_float(w[j] << 16);
            f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        }
    }
};
struct QF16 {
    typedef uint16_t elem;
    static constexpr int NT = ACT_NT, EPG = 8;
    static __device__ __forceinline__ float widen(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
    static __device__ __forceinline__ void unpack(const uint4 &g, float (&f)[8])
    {
        const unsigned w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            f[2 * j] = widen((uint16_t)(w[j] & 0xffffu));
            f[2 * j + 1] = widen((uint16_t)(w[j] >> 16));
        }
    }
};

// The decision every kernel of the call makes from the same inputs, in two steps around the draw.
// Before it: the robot and `bad` as action_robot decides them (a -1 without q is left to as_resolve),
// and eps[n] in range; -> whether this agent draws at all.
__device__ __forceinline__ bool as_needs_draw(const float *eps, int n, int given, bool &bad, float &e)
{
    if (!eps) return false;
    e = eps[n];
    if (!(e >= 0.f && e <= 1.f)) bad = true;  // (a NaN fails both compares)
    return !bad && given < 0;
}
// After it: given beats drawn beats arg-max, and an agent left with the arg-max needs a Q block.
__device__ __forceinline__ void as_resolve(int drawn, bool have_q, int &given, bool &bad, int &explored)
{
    explored = 0;
    if (drawn >= 0) { given = drawn; explored = 1; }
    if (given < 0 && !have_q) bad = true;
}

template <typename Q>
__global__ void __launch_bounds__(Q::NT) action_decode_as_kernel(
    const simaps_agent *__restrict__ agents, const simaps_env *__restrict__ envs, const simaps_robot *__restrict__ robots,
    const typename Q::elem *__restrict__ q, const int64_t *__restrict__ q_off, const int32_t *__restrict__ actions_in,
    const float *__restrict__ eps, const uint64_t *__restrict__ rng, int flags, int max_pts,
    int32_t *__restrict__ out_action, double *__restrict__ out_source, double *__restrict__ out_target,
    double *__restrict__ out_xy, int32_t *__restrict__ out_count, uint8_t *__restrict__ out_explored, unsigned *fault)
{
    constexpr int NTH = Q::NT, EPG = Q::EPG;
    static_assert(NTH % 64 == 0, "whole waves: wv / wi hold one entry per wave");
    __shared__ float wv[NTH / 64];
    __shared__ int wi[NTH / 64];
    __shared__ int sh_drawn;
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const simaps_agent ag = agents[n];
    int type, given, explored;
    bool bad;
    const int r = action_robot(ag, envs, robots, actions_in, n, true, type, given, bad);
    const int total = action_channels(type) * ACT_PLANE;
    int drawn = -1;
    float e = 0.f;
    if (as_needs_draw(eps, n, given, bad, e)) {  // (workgroup-uniform) one thread draws, all of them learn it
        if (tid == 0) {
            int a;
            sh_drawn = simaps_philox::explore_draw(rng[0], rng[1], n, e, total, a) ? a : -1;
        }
        __syncthreads();
        drawn = sh_drawn;
    }
    as_resolve(drawn, q != nullptr, given, bad, explored);
    int action = given;
    if (!bad && given < 0) {  // (workgroup-uniform) the arg-max of the flattened block
        const typename Q::elem *blk = q + q_off[n];
        float bv = 0.f;
        int bi = 0x7fffffff;  // no candidate yet: any element is better
        bool have = false;
        auto take = [&](float v, int i) {
            if (!have || act_better(v, i, bv, bi)) { bv = v; bi = i; have = true; }
        };
        if ((reinterpret_cast<uintptr_t>(blk) & 15) == 0) {
            // 16-byte loads, group g = tid + NTH j: a wave reads 1 KiB contiguous per instruction
            const uint4 *b4 = reinterpret_cast<const uint4 *>(blk);
            const int groups = total / EPG;
            auto take_group = [&](const uint4 &g, int gi) {
                float f[EPG];
                Q::unpack(g, f);
#pragma unroll
                for (int k = 0; k < EPG; k++) take(f[k], EPG * gi + k);
            };
            if constexpr (EPG == 4) {
                // float32, as action_decode_kernel: one channel's three groups per thread in flight at a time
                constexpr int U = ACT_PLANE / EPG / NTH;
                static_assert(ACT_PLANE == U * EPG * NTH, "a channel is a whole number of rounds of 16-byte groups");
                for (int g0 = tid; g0 < groups; g0 += U * NTH) {
                    uint4 v[U];
#pragma unroll
                    for (int u = 0; u < U; u++) v[u] = b4[g0 + u * NTH];  // (in range: groups is a multiple of U NTH)
#pragma unroll
                    for (int u = 0; u < U; u++) take_group(v[u], g0 + u * NTH);
                }
            } else {
                // 16 bits: the whole block in one round of loads (workgroup-uniform branch on K)
                static_assert(2 * ACT_PLANE == 3 * EPG * NTH, "K = 2: three groups per thread; K = 1: one and a half");
                if (groups == 3 * NTH) {
                    uint4 v[3];
#pragma unroll
                    for (int u = 0; u < 3; u++) v[u] = b4[tid + u * NTH];  // (in range: 3 NTH groups)
#pragma unroll
                    for (int u = 0; u < 3; u++) take_group(v[u], tid + u * NTH);
                } else {  // 3 NTH / 2 groups: the lower half of the workgroup reads a second one
                    const bool second = tid < NTH / 2;
                    const uint4 v0 = b4[tid];
                    uint4 v1 = v0;
                    if (second) v1 = b4[NTH + tid];  // (in range: NTH + tid < 3 NTH / 2)
                    take_group(v0, tid);
                    if (second) take_group(v1, NTH + tid);
                }
            }
        } else {  // a block that is not 16-byte aligned: the same, one element at a time
            for (int i = tid; i < total; i += NTH) take(Q::widen(blk[i]), i);
        }
        // every thread has at least one element (total >= 9,216 > NTH), so `have` holds everywhere
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (act_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < NTH / 64; w++)
                if (act_better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
            action = bi;
        }
    }
    if (tid != 0) return;
    if (out_explored) out_explored[n] = (uint8_t)(bad ? 0 : explored);
#include "action_decode_body.inc"
}

__global__ void __launch_bounds__(ACT_FIN_NT) action_finish_as_kernel(
    int N, const simaps_agent *__restrict__ agents, const simaps_env *__restrict__ envs, simaps_robot *robots,
    double *paths, const int32_t *__restrict__ actions_in, const float *__restrict__ eps,
    const uint64_t *__restrict__ rng, int have_q, int flags, int max_pts, ActionOffsets offsets,
    const double *__restrict__ out_target, double *__restrict__ out_xy, double *__restrict__ out_heading,
    int32_t *__restrict__ out_count)
{
    const int n = blockIdx.x * ACT_FIN_NT + threadIdx.x;
    if (n >= N) return;
    const simaps_agent ag = agents[n];
    int type, given, explored;
    bool bad;
    const int r = action_robot(ag, envs, robots, actions_in, n, true, type, given, bad);
    int drawn = -1;
    float e = 0.f;
    if (as_needs_draw(eps, n, given, bad, e)) {  // the decode workgroup's draw again: rng is still as it read it
        int a;
        if (simaps_philox::explore_draw(rng[0], rng[1], n, e, action_channels(type) * ACT_PLANE, a)) drawn = a;
    }
    as_resolve(drawn, have_q != 0, given, bad, explored);
    if (bad) {  // (the decode kernel posted the fault; the path launch has since written a count)
        out_count[n] = 0;
        return;
    }
#include "action_finish_body.inc"
}

// {seed, step}: one more call has drawn from this step
__global__ void action_rng_advance_kernel(uint64_t *rng)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) rng[1] += 1;
}
}  // namespace

namespace simaps_action_as {
void launch_decode(int q_dtype, int N, const simaps_agent *agents, const simaps_env *envs, const simaps_robot *robots,
                   const void *q, const int64_t *q_off, const int32_t *actions_in, const float *eps,
                   const uint64_t *rng, int flags, int max_points, int32_t *out_action, double *out_source,
                   double *out_target, double *out_xy, int32_t *out_count, uint8_t *out_explored, unsigned *fault,
                   hipStream_t stream)
{
#define SIMAPS_DECODE_AS(Q)                                                                                          \
    hipLaunchKernelGGL(action_decode_as_kernel<Q>, dim3(N), dim3(Q::NT), 0, stream, agents, envs, robots,            \
                       static_cast<const Q::elem *>(q), q_off, actions_in, eps, rng, flags, max_points, out_action, \
                       out_source, out_target, out_xy, out_count, out_explored, fault)
    if (q_dtype == SIMAPS_STATE_BF16) SIMAPS_DECODE_AS(QBF16);
    else if (q_dtype == SIMAPS_STATE_F16) SIMAPS_DECODE_AS(QF16);
    else SIMAPS_DECODE_AS(QF32);
#undef SIMAPS_DECODE_AS
}

void launch_finish(int N, const simaps_agent *agents, const simaps_env *envs, simaps_robot *robots, double *paths,
                   const int32_t *actions_in, const float *eps, uint64_t *rng, bool have_q, int flags, int max_points,
                   const double ee[4], const double *out_target, double *out_xy, double *out_heading,
                   int32_t *out_count, hipStream_t stream)
{
    ActionOffsets off;
    for (int t = 0; t < 4; t++) off.ee[t] = ee[t];
    hipLaunchKernelGGL(action_finish_as_kernel, dim3((N + ACT_FIN_NT - 1) / ACT_FIN_NT), dim3(ACT_FIN_NT), 0, stream, N,
                       agents, envs, robots, paths, actions_in, eps, rng, have_q ? 1 : 0, flags, max_points, off,
                       out_target, out_xy, out_heading, out_count);
    if (rng) hipLaunchKernelGGL(action_rng_advance_kernel, dim3(1), dim3(1), 0, stream, rng);
}
}  // namespace simaps_action_as
