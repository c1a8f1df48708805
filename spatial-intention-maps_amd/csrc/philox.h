// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and
// the exploration draw of include/simaps_action_as.h built on it.  Host and device: the host side is
// for checking the published known answers.
#pragma once
#include <stdint.h>

#define SIMAPS_PHILOX_HD __host__ __device__ __forceinline__

namespace simaps_philox {
// out = Philox4x32-10(counter c, key k)
SIMAPS_PHILOX_HD void philox4x32_10(const uint32_t c[4], const uint32_t k[2], uint32_t out[4])
{
    uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;  // (the key schedule: bumped after every round, the last bump unused)
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Agent n's draw at (seed, step): true iff it explores with probability e, and then `action` is uniform
// over [0, total) by multiply-shift (include/simaps_action_as.h states the function).
SIMAPS_PHILOX_HD bool explore_draw(uint64_t seed, uint64_t step, int n, float e, int total, int &action)
{
    const uint32_t c[4] = {(uint32_t)n, 0u, (uint32_t)step, (uint32_t)(step >> 32)};
    const uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox4x32_10(c, k, w);
    action = (int)(((uint64_t)w[1] * (uint32_t)total) >> 32);
    return (float)(w[0] >> 8) * 0x1p-24f < e;
}
}  // namespace simaps_philox
