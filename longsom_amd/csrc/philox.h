// The library's random stream: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) of four
// 32-bit counters under a 64-bit key, and the uniform in (0, 1) made of two of its words.  bnpc_sampler.hip keys it by the chain's
// seed, bbfit.hip by --seed; longsom_amd/bnpc_sampler.py (philox, to_double) is the numpy twin both are held to.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace lsg {

__host__ __device__ inline void philox4x32(uint64_t key, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t w[4]) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__host__ __device__ inline double to_double(uint32_t lo, uint32_t hi) { return ((double)((((uint64_t)hi << 32) | lo) >> 12) + 0.5) * 0x1p-52; }

} // namespace lsg
