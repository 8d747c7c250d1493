// rover_philox.h — Philox4x32-10 (Salmon et al. 2011, Random123's philox4x32 with 10 rounds): the ONE copy of the round function.
// Users: the goal / reset-yaw draws (rover_reset.hip, counter word 3 = 0), the policy's action noise (rover_mlp.hip, counter word
// 3 = 0x50000000 | component pair), the exteroception noise (rover_noise.hip, 0x60000000 | column pair and 0x70000000) and the host
// entry rover_philox4x32 (rover_capi_learn.cpp), which pins the generator on the CPU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rover {

// c[0..3]: the counter, replaced by the four output words; (k0, k1): the key
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

}  // namespace rover
