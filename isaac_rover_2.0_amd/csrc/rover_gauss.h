// rover_gauss.h — the Box-Muller pair of the counter-based noise: the ONE copy of the transform from two Philox words to two standard
// normals.  Users: the actor's Gaussian head (rover_mlp.hip gauss_eps_pair, counter word 3 = 0x50000000 | component pair) and the
// exteroception noise (rover_noise.hip, counter word 3 = 0x60000000 | column pair and 0x70000000).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rover {

// u0 = (24 bits + 1) 2^-24 in (0, 1] keeps the logarithm finite: |e| <= sqrt(48 ln 2).  sincospif takes the angle in half turns, so
// 2 pi u1 is never rounded.  e0: the cos branch, e1: the sin branch.
__device__ __forceinline__ void gauss_pair_of_words(uint32_t w0, uint32_t w1, float& e0, float& e1) {
    const float u0 = (float)((w0 >> 8) + 1u) * (1.0f / 16777216.0f);
    const float u1 = (float)(w1 >> 8) * (1.0f / 16777216.0f);
    const float rad = sqrtf(-2.0f * logf(u0));
    float sn, cs;
    sincospif(2.0f * u1, &sn, &cs);
    e0 = rad * cs;
    e1 = rad * sn;
}

}  // namespace rover
