// rover_bf16.h — THE rounding of the bf16 kernels (rover_mlp.hip: chain_bf16<...>; rover_bf16_tile.hip: gru_cell_bf16, linear_bf16), one
// definition for the device and the host, and the pieces every one of them stages its k-slabs with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rover {

// f32 -> bf16, round to nearest even; NaN stays NaN, +-Inf stays +-Inf, a finite f32 above the largest bf16 becomes Inf.  The kernels
// apply it to every input, weight and hidden activation as they read them (hipcc emits v_cvt_pk_bf16_f32 for the cast);
// rover_bf16_round applies it on the host, where tests/test_mlp_bf16_host.py pins it against integer arithmetic on the bits.
__host__ __device__ inline __bf16 bf16_rne(float v) { return (__bf16)v; }

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));       // a float4 at any float address (global_load_dwordx4)
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// LDS rows of 32 bf16 (one k-step of v_mfma_f32_16x16x32_bf16) at a pitch of 40: the 16-byte operand reads of 8 lanes fall on 8
// different bank groups
#define B16_P 40

__device__ __forceinline__ bf16x4 b16_round4(const f32x4& v) { return bf16x4{bf16_rne(v[0]), bf16_rne(v[1]), bf16_rne(v[2]), bf16_rne(v[3])}; }

// elements k .. k + 3 of a row of `len` floats, zero past its end or when the row does not exist
__device__ __forceinline__ f32x4 b16_load4(const float* __restrict__ p, uint32_t k, uint32_t len, bool row_ok) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row_ok) {
        if (k + 4u <= len) v = *reinterpret_cast<const f32x4u*>(p + k);
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (k + e < len) v[e] = p[k + e];
        }
    }
    return v;
}

}  // namespace rover
