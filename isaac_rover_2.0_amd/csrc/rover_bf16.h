// rover_bf16.h — THE rounding of the bf16 chain kernels (rover_mlp.hip: chain_bf16<...>), one definition for the device and the host.
#pragma once
#include <hip/hip_runtime.h>

namespace rover {

// f32 -> bf16, round to nearest even; NaN stays NaN, +-Inf stays +-Inf, a finite f32 above the largest bf16 becomes Inf.  The kernels
// apply it to every input, weight and hidden activation as they read them (hipcc emits v_cvt_pk_bf16_f32 for the cast);
// rover_bf16_round applies it on the host, where tests/test_mlp_bf16_host.py pins it against integer arithmetic on the bits.
__host__ __device__ inline __bf16 bf16_rne(float v) { return (__bf16)v; }

}  // namespace rover
