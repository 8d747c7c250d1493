// rover_act.h — the scalar activations of the policy kernels, one definition for the f32 kernels (rover_mlp.hip, rover_gru.hip) and the
// bf16 ones (rover_bf16_tile.hip): a bf16 kernel's epilogue is the f32 kernel's, operation for operation.
#pragma once
#include <hip/hip_runtime.h>

namespace rover {

__device__ __forceinline__ float mlp_act(float v, int act) {
    switch (act) {
        case 1: return v > 0.0f ? v : 0.01f * v;                    // nn.LeakyReLU() default slope (model.py:112)
        case 2: return tanhf(v);                                    // nn.Tanh (model.py:115,182)
        case 3: return v > 0.0f ? v : 0.0f;                         // nn.ReLU
        case 4: return v > 0.0f ? v : expm1f(v);                    // nn.ELU (alpha 1)
        default: return v;
    }
}

__device__ __forceinline__ float gru_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }     // expf(+big) = inf -> 0, expf(-big) = 0 -> 1: no NaN

}  // namespace rover
