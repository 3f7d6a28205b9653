// The one piece the option-critic's launches share (option.hip: asac_option_return, asac_termination_loss_grad;
// discrete.hip: asac_option_discrete_return): the mean of the options' values at one state.  ONE implementation: the
// three launches form it with the same bits.
#pragma once
#include "asac_common.h"

namespace asac {

// mean_o V[b, t, o]: loads in groups of four requested together (indices beyond O re-read the last option: a valid
// address, the value is not added), added in option order
__device__ __forceinline__ float option_mean(const float* v, int64_t so, int O) {
    float s = 0.f;
    for (int o0 = 0; o0 < O; o0 += 4) {
        float x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = v[(int64_t)min(o0 + j, O - 1) * so];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (o0 + j < O) s += x[j];
    }
    return s / (float)O;
}

}  // namespace asac
