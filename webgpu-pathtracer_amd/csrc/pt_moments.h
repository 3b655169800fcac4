// pt_moments.h -- what the kernels that READ the moments image (include/mi3pt.h: mi3pt_set_moments) share: pt_guided.hip
// (MI3PT_GUIDED_VARIANCE) and pt_converge.hip (mi3pt_estimate_convergence)
#pragma once
#include "pt_devmath.h"

namespace pt {

// v of one moments texel: the variance of the mean summed over rgb, 0 with fewer than two samples; fmaxf drops a NaN
PT_DEV float moments_variance(const float4 m)
{
    const float sum = (m.x + m.y) + m.z;
    return m.w >= 2.0f ? fmaxf(sum / (m.w * (m.w - 1.0f)), 0.0f) : 0.0f;
}

}  // namespace pt
