// svgd_imq_dev.h -- device helpers the inverse multiquadric kernels share
// (svgd_imq.hip, svgd_ksd_imq.hip; internal, device code only).
#pragma once
#include <hip/hip_runtime.h>

namespace svgd_amd {
namespace imq {

// s^(-1/2) for 1 <= s <= 1e300, to fp64 rounding: the hardware seed, one
// third-order step and one Newton step, each on the residual e = 1 - s y^2
// (the second step leaves a seed of relative error as large as 1e-4 below
// 1e-16); no division
__device__ __forceinline__ double rsqrt_full(double s)
{
    double y = __builtin_amdgcn_rsq(s);
    double e = fma(-(s * y), y, 1.0);
    y = fma(y * e, fma(0.375, e, 0.5), y);
    e = fma(-(s * y), y, 1.0);
    return fma(0.5 * y, e, y);
}

} // namespace imq
} // namespace svgd_amd
