// svgd_glm_dev.h -- what the GLM kernels' translation units (svgd_glm.hip,
// svgd_glm_predict.hip) share on the device side: the table exponential and
// the occupancy of an 8-wave work-group (internal; device code only).
// Included inside namespace svgd_amd::glm.
#pragma once

#include "svgd_exp_table.h" // EXP2_TAB4096 (each translation unit's copy)

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr double LOG2E = 0x1.71547652b82fep+0;
constexpr int EXP_TB = 4096; // exp table entries
constexpr int NT = 64 * GLM_WAVES;
// exponents below 2^-1100 give exactly 0 (the smallest subnormal is 2^-1074)
constexpr double U_MIN = -1100.0 * EXP_TB;

// 2^(f/4096), |f| <= 1/2: 1 + c1 f + c2 f^2 with the coefficients levelled
// over the interval (relative error <= 2.6e-14, tools/make_exp_table.py)
__device__ __forceinline__ double exp2_4096_poly(double f)
{
    return fma(fma(0x1.ebfbdff82c58fp-27, f, 0x1.62e42ff4f7b0ap-13), f, 1.0);
}

// work-groups of 8 waves that one CU holds at a time: two waves per SIMD each
// (512 VGPRs per lane, allocated in eights), capped by the 160 KiB of LDS
inline int blocks_per_cu(const void *f)
{
    hipFuncAttributes fa;
    if (!f || hipFuncGetAttributes(&fa, f) != hipSuccess) return 1;
    const int regs = (fa.numRegs > 0 ? fa.numRegs + 7 : 8) / 8 * 8;
    const int by_regs = 512 / regs / 2 < 4 ? 512 / regs / 2 : 4;
    const int by_lds = fa.sharedSizeBytes > 0 ? (int)(163840 / fa.sharedSizeBytes) : 4;
    const int b = by_regs < by_lds ? by_regs : by_lds;
    return b > 1 ? b : 1;
}
