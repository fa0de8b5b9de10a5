// svgd_gauss_hess.h -- host-callable launcher of the device Hessian sum of the
// built-in Gaussian-sum model (svgd_gauss_hess.hip; internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svgd_amd {

constexpr int GAUSS_HESS_MAXGRID = 256; // work-groups, each a contiguous range of particle chunks

// work-groups a sum over `rows` particles launches (the rows of `part`)
int gauss_hess_grid(int64_t rows);

// H (d x d row-major) = -sum_i hess log p(x_i) over the `rows` particles X
// (stride d), d <= 64, k components mu (k x d) and prec (k x d x d); part holds
// gauss_hess_grid(rows) * d * d doubles; rows == 0 gives zeros
hipError_t launch_gauss_hess_sum(const double *X, int64_t rows, int d, int k, const double *mu,
                                 const double *prec, double *part, double *H, hipStream_t stream);

} // namespace svgd_amd
