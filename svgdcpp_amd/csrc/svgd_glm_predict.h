// svgd_glm_predict.h -- host-callable launchers of the device GLM posterior
// prediction (svgd_glm_predict.hip; internal).
//
// For the test records a_m (m < count; [a | 0.. | y | 0..] at glm_rec_stride(d),
// one zero tile behind them) and the particles theta_i:
//   z_im = a_m . theta_i,  mu = sigma (logistic) or the identity (Gaussian link)
//   c_m  = mu(a_m . theta_bar)                  the centre, theta_bar the particles' mean
//   A_m  = sum_i (mu(z_im) - c_m)
//   B_m  = sum_i (mu(z_im) - c_m)^2
//   L_m  = sum_i exp(l(y_m, z_im))              (has_y)
//     logistic  exp(l) = exp(-|z| t) / (1 + e^-|z|),  t = (z >= 0 ? 1 - y : y)
//     Gaussian  exp(l) = exp(-half_s (y - z)^2)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svgd_glm.h"

namespace svgd_amd {

// work-groups of the pass for this (d, link, has_y) that one CU holds at a time
int glm_predict_blocks_per_cu(int d, int link, int has_y);

// cvec[m] = c_m for m < count: one thread per record, the dot product in
// coordinate order; mu holds the d column means of the particles
hipError_t launch_glm_predict_center(int d, int link, const double *rec, int64_t count, const double *mu,
                                     double *cvec, hipStream_t stream);
// sums[q][m] (q < 2 + has_y: A, B, L; stride count) over the `nrows` particles
// X (stride d), in S ranges of the particles' tiles (1 <= S <= glm_tiles(nrows))
// added in ascending order; part holds S * 3 * glm_wgroups(count) *
// GLM_ROWS_PER_WG doubles.  nrows == 0: zeros, nothing is launched.
hipError_t launch_glm_predict(int d, int link, int has_y, double half_s, const double *X, int64_t nrows,
                              const double *rec, const double *cvec, int64_t count, int S, double *part,
                              double *sums, hipStream_t stream);

} // namespace svgd_amd
