// Internal layout of the generalized-linear-model handle (host_glm.cpp),
// shared with the C ABI so a context can mirror the data on the device.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/svgdcpp_amd/svgd_capi.h"

namespace svgd_amd {
struct HostGlm {
    int d = 0;
    int64_t m = 0;         // data rows
    int link = 0;          // SVGD_GLM_LOGISTIC / SVGD_GLM_GAUSSIAN
    double lik_scale = 1;  // s
    double prior_prec = 1; // lambda
    int64_t m0 = 0, count = 0; // batch window [m0, m0 + count)
    std::vector<double> A; // m x d, row-major
    std::vector<double> y; // m
};
// sigma(z) from e = exp(-|z|) in both tails (no overflow, no cancellation)
double glm_sigmoid(double z);

// ---- posterior prediction (svgd_glm_predict_host, svgd_glm_predict)
// The argument checks both entry points share: SVGD_OK, or the code of the
// first refusal (svgd_capi.h).
int glm_predict_check(int link, double lik_scale, int dim, const double *A, const double *y, int64_t m,
                      const double *lpd_out);
// mean, variance and log predictive density of one record from its centred
// sums over all N particles: c = mu(a . theta_bar), sa = sum (mu - c),
// sb = sum (mu - c)^2, sl = sum exp(l); lconst = log(s / 2 pi) / 2 (Gaussian
// link) or 0.  Any output may be null.
inline void glm_predict_finalize(double c, double sa, double sb, double sl, double N, double lconst,
                                 double *mean, double *var, double *lpd)
{
    const double ma = sa / N;
    if (mean) *mean = c + ma;
    if (var) *var = std::fmax(0.0, sb / N - ma * ma);
    if (lpd) *lpd = std::log(sl / N) + lconst;
}
// lconst of the link
inline double glm_predict_lconst(int link, double lik_scale)
{
    return link == SVGD_GLM_GAUSSIAN ? 0.5 * std::log(lik_scale / 6.283185307179586476925) : 0.0;
}
} // namespace svgd_amd
