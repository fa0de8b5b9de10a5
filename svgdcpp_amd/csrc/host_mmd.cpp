// host_mmd.cpp -- the maximum mean discrepancy between two point sets on the
// host, by direct differences (svgd_mmd_host), for both kernels.  With
// t = |x - y|^2:
//
//   RBF  k = exp(-a t)            IMQ  k = (1 + a t)^(-1/2)
//   Sxx = sum_{i,j<N} k(x_i, x_j), Syy = sum_{i,j<M} k(y_i, y_j)   (the diagonal counts 1 each)
//   Sxy = sum_{i<N} sum_{j<M} k(x_i, y_j)
//   MMD2_V = Sxx / N^2 + Syy / M^2 - 2 Sxy / (N M)
//   MMD2_U = (Sxx - N) / (N (N - 1)) + (Syy - M) / (M (M - 1)) - 2 Sxy / (N M)
//   wit_i  = (1/N) sum_j k(x_i, x_j) - (1/M) sum_j k(x_i, y_j)
//
// No centring and no Gram form.  Rows are evaluated in parallel with OpenMP,
// each row's sum in column order; the sums over rows run serially in row
// order, so the result does not depend on the thread count.  The device form
// (svgd_mmd.hip) is checked against this one and against the tests' long
// double restatement.
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include <omp.h>

#include "../../include/svgdcpp_amd/svgd_capi.h"

namespace {

// row sums of k(a_i, b_j) over j < nb for every i < na; same: the two sets are
// one, and the column j = i counts exactly 1
void row_sums(bool imq, int d, double a, int64_t na, const double *A, int64_t nb, const double *B, bool same,
              double *rows)
{
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < na; ++i) {
        const double *xi = A + i * d;
        double acc = 0.0;
        for (int64_t j = 0; j < nb; ++j) {
            if (same && j == i) {
                acc += 1.0;
                continue;
            }
            const double *yj = B + j * d;
            double t = 0.0;
            for (int c = 0; c < d; ++c) {
                const double r = xi[c] - yj[c];
                t += r * r;
            }
            acc += imq ? 1.0 / std::sqrt(1.0 + a * t) : std::exp(-a * t);
        }
        rows[i] = acc;
    }
}

double sum_in_order(const std::vector<double> &v)
{
    double s = 0.0;
    for (double x : v) s += x;
    return s;
}

} // namespace

extern "C" int svgd_mmd_host(int kernel, int dim, int64_t n, const double *X, int64_t m, const double *Y,
                             double a, double *mmd2_v, double *mmd2_u, double *means3_out,
                             double *witness_out)
{
    if (!X || !Y) return SVGD_ERR_ARG;
    if (kernel != SVGD_KERNEL_RBF && kernel != SVGD_KERNEL_IMQ) return SVGD_ERR_ARG;
    if (dim < 1 || n < 1 || m < 1) return SVGD_ERR_DIM;
    if (!std::isfinite(a) || !(a > 0.0)) return SVGD_ERR_ARG;
    for (int64_t e = 0; e < m * dim; ++e)
        if (!std::isfinite(Y[e])) return SVGD_ERR_ARG;
    const bool imq = kernel == SVGD_KERNEL_IMQ;
    std::vector<double> rxx((size_t)n), rxy((size_t)n), ryy((size_t)m);
    row_sums(imq, dim, a, n, X, n, X, true, rxx.data());
    row_sums(imq, dim, a, n, X, m, Y, false, rxy.data());
    row_sums(imq, dim, a, m, Y, m, Y, true, ryy.data());
    const double sxx = sum_in_order(rxx), sxy = sum_in_order(rxy), syy = sum_in_order(ryy);
    const double N = (double)n, M = (double)m;
    const double mxx = sxx / (N * N), myy = syy / (M * M), mxy = sxy / (N * M);
    if (mmd2_v) *mmd2_v = mxx + myy - 2.0 * mxy;
    if (mmd2_u)
        *mmd2_u = n < 2 || m < 2 ? std::numeric_limits<double>::quiet_NaN()
                                 : (sxx - N) / (N * (N - 1.0)) + (syy - M) / (M * (M - 1.0)) - 2.0 * mxy;
    if (means3_out) {
        means3_out[0] = mxx;
        means3_out[1] = myy;
        means3_out[2] = mxy;
    }
    if (witness_out)
        for (int64_t i = 0; i < n; ++i) witness_out[i] = rxx[(size_t)i] / N - rxy[(size_t)i] / M;
    return SVGD_OK;
}
