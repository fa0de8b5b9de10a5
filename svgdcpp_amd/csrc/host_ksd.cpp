// host_ksd.cpp -- the kernelized Stein discrepancy on the host, by direct
// differences (svgd_ksd_host), for both kernels.  With s_i = grad log p(x_i),
// r = x_i - x_j, t = |r|^2:
//
//   RBF  k = exp(-a t):        u_ij = k [ s_i.s_j + 2a (s_i - s_j).r + 2ad - 4a^2 t ]
//   IMQ  k = (1 + a t)^(-1/2): u_ij = k s_i.s_j + a k^3 (s_i - s_j).r + a d k^3 - 3 a^2 k^5 t
//
// (both are k s_i.s_j + s_i.grad_y k + s_j.grad_x k + tr grad_x grad_y k of a
// radial k = Psi(t)).  u_ii is taken as |s_i|^2 + 2ad resp. |s_i|^2 + ad.
//   row_i = (1/N) sum_j u_ij,  V = (1/N) sum_i row_i,  U = sum_{i != j} u_ij / (N (N - 1))
//
// Rows are evaluated in parallel with OpenMP, each row's sum in particle
// order; the sums over rows run serially in row order, so the result does not
// depend on the thread count.  The device forms (svgd_ksd.hip,
// svgd_ksd_imq.hip) are checked against this one and against the tests' long
// double restatement.
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include <omp.h>

#include "../../include/svgdcpp_amd/svgd_capi.h"

extern "C" int svgd_ksd_host(int kernel, int dim, int64_t n, const double *X, const double *G, double a,
                             double *ksd2_v, double *ksd2_u, double *rows_out)
{
    if (!X || !G) return SVGD_ERR_ARG;
    if (kernel != SVGD_KERNEL_RBF && kernel != SVGD_KERNEL_IMQ) return SVGD_ERR_ARG;
    if (dim < 1 || n < 1) return SVGD_ERR_DIM;
    if (!std::isfinite(a) || !(a > 0.0)) return SVGD_ERR_ARG;
    const int d = dim;
    const bool imq = kernel == SVGD_KERNEL_IMQ;
    const double inv_n = 1.0 / (double)n;
    std::vector<double> own;
    double *rows = rows_out;
    if (!rows) {
        own.resize((size_t)n);
        rows = own.data();
    }
    std::vector<double> diag((size_t)n);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < n; ++i) {
        const double *xi = X + i * d, *si = G + i * d;
        double ss_i = 0.0;
        for (int c = 0; c < d; ++c) ss_i += si[c] * si[c];
        const double uii = ss_i + (imq ? a * d : 2.0 * a * d);
        double acc = 0.0;
        for (int64_t j = 0; j < n; ++j) {
            if (j == i) {
                acc += uii;
                continue;
            }
            const double *xj = X + j * d, *sj = G + j * d;
            double t = 0.0, ss = 0.0, sr = 0.0;
            for (int c = 0; c < d; ++c) {
                const double r = xi[c] - xj[c];
                t += r * r;
                ss += si[c] * sj[c];
                sr += (si[c] - sj[c]) * r;
            }
            if (imq) {
                const double k = 1.0 / std::sqrt(1.0 + a * t);
                const double k3 = k * k * k;
                acc += k * ss + a * k3 * (sr + d) - 3.0 * a * a * (k3 * k * k) * t;
            } else {
                acc += std::exp(-a * t) * (ss + 2.0 * a * sr + 2.0 * a * d - 4.0 * a * a * t);
            }
        }
        rows[i] = acc * inv_n;
        diag[i] = uii;
    }
    double sr = 0.0, sd = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        sr += rows[i];
        sd += diag[i];
    }
    const double N = (double)n;
    if (ksd2_v) *ksd2_v = sr / N;
    if (ksd2_u) *ksd2_u = n < 2 ? std::numeric_limits<double>::quiet_NaN() : (N * sr - sd) / (N * (N - 1.0));
    return SVGD_OK;
}
