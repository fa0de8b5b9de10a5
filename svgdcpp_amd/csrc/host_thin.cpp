// host_thin.cpp -- Stein thinning on the host (svgd_stein_thin_host): the
// greedy choice of m points whose empirical measure has the smallest
// kernelized Stein discrepancy (Riabiz et al. 2022), for both kernels, by
// direct differences.  With u_ij and u_ii of host_ksd.cpp:
//
//   acc_0[j] = 0
//   for t = 1..m:
//       obj_t[j] = u_jj / 2 + acc_{t-1}[j]
//       pi_t     = the smallest j that attains min_j obj_t[j]
//       S_t      = S_{t-1} + 2 acc_{t-1}[pi_t] + u_{pi_t pi_t}
//       ksd2_t   = S_t / t^2        (= KSD^2_V of the multiset {pi_1..pi_t})
//       acc_t[j] = acc_{t-1}[j] + u(pi_t, j)      (u(pi, pi) = u_{pi pi} by index)
//
// Inside a pick, j runs in parallel with OpenMP over fixed blocks of BLK
// candidates: each block updates its acc and leaves its own (min, argmin); the
// blocks' minima are compared serially in block order.  A minimum of exact
// comparisons does not depend on how it is grouped, so the result does not
// depend on the thread count.  An objective that is not a number counts as
// +inf (the rule of svgd_thin.hip).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include <omp.h>

#include "../../include/svgdcpp_amd/svgd_capi.h"

extern "C" int svgd_stein_thin_host(int kernel, int dim, int64_t n, const double *X, const double *G, double a,
                                    int64_t m, int64_t *idx_out, double *ksd2_out)
{
    if (!X || !G) return SVGD_ERR_ARG;
    if (kernel != SVGD_KERNEL_RBF && kernel != SVGD_KERNEL_IMQ) return SVGD_ERR_ARG;
    if (dim < 1 || n < 1) return SVGD_ERR_DIM;
    if (!std::isfinite(a) || !(a > 0.0)) return SVGD_ERR_ARG;
    if (m < 1) return SVGD_ERR_ARG;
    const int d = dim;
    const bool imq = kernel == SVGD_KERNEL_IMQ;
    const double inf = std::numeric_limits<double>::infinity();
    constexpr int64_t BLK = 1024;
    const int64_t nblk = (n + BLK - 1) / BLK;
    std::vector<double> diag((size_t)n), acc((size_t)n, 0.0), bval((size_t)nblk);
    std::vector<int64_t> bidx((size_t)nblk);
    // obj_1 = u_jj / 2
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < nblk; ++b) {
        double best = inf;
        int64_t bj = b * BLK;
        for (int64_t j = b * BLK; j < std::min(n, (b + 1) * BLK); ++j) {
            const double *sj = G + j * d;
            double ss = 0.0;
            for (int c = 0; c < d; ++c) ss += sj[c] * sj[c];
            diag[j] = ss + (imq ? a * d : 2.0 * a * d);
            const double obj = 0.5 * diag[j];
            if (obj < best) {
                best = obj;
                bj = j;
            }
        }
        bval[b] = best;
        bidx[b] = bj;
    }
    double S = 0.0;
    bool finite = true;
    for (int64_t t = 1; t <= m; ++t) {
        double best = bval[0];
        int64_t pi = bidx[0];
        for (int64_t b = 1; b < nblk; ++b)
            if (bval[b] < best) {
                best = bval[b];
                pi = bidx[b];
            }
        S += 2.0 * acc[pi] + diag[pi];
        const double ksd2 = S / ((double)t * (double)t);
        finite = finite && std::isfinite(ksd2);
        if (idx_out) idx_out[t - 1] = pi;
        if (ksd2_out) ksd2_out[t - 1] = ksd2;
        if (t == m) break;
        const double *xi = X + pi * d, *si = G + pi * d;
#pragma omp parallel for schedule(static)
        for (int64_t b = 0; b < nblk; ++b) {
            double bb = inf;
            int64_t bj = b * BLK;
            for (int64_t j = b * BLK; j < std::min(n, (b + 1) * BLK); ++j) {
                double u = diag[j];
                if (j != pi) {
                    const double *xj = X + j * d, *sj = G + j * d;
                    double r2 = 0.0, ss = 0.0, sr = 0.0;
                    for (int c = 0; c < d; ++c) {
                        const double r = xi[c] - xj[c];
                        r2 += r * r;
                        ss += si[c] * sj[c];
                        sr += (si[c] - sj[c]) * r;
                    }
                    if (imq) {
                        const double k = 1.0 / std::sqrt(1.0 + a * r2);
                        const double k3 = k * k * k;
                        u = k * ss + a * k3 * (sr + d) - 3.0 * a * a * (k3 * k * k) * r2;
                    } else {
                        u = std::exp(-a * r2) * (ss + 2.0 * a * sr + 2.0 * a * d - 4.0 * a * a * r2);
                    }
                }
                acc[j] += u;
                const double obj = 0.5 * diag[j] + acc[j];
                if (obj < bb) { // (false for a NaN: it counts as +inf)
                    bb = obj;
                    bj = j;
                }
            }
            bval[b] = bb;
            bidx[b] = bj;
        }
    }
    return finite ? SVGD_OK : SVGD_ERR_RUNTIME;
}
