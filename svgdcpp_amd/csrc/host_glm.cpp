// host_glm.cpp -- Bayesian generalized linear model posterior on the host.
//
// Data A (M x d), y (M); prior N(0, I / lambda); a batch window [m0, m0 + B)
// whose sums are scaled by M / B (an unbiased estimate of the full sum):
//
//   z_m     = a_m . theta
//   log p   = s (M/B) sum_m l(y_m, z_m) - (lambda/2) |theta|^2
//   grad    = s (M/B) sum_m r(y_m, z_m) a_m - lambda theta
//   -hess   = s (M/B) sum_m w_m a_m a_m^T + lambda I
//
//   logistic  l = y z - log(1 + e^z),  r = y - sigma(z),  w = sigma (1 - sigma)
//   Gaussian  l = -(y - z)^2 / 2,      r = y - z,         w = 1
//
// log(1 + e^z) is max(z, 0) + log1p(e^-|z|) and sigma(z) is 1 / (1 + e) or
// e / (1 + e) with e = e^-|z|: no overflow and no cancellation in either
// tail.  Particles (rows of X) are evaluated in parallel with OpenMP, each
// row's sums in data order, so the result does not depend on the thread
// count.
#include <cmath>
#include <cstdint>
#include <new>
#include <omp.h>
#include <vector>

#include "../../include/svgdcpp_amd/svgd_capi.h"
#include "host_glm.h"

using svgd_amd::HostGlm;

namespace svgd_amd {
double glm_sigmoid(double z)
{
    const double e = std::exp(-std::fabs(z));
    return z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

int glm_predict_check(int link, double lik_scale, int dim, const double *A, const double *y, int64_t m,
                      const double *lpd_out)
{
    if (!A) return SVGD_ERR_ARG;
    if (link != SVGD_GLM_LOGISTIC && link != SVGD_GLM_GAUSSIAN) return SVGD_ERR_ARG;
    if (!(lik_scale > 0.0) || !std::isfinite(lik_scale)) return SVGD_ERR_ARG;
    if (lpd_out && !y) return SVGD_ERR_ARG;
    if (dim < 1 || m < 1) return SVGD_ERR_DIM;
    for (int64_t e = 0; e < m * dim; ++e)
        if (!std::isfinite(A[e])) return SVGD_ERR_ARG;
    if (y)
        for (int64_t e = 0; e < m; ++e) {
            if (!std::isfinite(y[e])) return SVGD_ERR_ARG;
            if (link == SVGD_GLM_LOGISTIC && !(y[e] >= 0.0 && y[e] <= 1.0)) return SVGD_ERR_ARG;
        }
    return SVGD_OK;
}
} // namespace svgd_amd

namespace {

inline double dotd(const double *a, const double *x, int d)
{
    double z = 0.0;
    for (int k = 0; k < d; ++k) z += a[k] * x[k];
    return z;
}

template <int LINK> void grad_rows(const HostGlm *g, const double *X, int64_t nrows, double *G)
{
    const int d = g->d;
    const double scale = g->lik_scale * ((double)g->m / (double)g->count), lam = g->prior_prec;
    const double *A = g->A.data() + (size_t)g->m0 * d, *y = g->y.data() + g->m0;
    const int64_t B = g->count;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < nrows; ++i) {
        const double *x = X + i * d;
        double *gi = G + i * d;
        for (int k = 0; k < d; ++k) gi[k] = 0.0;
        for (int64_t m = 0; m < B; ++m) {
            const double *a = A + m * d;
            const double z = dotd(a, x, d);
            const double r = LINK == SVGD_GLM_LOGISTIC ? y[m] - svgd_amd::glm_sigmoid(z) : y[m] - z;
            for (int k = 0; k < d; ++k) gi[k] += r * a[k];
        }
        for (int k = 0; k < d; ++k) gi[k] = scale * gi[k] - lam * x[k];
    }
}

// The centred sums of svgd_glm_predict_host for every record: OpenMP over the
// records, each record's sums in particle order.
template <int LINK>
void predict_rows(double lik_scale, int d, const double *A, const double *y, int64_t m, const double *X,
                  int64_t nrows, const double *xbar, double *mean_out, double *var_out, double *lpd_out)
{
    const double N = (double)nrows, half_s = 0.5 * lik_scale;
    const double lconst = svgd_amd::glm_predict_lconst(LINK, lik_scale);
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < m; ++j) {
        const double *a = A + j * d;
        const double zbar = dotd(a, xbar, d);
        const double c = LINK == SVGD_GLM_LOGISTIC ? svgd_amd::glm_sigmoid(zbar) : zbar;
        const double yj = y ? y[j] : 0.0;
        double sa = 0.0, sb = 0.0, sl = 0.0;
        for (int64_t i = 0; i < nrows; ++i) {
            const double z = dotd(a, X + i * d, d);
            double dv, pv = 0.0;
            if (LINK == SVGD_GLM_LOGISTIC) {
                // sigma and exp(l) from e = exp(-|z|): no cancelling 1 - sigma
                const double az = std::fabs(z), e = std::exp(-az), q = 1.0 + e;
                dv = (z >= 0.0 ? 1.0 : e) / q - c;
                if (y) {
                    const double t = z >= 0.0 ? 1.0 - yj : yj;
                    pv = (t == 0.0 ? 1.0 : t == 1.0 ? e : std::exp(-(az * t))) / q;
                }
            } else {
                dv = z - c;
                if (y) {
                    const double r = yj - z;
                    pv = std::exp(-((half_s * r) * r));
                }
            }
            sa += dv;
            sb += dv * dv;
            sl += pv;
        }
        svgd_amd::glm_predict_finalize(c, sa, sb, sl, N, lconst, mean_out ? mean_out + j : nullptr,
                                       var_out ? var_out + j : nullptr, lpd_out ? lpd_out + j : nullptr);
    }
}

} // namespace

extern "C" {

int svgd_glm_predict_host(int link, double lik_scale, int dim, const double *A, const double *y, int64_t m,
                          const double *X, int64_t nrows, double *mean_out, double *var_out, double *lpd_out)
{
    // mean_m = (1/N) sum_i mu(z_im), var_m its spread over the particles and
    // lpd_m = log (1/N) sum_i p(y_m | z_im), from sums centred on
    // c_m = mu(a_m . theta_bar) so that the variance does not cancel
    const int rc = svgd_amd::glm_predict_check(link, lik_scale, dim, A, y, m, lpd_out);
    if (rc != SVGD_OK) return rc;
    if (!X) return SVGD_ERR_ARG;
    if (nrows < 1) return SVGD_ERR_DIM;
    std::vector<double> xbar;
    try {
        xbar.assign((size_t)dim, 0.0);
    } catch (const std::bad_alloc &) {
        return SVGD_ERR_RUNTIME;
    }
    for (int64_t i = 0; i < nrows; ++i)
        for (int k = 0; k < dim; ++k) xbar[(size_t)k] += X[i * dim + k];
    for (int k = 0; k < dim; ++k) xbar[(size_t)k] /= (double)nrows;
    if (link == SVGD_GLM_LOGISTIC)
        predict_rows<SVGD_GLM_LOGISTIC>(lik_scale, dim, A, y, m, X, nrows, xbar.data(), mean_out, var_out, lpd_out);
    else
        predict_rows<SVGD_GLM_GAUSSIAN>(lik_scale, dim, A, y, m, X, nrows, xbar.data(), mean_out, var_out, lpd_out);
    return SVGD_OK;
}

int svgd_glm_create(void **out, int dim, int64_t m, const double *A, const double *y, int link,
                    double lik_scale, double prior_prec)
{
    if (!out || !A || !y) return SVGD_ERR_ARG;
    if (dim < 1 || m < 1) return SVGD_ERR_DIM;
    if (link != SVGD_GLM_LOGISTIC && link != SVGD_GLM_GAUSSIAN) return SVGD_ERR_ARG;
    if (!(lik_scale > 0.0) || !std::isfinite(lik_scale)) return SVGD_ERR_ARG;
    if (!(prior_prec >= 0.0) || !std::isfinite(prior_prec)) return SVGD_ERR_ARG;
    for (int64_t e = 0; e < m * dim; ++e)
        if (!std::isfinite(A[e])) return SVGD_ERR_ARG;
    for (int64_t e = 0; e < m; ++e) {
        if (!std::isfinite(y[e])) return SVGD_ERR_ARG;
        if (link == SVGD_GLM_LOGISTIC && !(y[e] >= 0.0 && y[e] <= 1.0)) return SVGD_ERR_ARG;
    }
    HostGlm *g = new (std::nothrow) HostGlm();
    if (!g) return SVGD_ERR_RUNTIME;
    try {
        g->A.assign(A, A + (size_t)m * dim);
        g->y.assign(y, y + (size_t)m);
    } catch (const std::bad_alloc &) {
        delete g;
        return SVGD_ERR_RUNTIME;
    }
    g->d = dim;
    g->m = m;
    g->link = link;
    g->lik_scale = lik_scale;
    g->prior_prec = prior_prec;
    g->m0 = 0;
    g->count = m;
    *out = g;
    return SVGD_OK;
}

int svgd_glm_destroy(void *model)
{
    delete static_cast<HostGlm *>(model);
    return SVGD_OK;
}

int svgd_glm_set_batch(void *model, int64_t m0, int64_t count)
{
    HostGlm *g = static_cast<HostGlm *>(model);
    if (!g) return SVGD_ERR_ARG;
    if (m0 < 0 || count < 1 || m0 > g->m || count > g->m - m0) return SVGD_ERR_ARG;
    g->m0 = m0;
    g->count = count;
    return SVGD_OK;
}

int svgd_glm_logp(void *model, const double *X, int64_t nrows, double *out)
{
    const HostGlm *g = static_cast<const HostGlm *>(model);
    if (!g || nrows < 0 || (!X && nrows > 0) || (!out && nrows > 0)) return SVGD_ERR_ARG;
    const int d = g->d;
    const double scale = g->lik_scale * ((double)g->m / (double)g->count), lam = g->prior_prec;
    const double *A = g->A.data() + (size_t)g->m0 * d, *y = g->y.data() + g->m0;
    const int64_t B = g->count;
    const bool logistic = g->link == SVGD_GLM_LOGISTIC;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < nrows; ++i) {
        const double *x = X + i * d;
        double sum = 0.0;
        for (int64_t m = 0; m < B; ++m) {
            const double z = dotd(A + m * d, x, d);
            if (logistic) {
                sum += y[m] * z - (std::fmax(z, 0.0) + std::log1p(std::exp(-std::fabs(z))));
            } else {
                const double r = y[m] - z;
                sum -= 0.5 * r * r;
            }
        }
        out[i] = scale * sum - 0.5 * lam * dotd(x, x, d);
    }
    return SVGD_OK;
}

int svgd_glm_logp_grad(void *model, const double *X, int64_t nrows, double *G)
{
    const HostGlm *g = static_cast<const HostGlm *>(model);
    if (!g || nrows < 0 || (!X && nrows > 0) || (!G && nrows > 0)) return SVGD_ERR_ARG;
    if (g->link == SVGD_GLM_LOGISTIC) grad_rows<SVGD_GLM_LOGISTIC>(g, X, nrows, G);
    else grad_rows<SVGD_GLM_GAUSSIAN>(g, X, nrows, G);
    return SVGD_OK;
}

int svgd_glm_neg_hess_sum(void *model, const double *X, int64_t nrows, double *H)
{
    // sum_i [ s (M/B) sum_m w_im a_m a_m^T + lambda I ]: the per-row weights
    // are summed over the particles first (W_m = sum_i w_im, i ascending),
    // then one weighted Gram product of the data
    const HostGlm *g = static_cast<const HostGlm *>(model);
    if (!g || !H || nrows < 0 || (!X && nrows > 0)) return SVGD_ERR_ARG;
    const int d = g->d;
    const double scale = g->lik_scale * ((double)g->m / (double)g->count), lam = g->prior_prec;
    const double *A = g->A.data() + (size_t)g->m0 * d;
    const int64_t B = g->count;
    std::vector<double> W;
    try {
        W.assign((size_t)B, (double)nrows);
    } catch (const std::bad_alloc &) {
        return SVGD_ERR_RUNTIME;
    }
    if (g->link == SVGD_GLM_LOGISTIC) {
#pragma omp parallel for schedule(static)
        for (int64_t m = 0; m < B; ++m) {
            double w = 0.0;
            for (int64_t i = 0; i < nrows; ++i) {
                const double sg = svgd_amd::glm_sigmoid(dotd(A + m * d, X + i * d, d));
                w += sg * (1.0 - sg);
            }
            W[(size_t)m] = w;
        }
    }
    for (int r = 0; r < d; ++r)
        for (int l = 0; l < d; ++l) {
            double h = 0.0;
            for (int64_t m = 0; m < B; ++m) h += W[(size_t)m] * A[m * d + r] * A[m * d + l];
            H[(size_t)r * d + l] = scale * h + (r == l ? lam * (double)nrows : 0.0);
        }
    return SVGD_OK;
}

} // extern "C"
