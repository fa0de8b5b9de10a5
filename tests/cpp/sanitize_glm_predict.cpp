// Self-checking driver of the host GLM prediction (svgd_glm_predict_host of
// svgdcpp_amd/csrc/host_glm.cpp) for the ASan + UBSan build
// (`make sanitize_glm_predict`): sizes that reach the edges -- one record, one
// particle, one column, d = 64 -- with and without labels, every optional
// output absent in turn, every refusal, each result checked against the
// definition evaluated here in long double, and guard slots behind every
// output.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/svgdcpp_amd/svgd_capi.h"

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            ++g_fail;                                                                \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                            \
    } while (0)

static double uniform(uint64_t &s) // (-1, 1), splitmix64
{
    s += 0x9e3779b97f4a7c15ULL;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) / 4503599627370496.0 - 1.0;
}

static void one_case(int d, int64_t m, int64_t n, int link)
{
    uint64_t seed = 1000 * (uint64_t)d + 10 * (uint64_t)m + (uint64_t)link;
    std::vector<double> A((size_t)m * d), y((size_t)m), X((size_t)n * d);
    for (double &v : A) v = uniform(seed);
    for (size_t j = 0; j < y.size(); ++j)
        y[j] = link == SVGD_GLM_LOGISTIC ? (j % 3 == 2 ? 0.5 * (uniform(seed) + 1.0) : (uniform(seed) > 0 ? 1.0 : 0.0))
                                         : 3.0 * uniform(seed);
    for (double &v : X) v = 8.0 / std::sqrt((double)d) * uniform(seed);
    const double s = 0.7;
    std::vector<double> mean((size_t)m + 1, -7.0), var((size_t)m + 1, -7.0), lpd((size_t)m + 1, -7.0);
    CHECK(svgd_glm_predict_host(link, s, d, A.data(), y.data(), m, X.data(), n, mean.data(), var.data(),
                                lpd.data()) == SVGD_OK);
    CHECK(mean[(size_t)m] == -7.0 && var[(size_t)m] == -7.0 && lpd[(size_t)m] == -7.0); // nothing past the records
    const long double pi = 3.14159265358979323846264338327950288L;
    for (int64_t j = 0; j < m; ++j) {
        std::vector<long double> mu((size_t)n);
        long double sm = 0.0L, sp = 0.0L, tmean = 0.0L, tmax = 0.0L;
        for (int64_t i = 0; i < n; ++i) {
            long double z = 0.0L, t = 0.0L;
            for (int k = 0; k < d; ++k) {
                z += (long double)A[(size_t)j * d + k] * (long double)X[(size_t)i * d + k];
                t += std::fabs((long double)A[(size_t)j * d + k] * (long double)X[(size_t)i * d + k]);
            }
            tmean += t / (long double)n;
            tmax = std::fmax(tmax, t);
            const long double yj = y[(size_t)j];
            if (link == SVGD_GLM_LOGISTIC) {
                mu[(size_t)i] = 1.0L / (1.0L + std::exp(-z));
                sp += std::exp(yj * z - (std::fmax(z, 0.0L) + std::log1p(std::exp(-std::fabs(z)))));
            } else {
                mu[(size_t)i] = z;
                sp += std::sqrt((long double)s / (2.0L * pi)) * std::exp(-(long double)s * (yj - z) * (yj - z) / 2.0L);
            }
            sm += mu[(size_t)i];
        }
        const long double mref = sm / (long double)n;
        long double vref = 0.0L;
        for (int64_t i = 0; i < n; ++i) vref += (mu[(size_t)i] - mref) * (mu[(size_t)i] - mref);
        vref /= (long double)n;
        const long double lref = std::log(sp / (long double)n);
        // generous forms of the bars of tests/_glm_predict.py (Tbar <= mean T
        // is not guaranteed: 2 tmax covers T + Tbar)
        const long double ay = std::fabs((long double)y[(size_t)j]);
        CHECK(std::fabs((long double)mean[(size_t)j] - mref) <= 1e-13L * (1.0L + 2.0L * tmax));
        CHECK(std::fabs((long double)var[(size_t)j] - vref) <= 1e-13L * (1.0L + 4.0L * tmax * tmax));
        CHECK(var[(size_t)j] >= 0.0);
        CHECK(std::fabs((long double)lpd[(size_t)j] - lref) <=
              2e-13L * (1.0L + (1.0L + ay) * tmax + (long double)s * (ay + tmax) * (ay + tmax) / 2.0L));
        (void)tmean;
    }
    // every optional output absent in turn, and no labels: the same values
    for (int mask = 0; mask < 8; ++mask) {
        std::vector<double> m2((size_t)m + 1, -7.0), v2((size_t)m + 1, -7.0), l2((size_t)m + 1, -7.0);
        const bool labels = (mask & 4) != 0;
        CHECK(svgd_glm_predict_host(link, s, d, A.data(), labels ? y.data() : nullptr, m, X.data(), n,
                                    mask & 1 ? m2.data() : nullptr, mask & 2 ? v2.data() : nullptr,
                                    labels ? l2.data() : nullptr) == SVGD_OK);
        for (int64_t j = 0; j <= m; ++j) {
            CHECK(m2[(size_t)j] == (mask & 1 && j < m ? mean[(size_t)j] : -7.0));
            CHECK(v2[(size_t)j] == (mask & 2 && j < m ? var[(size_t)j] : -7.0));
            CHECK(l2[(size_t)j] == (labels && j < m ? lpd[(size_t)j] : -7.0));
        }
    }
}

static void refusals()
{
    const double A[6] = {0.5, -0.5, 0.25, 1.0, 0.0, -1.0}, y[3] = {0.0, 1.0, 0.5}, X[4] = {0.1, 0.2, -0.3, 0.4};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    double mean[3], var[3], lpd[3];
    CHECK(svgd_glm_predict_host(0, 1.0, 2, A, y, 3, X, 2, mean, var, lpd) == SVGD_OK);
    CHECK(svgd_glm_predict_host(0, 1.0, 2, nullptr, y, 3, X, 2, mean, var, lpd) == SVGD_ERR_ARG);
    CHECK(svgd_glm_predict_host(0, 1.0, 2, A, y, 3, nullptr, 2, mean, var, lpd) == SVGD_ERR_ARG);
    CHECK(svgd_glm_predict_host(7, 1.0, 2, A, y, 3, X, 2, mean, var, lpd) == SVGD_ERR_ARG);
    CHECK(svgd_glm_predict_host(0, 0.0, 2, A, y, 3, X, 2, mean, var, lpd) == SVGD_ERR_ARG);
    CHECK(svgd_glm_predict_host(0, nan, 2, A, y, 3, X, 2, mean, var, lpd) == SVGD_ERR_ARG);
    CHECK(svgd_glm_predict_host(0, 1.0, 2, A, nullptr, 3, X, 2, mean, var, lpd) == SVGD_ERR_ARG);
    CHECK(svgd_glm_predict_host(0, 1.0, 2, A, nullptr, 3, X, 2, mean, var, nullptr) == SVGD_OK);
    CHECK(svgd_glm_predict_host(0, 1.0, 2, A, y, 0, X, 2, mean, var, lpd) == SVGD_ERR_DIM);
    CHECK(svgd_glm_predict_host(0, 1.0, 0, A, y, 3, X, 2, mean, var, lpd) == SVGD_ERR_DIM);
    CHECK(svgd_glm_predict_host(0, 1.0, 2, A, y, 3, X, 0, mean, var, lpd) == SVGD_ERR_DIM);
    for (double bad : {inf, -inf, nan}) {
        double B[6], z[3];
        for (int e = 0; e < 6; ++e) B[e] = A[e];
        for (int e = 0; e < 3; ++e) z[e] = y[e];
        B[5] = bad;
        z[2] = bad;
        CHECK(svgd_glm_predict_host(0, 1.0, 2, B, y, 3, X, 2, mean, var, lpd) == SVGD_ERR_ARG);
        CHECK(svgd_glm_predict_host(1, 1.0, 2, A, z, 3, X, 2, mean, var, lpd) == SVGD_ERR_ARG);
    }
    const double y2[3] = {0.0, 1.5, 0.5};
    CHECK(svgd_glm_predict_host(0, 1.0, 2, A, y2, 3, X, 2, mean, var, lpd) == SVGD_ERR_ARG);
    CHECK(svgd_glm_predict_host(1, 1.0, 2, A, y2, 3, X, 2, mean, var, lpd) == SVGD_OK);
}

int main()
{
    for (int link : {SVGD_GLM_LOGISTIC, SVGD_GLM_GAUSSIAN}) {
        one_case(1, 1, 1, link);
        one_case(3, 5, 63, link);
        one_case(17, 2, 100, link);
        one_case(64, 9, 70, link);
        one_case(8, 130, 3, link);
    }
    refusals();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
