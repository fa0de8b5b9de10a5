// Self-checking driver of the host GLM (svgdcpp_amd/csrc/host_glm.cpp) for the
// ASan + UBSan build (`make sanitize_glm`): every svgd_glm_* entry point at
// sizes that reach the edges -- one row, one column, windows at both ends of
// the data, zero particles -- plus every refusal, each result checked against
// the definition evaluated here in long double.
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

static void one_case(int d, int64_t M, int link, int64_t m0, int64_t cnt, int64_t n)
{
    uint64_t seed = 1000 * (uint64_t)d + (uint64_t)M + (uint64_t)link;
    std::vector<double> A((size_t)M * d), y((size_t)M), X((size_t)n * d + 1);
    for (double &v : A) v = uniform(seed);
    for (double &v : y) v = link == SVGD_GLM_LOGISTIC ? (uniform(seed) > 0 ? 1.0 : 0.0) : 3.0 * uniform(seed);
    for (double &v : X) v = 8.0 / std::sqrt((double)d) * uniform(seed);
    const double s = 0.7, lam = 1.3;
    void *h = nullptr;
    CHECK(svgd_glm_create(&h, d, M, A.data(), y.data(), link, s, lam) == SVGD_OK);
    CHECK(svgd_glm_set_batch(h, m0, cnt) == SVGD_OK);
    std::vector<double> G((size_t)n * d + 1, -7.0), lp((size_t)n + 1, -7.0), H((size_t)d * d);
    CHECK(svgd_glm_logp_grad(h, X.data(), n, G.data()) == SVGD_OK);
    CHECK(svgd_glm_logp(h, X.data(), n, lp.data()) == SVGD_OK);
    CHECK(svgd_glm_neg_hess_sum(h, X.data(), n, H.data()) == SVGD_OK);
    CHECK(G[(size_t)n * d] == -7.0 && lp[(size_t)n] == -7.0); // nothing written past the rows
    const long double f = (long double)s * (long double)M / (long double)cnt;
    std::vector<long double> Href((size_t)d * d, 0.0L);
    for (int64_t i = 0; i < n; ++i) {
        std::vector<long double> g((size_t)d, 0.0L), mag((size_t)d, 0.0L);
        long double l = 0.0L, lmag = 0.0L, nrm = 0.0L;
        for (int64_t m = m0; m < m0 + cnt; ++m) {
            long double z = 0.0L;
            for (int k = 0; k < d; ++k) z += (long double)A[(size_t)m * d + k] * (long double)X[(size_t)i * d + k];
            long double r, w, lm;
            if (link == SVGD_GLM_LOGISTIC) {
                const long double sg = 1.0L / (1.0L + std::exp(-z));
                r = (long double)y[(size_t)m] - sg;
                w = sg * (1.0L - sg);
                lm = (long double)y[(size_t)m] * z - (std::fmax(z, 0.0L) + std::log1p(std::exp(-std::fabs(z))));
            } else {
                r = (long double)y[(size_t)m] - z;
                w = 1.0L;
                lm = -r * r / 2.0L;
            }
            l += lm;
            lmag += std::fabs(lm) + std::fabs(z) + 1.0L;
            for (int k = 0; k < d; ++k) {
                g[(size_t)k] += r * (long double)A[(size_t)m * d + k];
                mag[(size_t)k] += (std::fabs(r) + 1.0L) * std::fabs((long double)A[(size_t)m * d + k]);
                for (int q = 0; q < d; ++q)
                    Href[(size_t)k * d + q] += f * w * (long double)A[(size_t)m * d + k] * (long double)A[(size_t)m * d + q];
            }
        }
        for (int k = 0; k < d; ++k) {
            const long double x = X[(size_t)i * d + k];
            nrm += x * x;
            const long double ref = f * g[(size_t)k] - (long double)lam * x;
            const long double bar = 1e-13L * (f * mag[(size_t)k] + (long double)lam * std::fabs(x));
            CHECK(std::fabs((long double)G[(size_t)i * d + k] - ref) <= bar);
            Href[(size_t)k * d + k] += (long double)lam;
        }
        const long double lref = f * l - (long double)lam / 2.0L * nrm;
        CHECK(std::fabs((long double)lp[(size_t)i] - lref) <= 1e-13L * (f * lmag + (long double)lam * nrm));
    }
    for (int k = 0; k < d; ++k)
        for (int q = 0; q < d; ++q)
            CHECK(std::fabs((long double)H[(size_t)k * d + q] - Href[(size_t)k * d + q]) <=
                  1e-12L * (std::fabs(Href[(size_t)k * d + q]) + f * (long double)cnt * (long double)n + 1.0L));
    CHECK(svgd_glm_destroy(h) == SVGD_OK);
}

static void refusals()
{
    const double A[6] = {0.5, -0.5, 0.25, 1.0, 0.0, -1.0}, y[3] = {0.0, 1.0, 0.5};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    void *h = nullptr;
    CHECK(svgd_glm_create(nullptr, 2, 3, A, y, 0, 1.0, 1.0) == SVGD_ERR_ARG);
    CHECK(svgd_glm_create(&h, 2, 3, nullptr, y, 0, 1.0, 1.0) == SVGD_ERR_ARG);
    CHECK(svgd_glm_create(&h, 2, 3, A, nullptr, 0, 1.0, 1.0) == SVGD_ERR_ARG);
    CHECK(svgd_glm_create(&h, 0, 3, A, y, 0, 1.0, 1.0) == SVGD_ERR_DIM);
    CHECK(svgd_glm_create(&h, 2, 0, A, y, 0, 1.0, 1.0) == SVGD_ERR_DIM);
    CHECK(svgd_glm_create(&h, 2, 3, A, y, 7, 1.0, 1.0) == SVGD_ERR_ARG);
    CHECK(svgd_glm_create(&h, 2, 3, A, y, 0, 0.0, 1.0) == SVGD_ERR_ARG);
    CHECK(svgd_glm_create(&h, 2, 3, A, y, 0, nan, 1.0) == SVGD_ERR_ARG);
    CHECK(svgd_glm_create(&h, 2, 3, A, y, 0, 1.0, -1.0) == SVGD_ERR_ARG);
    for (double bad : {inf, -inf, nan}) {
        double B[6], z[3];
        for (int e = 0; e < 6; ++e) B[e] = A[e];
        for (int e = 0; e < 3; ++e) z[e] = y[e];
        B[5] = bad;
        z[2] = bad;
        CHECK(svgd_glm_create(&h, 2, 3, B, y, 0, 1.0, 1.0) == SVGD_ERR_ARG);
        CHECK(svgd_glm_create(&h, 2, 3, A, z, 1, 1.0, 1.0) == SVGD_ERR_ARG);
    }
    const double y2[3] = {0.0, 1.5, 0.5};
    CHECK(svgd_glm_create(&h, 2, 3, A, y2, 0, 1.0, 1.0) == SVGD_ERR_ARG);
    CHECK(h == nullptr);
    CHECK(svgd_glm_create(&h, 2, 3, A, y2, 1, 1.0, 0.0) == SVGD_OK);
    CHECK(svgd_glm_set_batch(h, 0, 0) == SVGD_ERR_ARG);
    CHECK(svgd_glm_set_batch(h, 2, 2) == SVGD_ERR_ARG);
    CHECK(svgd_glm_set_batch(h, 3, 1) == SVGD_ERR_ARG);
    CHECK(svgd_glm_set_batch(h, -1, 1) == SVGD_ERR_ARG);
    CHECK(svgd_glm_set_batch(h, INT64_MAX, INT64_MAX) == SVGD_ERR_ARG);
    CHECK(svgd_glm_set_batch(nullptr, 0, 1) == SVGD_ERR_ARG);
    CHECK(svgd_glm_set_batch(h, 2, 1) == SVGD_OK);
    double X[2] = {0.1, 0.2}, G[2], H[4], lp;
    CHECK(svgd_glm_logp_grad(h, nullptr, 1, G) == SVGD_ERR_ARG);
    CHECK(svgd_glm_logp_grad(h, X, 1, nullptr) == SVGD_ERR_ARG);
    CHECK(svgd_glm_logp_grad(nullptr, X, 1, G) == SVGD_ERR_ARG);
    CHECK(svgd_glm_logp_grad(h, X, -1, G) == SVGD_ERR_ARG);
    CHECK(svgd_glm_logp(h, X, 1, nullptr) == SVGD_ERR_ARG);
    CHECK(svgd_glm_neg_hess_sum(h, X, 1, nullptr) == SVGD_ERR_ARG);
    CHECK(svgd_glm_logp_grad(h, nullptr, 0, nullptr) == SVGD_OK); // no rows: nothing read
    CHECK(svgd_glm_logp(h, X, 1, &lp) == SVGD_OK);
    CHECK(svgd_glm_neg_hess_sum(h, X, 1, H) == SVGD_OK);
    CHECK(svgd_glm_destroy(h) == SVGD_OK);
    CHECK(svgd_glm_destroy(nullptr) == SVGD_OK);
}

int main()
{
    for (int link : {SVGD_GLM_LOGISTIC, SVGD_GLM_GAUSSIAN}) {
        one_case(1, 1, link, 0, 1, 3);
        one_case(3, 63, link, 0, 63, 5);
        one_case(3, 64, link, 3, 61, 5);
        one_case(17, 100, link, 99, 1, 2);
        one_case(64, 70, link, 6, 64, 9);
        one_case(8, 10, link, 0, 10, 0);
    }
    refusals();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
