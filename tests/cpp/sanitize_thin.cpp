// Self-checking driver of the host Stein thinning (svgd_stein_thin_host of
// svgdcpp_amd/csrc/host_thin.cpp) for the ASan + UBSan build
// (`make sanitize_thin`): both kernels, sizes that reach the edges -- one
// particle, one column, d = 64, a candidate count past one block of the
// host's 1024, m > n -- into exactly sized heap buffers, every combination of
// NULL outputs, every refusal, each selection replayed through the definition
// evaluated here in long double, and a guard slot behind each output.
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

static void one_case(int kernel, int d, int64_t n, double a, int64_t m)
{
    uint64_t seed = 1000 * (uint64_t)d + (uint64_t)n;
    std::vector<double> X((size_t)n * d), G((size_t)n * d);
    for (double &v : X) v = 2.0 * uniform(seed);
    for (double &v : G) v = 8.0 * uniform(seed);
    std::vector<int64_t> idx((size_t)m + 1, -7);
    std::vector<double> ksd2((size_t)m + 1, -7.0);
    for (int mask : {3, 0, 1, 2}) { // which outputs are asked for; both first
        std::vector<int64_t> i2((size_t)m + 1, -7);
        std::vector<double> k2((size_t)m + 1, -7.0);
        CHECK(svgd_stein_thin_host(kernel, d, n, X.data(), G.data(), a, m, mask & 1 ? i2.data() : nullptr,
                                   mask & 2 ? k2.data() : nullptr) == SVGD_OK);
        CHECK(i2[(size_t)m] == -7 && k2[(size_t)m] == -7.0); // nothing past the m slots
        if (!(mask & 1)) CHECK(i2[0] == -7);
        if (!(mask & 2)) CHECK(k2[0] == -7.0);
        if (mask == 3) {
            idx = i2;
            ksd2 = k2;
        } else { // the same bits whatever else is asked for
            if (mask & 1) CHECK(i2 == idx);
            if (mask & 2) CHECK(k2 == ksd2);
        }
    }
    // replay the picks through the definition in long double
    const long double al = a;
    const bool imq = kernel == SVGD_KERNEL_IMQ;
    std::vector<long double> diag((size_t)n), acc((size_t)n, 0.0L), aabs((size_t)n, 0.0L);
    for (int64_t j = 0; j < n; ++j) {
        long double ss = 0.0L;
        for (int c = 0; c < d; ++c) ss += (long double)G[(size_t)j * d + c] * G[(size_t)j * d + c];
        diag[(size_t)j] = ss + (imq ? al * d : 2.0L * al * d);
    }
    long double S = 0.0L, Sabs = 0.0L;
    for (int64_t t = 1; t <= m; ++t) {
        const int64_t pi = idx[(size_t)t - 1];
        CHECK(pi >= 0 && pi < n);
        if (pi < 0 || pi >= n) return;
        long double omin = INFINITY, omax = 0.0L;
        for (int64_t j = 0; j < n; ++j) {
            omin = std::fmin(omin, diag[(size_t)j] / 2 + acc[(size_t)j]);
            omax = std::fmax(omax, diag[(size_t)j] / 2 + aabs[(size_t)j]);
        }
        CHECK(diag[(size_t)pi] / 2 + acc[(size_t)pi] <= omin + 1e-12L * std::fmax(1.0L, omax));
        S += 2 * acc[(size_t)pi] + diag[(size_t)pi];
        Sabs += 2 * aabs[(size_t)pi] + diag[(size_t)pi];
        const long double tt = (long double)t * (long double)t;
        CHECK(std::fabs((long double)ksd2[(size_t)t - 1] - S / tt) <= 1e-12L * std::fmax(1.0L, Sabs / tt));
        for (int64_t j = 0; j < n; ++j) {
            long double u = diag[(size_t)j];
            if (j != pi) {
                long double r2 = 0.0L, ss = 0.0L, dsr = 0.0L;
                for (int c = 0; c < d; ++c) {
                    const long double r = (long double)X[(size_t)pi * d + c] - (long double)X[(size_t)j * d + c];
                    const long double si = G[(size_t)pi * d + c], sj = G[(size_t)j * d + c];
                    r2 += r * r;
                    ss += si * sj;
                    dsr += (si - sj) * r;
                }
                if (imq) {
                    const long double k = 1.0L / std::sqrt(1.0L + al * r2), k3 = k * k * k;
                    u = k * ss + al * k3 * dsr + al * d * k3 - 3.0L * al * al * k3 * k * k * r2;
                } else {
                    u = std::exp(-al * r2) * (ss + 2.0L * al * dsr + 2.0L * al * d - 4.0L * al * al * r2);
                }
            }
            acc[(size_t)j] += u;
            aabs[(size_t)j] += std::fabs(u);
        }
    }
}

int main()
{
    const int dims[] = {1, 3, 8, 17, 64};
    const int64_t ns[] = {1, 2, 15, 129};
    for (int kernel : {SVGD_KERNEL_RBF, SVGD_KERNEL_IMQ})
        for (int d : dims)
            for (int64_t n : ns) one_case(kernel, d, n, 0.37 / d, n < 15 ? 5 : 20);
    for (int kernel : {SVGD_KERNEL_RBF, SVGD_KERNEL_IMQ}) {
        one_case(kernel, 3, 2500, 0.1, 6); // three blocks of candidates, the last one short
        one_case(kernel, 5, 40, 1e6, 50);
        one_case(kernel, 5, 40, 1e-8, 50);
    }
    // refusals: nothing is read or written
    double x[6] = {0, 1, 2, 3, 4, 5}, g[6] = {1, 1, 1, 1, 1, 1}, k2[2] = {-7.0, -7.0};
    int64_t ix[2] = {-7, -7};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int kernel : {SVGD_KERNEL_RBF, SVGD_KERNEL_IMQ}) {
        CHECK(svgd_stein_thin_host(kernel, 0, 2, x, g, 1.0, 2, ix, k2) == SVGD_ERR_DIM);
        CHECK(svgd_stein_thin_host(kernel, 3, 0, x, g, 1.0, 2, ix, k2) == SVGD_ERR_DIM);
        CHECK(svgd_stein_thin_host(kernel, 3, 2, x, g, 0.0, 2, ix, k2) == SVGD_ERR_ARG);
        CHECK(svgd_stein_thin_host(kernel, 3, 2, x, g, -1.0, 2, ix, k2) == SVGD_ERR_ARG);
        CHECK(svgd_stein_thin_host(kernel, 3, 2, x, g, nan, 2, ix, k2) == SVGD_ERR_ARG);
        CHECK(svgd_stein_thin_host(kernel, 3, 2, x, g, inf, 2, ix, k2) == SVGD_ERR_ARG);
        CHECK(svgd_stein_thin_host(kernel, 3, 2, x, g, 1.0, 0, ix, k2) == SVGD_ERR_ARG);
        CHECK(svgd_stein_thin_host(kernel, 3, 2, x, g, 1.0, -1, ix, k2) == SVGD_ERR_ARG);
        CHECK(svgd_stein_thin_host(kernel, 3, 2, nullptr, g, 1.0, 2, ix, k2) == SVGD_ERR_ARG);
        CHECK(svgd_stein_thin_host(kernel, 3, 2, x, nullptr, 1.0, 2, ix, k2) == SVGD_ERR_ARG);
    }
    CHECK(svgd_stein_thin_host(2, 3, 2, x, g, 1.0, 2, ix, k2) == SVGD_ERR_ARG);
    CHECK(svgd_stein_thin_host(-1, 3, 2, x, g, 1.0, 2, ix, k2) == SVGD_ERR_ARG);
    CHECK(ix[0] == -7 && ix[1] == -7 && k2[0] == -7.0 && k2[1] == -7.0);
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
