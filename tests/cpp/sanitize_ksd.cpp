// Self-checking driver of the host KSD (svgd_ksd_host of
// svgdcpp_amd/csrc/host_ksd.cpp) for the ASan + UBSan build
// (`make sanitize_ksd`): both kernels, sizes that reach the edges -- one
// particle, one column, d = 64 -- into exactly sized heap buffers, every
// combination of NULL outputs, every refusal, each result checked against
// the definition evaluated here in long double, and a guard slot behind the
// rows.
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

static void one_case(int kernel, int d, int64_t n, double a)
{
    uint64_t seed = 1000 * (uint64_t)d + (uint64_t)n;
    std::vector<double> X((size_t)n * d), G((size_t)n * d);
    for (double &v : X) v = 2.0 * uniform(seed);
    for (double &v : G) v = 8.0 * uniform(seed);
    // the definition in long double
    const long double al = a;
    std::vector<long double> rows((size_t)n, 0.0L), rowabs((size_t)n, 0.0L);
    long double all = 0.0L, off = 0.0L, absum = 0.0L;
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t j = 0; j < n; ++j) {
            long double r2 = 0.0L, ss = 0.0L, dsr = 0.0L;
            for (int c = 0; c < d; ++c) {
                const long double r = (long double)X[(size_t)i * d + c] - (long double)X[(size_t)j * d + c];
                const long double si = G[(size_t)i * d + c], sj = G[(size_t)j * d + c];
                r2 += r * r;
                ss += si * sj;
                dsr += (si - sj) * r;
            }
            long double u;
            if (kernel == SVGD_KERNEL_IMQ) {
                const long double k = 1.0L / std::sqrt(1.0L + al * r2), k3 = k * k * k;
                u = k * ss + al * k3 * dsr + al * d * k3 - 3.0L * al * al * k3 * k * k * r2;
            } else {
                u = std::exp(-al * r2) * (ss + 2.0L * al * dsr + 2.0L * al * d - 4.0L * al * al * r2);
            }
            rows[(size_t)i] += u;
            rowabs[(size_t)i] += std::fabs(u);
            all += u;
            absum += std::fabs(u);
            if (i != j) off += u;
        }
        rows[(size_t)i] /= (long double)n;
    }
    const long double N = (long double)n;
    const long double bar = 1e-12L * std::fmax(1.0L, absum / (N * N));
    const long double v_ref = all / (N * N), u_ref = n < 2 ? 0.0L : off / (N * (N - 1.0L));
    for (int mask = 0; mask < 8; ++mask) { // which outputs are asked for
        double v = -7.0, u = -7.0;
        std::vector<double> out((size_t)n + 1, -7.0);
        CHECK(svgd_ksd_host(kernel, d, n, X.data(), G.data(), a, mask & 1 ? &v : nullptr, mask & 2 ? &u : nullptr,
                            mask & 4 ? out.data() : nullptr) == SVGD_OK);
        CHECK(out[(size_t)n] == -7.0); // nothing past the rows
        if (mask & 1) CHECK(std::fabs((long double)v - v_ref) <= bar);
        if (mask & 2) CHECK(n < 2 ? std::isnan(u) : std::fabs((long double)u - u_ref) <= bar);
        if (mask & 4)
            for (int64_t i = 0; i < n; ++i) // (a row's bar takes that row's mean |u|)
                CHECK(std::fabs((long double)out[(size_t)i] - rows[(size_t)i]) <=
                      1e-12L * std::fmax(1.0L, rowabs[(size_t)i] / N));
        if (!(mask & 4)) CHECK(out[0] == -7.0);
    }
}

int main()
{
    const int dims[] = {1, 3, 8, 17, 64};
    const int64_t ns[] = {1, 2, 15, 129};
    for (int kernel : {SVGD_KERNEL_RBF, SVGD_KERNEL_IMQ})
        for (int d : dims)
            for (int64_t n : ns) one_case(kernel, d, n, 0.37 / d);
    one_case(SVGD_KERNEL_IMQ, 5, 40, 1e6);
    one_case(SVGD_KERNEL_IMQ, 5, 40, 1e-8);
    one_case(SVGD_KERNEL_RBF, 5, 40, 1e6);
    // refusals: nothing is read or written
    double x[6] = {0, 1, 2, 3, 4, 5}, g[6] = {1, 1, 1, 1, 1, 1}, v = -7.0, u = -7.0, o[2] = {-7.0, -7.0};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int kernel : {SVGD_KERNEL_RBF, SVGD_KERNEL_IMQ}) {
        CHECK(svgd_ksd_host(kernel, 0, 2, x, g, 1.0, &v, &u, o) == SVGD_ERR_DIM);
        CHECK(svgd_ksd_host(kernel, 3, 0, x, g, 1.0, &v, &u, o) == SVGD_ERR_DIM);
        CHECK(svgd_ksd_host(kernel, 3, 2, x, g, 0.0, &v, &u, o) == SVGD_ERR_ARG);
        CHECK(svgd_ksd_host(kernel, 3, 2, x, g, -1.0, &v, &u, o) == SVGD_ERR_ARG);
        CHECK(svgd_ksd_host(kernel, 3, 2, x, g, nan, &v, &u, o) == SVGD_ERR_ARG);
        CHECK(svgd_ksd_host(kernel, 3, 2, x, g, inf, &v, &u, o) == SVGD_ERR_ARG);
        CHECK(svgd_ksd_host(kernel, 3, 2, nullptr, g, 1.0, &v, &u, o) == SVGD_ERR_ARG);
        CHECK(svgd_ksd_host(kernel, 3, 2, x, nullptr, 1.0, &v, &u, o) == SVGD_ERR_ARG);
    }
    CHECK(svgd_ksd_host(2, 3, 2, x, g, 1.0, &v, &u, o) == SVGD_ERR_ARG);
    CHECK(svgd_ksd_host(-1, 3, 2, x, g, 1.0, &v, &u, o) == SVGD_ERR_ARG);
    CHECK(v == -7.0 && u == -7.0 && o[0] == -7.0 && o[1] == -7.0);
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
