// Self-checking driver of the host MMD (svgd_mmd_host of
// svgdcpp_amd/csrc/host_mmd.cpp) for the ASan + UBSan build
// (`make sanitize_mmd`): both kernels, sizes that reach the edges -- one
// point on either side, d = 64, N != M either way -- from exactly sized heap
// buffers, every combination of NULL outputs, every refusal, each result
// against the definition evaluated here in long double (1e-12 absolute), and
// a guard slot behind each output.
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

static long double kern(bool imq, long double a, int d, const double *x, const double *y)
{
    long double t = 0.0L;
    for (int c = 0; c < d; ++c) {
        const long double r = (long double)x[c] - (long double)y[c];
        t += r * r;
    }
    return imq ? 1.0L / std::sqrt(1.0L + a * t) : std::exp(-a * t);
}

static void one_case(int kernel, int d, int64_t n, int64_t m, double a)
{
    uint64_t seed = 1000 * (uint64_t)d + 31 * (uint64_t)n + (uint64_t)m;
    std::vector<double> X((size_t)n * d), Y((size_t)m * d);
    for (double &v : X) v = 2.0 * uniform(seed);
    for (double &v : Y) v = 0.5 + 1.5 * uniform(seed);
    double v0 = 0, u0 = 0;
    std::vector<double> m0, w0;
    for (int mask : {15, 0, 1, 2, 4, 8, 5, 10}) { // which outputs are asked for; all first
        double v = -7.0, u = -7.0;
        std::vector<double> m3(4, -7.0), wit((size_t)n + 1, -7.0);
        CHECK(svgd_mmd_host(kernel, d, n, X.data(), m, Y.data(), a, mask & 1 ? &v : nullptr, mask & 2 ? &u : nullptr,
                            mask & 4 ? m3.data() : nullptr, mask & 8 ? wit.data() : nullptr) == SVGD_OK);
        CHECK(m3[3] == -7.0 && wit[(size_t)n] == -7.0); // nothing past the slots
        if (!(mask & 1)) CHECK(v == -7.0);
        if (!(mask & 2)) CHECK(u == -7.0);
        if (!(mask & 4)) CHECK(m3[0] == -7.0);
        if (!(mask & 8)) CHECK(wit[0] == -7.0);
        if (mask == 15) {
            v0 = v, u0 = u, m0 = m3, w0 = wit;
        } else { // the same bits whatever else is asked for
            if (mask & 1) CHECK(v == v0);
            if (mask & 2) CHECK(u == u0 || (std::isnan(u) && std::isnan(u0)));
            if (mask & 4) CHECK(m3 == m0);
            if (mask & 8) CHECK(wit == w0);
        }
    }
    // the definition in long double
    const bool imq = kernel == SVGD_KERNEL_IMQ;
    const long double al = a, N = n, M = m;
    long double sxx = 0.0L, sxy = 0.0L, syy = 0.0L;
    for (int64_t i = 0; i < n; ++i) {
        long double rx = 0.0L, ry = 0.0L;
        for (int64_t j = 0; j < n; ++j) rx += kern(imq, al, d, &X[(size_t)i * d], &X[(size_t)j * d]);
        for (int64_t j = 0; j < m; ++j) ry += kern(imq, al, d, &X[(size_t)i * d], &Y[(size_t)j * d]);
        sxx += rx;
        sxy += ry;
        CHECK(std::fabs((long double)w0[(size_t)i] - (rx / N - ry / M)) <= 1e-12L);
    }
    for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j < m; ++j) syy += kern(imq, al, d, &Y[(size_t)i * d], &Y[(size_t)j * d]);
    const long double mxx = sxx / (N * N), myy = syy / (M * M), mxy = sxy / (N * M);
    CHECK(std::fabs((long double)m0[0] - mxx) <= 1e-12L);
    CHECK(std::fabs((long double)m0[1] - myy) <= 1e-12L);
    CHECK(std::fabs((long double)m0[2] - mxy) <= 1e-12L);
    CHECK(std::fabs((long double)v0 - (mxx + myy - 2 * mxy)) <= 1e-12L);
    if (n < 2 || m < 2)
        CHECK(std::isnan(u0));
    else
        CHECK(std::fabs((long double)u0 - ((sxx - N) / (N * (N - 1)) + (syy - M) / (M * (M - 1)) - 2 * mxy)) <= 1e-12L);
}

int main()
{
    const int dims[] = {1, 3, 8, 17, 64};
    const int64_t ns[][2] = {{1, 1}, {2, 1}, {1, 2}, {15, 129}, {129, 15}};
    for (int kernel : {SVGD_KERNEL_RBF, SVGD_KERNEL_IMQ})
        for (int d : dims)
            for (const auto &nm : ns) one_case(kernel, d, nm[0], nm[1], 0.37 / d);
    for (int kernel : {SVGD_KERNEL_RBF, SVGD_KERNEL_IMQ}) {
        one_case(kernel, 5, 40, 33, 1e6);
        one_case(kernel, 5, 40, 33, 1e-8);
    }
    // refusals: nothing is written
    double x[6] = {0, 1, 2, 3, 4, 5}, y[6] = {1, 1, 1, 2, 2, 2}, out[5] = {-7.0, -7.0, -7.0, -7.0, -7.0};
    double w[2] = {-7.0, -7.0};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double ybad[6] = {1, 1, 1, 2, nan, 2}, yinf[6] = {1, 1, 1, 2, 2, -inf};
    for (int kernel : {SVGD_KERNEL_RBF, SVGD_KERNEL_IMQ}) {
        CHECK(svgd_mmd_host(kernel, 0, 2, x, 2, y, 1.0, out, out + 1, out + 2, w) == SVGD_ERR_DIM);
        CHECK(svgd_mmd_host(kernel, 3, 0, x, 2, y, 1.0, out, out + 1, out + 2, w) == SVGD_ERR_DIM);
        CHECK(svgd_mmd_host(kernel, 3, 2, x, 0, y, 1.0, out, out + 1, out + 2, w) == SVGD_ERR_DIM);
        CHECK(svgd_mmd_host(kernel, 3, 2, x, -1, y, 1.0, out, out + 1, out + 2, w) == SVGD_ERR_DIM);
        for (double a : {0.0, -1.0, nan, inf})
            CHECK(svgd_mmd_host(kernel, 3, 2, x, 2, y, a, out, out + 1, out + 2, w) == SVGD_ERR_ARG);
        CHECK(svgd_mmd_host(kernel, 3, 2, nullptr, 2, y, 1.0, out, out + 1, out + 2, w) == SVGD_ERR_ARG);
        CHECK(svgd_mmd_host(kernel, 3, 2, x, 2, nullptr, 1.0, out, out + 1, out + 2, w) == SVGD_ERR_ARG);
        CHECK(svgd_mmd_host(kernel, 3, 2, x, 2, ybad, 1.0, out, out + 1, out + 2, w) == SVGD_ERR_ARG);
        CHECK(svgd_mmd_host(kernel, 3, 2, x, 2, yinf, 1.0, out, out + 1, out + 2, w) == SVGD_ERR_ARG);
    }
    CHECK(svgd_mmd_host(2, 3, 2, x, 2, y, 1.0, out, out + 1, out + 2, w) == SVGD_ERR_ARG);
    CHECK(svgd_mmd_host(-1, 3, 2, x, 2, y, 1.0, out, out + 1, out + 2, w) == SVGD_ERR_ARG);
    for (double v : out) CHECK(v == -7.0);
    CHECK(w[0] == -7.0 && w[1] == -7.0);
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
