// SVGD::ComputeKSD(unbiased, SVGD_KERNEL_IMQ) (svgd_ksd_kernel on the device)
// against the direct double-loop formula on the host: N = 300 particles,
// d = 2, the mvn_example target.
//
//   k = (1 + a |r|^2)^(-1/2),  r = x_i - x_j
//   u_ij = k s_i.s_j + a k^3 (s_i - s_j).r + a d k^3 - 3 a^2 k^5 |r|^2
//   KSD2_V = (1/N^2) sum_ij u_ij,   KSD2_U = (1/(N(N-1))) sum_{i != j} u_ij
// with s = grad log p = -Sigma^-1 (x - mu), evaluated here in long double.
// Bound: 1e-12 max(1, mean |u_ij|), the bar of the device statistic.
//
//   ./test_ksd_imq       (needs a GPU)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "Core"
#include "Kernel"
#include "Model"
#include "Optimizer"

static int g_fail = 0, g_pass = 0;
#define CHECK(cond)                                                              \
    do                                                                           \
    {                                                                            \
        if (cond)                                                                \
            ++g_pass;                                                            \
        else                                                                     \
        {                                                                        \
            ++g_fail;                                                            \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                        \
    } while (0)

struct HostKsd
{
    double v, u, mean_abs;
};

// X: d x n column-major (particle j at X[j d ..]); s = -P (x - mu), P = Sigma^-1
static HostKsd DirectKsd(const Eigen::MatrixXd &X, const double mu[2], const double P[2][2], double a, bool imq)
{
    const long n = X.cols(), d = 2;
    std::vector<long double> s((size_t)n * d);
    for (long i = 0; i < n; ++i)
        for (long r = 0; r < d; ++r)
        {
            long double t = 0.0L;
            for (long c = 0; c < d; ++c)
                t -= (long double)P[r][c] * ((long double)X(c, i) - (long double)mu[c]);
            s[(size_t)(i * d + r)] = t;
        }
    const long double al = a;
    long double all = 0.0L, off = 0.0L, absum = 0.0L;
    for (long i = 0; i < n; ++i)
        for (long j = 0; j < n; ++j)
        {
            long double r2 = 0.0L, ss = 0.0L, dsr = 0.0L;
            for (long k = 0; k < d; ++k)
            {
                const long double r = (long double)X(k, i) - (long double)X(k, j);
                const long double si = s[(size_t)(i * d + k)], sj = s[(size_t)(j * d + k)];
                r2 += r * r;
                ss += si * sj;
                dsr += (si - sj) * r;
            }
            long double u;
            if (imq)
            {
                const long double k = 1.0L / std::sqrt(1.0L + al * r2), k3 = k * k * k;
                u = k * ss + al * k3 * dsr + al * d * k3 - 3.0L * al * al * k3 * k * k * r2;
            }
            else
                u = std::exp(-al * r2) * (ss + 2.0L * al * dsr + 2.0L * al * d - 4.0L * al * al * r2);
            all += u;
            absum += std::fabs(u);
            if (i != j)
                off += u;
        }
    const long double N = (long double)n;
    return {(double)(all / (N * N)), (double)(off / (N * (N - 1.0L))), (double)(absum / (N * N))};
}

int main()
{
    const size_t dim = 2, n = 300;
    const double mu_v[2] = {-0.6871, 0.8010};
    const double S[2][2] = {{5 * 0.2260, 5 * 0.1652}, {5 * 0.1652, 5 * 0.6779}};
    const double det = S[0][0] * S[1][1] - S[0][1] * S[1][0];
    const double P[2][2] = {{S[1][1] / det, -S[0][1] / det}, {-S[1][0] / det, S[0][0] / det}};

    Eigen::Vector2d mu(mu_v[0], mu_v[1]);
    Eigen::Matrix2d sigma;
    sigma << S[0][0], S[0][1], S[1][0], S[1][1];
    std::shared_ptr<Model> target = std::make_shared<MultivariateNormal>(mu, sigma);

    // an RBF SVGD, median scale: a = ln N / med^2 of the particles for both statistics
    {
        auto particles = std::make_shared<Eigen::MatrixXd>(3 * Eigen::MatrixXd::Random(dim, n));
        auto kernel = std::make_shared<GaussianRBFKernel>(particles, GaussianRBFKernel::ScaleMethod::Median, target);
        auto optimizer = std::make_shared<AdaGrad>(dim, n, 1.0e-1);
        SVGD svgd(dim, 20, particles, kernel, target, optimizer);
        svgd.Initialize();
        const double v = svgd.ComputeKSD(false, SVGD_KERNEL_IMQ), u = svgd.ComputeKSD(true, SVGD_KERNEL_IMQ);
        double a = 0.0;
        CHECK(svgd_median_scale(svgd.Context(), &a, nullptr) == SVGD_OK);
        const HostKsd h = DirectKsd(*particles, mu_v, P, a, true);
        const double bar = 1e-12 * std::max(1.0, h.mean_abs);
        std::printf("median a=%.6g  V=%.15g (host %.15g, err %.3g)  U=%.15g (host %.15g, err %.3g)  bar %.3g\n", a,
                    v, h.v, std::fabs(v - h.v), u, h.u, std::fabs(u - h.u), bar);
        CHECK(std::fabs(v - h.v) <= bar);
        CHECK(std::fabs(u - h.u) <= bar);
        CHECK(v >= 0.0);
        // the RBF statistic through the overload is ComputeKSD(bool)
        CHECK(svgd.ComputeKSD(false, SVGD_KERNEL_RBF) == svgd.ComputeKSD());
        CHECK(svgd.ComputeKSD(true, SVGD_KERNEL_RBF) == svgd.ComputeKSD(true));
        const HostKsd hr = DirectKsd(*particles, mu_v, P, a, false);
        CHECK(std::fabs(svgd.ComputeKSD() - hr.v) <= 1e-10 * std::max(1.0, hr.mean_abs));
        bool threw = false;
        try
        {
            svgd.ComputeKSD(false, 7);
        }
        catch (const std::invalid_argument &)
        {
            threw = true;
        }
        CHECK(threw);
        // 20 AdaGrad steps towards the target lower it
        svgd.Run();
        const double v1 = svgd.ComputeKSD(false, SVGD_KERNEL_IMQ);
        std::printf("after 20 steps V=%.6g (from %.6g)\n", v1, v);
        CHECK(v1 < v);
    }
    // an IMQ SVGD with a constant scale: the kernel's own a
    {
        auto pts = std::make_shared<Eigen::MatrixXd>(3 * Eigen::MatrixXd::Random(dim, n));
        auto kernel =
            std::make_shared<InverseMultiquadricKernel>(pts, InverseMultiquadricKernel::ScaleMethod::Constant, 0.37);
        auto optimizer = std::make_shared<AdaGrad>(dim, n, 1.0e-1);
        SVGD svgd(dim, 1, pts, kernel, target, optimizer);
        svgd.Initialize();
        const double v = svgd.ComputeKSD(false, SVGD_KERNEL_IMQ), u = svgd.ComputeKSD(true, SVGD_KERNEL_IMQ);
        const HostKsd h = DirectKsd(*pts, mu_v, P, 0.37, true);
        const double bar = 1e-12 * std::max(1.0, h.mean_abs);
        std::printf("constant a=0.37  V err %.3g  U err %.3g  bar %.3g\n", std::fabs(v - h.v), std::fabs(u - h.u),
                    bar);
        CHECK(std::fabs(v - h.v) <= bar);
        CHECK(std::fabs(u - h.u) <= bar);
    }
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
