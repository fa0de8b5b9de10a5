// SVGD::Thin (svgd_stein_thin on the device) against the definition evaluated
// here in long double: N = 300 particles, d = 2, the mvn_example target.
//
//   acc_0[j] = 0;  for t = 1..m:
//     obj_t[j] = u_jj / 2 + acc_{t-1}[j],   pi_t = the smallest argmin,
//     S_t = S_{t-1} + 2 acc_{t-1}[pi_t] + u_{pi_t pi_t},   ksd2_t = S_t / t^2,
//     acc_t[j] = acc_{t-1}[j] + u(pi_t, j)
// with u_ij of tests/cpp/test_ksd_imq.cpp and s = -Sigma^-1 (x - mu).  Along
// the device's own picks: obj_t[pi_t] <= min_j obj_t[j] + bar_t with
// bar_t = 1e-12 max(1, max_j (u_jj / 2 + sum_{s<t} |u(pi_s, j)|)), and
// |ksd2_t - ref| <= 1e-12 max(1, mean |u| over the picked t x t block).
//
//   ./test_thin       (needs a GPU)
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

// Replays `picks` through the definition; returns the worst
// (obj_t[pi_t] - min) / bar_t and the worst ksd2 error over its bar.
static void Replay(const Eigen::MatrixXd &X, const double mu[2], const double P[2][2], double a, bool imq,
                   const std::vector<int64_t> &picks, const Eigen::VectorXd &ksd2, double *worst_obj,
                   double *worst_ksd)
{
    const long n = X.cols(), d = 2;
    std::vector<long double> s((size_t)n * d), diag((size_t)n), acc((size_t)n, 0.0L), aabs((size_t)n, 0.0L);
    const long double al = a;
    for (long i = 0; i < n; ++i)
    {
        long double ss = 0.0L;
        for (long r = 0; r < d; ++r)
        {
            long double t = 0.0L;
            for (long c = 0; c < d; ++c)
                t -= (long double)P[r][c] * ((long double)X(c, i) - (long double)mu[c]);
            s[(size_t)(i * d + r)] = t;
            ss += t * t;
        }
        diag[(size_t)i] = ss + (imq ? al * d : 2.0L * al * d);
    }
    long double S = 0.0L, Sabs = 0.0L;
    *worst_obj = *worst_ksd = 0.0;
    for (size_t t = 1; t <= picks.size(); ++t)
    {
        const long pi = (long)picks[t - 1];
        long double omin = INFINITY, omax = 0.0L;
        for (long j = 0; j < n; ++j)
        {
            omin = std::min(omin, diag[(size_t)j] / 2 + acc[(size_t)j]);
            omax = std::max(omax, diag[(size_t)j] / 2 + aabs[(size_t)j]);
        }
        const long double bar = 1e-12L * std::max(1.0L, omax);
        *worst_obj = std::max(*worst_obj, (double)((diag[(size_t)pi] / 2 + acc[(size_t)pi] - omin) / bar));
        S += 2 * acc[(size_t)pi] + diag[(size_t)pi];
        Sabs += 2 * aabs[(size_t)pi] + diag[(size_t)pi];
        const long double tt = (long double)t * (long double)t;
        const long double kbar = 1e-12L * std::max(1.0L, Sabs / tt);
        *worst_ksd = std::max(*worst_ksd, (double)(std::fabs((long double)ksd2[(long)t - 1] - S / tt) / kbar));
        for (long j = 0; j < n; ++j)
        {
            long double u = diag[(size_t)j];
            if (j != pi)
            {
                long double r2 = 0.0L, ss = 0.0L, dsr = 0.0L;
                for (long k = 0; k < d; ++k)
                {
                    const long double r = (long double)X(k, pi) - (long double)X(k, j);
                    const long double si = s[(size_t)(pi * d + k)], sj = s[(size_t)(j * d + k)];
                    r2 += r * r;
                    ss += si * sj;
                    dsr += (si - sj) * r;
                }
                if (imq)
                {
                    const long double k = 1.0L / std::sqrt(1.0L + al * r2), k3 = k * k * k;
                    u = k * ss + al * k3 * dsr + al * d * k3 - 3.0L * al * al * k3 * k * k * r2;
                }
                else
                    u = std::exp(-al * r2) * (ss + 2.0L * al * dsr + 2.0L * al * d - 4.0L * al * al * r2);
            }
            acc[(size_t)j] += u;
            aabs[(size_t)j] += std::fabs(u);
        }
    }
}

int main()
{
    const size_t dim = 2, n = 300;
    const int64_t m = 12;
    const double mu_v[2] = {-0.6871, 0.8010};
    const double S[2][2] = {{5 * 0.2260, 5 * 0.1652}, {5 * 0.1652, 5 * 0.6779}};
    const double det = S[0][0] * S[1][1] - S[0][1] * S[1][0];
    const double P[2][2] = {{S[1][1] / det, -S[0][1] / det}, {-S[1][0] / det, S[0][0] / det}};

    Eigen::Vector2d mu(mu_v[0], mu_v[1]);
    Eigen::Matrix2d sigma;
    sigma << S[0][0], S[0][1], S[1][0], S[1][1];
    std::shared_ptr<Model> target = std::make_shared<MultivariateNormal>(mu, sigma);

    // an RBF SVGD, median scale: a = ln N / med^2 of the particles for both kernels
    {
        auto particles = std::make_shared<Eigen::MatrixXd>(3 * Eigen::MatrixXd::Random(dim, n));
        auto kernel = std::make_shared<GaussianRBFKernel>(particles, GaussianRBFKernel::ScaleMethod::Median, target);
        auto optimizer = std::make_shared<AdaGrad>(dim, n, 1.0e-1);
        SVGD svgd(dim, 20, particles, kernel, target, optimizer);
        svgd.Initialize();
        double a = 0.0;
        for (int kind : {SVGD_KERNEL_IMQ, SVGD_KERNEL_RBF})
        {
            const SVGD::Thinned th = svgd.Thin(m, kind);
            CHECK(svgd_median_scale(svgd.Context(), &a, nullptr) == SVGD_OK);
            CHECK((int64_t)th.index.size() == m && th.ksd2.size() == m && th.points.rows() == (long)dim &&
                  th.points.cols() == m);
            bool in_range = true, cols = true;
            for (int64_t t = 0; t < m; ++t)
            {
                in_range = in_range && th.index[(size_t)t] >= 0 && th.index[(size_t)t] < (int64_t)n;
                if (in_range)
                    cols = cols && th.points.col(t) == particles->col(th.index[(size_t)t]);
            }
            CHECK(in_range);
            CHECK(cols);
            if (!in_range)
                continue;
            double wo = 0.0, wk = 0.0;
            Replay(*particles, mu_v, P, a, kind == SVGD_KERNEL_IMQ, th.index, th.ksd2, &wo, &wk);
            std::printf("%s median a=%.6g  ksd2 %.6g -> %.6g  obj excess/bar %.3g  ksd2 err/bar %.3g\n",
                        kind == SVGD_KERNEL_IMQ ? "imq" : "rbf", a, th.ksd2[0], th.ksd2[m - 1], wo, wk);
            CHECK(wo <= 1.0);
            CHECK(wk <= 1.0);
        }
        // the default kernel is the IMQ one; two calls give the same bits
        const SVGD::Thinned t0 = svgd.Thin(m), t1 = svgd.Thin(m, SVGD_KERNEL_IMQ);
        CHECK(t0.index == t1.index && t0.ksd2 == t1.ksd2);
        for (int64_t bad_m : {(int64_t)0, (int64_t)-1})
        {
            bool threw = false;
            try
            {
                svgd.Thin(bad_m);
            }
            catch (const std::invalid_argument &)
            {
                threw = true;
            }
            CHECK(threw);
        }
        bool threw = false;
        try
        {
            svgd.Thin(m, 7);
        }
        catch (const std::invalid_argument &)
        {
            threw = true;
        }
        CHECK(threw);
    }
    // an IMQ SVGD with a constant scale: the kernel's own a
    {
        auto pts = std::make_shared<Eigen::MatrixXd>(3 * Eigen::MatrixXd::Random(dim, n));
        auto kernel =
            std::make_shared<InverseMultiquadricKernel>(pts, InverseMultiquadricKernel::ScaleMethod::Constant, 0.37);
        auto optimizer = std::make_shared<AdaGrad>(dim, n, 1.0e-1);
        SVGD svgd(dim, 1, pts, kernel, target, optimizer);
        svgd.Initialize();
        const SVGD::Thinned th = svgd.Thin(m);
        double wo = 0.0, wk = 0.0;
        Replay(*pts, mu_v, P, 0.37, true, th.index, th.ksd2, &wo, &wk);
        std::printf("imq constant a=0.37  obj excess/bar %.3g  ksd2 err/bar %.3g\n", wo, wk);
        CHECK(wo <= 1.0);
        CHECK(wk <= 1.0);
    }
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
