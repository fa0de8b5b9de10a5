// SVGD::ComputeMMD (svgd_mmd on the device) against svgd_mmd_host (direct
// differences on the host): N = 300 particles, d = 2, a sample of M = 177
// points, both kernels, V and U within 1e-12 absolute (|k| <= 1).
//
//   ./test_mmd        (needs a GPU)
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

// V and U of the host form on the d x N / d x M matrices (columns are points:
// the column-major storage is the row-major N x d the C ABI takes)
static void Host(int kind, const Eigen::MatrixXd &X, const Eigen::MatrixXd &Y, double a, double *v, double *u)
{
    CHECK(svgd_mmd_host(kind, (int)X.rows(), (int64_t)X.cols(), X.data(), (int64_t)Y.cols(), Y.data(), a, v, u,
                        nullptr, nullptr) == SVGD_OK);
}

int main()
{
    const size_t dim = 2, n = 300;
    const long m = 177;
    Eigen::Vector2d mu(-0.6871, 0.8010);
    Eigen::Matrix2d sigma;
    sigma << 5 * 0.2260, 5 * 0.1652, 5 * 0.1652, 5 * 0.6779;
    std::shared_ptr<Model> target = std::make_shared<MultivariateNormal>(mu, sigma);
    const Eigen::MatrixXd Y = 2 * Eigen::MatrixXd::Random(dim, m) + Eigen::MatrixXd::Constant(dim, m, 0.5);

    // an RBF SVGD, median scale: a = ln N / med^2 of the particles for both kernels
    {
        auto particles = std::make_shared<Eigen::MatrixXd>(3 * Eigen::MatrixXd::Random(dim, n));
        auto kernel = std::make_shared<GaussianRBFKernel>(particles, GaussianRBFKernel::ScaleMethod::Median, target);
        auto optimizer = std::make_shared<AdaGrad>(dim, n, 1.0e-1);
        SVGD svgd(dim, 20, particles, kernel, target, optimizer);
        svgd.Initialize();
        for (int kind : {SVGD_KERNEL_RBF, SVGD_KERNEL_IMQ})
        {
            const double v = svgd.ComputeMMD(Y, false, kind), u = svgd.ComputeMMD(Y, true, kind);
            double a = 0.0, hv = 0.0, hu = 0.0;
            CHECK(svgd_median_scale(svgd.Context(), &a, nullptr) == SVGD_OK);
            Host(kind, *particles, Y, a, &hv, &hu);
            std::printf("%s median a=%.6g  V=%.12g U=%.12g  err V %.3g  err U %.3g (bar 1e-12)\n",
                        kind == SVGD_KERNEL_IMQ ? "imq" : "rbf", a, v, u, std::fabs(v - hv), std::fabs(u - hu));
            CHECK(std::fabs(v - hv) <= 1e-12);
            CHECK(std::fabs(u - hu) <= 1e-12);
            CHECK(v > 0.0);
            // two calls give the same bits
            CHECK(svgd.ComputeMMD(Y, false, kind) == v);
        }
        // the defaults: the biased RBF statistic
        CHECK(svgd.ComputeMMD(Y) == svgd.ComputeMMD(Y, false, SVGD_KERNEL_RBF));
        // the particles against themselves
        CHECK(std::fabs(svgd.ComputeMMD(*particles)) <= 1e-12);
        bool threw = false;
        try
        {
            svgd.ComputeMMD(Eigen::MatrixXd::Zero(dim + 1, m));
        }
        catch (const DimensionMismatchException &)
        {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try
        {
            svgd.ComputeMMD(Y, false, 7);
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
        double hv = 0.0, hu = 0.0;
        Host(SVGD_KERNEL_IMQ, *pts, Y, 0.37, &hv, &hu);
        const double v = svgd.ComputeMMD(Y, false, SVGD_KERNEL_IMQ), u = svgd.ComputeMMD(Y, true, SVGD_KERNEL_IMQ);
        std::printf("imq constant a=0.37  err V %.3g  err U %.3g (bar 1e-12)\n", std::fabs(v - hv), std::fabs(u - hu));
        CHECK(std::fabs(v - hv) <= 1e-12);
        CHECK(std::fabs(u - hu) <= 1e-12);
    }
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
