// SVGD::Predict (C++ API): the device posterior predictive of a
// GeneralizedLinearModel against GeneralizedLinearModel::Predict on the host,
// at the coordinates Run() returned -- M = 200 rows, d = 5, N = 300 particles,
// 129 held-out rows, both links, within the bars of tests/_glm_predict.py:
//   T_im = |a_m| . |theta_i|,  Tbar_m = |a_m| . |theta_bar|
//   mean  1e-13 (1 + mean_i T)            | 1e-13 (mean_i T + Tbar)
//   var   1e-13 (1 + mean_i T)            | 1e-13 mean_i (T + Tbar)^2
//   lpd   2e-13 (1 + (1 + |y|) max_i T)   | 2e-13 (1 + s max_i (|y| + T)^2 / 2)
// (logistic | Gaussian link).  Also: no labels, and a model of another type.
//
//   ./test_glm_predict       (needs a GPU)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
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

static const long M = 200, MT = 129, D = 5, N = 300;
static const size_t ITERS = 4;

static double Uniform(unsigned long long &s) // (-1, 1), splitmix64
{
    s += 0x9e3779b97f4a7c15ULL;
    unsigned long long z = s;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) / 4503599627370496.0 - 1.0;
}

static void Data(unsigned long long &seed, long rows, bool logistic, Eigen::MatrixXd *A, Eigen::VectorXd *y)
{
    A->resize(rows, D);
    y->resize(rows);
    for (long m = 0; m < rows; ++m)
    {
        for (long k = 0; k < D; ++k)
            (*A)(m, k) = Uniform(seed);
        (*y)(m) = logistic ? (Uniform(seed) > 0.0 ? 1.0 : 0.0) : 3.0 * Uniform(seed);
    }
}

// worst |device - host| / bar over the records, per quantity
static void Excess(const Eigen::MatrixXd &A, const Eigen::VectorXd &y, const Eigen::MatrixXd &X, bool logistic,
                   double s, const SVGD::Prediction &dev, const Eigen::VectorXd &mean, const Eigen::VectorXd &var,
                   const Eigen::VectorXd &lpd, double ex[3])
{
    ex[0] = ex[1] = ex[2] = 0.0;
    Eigen::VectorXd xbar = Eigen::VectorXd::Zero(D);
    for (long i = 0; i < N; ++i)
        xbar += X.col(i) / (double)N;
    for (long m = 0; m < A.rows(); ++m)
    {
        double tbar = 0.0, tmean = 0.0, tmax = 0.0, t2 = 0.0;
        for (long k = 0; k < D; ++k)
            tbar += std::fabs(A(m, k)) * std::fabs(xbar(k));
        for (long i = 0; i < N; ++i)
        {
            double t = 0.0;
            for (long k = 0; k < D; ++k)
                t += std::fabs(A(m, k)) * std::fabs(X(k, i));
            tmean += t / (double)N;
            tmax = std::max(tmax, t);
            t2 += (t + tbar) * (t + tbar) / (double)N;
        }
        const double ay = std::fabs(y(m));
        const double bm = logistic ? 1e-13 * (1.0 + tmean) : 1e-13 * (tmean + tbar);
        const double bv = logistic ? 1e-13 * (1.0 + tmean) : 1e-13 * t2;
        const double bl = logistic ? 2e-13 * (1.0 + (1.0 + ay) * tmax) : 2e-13 * (1.0 + s * (ay + tmax) * (ay + tmax) / 2.0);
        ex[0] = std::max(ex[0], std::fabs(dev.mean(m) - mean(m)) / bm);
        ex[1] = std::max(ex[1], std::fabs(dev.var(m) - var(m)) / bv);
        ex[2] = std::max(ex[2], std::fabs(dev.lpd(m) - lpd(m)) / bl);
    }
}

int main()
{
    unsigned long long seed = 97531;
    for (int gaussian = 0; gaussian < 2; ++gaussian)
    {
        const bool logistic = !gaussian;
        const double s = logistic ? 1.0 : 0.7;
        Eigen::MatrixXd A, At;
        Eigen::VectorXd y, yt;
        Data(seed, M, logistic, &A, &y);
        Data(seed, MT, logistic, &At, &yt);
        auto pts = std::make_shared<Eigen::MatrixXd>(D, N);
        for (long i = 0; i < N; ++i)
            for (long k = 0; k < D; ++k)
                (*pts)(k, i) = 0.5 * Uniform(seed);
        auto glm = std::make_shared<GeneralizedLinearModel>(
            A, y, logistic ? GeneralizedLinearModel::Link::Logistic : GeneralizedLinearModel::Link::Gaussian, s, 1.0);
        auto kernel = std::make_shared<GaussianRBFKernel>(pts, GaussianRBFKernel::ScaleMethod::Median, glm);
        SVGD svgd(D, ITERS, pts, kernel, glm, std::make_shared<Adam>(D, N, 0.05, 0.9, 0.999));
        svgd.Initialize();
        svgd.Run();
        const SVGD::Prediction dev = svgd.Predict(At, &yt);
        CHECK(dev.mean.rows() == MT && dev.var.rows() == MT && dev.lpd.rows() == MT);
        Eigen::VectorXd mean, var, lpd;
        glm->Predict(pts->data(), N, At, &yt, &mean, &var, &lpd);
        double ex[3];
        Excess(At, yt, *pts, logistic, s, dev, mean, var, lpd, ex);
        std::printf("%s: SVGD::Predict vs GeneralizedLinearModel::Predict: mean %.3g var %.3g lpd %.3g of the bar\n",
                    logistic ? "logistic" : "gaussian", ex[0], ex[1], ex[2]);
        CHECK(ex[0] <= 1.0 && ex[1] <= 1.0 && ex[2] <= 1.0);
        bool finite = true, nonneg = true;
        for (long m = 0; m < MT; ++m)
        {
            finite = finite && std::isfinite(dev.mean(m)) && std::isfinite(dev.var(m)) && std::isfinite(dev.lpd(m));
            nonneg = nonneg && dev.var(m) >= 0.0;
        }
        CHECK(finite);
        CHECK(nonneg);
        // no labels: the same mean and var bits, no lpd
        const SVGD::Prediction nol = svgd.Predict(At);
        CHECK(nol.lpd.rows() == 0);
        bool same = true;
        for (long m = 0; m < MT; ++m)
            same = same && nol.mean(m) == dev.mean(m) && nol.var(m) == dev.var(m);
        CHECK(same);
        // Run() goes on from the same particles afterwards
        svgd.Run();
    }

    // a model of another type is refused
    {
        auto mvn = std::make_shared<MultivariateNormal>(Eigen::VectorXd::Zero(D), Eigen::MatrixXd::Identity(D, D));
        auto pts = std::make_shared<Eigen::MatrixXd>(Eigen::MatrixXd::Zero(D, N));
        auto kernel = std::make_shared<GaussianRBFKernel>(pts, GaussianRBFKernel::ScaleMethod::Median, mvn);
        SVGD svgd(D, 1, pts, kernel, mvn, std::make_shared<Adam>(D, N, 0.05, 0.9, 0.999));
        bool threw = false;
        try
        {
            svgd.Predict(Eigen::MatrixXd::Zero(3, D));
        }
        catch (const std::invalid_argument &)
        {
            threw = true;
        }
        CHECK(threw);
    }
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
