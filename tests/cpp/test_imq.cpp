// InverseMultiquadricKernel (C++ API) on the device path of SVGD:
//   1. Constant scale, N = 64, d = 3, 10 steps: the device run against the
//      same run on the generic host path (a plain Kernel given the class's
//      closed form through UpdateKernel): <= 1e-10
//   2. Median scale, 5 steps, against a manual loop (the class's host median,
//      phi by direct differences in long double, Adam::Step): <= 1e-9
//   3. the logged Kernel= / KernelGrad= of step 1 at N = 10 against the
//      definition in long double: <= 1e-12
//   4. the closed-form gradient against central differences; a composition
//      takes the host path; refusals
//
//   ./test_imq       (needs a GPU)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
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

static double Uniform(unsigned long long &s) // (-1, 1), splitmix64
{
    s += 0x9e3779b97f4a7c15ULL;
    unsigned long long z = s;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) / 4503599627370496.0 - 1.0;
}

static std::shared_ptr<Eigen::MatrixXd> Cloud(long d, long n, unsigned long long seed)
{
    auto pts = std::make_shared<Eigen::MatrixXd>(d, n);
    for (long i = 0; i < n; ++i)
        for (long k = 0; k < d; ++k)
            (*pts)(k, i) = Uniform(seed);
    return pts;
}

static std::shared_ptr<Model> Target(long d)
{
    Eigen::VectorXd mu = Eigen::VectorXd::Constant(d, 0.3);
    return std::make_shared<MultivariateNormal>(mu, 0.8 * Eigen::MatrixXd::Identity(d, d));
}

static double MaxDiff(const Eigen::MatrixXd &A, const Eigen::MatrixXd &B)
{
    double m = 0.0;
    for (long c = 0; c < A.cols(); ++c)
        for (long r = 0; r < A.rows(); ++r)
            m = std::max(m, std::fabs(A(r, c) - B(r, c)));
    return m;
}

// phi (d x n) by direct differences in long double
static Eigen::MatrixXd Phi(const Eigen::MatrixXd &X, const Eigen::MatrixXd &G, double a)
{
    const long d = X.rows(), n = X.cols();
    Eigen::MatrixXd phi(d, n);
    for (long i = 0; i < n; ++i)
    {
        std::vector<long double> acc((size_t)d, 0.0L);
        for (long j = 0; j < n; ++j)
        {
            long double r2 = 0.0L;
            for (long k = 0; k < d; ++k)
                r2 += ((long double)X(k, i) - X(k, j)) * ((long double)X(k, i) - X(k, j));
            const long double kv = 1.0L / std::sqrt(1.0L + (long double)a * r2);
            for (long k = 0; k < d; ++k)
                acc[(size_t)k] += kv * G(k, j) + (long double)a * kv * kv * kv * ((long double)X(k, i) - X(k, j));
        }
        for (long k = 0; k < d; ++k)
            phi(k, i) = (double)(acc[(size_t)k] / (long double)n);
    }
    return phi;
}

int main()
{
    // 1. device path vs generic host path, Constant scale
    {
        const long d = 3, n = 64;
        const double a = 0.8;
        auto dev = Cloud(d, n, 11), host = Cloud(d, n, 11);
        auto imq = std::make_shared<InverseMultiquadricKernel>(dev, InverseMultiquadricKernel::ScaleMethod::Constant, a);
        SVGD sd(d, 10, dev, imq, Target(d), std::make_shared<Adam>(d, n, 0.1, 0.9, 0.999));
        CHECK(sd.UsesDevicePath());
        sd.Initialize();
        int kind = -1;
        CHECK(svgd_get_kernel(sd.Context(), &kind) == SVGD_OK && kind == SVGD_KERNEL_IMQ);
        sd.Run();
        auto plain = std::make_shared<Kernel>((size_t)d);
        plain->UpdateKernel(&InverseMultiquadricKernel::Value, &InverseMultiquadricKernel::Grad);
        plain->UpdateParameters({Eigen::MatrixXd::Constant(1, 1, a)});
        SVGD sh(d, 10, host, plain, Target(d), std::make_shared<Adam>(d, n, 0.1, 0.9, 0.999));
        CHECK(!sh.UsesDevicePath());
        sh.Initialize();
        sh.Run();
        const double err = MaxDiff(*dev, *host);
        std::printf("imq class device vs generic host path: %.3g (bar 1e-10)\n", err);
        CHECK(err <= 1e-10);
        CHECK(MaxDiff(*dev, *Cloud(d, n, 11)) > 1e-3); // the particles moved
    }
    // 2. Median scale vs a manual loop
    {
        const long d = 3, n = 64;
        const size_t iters = 5;
        auto dev = Cloud(d, n, 13), man = Cloud(d, n, 13);
        auto imq = std::make_shared<InverseMultiquadricKernel>(dev);
        auto model = Target(d);
        SVGD sd(d, iters, dev, imq, model, std::make_shared<Adam>(d, n, 0.1, 0.9, 0.999));
        sd.Initialize();
        sd.Run();
        InverseMultiquadricKernel med(man);
        Adam opt(d, n, 0.1, 0.9, 0.999);
        opt.Initialize();
        double a = 0.0;
        for (size_t it = 0; it < iters; ++it)
        {
            med.Step(); // the host restatement of the median heuristic at X_t
            a = med.GetScale();
            Eigen::MatrixXd G(d, n);
            model->LogModelGradBatch(man->data(), n, G.data());
            *man += opt.Step(Phi(*man, G, a));
        }
        const double err = MaxDiff(*dev, *man);
        std::printf("imq class median scale vs manual loop: %.3g (bar 1e-9)\n", err);
        CHECK(err <= 1e-9);
        // Run() leaves the last step's a in the kernel
        CHECK(std::fabs(imq->GetScale() - a) <= 1e-12 * a);
    }
    // 3. logged matrices of step 1
    {
        const long d = 2, n = 10;
        auto pts = Cloud(d, n, 17);
        const Eigen::MatrixXd X0 = *pts;
        SVGDOptions o;
        o.Dimension = d;
        o.NumIterations = 2;
        o.CoordinateMatrixPtr = pts;
        o.KernelPtr = std::make_shared<InverseMultiquadricKernel>(pts);
        o.ModelPtr = Target(d);
        o.OptimizerPtr = std::make_shared<Adam>(d, n, 0.1, 0.9, 0.999);
        o.LogIntermediateMatrices = true;
        o.IntermediateMatricesOutputPath = "test_imq_log.txt";
        o.IntermediateMatricesPrecision = 17;
        auto x0 = std::make_shared<Eigen::MatrixXd>(X0);
        InverseMultiquadricKernel med(x0);
        med.Step();
        const double a = med.GetScale();
        SVGD s(o);
        s.Initialize();
        s.Run();
        std::ifstream f("test_imq_log.txt");
        std::stringstream ss;
        ss << f.rdbuf();
        const std::string text = ss.str();
        const size_t pk = text.find("Kernel=\n"), pg = text.find("KernelGrad=\n");
        CHECK(pk != std::string::npos && pg != std::string::npos);
        if (pk != std::string::npos && pg != std::string::npos)
        {
            std::istringstream sk(text.substr(pk + 8)), sg(text.substr(pg + 12));
            double worst = 0.0;
            bool read = true;
            for (long j = 0; j < n; ++j) // K(j, i) = k(x_j, x_i), rows j
                for (long i = 0; i < n; ++i)
                {
                    double v = 0.0;
                    read = read && (bool)(sk >> v);
                    long double r2 = 0.0L;
                    for (long k = 0; k < d; ++k)
                        r2 += ((long double)X0(k, j) - X0(k, i)) * ((long double)X0(k, j) - X0(k, i));
                    worst = std::max(worst, (double)std::fabs(v - 1.0L / std::sqrt(1.0L + (long double)a * r2)));
                }
            for (long j = 0; j < n; ++j) // Kg(j d + k, i) = grad_{x_j} k(x_j, x_i)
                for (long k = 0; k < d; ++k)
                    for (long i = 0; i < n; ++i)
                    {
                        double v = 0.0;
                        read = read && (bool)(sg >> v);
                        long double r2 = 0.0L;
                        for (long q = 0; q < d; ++q)
                            r2 += ((long double)X0(q, j) - X0(q, i)) * ((long double)X0(q, j) - X0(q, i));
                        const long double kv = 1.0L / std::sqrt(1.0L + (long double)a * r2);
                        const long double want = -(long double)a * ((long double)X0(k, j) - X0(k, i)) * kv * kv * kv;
                        worst = std::max(worst, (double)std::fabs(v - want));
                    }
            CHECK(read);
            std::printf("imq class logged K, Kg vs the definition: %.3g (bar 1e-12)\n", worst);
            CHECK(worst <= 1e-12);
        }
        std::remove("test_imq_log.txt");
    }
    // 4. closed forms, compositions, refusals
    {
        const long d = 4;
        auto pts = Cloud(d, 6, 19);
        InverseMultiquadricKernel k(pts, InverseMultiquadricKernel::ScaleMethod::Constant, 0.7);
        k.UpdateParameters({Eigen::MatrixXd::Constant(1, 1, 1.3)});
        CHECK(k.GetScale() == 1.3);
        Eigen::VectorXd loc = pts->col(0), x = pts->col(1);
        k.UpdateLocation(loc);
        const Eigen::VectorXd g = k.EvaluateKernelGrad(x);
        bool fd_ok = true;
        for (long c = 0; c < d; ++c)
        {
            Eigen::VectorXd xp = x, xm = x;
            xp(c) += 1e-6;
            xm(c) -= 1e-6;
            fd_ok = fd_ok && std::fabs(g(c) - (k.EvaluateKernel(xp) - k.EvaluateKernel(xm)) / 2e-6) < 1e-9;
        }
        CHECK(fd_ok);
        bool threw = false;
        try
        {
            k.UpdateParameters({Eigen::MatrixXd::Constant(1, 1, -1.0)});
        }
        catch (const std::invalid_argument &)
        {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try
        {
            k.UpdateParameters({Eigen::MatrixXd::Identity(d, d)});
        }
        catch (const DimensionMismatchException &)
        {
            threw = true;
        }
        CHECK(threw);
        // a Hessian or matrix scale on a context with the IMQ kernel, either order
        auto imq = std::make_shared<InverseMultiquadricKernel>(pts);
        SVGD s(d, 1, pts, imq, Target(d), std::make_shared<Adam>(d, 6, 0.1, 0.9, 0.999));
        s.Initialize();
        std::vector<double> M((size_t)(d * d), 0.0);
        for (long r = 0; r < d; ++r)
            M[(size_t)(r * d + r)] = 1.0;
        CHECK(svgd_set_scale(s.Context(), SVGD_SCALE_HESSIAN, 0.0) == SVGD_ERR_ARG);
        CHECK(svgd_set_scale_matrix(s.Context(), M.data()) == SVGD_ERR_ARG);
        CHECK(std::string(svgd_last_error(s.Context())).rfind("SVGDCpp: [Argument Error]", 0) == 0);
        CHECK(svgd_set_kernel(s.Context(), 7) == SVGD_ERR_ARG);
        CHECK(svgd_set_kernel(s.Context(), SVGD_KERNEL_RBF) == SVGD_OK);
        CHECK(svgd_set_scale_matrix(s.Context(), M.data()) == SVGD_OK);
        CHECK(svgd_set_kernel(s.Context(), SVGD_KERNEL_IMQ) == SVGD_ERR_ARG);
    }
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
