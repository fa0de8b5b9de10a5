// The SVGD class's device step under the Hessian scale (C++ API): Bayesian
// logistic regression on M = 200 rows, d = 5, N = 300 particles.
//
//   device step     a Hessian kernel whose target model is the stepped
//                   GeneralizedLinearModel: UsesDeviceModelStep(), and Run()
//                   against a manual loop of the split C calls with the host
//                   Hessian sum and host gradients, <= 1e-9 (the bar of
//                   Hessian-scale steps), with a window that moves every step
//   another target  a kernel on a second model object keeps the split calls
//   a subclass      keeps the split calls
//
//   ./test_glm_hess       (needs a GPU)
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

static const long M = 200, D = 5, N = 300;
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

static void Window(size_t t, int64_t *m0, int64_t *count)
{
    *m0 = (int64_t)((37 * t) % (size_t)(M - 120));
    *count = 100 + (int64_t)t;
}

class SubGlm : public GeneralizedLinearModel
{
public:
    using GeneralizedLinearModel::GeneralizedLinearModel;
    std::shared_ptr<Model> CloneSharedPointer() const override { return std::make_shared<SubGlm>(*this); }
};

static double MaxAbsDiff(const Eigen::MatrixXd &a, const Eigen::MatrixXd &b)
{
    double m = 0.0;
    for (long e = 0; e < a.size(); ++e)
        m = std::max(m, std::fabs(a.data()[e] - b.data()[e]));
    return m;
}

int main()
{
    unsigned long long seed = 4321;
    Eigen::MatrixXd A(M, D);
    Eigen::VectorXd y(M);
    for (long m = 0; m < M; ++m)
    {
        for (long k = 0; k < D; ++k)
            A(m, k) = Uniform(seed);
        y(m) = Uniform(seed) > 0.0 ? 1.0 : 0.0;
    }
    Eigen::MatrixXd X0(D, N);
    for (long i = 0; i < N; ++i)
        for (long k = 0; k < D; ++k)
            X0(k, i) = 0.5 * Uniform(seed);

    // the manual loop: split C calls, host Hessian sum and host gradients
    Eigen::MatrixXd Xmanual = X0;
    {
        GeneralizedLinearModel glm(A, y, GeneralizedLinearModel::Link::Logistic, 1.0, 1.0);
        svgd_ctx *c = nullptr;
        CHECK(svgd_create(&c, (int)D, (int64_t)N, SVGD_F64, 0) == SVGD_OK);
        CHECK(svgd_set_particles(c, Xmanual.data()) == SVGD_OK);
        CHECK(svgd_set_optimizer(c, SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8) == SVGD_OK);
        CHECK(svgd_set_scale(c, SVGD_SCALE_HESSIAN, 0.0) == SVGD_OK);
        double *hx = nullptr, *hg = nullptr;
        CHECK(svgd_host_buffers(c, &hx, &hg) == SVGD_OK);
        std::vector<double> H((size_t)D * D);
        for (size_t t = 0; t < ITERS; ++t)
        {
            int64_t m0, cnt;
            Window(t, &m0, &cnt);
            glm.SetBatch(m0, cnt);
            CHECK(svgd_begin_step(c, hx) == SVGD_OK);
            glm.NegHessSumBatch(hx, N, H.data());
            CHECK(svgd_set_step_hessian_sum(c, H.data()) == SVGD_OK);
            glm.LogModelGradBatch(hx, N, hg);
            CHECK(svgd_finish_step(c, hg) == SVGD_OK);
        }
        CHECK(svgd_get_particles(c, Xmanual.data()) == SVGD_OK);
        svgd_destroy(c);
    }

    // the SVGD class, one step per Run() so the window can move between steps:
    // target 0 the stepped model itself, 1 a second object with the same data
    for (int other = 0; other < 2; ++other)
    {
        auto glm = std::make_shared<GeneralizedLinearModel>(A, y, GeneralizedLinearModel::Link::Logistic, 1.0, 1.0);
        auto target = other ? std::make_shared<GeneralizedLinearModel>(A, y, GeneralizedLinearModel::Link::Logistic,
                                                                     1.0, 1.0)
                            : glm;
        auto pts = std::make_shared<Eigen::MatrixXd>(X0);
        auto kernel = std::make_shared<GaussianRBFKernel>(pts, GaussianRBFKernel::ScaleMethod::Hessian, target);
        auto optimizer = std::make_shared<Adam>(D, N, 0.05, 0.9, 0.999);
        SVGD svgd(D, 1, pts, kernel, glm, optimizer);
        int64_t m0, cnt;
        Window(0, &m0, &cnt);
        glm->SetBatch(m0, cnt);
        target->SetBatch(m0, cnt);
        svgd.Initialize();
        CHECK(svgd.UsesDeviceModelStep() == (other == 0));
        CHECK(!svgd.UsesPipelinedStep());
        for (size_t t = 0; t < ITERS; ++t)
        {
            Window(t, &m0, &cnt);
            glm->SetBatch(m0, cnt);
            target->SetBatch(m0, cnt);
            svgd.Run();
        }
        const double err = MaxAbsDiff(*pts, Xmanual);
        std::printf("%s: Run vs the manual split loop %.3g\n",
                    other ? "another target model (split calls)" : "device Hessian step", err);
        CHECK(err <= 1e-9);
    }

    // a subclass keeps the split calls
    {
        auto sub = std::make_shared<SubGlm>(A, y, GeneralizedLinearModel::Link::Logistic, 1.0, 1.0);
        auto pts = std::make_shared<Eigen::MatrixXd>(X0);
        auto kernel = std::make_shared<GaussianRBFKernel>(pts, GaussianRBFKernel::ScaleMethod::Hessian, sub);
        SVGD host(D, 1, pts, kernel, sub, std::make_shared<Adam>(D, N, 0.05, 0.9, 0.999));
        host.Initialize();
        CHECK(!host.UsesDeviceModelStep());
    }
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
