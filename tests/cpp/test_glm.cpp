// GeneralizedLinearModel (C++ API) and the SVGD class's device-model step:
// Bayesian logistic regression on M = 200 rows, d = 5, N = 300 particles.
//
//   closed forms    EvaluateLogModelGrad against the definition in long double,
//                   1e-13 of sum_m |a_mk| s M/B + lambda |theta_k| (tests/_glm.py)
//   device step     UsesDeviceModelStep(); Run() against a manual loop of the
//                   split C calls with host gradients, <= 1e-10, with a window
//                   that moves every step
//   matrix logging  takes the split calls and gives the same result (<= 1e-10)
//   a subclass      keeps the split calls
//   ComputeKSD      the device score against a subclass's host score, at the
//                   KSD's bar 1e-10 max(1, |V|)
//
//   ./test_glm       (needs a GPU)
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

// moves its window before every step, as a user's loop would -- not in a
// subclass (a subclass keeps the split calls): the driver calls Move()
struct Mover
{
    std::shared_ptr<GeneralizedLinearModel> glm;
    size_t t = 0;
    void Move()
    {
        int64_t m0, cnt;
        Window(t++, &m0, &cnt);
        glm->SetBatch(m0, cnt);
    }
};

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
    unsigned long long seed = 12345;
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
    const double s = 0.7, lam = 1.3;

    // closed forms against the definition
    {
        GeneralizedLinearModel glm(A, y, GeneralizedLinearModel::Link::Logistic, s, lam);
        glm.SetBatch(3, 61);
        double worst = 0.0;
        for (long i = 0; i < 10; ++i)
        {
            Eigen::VectorXd x(D);
            for (long k = 0; k < D; ++k)
                x(k) = 4.0 * X0(k, i);
            const Eigen::VectorXd g = glm.EvaluateLogModelGrad(x);
            for (long k = 0; k < D; ++k)
            {
                long double acc = 0.0L, mag = 0.0L;
                for (long m = 3; m < 64; ++m)
                {
                    long double z = 0.0L;
                    for (long q = 0; q < D; ++q)
                        z += (long double)A(m, q) * (long double)x(q);
                    const long double sig = 1.0L / (1.0L + std::exp(-z));
                    acc += ((long double)y(m) - sig) * (long double)A(m, k);
                    mag += std::fabs((long double)A(m, k));
                }
                const long double f = (long double)s * (long double)M / 61.0L;
                const long double ref = f * acc - (long double)lam * (long double)x(k);
                const long double bar = 1e-13L * (f * mag + (long double)lam * std::fabs((long double)x(k)));
                worst = std::max(worst, (double)(std::fabs((long double)g(k) - ref) / bar));
            }
        }
        std::printf("closed-form gradient: %.3g of the bar\n", worst);
        CHECK(worst <= 1.0);
        CHECK(glm.BatchBegin() == 3 && glm.BatchCount() == 61 && glm.NumRows() == M);
        bool threw = false;
        try
        {
            glm.SetBatch(150, 51);
        }
        catch (const std::exception &)
        {
            threw = true;
        }
        CHECK(threw);
        // a copy owns its own handle and keeps the window
        GeneralizedLinearModel copy(glm);
        CHECK(copy.GlmHandle() != glm.GlmHandle() && copy.BatchBegin() == 3);
        Eigen::VectorXd x(D);
        for (long k = 0; k < D; ++k)
            x(k) = X0(k, 0);
        CHECK(MaxAbsDiff(copy.EvaluateLogModelGrad(x), glm.EvaluateLogModelGrad(x)) == 0.0);
    }

    // the manual loop: split C calls with host gradients
    Eigen::MatrixXd Xmanual = X0;
    {
        GeneralizedLinearModel glm(A, y, GeneralizedLinearModel::Link::Logistic, 1.0, 1.0);
        svgd_ctx *c = nullptr;
        CHECK(svgd_create(&c, (int)D, (int64_t)N, SVGD_F64, 0) == SVGD_OK);
        CHECK(svgd_set_particles(c, Xmanual.data()) == SVGD_OK);
        CHECK(svgd_set_optimizer(c, SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8) == SVGD_OK);
        double *hx = nullptr, *hg = nullptr;
        CHECK(svgd_host_buffers(c, &hx, &hg) == SVGD_OK);
        for (size_t t = 0; t < ITERS; ++t)
        {
            int64_t m0, cnt;
            Window(t, &m0, &cnt);
            glm.SetBatch(m0, cnt);
            CHECK(svgd_begin_step(c, hx) == SVGD_OK);
            glm.LogModelGradBatch(hx, N, hg);
            CHECK(svgd_finish_step(c, hg) == SVGD_OK);
        }
        CHECK(svgd_get_particles(c, Xmanual.data()) == SVGD_OK);
        svgd_destroy(c);
    }

    // the SVGD class, one step per Run() so the window can move between steps
    for (int logging = 0; logging < 2; ++logging)
    {
        auto glm = std::make_shared<GeneralizedLinearModel>(A, y, GeneralizedLinearModel::Link::Logistic, 1.0, 1.0);
        auto pts = std::make_shared<Eigen::MatrixXd>(X0);
        auto kernel = std::make_shared<GaussianRBFKernel>(pts, GaussianRBFKernel::ScaleMethod::Median, glm);
        auto optimizer = std::make_shared<Adam>(D, N, 0.05, 0.9, 0.999);
        SVGD svgd(D, 1, pts, kernel, glm, optimizer, Eigen::VectorXd::Constant(1, -INFINITY),
                  Eigen::VectorXd::Constant(1, INFINITY), false, logging != 0, "test_glm_log.txt");
        Mover mover{glm};
        mover.Move();
        svgd.Initialize();
        CHECK(svgd.UsesDeviceModelStep() == (logging == 0));
        CHECK(!svgd.UsesPipelinedStep());
        for (size_t t = 0; t < ITERS; ++t)
        {
            if (t > 0)
                mover.Move();
            svgd.Run();
        }
        const double err = MaxAbsDiff(*pts, Xmanual);
        std::printf("%s: Run vs the manual host-gradient loop %.3g\n",
                    logging ? "matrix logging (split calls)" : "device-model step", err);
        CHECK(err <= 1e-10);
        if (!logging)
        {
            // the KSD from the device score against a subclass's host score
            const double v = svgd.ComputeKSD(), u = svgd.ComputeKSD(true);
            auto sub = std::make_shared<SubGlm>(A, y, GeneralizedLinearModel::Link::Logistic, 1.0, 1.0);
            sub->SetBatch(glm->BatchBegin(), glm->BatchCount());
            auto pts2 = std::make_shared<Eigen::MatrixXd>(*pts);
            auto kernel2 = std::make_shared<GaussianRBFKernel>(pts2, GaussianRBFKernel::ScaleMethod::Median, sub);
            SVGD host(D, 1, pts2, kernel2, sub, std::make_shared<Adam>(D, N, 0.05, 0.9, 0.999));
            host.Initialize();
            CHECK(!host.UsesDeviceModelStep());
            const double vh = host.ComputeKSD(), uh = host.ComputeKSD(true);
            const double bar = 1e-10 * std::max(1.0, std::fabs(vh));
            std::printf("KSD V=%.12g (host score %.12g)  U=%.12g (host score %.12g)  bar %.3g\n", v, vh, u, uh, bar);
            CHECK(std::fabs(v - vh) <= bar);
            CHECK(std::fabs(u - uh) <= bar);
        }
    }
    std::remove("test_glm_log.txt");
    std::printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
