/**
 * @file GeneralizedLinearModel.hpp
 * @brief Posterior of Bayesian logistic / linear regression (an extension
 *        beyond the reference).
 *
 * Data A (M x d) and y (M), prior N(0, I / prior_prec); for a particle theta
 *   z_m   = a_m . theta
 *   log p = s (M/B) sum_m l(y_m, z_m) - (prior_prec / 2) |theta|^2
 *   Logistic  l = y z - log(1 + e^z)   (y in [0, 1])
 *   Gaussian  l = -(y - z)^2 / 2
 * with s = lik_scale and the sum over the batch window [m0, m0 + B) of the
 * rows (SetBatch; all rows by default), scaled by M / B.  Everything is
 * evaluated in closed form by the C host model (svgd_glm_*); an SVGD with a
 * model of exactly this type mirrors it on the device and runs the whole
 * step there (SVGD::UsesDeviceModelStep).
 */
#ifndef SVGDCPP_AMD_GENERALIZED_LINEAR_MODEL_HPP
#define SVGDCPP_AMD_GENERALIZED_LINEAR_MODEL_HPP

#include "../Core.hpp"
#include "Model.hpp"

class GeneralizedLinearModel : public Model
{
public:
    enum class Link
    {
        Logistic = SVGD_GLM_LOGISTIC,
        Gaussian = SVGD_GLM_GAUSSIAN
    };

    GeneralizedLinearModel() {}

    /** A: M x d (one data row per matrix row), y: M. */
    GeneralizedLinearModel(const Eigen::MatrixXd &A, const Eigen::VectorXd &y, Link link = Link::Logistic,
                           double lik_scale = 1.0, double prior_prec = 1.0)
        : Model((size_t)A.cols()), rows_((int64_t)A.rows()), link_(link), lik_scale_(lik_scale),
          prior_prec_(prior_prec), m0_(0), count_((int64_t)A.rows())
    {
        if (A.rows() != y.rows())
            throw DimensionMismatchException("GLM data: A must be M x d and y of size M.");
        a_.resize((size_t)A.rows() * A.cols());
        for (long r = 0; r < A.rows(); ++r)
            for (long c = 0; c < A.cols(); ++c)
                a_[(size_t)r * A.cols() + c] = A(r, c);
        y_.assign(y.data(), y.data() + y.rows());
        Build();
    }

    GeneralizedLinearModel(const GeneralizedLinearModel &o) : Model(o) { CopyFrom(o); }
    GeneralizedLinearModel &operator=(const GeneralizedLinearModel &o)
    {
        Model::operator=(o);
        CopyFrom(o);
        return *this;
    }

    std::unique_ptr<Model> CloneUniquePointer() const override
    {
        return std::make_unique<GeneralizedLinearModel>(*this);
    }
    std::shared_ptr<Model> CloneSharedPointer() const override
    {
        return std::make_shared<GeneralizedLinearModel>(*this);
    }

    void Initialize() override
    {
        if (dimension_ <= 0)
            throw UnsetException("Model dimension (" + std::to_string(dimension_) + ") is improperly or not set.");
        GlmHandle();
    }

    /** The batch window [m0, m0 + count) of the data rows. */
    void SetBatch(int64_t m0, int64_t count)
    {
        if (svgd_glm_set_batch(const_cast<void *>(GlmHandle()), m0, count) != SVGD_OK)
            svgdcpp::ThrowFromCode(SVGD_ERR_ARG, SVGDCPP_LOG_PREFIX + "[Argument Error] Batch window outside the data.");
        m0_ = m0;
        count_ = count;
    }
    int64_t BatchBegin() const { return m0_; }
    int64_t BatchCount() const { return count_; }
    int64_t NumRows() const { return rows_; }

    /** The C handle (svgd_glm_create; built on first use), for
     *  svgd_set_device_glm.  Owned by this object. */
    const void *GlmHandle()
    {
        if (!glm_)
            Build();
        return glm_.get();
    }

    double EvaluateLogModel(const Eigen::VectorXd &x) override
    {
        double v = 0.0;
        CheckRc(svgd_glm_logp(const_cast<void *>(GlmHandle()), x.data(), 1, &v));
        return v;
    }
    double EvaluateModel(const Eigen::VectorXd &x) override { return std::exp(EvaluateLogModel(x)); }
    Eigen::VectorXd EvaluateLogModelGrad(const Eigen::VectorXd &x) override
    {
        Eigen::VectorXd g(dimension_);
        LogModelGradBatch(x.data(), 1, g.data());
        return g;
    }
    Eigen::VectorXd EvaluateModelGrad(const Eigen::VectorXd &x) override
    {
        return EvaluateModel(x) * EvaluateLogModelGrad(x);
    }
    Eigen::MatrixXd EvaluateLogModelHessian(const Eigen::VectorXd &x) override
    {
        Eigen::MatrixXd H((long)dimension_, (long)dimension_);
        NegHessSumBatch(x.data(), 1, H.data()); // symmetric: the storage order does not matter
        for (long e = 0; e < H.size(); ++e)
            H(e) = -H(e);
        return H;
    }
    Eigen::MatrixXd EvaluateModelHessian(const Eigen::VectorXd &x) override
    {
        const Eigen::VectorXd g = EvaluateLogModelGrad(x);
        return EvaluateModel(x) * (EvaluateLogModelHessian(x) + g * g.transpose());
    }

    void LogModelGradBatch(const double *X, int64_t n, double *G) override
    {
        CheckRc(svgd_glm_logp_grad(const_cast<void *>(GlmHandle()), X, n, G));
    }
    void NegHessSumBatch(const double *X, int64_t n, double *H) override
    {
        CheckRc(svgd_glm_neg_hess_sum(const_cast<void *>(GlmHandle()), X, n, H));
    }

    Link GetLink() const { return link_; }
    double GetLikScale() const { return lik_scale_; }

    /** Posterior predictive on the m held-out rows A (m x d, one test row per
     *  matrix row; labels y optional) over the n particles X (n x d
     *  row-major), on the host with the model's own link and lik_scale
     *  (svgd_glm_predict_host).  Any output may be null; lpd needs y. */
    void Predict(const double *X, int64_t n, const Eigen::MatrixXd &A, const Eigen::VectorXd *y,
                 Eigen::VectorXd *mean, Eigen::VectorXd *var, Eigen::VectorXd *lpd) const
    {
        if ((size_t)A.cols() != (size_t)dimension_ || (y && y->rows() != A.rows()))
            throw DimensionMismatchException("Test rows do not match the model dimension or the labels.");
        const std::vector<double> a = RowMajor(A);
        const int64_t m = (int64_t)A.rows();
        for (Eigen::VectorXd *o : {mean, var, lpd})
            if (o)
                o->resize(A.rows());
        const int rc = svgd_glm_predict_host((int)link_, lik_scale_, (int)dimension_, a.data(), y ? y->data() : nullptr,
                                             m, X, n, mean ? mean->data() : nullptr, var ? var->data() : nullptr,
                                             lpd ? lpd->data() : nullptr);
        if (rc == SVGD_ERR_DIM)
            throw DimensionMismatchException("Prediction needs at least one test row and one particle.");
        if (rc != SVGD_OK)
            svgdcpp::ThrowFromCode(rc, SVGDCPP_LOG_PREFIX + "[Argument Error] Prediction: the test data must be "
                                                            "finite and logistic labels in [0, 1].");
    }

    /** A (rows x cols) as row-major doubles. */
    static std::vector<double> RowMajor(const Eigen::MatrixXd &A)
    {
        std::vector<double> a((size_t)A.rows() * A.cols());
        for (long r = 0; r < A.rows(); ++r)
            for (long c = 0; c < A.cols(); ++c)
                a[(size_t)r * A.cols() + c] = A(r, c);
        return a;
    }

protected:
    static void CheckRc(int rc)
    {
        if (rc != SVGD_OK)
            svgdcpp::ThrowFromCode(rc, SVGDCPP_LOG_PREFIX + "[Runtime Error] host model evaluation failed.");
    }

    void CopyFrom(const GeneralizedLinearModel &o)
    {
        a_ = o.a_;
        y_ = o.y_;
        rows_ = o.rows_;
        link_ = o.link_;
        lik_scale_ = o.lik_scale_;
        prior_prec_ = o.prior_prec_;
        m0_ = o.m0_;
        count_ = o.count_;
        glm_.reset(); // a handle belongs to one object: rebuilt on first use
    }

    void Build()
    {
        void *h = nullptr;
        const int rc = svgd_glm_create(&h, dimension_, rows_, a_.data(), y_.data(), (int)link_, lik_scale_,
                                       prior_prec_);
        if (rc == SVGD_ERR_DIM)
            throw DimensionMismatchException("GLM data: at least one row and one column are needed.");
        if (rc != SVGD_OK)
            svgdcpp::ThrowFromCode(rc, SVGDCPP_LOG_PREFIX + "[Argument Error] GLM: the data must be finite, logistic "
                                                            "labels in [0, 1], lik_scale > 0 and prior_prec >= 0.");
        glm_.reset(h, [](void *p) { svgd_glm_destroy(p); });
        if (svgd_glm_set_batch(h, m0_, count_) != SVGD_OK)
            svgdcpp::ThrowFromCode(SVGD_ERR_ARG, SVGDCPP_LOG_PREFIX + "[Argument Error] Batch window outside the data.");
    }

    std::vector<double> a_, y_; // M x d row-major, M
    int64_t rows_ = 0;
    Link link_ = Link::Logistic;
    double lik_scale_ = 1.0, prior_prec_ = 1.0;
    int64_t m0_ = 0, count_ = 0;
    std::shared_ptr<void> glm_;
};

#endif
