/**
 * @file InverseMultiquadricKernel.hpp
 * @brief Inverse multiquadric kernel (extension; svgd_capi.h "inverse multiquadric kernel").
 *
 * k(x, x') = (1 + a |x - x'|^2)^(-1/2),  grad_x k = -a (x - x') k^3; the
 * exponent and the offset are fixed.
 *   ScaleMethod::Median   a = ln(N) / med^2, med = median of all N^2 pairwise
 *                         distances of the coordinate matrix (the RBF kernel's
 *                         median) -- recomputed every step ON THE DEVICE by
 *                         the SVGD driver.
 *   ScaleMethod::Constant a fixed a: the constructor's `scale`, or
 *                         UpdateParameters({a}) (a 1 x 1 matrix).
 * SVGD runs this kernel on the device like the GaussianRBFKernel
 * (svgd_set_kernel(SVGD_KERNEL_IMQ)).  The host methods below restate the
 * kernel for callers that use it directly and for compositions (imq + k,
 * imq * k, ... run on the generic host path).
 */
#ifndef SVGDCPP_AMD_INVERSE_MULTIQUADRIC_KERNEL_HPP
#define SVGDCPP_AMD_INVERSE_MULTIQUADRIC_KERNEL_HPP

#include "../Core.hpp"
#include "Kernel.hpp"

class InverseMultiquadricKernel : public Kernel
{
public:
    enum class ScaleMethod
    {
        Median = 0,
        Constant = 1
    };

    InverseMultiquadricKernel() {}

    InverseMultiquadricKernel(const std::shared_ptr<Eigen::MatrixXd> &coord_mat_ptr,
                              const ScaleMethod &method = ScaleMethod::Median, double scale = 1.0)
        : Kernel((size_t)coord_mat_ptr->rows()), scale_method_(method), coord_matrix_ptr_(coord_mat_ptr)
    {
        kernel_parameters_ = {Eigen::MatrixXd::Constant(1, 1, Checked(scale))};
        // the closed form as the kernel function too, so compositions work on
        // the generic host path as they do for the GaussianRBFKernel
        UpdateKernel(&InverseMultiquadricKernel::Value, &InverseMultiquadricKernel::Grad);
    }

    /** (1 + a |x - loc|^2)^(-1/2), a = params[0](0, 0). */
    static double Value(const Eigen::VectorXd &x, const std::vector<Eigen::MatrixXd> &params,
                        const Eigen::VectorXd &loc)
    {
        const double a = params.at(0)(0, 0);
        double r2 = 0.0;
        for (long c = 0; c < x.rows(); ++c)
            r2 += (x(c) - loc(c)) * (x(c) - loc(c));
        return 1.0 / std::sqrt(1.0 + a * r2);
    }

    /** grad_x: -a (x - loc) k^3. */
    static Eigen::VectorXd Grad(const Eigen::VectorXd &x, const std::vector<Eigen::MatrixXd> &params,
                                const Eigen::VectorXd &loc)
    {
        const double a = params.at(0)(0, 0);
        const double k = Value(x, params, loc);
        Eigen::VectorXd g(x.rows());
        for (long c = 0; c < x.rows(); ++c)
            g(c) = -a * (x(c) - loc(c)) * (k * k * k);
        return g;
    }

    std::unique_ptr<Kernel> CloneUniquePointer() const override
    {
        return std::make_unique<InverseMultiquadricKernel>(*this);
    }
    std::shared_ptr<Kernel> CloneSharedPointer() const override
    {
        return std::make_shared<InverseMultiquadricKernel>(*this);
    }

    ScaleMethod GetScaleMethod() const { return scale_method_; }

    /** The scale a (kernel_parameters_[0](0, 0)). */
    double GetScale() const { return kernel_parameters_.at(0)(0, 0); }

    void UpdateParameters(const std::vector<Eigen::MatrixXd> &params) override
    {
        const Eigen::MatrixXd &A = params.at(0);
        if (A.rows() != 1 || A.cols() != 1)
            throw DimensionMismatchException("The inverse multiquadric kernel takes one scalar scale.");
        kernel_parameters_ = {Eigen::MatrixXd::Constant(1, 1, Checked(A(0, 0)))};
    }

    double EvaluateKernel(const Eigen::VectorXd &x) override { return Value(x, kernel_parameters_, location_); }

    Eigen::VectorXd EvaluateKernelGrad(const Eigen::VectorXd &x) override
    {
        return Grad(x, kernel_parameters_, location_);
    }

    /** Host restatement of the median heuristic (O(N^2) memory, small N
     *  only); the SVGD driver computes the scale on the device. */
    void Step() override
    {
        if (scale_method_ != ScaleMethod::Median)
            return;
        const Eigen::MatrixXd &X = *coord_matrix_ptr_;
        const long n = X.cols(), d = X.rows();
        std::vector<double> dist((size_t)(n * n));
        for (long j = 0; j < n; ++j)
            for (long i = 0; i < n; ++i)
            {
                double s = 0.0;
                for (long k = 0; k < d; ++k)
                    s += (X(k, i) - X(k, j)) * (X(k, i) - X(k, j));
                dist[(size_t)(j * n + i)] = std::sqrt(s);
            }
        const size_t h = dist.size() / 2;
        std::nth_element(dist.begin(), dist.begin() + (long)h, dist.end());
        double med = dist[h];
        if (dist.size() % 2 == 0)
            med = (med + *std::max_element(dist.begin(), dist.begin() + (long)h)) / 2.0;
        kernel_parameters_ = {Eigen::MatrixXd::Constant(1, 1, std::log((double)n) / std::pow(med, 2))};
    }

protected:
    static double Checked(double a)
    {
        if (!(a >= 0.0) || !std::isfinite(a))
            throw std::invalid_argument(SVGDCPP_LOG_PREFIX +
                                        "[Argument Error] The inverse multiquadric scale must be finite and >= 0.");
        return a;
    }

    ScaleMethod scale_method_ = ScaleMethod::Median;
    std::shared_ptr<Eigen::MatrixXd> coord_matrix_ptr_;
};

#endif
