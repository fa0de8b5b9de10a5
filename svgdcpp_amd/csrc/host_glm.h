// Internal layout of the generalized-linear-model handle (host_glm.cpp),
// shared with the C ABI so a context can mirror the data on the device.
#pragma once
#include <cstdint>
#include <vector>

namespace svgd_amd {
struct HostGlm {
    int d = 0;
    int64_t m = 0;         // data rows
    int link = 0;          // SVGD_GLM_LOGISTIC / SVGD_GLM_GAUSSIAN
    double lik_scale = 1;  // s
    double prior_prec = 1; // lambda
    int64_t m0 = 0, count = 0; // batch window [m0, m0 + count)
    std::vector<double> A; // m x d, row-major
    std::vector<double> y; // m
};
// sigma(z) from e = exp(-|z|) in both tails (no overflow, no cancellation)
double glm_sigmoid(double z);
} // namespace svgd_amd
