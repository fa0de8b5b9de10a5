// svgd_gauss_hess.hip -- -sum_i hess log p(x_i) of the built-in Gaussian-sum
// model on the device, CDNA4 (gfx950), fp64 (host: svgd_model_neg_hess_sum,
// host_models.cpp):
//   p = sum_c exp(-q_c / 2),  q_c = (x - mu_c)^T P_c (x - mu_c)
//   w = softmax(-q / 2),  g_c = -P_c (x - mu_c),  gbar = sum_c w_c g_c
//   -hess log p = sum_c w_c (P_c - g_c g_c^T) + gbar gbar^T
//               = sum_c w_c (P_c - (g_c - gbar)(g_c - gbar)^T)
// (the second form has no cancelling pair of outer products).
//
// k_gauss_hess_sum   a work-group takes a contiguous range of 32-particle
//     chunks.  Per chunk, three sweeps over the components, each with the
//     product P_c (x - mu_c) by one thread per (particle, coordinate): q_min;
//     the weights' sum and gbar; then w_c, g_c - gbar in LDS and every thread
//     adds its elements of the d x d sum (kept in LDS) over the chunk's
//     particles in particle order.  No per-thread arrays: any d <= 64 runs
//     from registers and LDS, with no scratch.  -> part[work-group][d d]
// k_gauss_hess_finish   H = sum_b part[b] (b ascending)
// No atomics, every sum in a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svgd_gauss_hess.h"

namespace svgd_amd {
namespace {

constexpr int GH_THREADS = 256;
constexpr int GH_PB = 32; // particles per chunk

__global__ __launch_bounds__(GH_THREADS) void k_gauss_hess_sum(const double *__restrict__ X, int64_t rows,
                                                               int d, int k, const double *__restrict__ mu,
                                                               const double *__restrict__ prec,
                                                               int64_t nchunks, double *__restrict__ part)
{
    __shared__ double sx[GH_PB * 64], sg[GH_PB * 64], sb[GH_PB * 64];
    __shared__ double sqmin[GH_PB], sws[GH_PB], sw[GH_PB];
    // the work-group's d x d sum: element e belongs to thread e % GH_THREADS
    // alone (in LDS, not registers: the element loop has a run-time count)
    __shared__ double sacc[64 * 64];
    const int tid = threadIdx.x, dd = d * d, pd = GH_PB * d;
    for (int e = tid; e < dd; e += GH_THREADS) sacc[e] = 0.0;

    // sg[p][r] = (P_c (x_p - mu_c))_r
    auto matvec = [&](int c) {
        const double *P = prec + (size_t)c * dd, *m = mu + (size_t)c * d;
        for (int e = tid; e < pd; e += GH_THREADS) {
            const int p = e / d, r = e - p * d;
            double s = 0.0;
            for (int l = 0; l < d; ++l) s += P[r * d + l] * (sx[p * d + l] - m[l]);
            sg[e] = s;
        }
    };
    // q_c / 2 of particle p from sg
    auto half_q = [&](int c, int p) {
        const double *m = mu + (size_t)c * d;
        double qq = 0.0;
        for (int r = 0; r < d; ++r) qq += (sx[p * d + r] - m[r]) * sg[p * d + r];
        return 0.5 * qq;
    };

    const int64_t c0 = nchunks * blockIdx.x / gridDim.x, c1 = nchunks * (blockIdx.x + 1) / gridDim.x;
    for (int64_t ch = c0; ch < c1; ++ch) {
        const int64_t i0 = ch * GH_PB;
        const int np = (int)(rows - i0 < GH_PB ? rows - i0 : GH_PB);
        __syncthreads(); // the last chunk has been read
        // particles past the shard copy its last row (finite; their weight is 0)
        for (int e = tid; e < pd; e += GH_THREADS) {
            const int p = e / d, r = e - p * d;
            sx[e] = X[(i0 + (p < np ? p : np - 1)) * d + r];
            sb[e] = 0.0;
        }
        if (tid < GH_PB) {
            sqmin[tid] = __builtin_inf();
            sws[tid] = 0.0;
        }
        __syncthreads();
        for (int c = 0; c < k; ++c) {
            matvec(c);
            __syncthreads();
            if (tid < GH_PB) sqmin[tid] = fmin(sqmin[tid], half_q(c, tid));
            __syncthreads();
        }
        for (int c = 0; c < k; ++c) {
            matvec(c);
            __syncthreads();
            if (tid < GH_PB) {
                const double w = exp(-(half_q(c, tid) - sqmin[tid]));
                sws[tid] += w;
                sw[tid] = w;
            }
            __syncthreads();
            for (int e = tid; e < pd; e += GH_THREADS) sb[e] -= sw[e / d] * sg[e];
            __syncthreads();
        }
        for (int e = tid; e < pd; e += GH_THREADS) sb[e] /= sws[e / d];
        __syncthreads();
        for (int c = 0; c < k; ++c) {
            matvec(c);
            __syncthreads();
            if (tid < GH_PB)
                sw[tid] = tid < np ? exp(-(half_q(c, tid) - sqmin[tid])) / sws[tid] : 0.0;
            __syncthreads();
            for (int e = tid; e < pd; e += GH_THREADS) sg[e] = -sg[e] - sb[e]; // g_c - gbar
            __syncthreads();
            const double *P = prec + (size_t)c * dd;
            for (int e = tid; e < dd; e += GH_THREADS) {
                const int r = e / d, l = e - r * d;
                const double pe = P[e];
                double h = sacc[e];
                for (int p = 0; p < GH_PB; ++p) h += sw[p] * (pe - sg[p * d + r] * sg[p * d + l]);
                sacc[e] = h;
            }
            __syncthreads(); // sg is rewritten by the next component
        }
    }
    for (int e = tid; e < dd; e += GH_THREADS) part[(int64_t)blockIdx.x * dd + e] = sacc[e];
}

__global__ __launch_bounds__(GH_THREADS) void k_gauss_hess_finish(const double *__restrict__ part, int nb,
                                                                  int dd, double *__restrict__ H)
{
    const int e = blockIdx.x * GH_THREADS + threadIdx.x;
    if (e >= dd) return;
    double v = 0.0;
    for (int b = 0; b < nb; ++b) v += part[(int64_t)b * dd + e];
    H[e] = v;
}

} // namespace

int gauss_hess_grid(int64_t rows)
{
    const int64_t ch = (rows + GH_PB - 1) / GH_PB;
    return (int)(ch < 1 ? 1 : ch < GAUSS_HESS_MAXGRID ? ch : GAUSS_HESS_MAXGRID);
}

hipError_t launch_gauss_hess_sum(const double *X, int64_t rows, int d, int k, const double *mu,
                                 const double *prec, double *part, double *H, hipStream_t stream)
{
    if (d < 1 || d > 64 || k < 1) return hipErrorInvalidValue;
    if (rows <= 0) return hipMemsetAsync(H, 0, sizeof(double) * (size_t)d * d, stream);
    const int nb = gauss_hess_grid(rows);
    hipLaunchKernelGGL(k_gauss_hess_sum, dim3(nb), dim3(GH_THREADS), 0, stream, X, rows, d, k, mu, prec,
                       (rows + GH_PB - 1) / GH_PB, part);
    hipLaunchKernelGGL(k_gauss_hess_finish, dim3((d * d + GH_THREADS - 1) / GH_THREADS), dim3(GH_THREADS), 0,
                       stream, part, nb, d * d, H);
    return hipGetLastError();
}

} // namespace svgd_amd
