// svgd_thin.hip -- Stein thinning of the particle set, CDNA4 (gfx950), fp64
// whatever the context's dtype: the greedy choice of m points whose empirical
// measure has the smallest kernelized Stein discrepancy (the definition:
// host_thin.cpp).  One point against N per pick, so u(pi, j) is evaluated by
// direct differences r = x_pi - x_j: no centring, no Gram form.
//
// k_thin_prep       one thread per candidate: the coordinate-major copy
//     xs[c][j] = x_j[c], xs[d + c][j] = s_j[c] (zeros up to thin_padded(n)),
//     diag[j] = u_jj, acc[j] = 0, and the work-group's minimum of
//     obj_1 = u_jj / 2 into parity 0 of the partials.
// k_thin_pick<IMQ, U>  pick p = 0 .. m-1, one thread per candidate j:
//     1. every work-group reduces the partials it is handed (the last
//        launch's, or k_thin_select's one) to pi, the same in all of them;
//     2. x_pi and s_pi (2d doubles, row-major X and G) go to LDS and are read
//        from there by every lane at once (a broadcast), x_j and s_j stream
//        from xs, lane j at consecutive addresses, U coordinates a round with
//        all 2U loads issued before the first use (N = 65536 is one wave per
//        SIMD: the loads in flight are what hides the latency):
//        t = |r|^2, s_pi.s_j, (s_pi - s_j).r;
//     3. k = exp(-a t) (RBF, as k_ksd_tile) or rsqrt_full(1 + a t) (IMQ, as
//        k_ksd_imq_pass), u, with u_jj by index at j = pi; the thread j = pi
//        also appends pi and S_p = S_{p-1} + 2 acc[pi] + u_pipi;
//     4. acc[j] += u, obj = u_jj / 2 + acc[j] (+inf for a padding row or a
//        NaN), the work-group's (min, lowest index attaining it) into the
//        other parity of the partials.
// k_thin_select     one work-group: the partials to one.  The two-launch
//     form of a pick, kept for the measurement in DESIGN 4.9.2.
// Plain stream-ordered launches; no atomics; a minimum over exact
// comparisons of (value, index) does not depend on its grouping, so two
// calls on the same state give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "svgd_imq_dev.h"
#include "svgd_thin.h"

namespace svgd_amd {
namespace thin {

struct Best {
    double v;
    int i;
};

__device__ __forceinline__ Best better(Best a, Best b)
{
    return b.v < a.v || (b.v == a.v && b.i < a.i) ? b : a;
}

// the work-group's best, in every thread (sv, si: one slot per wave)
__device__ __forceinline__ Best wg_best(Best b, double *sv, int *si)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) b = better(b, Best{__shfl_xor(b.v, off), __shfl_xor(b.i, off)});
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads(); // the slots' last readers are done
    if (lane == 0) {
        sv[w] = b.v;
        si[w] = b.i;
    }
    __syncthreads();
    Best r{sv[0], si[0]};
#pragma unroll
    for (int q = 1; q < THIN_WG / 64; ++q) r = better(r, Best{sv[q], si[q]});
    return r;
}

__device__ __forceinline__ Best part_best(const double *__restrict__ pv, const int *__restrict__ pi,
                                          int npart, double *sv, int *si)
{
    Best b{INFINITY, 0x7fffffff};
    for (int q = threadIdx.x; q < npart; q += THIN_WG) b = better(b, Best{pv[q], pi[q]});
    return wg_best(b, sv, si);
}

__global__ __launch_bounds__(THIN_WG) void k_thin_prep(const double *__restrict__ X,
                                                       const double *__restrict__ G, double a2d, int d,
                                                       int64_t n, int64_t np, double *__restrict__ xs,
                                                       double *__restrict__ diag, double *__restrict__ acc,
                                                       double *__restrict__ pv, int *__restrict__ pi)
{
    __shared__ double sv[THIN_WG / 64];
    __shared__ int si[THIN_WG / 64];
    const int64_t j = (int64_t)blockIdx.x * THIN_WG + threadIdx.x; // < np
    const bool real = j < n;
    double ss = 0.0;
    for (int c = 0; c < d; ++c) {
        const double x = real ? X[j * d + c] : 0.0;
        const double s = real ? G[j * d + c] : 0.0;
        ss = fma(s, s, ss);
        xs[(int64_t)c * np + j] = x;
        xs[(int64_t)(d + c) * np + j] = s;
    }
    const double dg = real ? ss + a2d : 0.0;
    diag[j] = dg;
    acc[j] = 0.0;
    double obj = 0.5 * dg;
    obj = real && obj == obj ? obj : INFINITY;
    const Best b = wg_best(Best{obj, (int)j}, sv, si);
    if (threadIdx.x == 0) {
        pv[blockIdx.x] = b.v;
        pi[blockIdx.x] = b.i;
    }
}

__global__ __launch_bounds__(THIN_WG) void k_thin_select(const double *__restrict__ pv_in,
                                                         const int *__restrict__ pi_in, int npart,
                                                         double *__restrict__ pv_out,
                                                         int *__restrict__ pi_out)
{
    __shared__ double sv[THIN_WG / 64];
    __shared__ int si[THIN_WG / 64];
    const Best b = part_best(pv_in, pi_in, npart, sv, si);
    if (threadIdx.x == 0) {
        pv_out[0] = b.v;
        pi_out[0] = b.i;
    }
}

template <bool IMQ, int U>
__global__ __launch_bounds__(THIN_WG) void k_thin_pick(const double *__restrict__ X,
                                                       const double *__restrict__ G,
                                                       const double *__restrict__ xs,
                                                       const double *__restrict__ diag,
                                                       double *__restrict__ acc, double a, int d, int64_t n,
                                                       int64_t np, const double *__restrict__ pv_in,
                                                       const int *__restrict__ pi_in, int npart,
                                                       double *__restrict__ pv_out, int *__restrict__ pi_out,
                                                       int64_t *__restrict__ idx, double *__restrict__ S,
                                                       int64_t p)
{
    __shared__ double sv[THIN_WG / 64];
    __shared__ int si[THIN_WG / 64];
    __shared__ __attribute__((aligned(16))) double sel[2 * 64]; // (x_pi[c], s_pi[c]) pairs
    const int tid = threadIdx.x;
    int pi = part_best(pv_in, pi_in, npart, sv, si).i;
    // (the partials hold candidates' indices; whatever they hold, stay inside X)
    pi = pi < 0 ? 0 : (int64_t)pi < n ? pi : (int)(n - 1);
    if (tid < d)
        sel[2 * tid] = X[(int64_t)pi * d + tid];
    else if (tid < 2 * d)
        sel[2 * (tid - d) + 1] = G[(int64_t)pi * d + (tid - d)];
    __syncthreads();

    const int64_t j = (int64_t)blockIdx.x * THIN_WG + tid; // < np
    const double *xj = xs + j, *sj = xs + (int64_t)d * np + j;
    double t = 0.0, ss = 0.0, sr = 0.0;
    // U coordinates a round, all 2U loads issued before the first use; a round
    // past d reads row d - 1 again and adds exact zeros
    for (int c0 = 0; c0 < d; c0 += U) {
        double x[U], s[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int c = min(c0 + q, d - 1);
            x[q] = xj[(int64_t)c * np];
            s[q] = sj[(int64_t)c * np];
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const bool in = c0 + q < d;
            const int c = min(c0 + q, d - 1);
            const double sic = in ? sel[2 * c + 1] : 0.0, sjc = in ? s[q] : 0.0;
            const double r = in ? sel[2 * c] - x[q] : 0.0;
            t = fma(r, r, t);
            ss = fma(sic, sjc, ss);
            sr = fma(sic - sjc, r, sr);
        }
    }
    double u;
    if constexpr (IMQ) {
        const double k = imq::rsqrt_full(fmin(fma(a, t, 1.0), 1e300));
        const double k2 = k * k, k3 = k2 * k;
        u = fma(k, ss, k3 * (a * (sr + (double)d) - 3.0 * a * a * (k2 * t)));
    } else {
        u = exp(-a * t) * (fma(2.0 * a, sr, ss) + (2.0 * a * (double)d - 4.0 * a * a * t));
    }
    const double dg = diag[j], old = acc[j];
    if (j == pi) {
        u = dg;
        idx[p] = pi;
        S[p] = (p > 0 ? S[p - 1] : 0.0) + (2.0 * old + dg);
    }
    const double now = old + u;
    acc[j] = now;
    double obj = 0.5 * dg + now;
    obj = j < n && obj == obj ? obj : INFINITY;
    const Best b = wg_best(Best{obj, (int)j}, sv, si);
    if (tid == 0) {
        pv_out[blockIdx.x] = b.v;
        pi_out[blockIdx.x] = b.i;
    }
}

} // namespace thin

static bool thin_shape_ok(int d, int64_t n, const ThinArgs &w)
{
    return d >= 1 && d <= 64 && n >= 1 && n <= THIN_MAX_N && w.X && w.G && w.xs && w.diag && w.acc &&
           w.pval && w.pidx && w.idx && w.S;
}

hipError_t launch_thin_prep(bool imq, int d, int64_t n, double a, const ThinArgs &w,
                            hipStream_t stream)
{
    if (!thin_shape_ok(d, n, w)) return hipErrorInvalidValue;
    const int64_t np = thin_padded(n);
    const double a2d = (imq ? a : 2.0 * a) * (double)d;
    hipLaunchKernelGGL(thin::k_thin_prep, dim3((unsigned)thin_groups(n)), dim3(THIN_WG), 0, stream, w.X, w.G,
                       a2d, d, n, np, w.xs, w.diag, w.acc, w.pval, w.pidx);
    return hipGetLastError();
}

hipError_t launch_thin_picks(bool imq, int d, int64_t n, double a, int64_t m, bool select,
                             const ThinArgs &w, hipStream_t stream)
{
    if (!thin_shape_ok(d, n, w) || m < 1) return hipErrorInvalidValue;
    const int64_t np = thin_padded(n);
    const int g = (int)thin_groups(n);
    // coordinates per round of loads: 16 from d = 17 on (32 loads of a wave in flight)
    const auto pick = d > 16 ? (imq ? &thin::k_thin_pick<true, 16> : &thin::k_thin_pick<false, 16>)
                             : (imq ? &thin::k_thin_pick<true, 8> : &thin::k_thin_pick<false, 8>);
    for (int64_t p = 0; p < m; ++p) {
        const int in = (int)(p & 1) * g, out = (int)((p + 1) & 1) * g;
        const double *pv = w.pval + in;
        const int *pi = w.pidx + in;
        int npart = g;
        if (select) {
            hipLaunchKernelGGL(thin::k_thin_select, dim3(1), dim3(THIN_WG), 0, stream, pv, pi, g,
                               w.pval + 2 * g, w.pidx + 2 * g);
            pv = w.pval + 2 * g;
            pi = w.pidx + 2 * g;
            npart = 1;
        }
        hipLaunchKernelGGL(pick, dim3((unsigned)g), dim3(THIN_WG), 0, stream, w.X, w.G, w.xs, w.diag, w.acc,
                           a, d, n, np, pv, pi, npart, w.pval + out, w.pidx + out, w.idx, w.S, p);
    }
    return hipGetLastError();
}

} // namespace svgd_amd
