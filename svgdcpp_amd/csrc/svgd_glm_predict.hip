// svgd_glm_predict.hip -- posterior prediction of a generalized linear model
// on held-out records, CDNA4 (gfx950), fp64 (svgd_glm_predict.h has the sums,
// host_glm.cpp's svgd_glm_predict_host the same definition on the host).
//
// k_glm_predict_center   c_m = mu(a_m . theta_bar), one thread per record
// k_glm_predict<KP, LINK, HAS_Y>   the geometry of k_glm_wpass (svgd_glm.hip):
//     8 waves x 16 test records per work-group, the records as the Gram
//     MFMA's B operand in registers (lane (lo, hi): record lo, coordinate
//     4kk + hi); the shard's particles stream through two LDS buffers in
//     tiles of 64 rows as the A operand (the next tile in registers during
//     this tile's arithmetic, one barrier per tile).  Z by KP/4
//     v_mfma_f64_16x16x4_f64 leaves lane (lo, hi) with z of record lo and rows
//     hi + 4r; c_m and y_m are per-lane scalars, and the lane adds into its
//     own two or three registers: no cross-lane operation in the loop.  Rows
//     past the shard are masked by index in the tail tile only (mu(0) - c is
//     not 0: a zero row is not neutral).  A wave whose 16 labels are all 0 or
//     1 takes exp(l) = sigma(+-z) from the one exponential of sigma; a
//     fractional label costs the wave a second one.  Grid: record groups x S
//     ranges of the particle tiles -> part[S][3][ldw], the 4 hi partials
//     added in hi order.
// k_glm_predict_finish   sums[q][m] = sum_s part[s][q][m] (s ascending)
// No floating-point atomics, every sum in a fixed order: two calls on the
// same state give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/svgdcpp_amd/svgd_capi.h"
#include "dispatch.h"
#include "svgd_glm_predict.h"

namespace svgd_amd {
namespace glm {

#include "svgd_glm_dev.h" // the table exponential's pieces, d4, NT, blocks_per_cu

// exp(x) for x <= 0 from the table in LDS (relative error <= 2.6e-14 + |x|
// 2^-53); an underflowing result is exactly 0
__device__ __forceinline__ double exp_neg(double x, const double *__restrict__ tab)
{
    const double u = fmax(x * (EXP_TB * LOG2E), U_MIN);
    const double k = __builtin_rint(u);
    const double f = u - k;
    const int ki = (int)k;
    return __builtin_ldexp(exp2_4096_poly(f) * tab[ki & (EXP_TB - 1)], ki >> 12);
}

template <int KP, int LINK, int HAS_Y> struct PGeom {
    static constexpr int RS = glm_rec_stride(KP);
    static constexpr int TW = GLM_TILE * RS;                   // doubles per LDS tile
    static constexpr int NPRE = (GLM_TILE * KP + NT - 1) / NT; // per-thread prefetch registers
    static constexpr int TAB = LINK == SVGD_GLM_LOGISTIC || HAS_Y ? EXP_TB : 0;
    static constexpr int LDS = (2 * TW + TAB) * 8;             // two tile buffers + the table
    static constexpr int NQ = 2 + HAS_Y;                       // sums per record
};

__global__ __launch_bounds__(GLM_FIN_THREADS) void k_glm_predict_center(const double *__restrict__ rec, int RS,
                                                                        int d, int link, int64_t count,
                                                                        const double *__restrict__ mu,
                                                                        double *__restrict__ cvec)
{
    const int64_t m = (int64_t)blockIdx.x * GLM_FIN_THREADS + threadIdx.x;
    if (m >= count) return;
    double z = 0.0;
    for (int k = 0; k < d; ++k) z = fma(rec[m * RS + k], mu[k], z);
    if (link == SVGD_GLM_LOGISTIC) {
        const double e = exp(-fabs(z));
        z = (z >= 0.0 ? 1.0 : e) / (1.0 + e);
    }
    cvec[m] = z;
}

template <int KP, int LINK, int HAS_Y>
__global__ __launch_bounds__(NT) void k_glm_predict(const double *__restrict__ X, int d, int64_t nrows,
                                                    const double *__restrict__ rec,
                                                    const double *__restrict__ cvec, int64_t count, int S,
                                                    double half_s, double *__restrict__ part, int64_t ldw)
{
    typedef PGeom<KP, LINK, HAS_Y> GM;
    constexpr int RS = GM::RS, TW = GM::TW, NPRE = GM::NPRE, NQ = GM::NQ;
    constexpr bool LOGISTIC = LINK == SVGD_GLM_LOGISTIC;
    __shared__ __attribute__((aligned(16))) double smem[GM::LDS / 8];
    const double *tab = smem + 2 * TW;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lo = lane & 15, hi = lane >> 4;
    if constexpr (GM::TAB > 0)
        for (int m = tid; m < EXP_TB; m += NT) smem[2 * TW + m] = EXP2_TAB4096[m];
    // the coordinates d .. RS of a row are never written again: they stay 0
    for (int m = tid; m < 2 * TW; m += NT) smem[m] = 0.0;

    const int64_t grp = blockIdx.x / S;
    const int s = (int)(blockIdx.x - grp * S);
    const int64_t mbase = grp * GLM_ROWS_PER_WG + w * 16;
    // records past the data read its last record (valid memory; never stored)
    const int64_t ml = mbase + lo < count ? mbase + lo : count - 1;
    // B operand of the Gram MFMA: A^T, lane holds a[m = lo][k = 4kk + hi]
    // (the record's slots d .. KP are zero)
    double bR[KP / 4];
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) bR[kk] = rec[ml * RS + 4 * kk + hi];
    // the record's centre and label, and 1 - y (logistic)
    const double cm = cvec[ml];
    const double ym = HAS_Y ? rec[ml * RS + KP] : 0.0;
    const double omy = 1.0 - ym;
    // a fractional label among the wave's 16 records: exp(l) needs its own exponential
    const bool frac = LOGISTIC && HAS_Y && __any(ym != 0.0 && ym != 1.0);

    // this work-group's particle tiles [t0, t1); a tile is 64 d contiguous
    // doubles of X, copied element-wise into rows of stride RS.  Elements
    // past the shard read its last element: finite, and masked below.
    const int64_t T = (nrows + GLM_TILE - 1) / GLM_TILE;
    const int64_t t0 = T * s / S, t1 = T * (s + 1) / S, nt = t1 - t0;
    const int64_t tot = nrows * d;
    const int te = GLM_TILE * d; // elements per tile
    int loff[NPRE];
#pragma unroll
    for (int p = 0; p < NPRE; ++p) {
        const int e = p * NT + tid;
        loff[p] = e < te ? (e / d) * RS + e % d : -1;
    }
    double pre[NPRE];
    auto fetch = [&](int64_t t) {
        const int64_t g0 = (t0 + t) * te;
#pragma unroll
        for (int p = 0; p < NPRE; ++p) {
            const int64_t g = g0 + p * NT + tid;
            pre[p] = X[g < tot ? g : tot - 1];
        }
    };
    auto stash = [&](int64_t t) {
        double *b = smem + (t & 1) * TW;
#pragma unroll
        for (int p = 0; p < NPRE; ++p)
            if (loff[p] >= 0) b[loff[p]] = pre[p];
    };
    __syncthreads(); // the zeros are down before the first tile's elements
    if (nt > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();
    double accA = 0.0, accB = 0.0, accL = 0.0;
    auto tile = [&](int64_t t, auto masked, auto fractional) {
        const double *sT = smem + (t & 1) * TW;
        const int64_t left = nrows - (t0 + t) * GLM_TILE; // shard rows from this tile on
#pragma unroll
        for (int js = 0; js < 4; ++js) {
            d4 dot = {0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < KP / 4; ++kk)
                dot = __builtin_amdgcn_mfma_f64_16x16x4f64(sT[(js * 16 + lo) * RS + 4 * kk + hi], bR[kk],
                                                           dot, 0, 0, 0);
            // dot lane map: row i = js 16 + hi + 4r, record m = lo
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double z = dot[r];
                double dv, pv = 0.0;
                if constexpr (LOGISTIC) {
                    // sigma and exp(l) from e = exp(-|z|): no cancelling 1 - sigma
                    const double az = fabs(z);
                    const double e = exp_neg(-az, tab);
                    const double rq = 1.0 / (1.0 + e);
                    dv = (z >= 0.0 ? 1.0 : e) * rq - cm;
                    if constexpr (HAS_Y) {
                        const double tt = z >= 0.0 ? omy : ym;
                        if constexpr (decltype(fractional)::value)
                            pv = exp_neg(-(az * tt), tab) * rq;
                        else
                            pv = (tt == 0.0 ? 1.0 : e) * rq;
                    }
                } else {
                    dv = z - cm;
                    if constexpr (HAS_Y) {
                        const double rr = ym - z;
                        pv = exp_neg(-((half_s * rr) * rr), tab);
                    }
                }
                if constexpr (decltype(masked)::value) {
                    const bool in = js * 16 + hi + 4 * r < left;
                    dv = in ? dv : 0.0;
                    pv = in ? pv : 0.0;
                }
                accA += dv;
                accB = fma(dv, dv, accB);
                if constexpr (HAS_Y) accL += pv;
            }
            // the tail tile runs once: keep its 16-row groups apart, so the
            // next group's operands are not loaded across this one's arithmetic
            if constexpr (decltype(masked)::value) __builtin_amdgcn_sched_barrier(0);
        }
    };
    // only the shard's last tile can be partial
    const bool tail = nt > 0 && t1 == T && nrows % GLM_TILE != 0;
    const int64_t nfull = tail ? nt - 1 : nt;
    for (int64_t t = 0; t < nfull; ++t) {
        if (t + 1 < nt) fetch(t + 1); // in flight during this tile's arithmetic
        if (frac) tile(t, std::false_type{}, std::true_type{});
        else tile(t, std::false_type{}, std::false_type{});
        if (t + 1 < nt) stash(t + 1); // the buffer tile t - 1 was read from
        __syncthreads();
    }
    if (tail) {
        if (frac) tile(nt - 1, std::true_type{}, std::true_type{});
        else tile(nt - 1, std::true_type{}, std::false_type{});
    }
    // the 4 hi partials of record lo, added in hi order
    const double acc[3] = {accA, accB, accL};
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const double p0 = __shfl(acc[q], lo), p1 = __shfl(acc[q], lo + 16), p2 = __shfl(acc[q], lo + 32),
                     p3 = __shfl(acc[q], lo + 48);
        if (hi == 0 && mbase + lo < count)
            part[((int64_t)s * 3 + q) * ldw + mbase + lo] = ((p0 + p1) + p2) + p3;
    }
}

__global__ __launch_bounds__(GLM_FIN_THREADS) void k_glm_predict_finish(const double *__restrict__ part, int S,
                                                                        int64_t ldw, int64_t count, int nq,
                                                                        double *__restrict__ sums)
{
    const int64_t e = (int64_t)blockIdx.x * GLM_FIN_THREADS + threadIdx.x;
    if (e >= count * nq) return;
    const int q = (int)(e / count);
    const int64_t m = e - q * count;
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += part[((int64_t)s * 3 + q) * ldw + m];
    sums[e] = v;
}

typedef void (*PredictFn)(const double *, int, int64_t, const double *, const double *, int64_t, int, double,
                          double *, int64_t);

PredictFn predict_fn(int kp, int link, int has_y)
{
    // KP = 4, 8, .., 64
    PredictFn f = nullptr;
    if (kp % 4 == 0)
        dispatch_range<1, 16>(kp / 4, [&](auto q) {
            constexpr int K = 4 * decltype(q)::value;
            if (link == SVGD_GLM_LOGISTIC)
                f = has_y ? &k_glm_predict<K, SVGD_GLM_LOGISTIC, 1> : &k_glm_predict<K, SVGD_GLM_LOGISTIC, 0>;
            else
                f = has_y ? &k_glm_predict<K, SVGD_GLM_GAUSSIAN, 1> : &k_glm_predict<K, SVGD_GLM_GAUSSIAN, 0>;
        });
    return f;
}

} // namespace glm

int glm_predict_blocks_per_cu(int d, int link, int has_y)
{
    const glm::PredictFn f = d >= 1 && d <= 64 ? glm::predict_fn(glm_kp(d), link, has_y) : nullptr;
    return glm::blocks_per_cu(reinterpret_cast<const void *>(f));
}

hipError_t launch_glm_predict_center(int d, int link, const double *rec, int64_t count, const double *mu,
                                     double *cvec, hipStream_t stream)
{
    if (d < 1 || d > 64 || count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(glm::k_glm_predict_center, dim3((unsigned)((count + GLM_FIN_THREADS - 1) / GLM_FIN_THREADS)),
                       dim3(GLM_FIN_THREADS), 0, stream, rec, glm_rec_stride(d), d, link, count, mu, cvec);
    return hipGetLastError();
}

hipError_t launch_glm_predict(int d, int link, int has_y, double half_s, const double *X, int64_t nrows,
                              const double *rec, const double *cvec, int64_t count, int S, double *part,
                              double *sums, hipStream_t stream)
{
    if (d < 1 || d > 64 || (link != SVGD_GLM_LOGISTIC && link != SVGD_GLM_GAUSSIAN) || count < 1)
        return hipErrorInvalidValue;
    const int nq = 2 + (has_y ? 1 : 0);
    if (nrows <= 0) return hipMemsetAsync(sums, 0, sizeof(double) * (size_t)count * nq, stream);
    if (S < 1 || S > glm_tiles(nrows)) return hipErrorInvalidValue;
    const glm::PredictFn f = glm::predict_fn(glm_kp(d), link, has_y ? 1 : 0);
    const int64_t groups = glm_wgroups(count), ldw = groups * GLM_ROWS_PER_WG;
    if (!f || groups * S > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f, dim3((unsigned)(groups * S)), dim3(glm::NT), 0, stream, X, d, nrows, rec, cvec, count,
                       S, half_s, part, ldw);
    hipLaunchKernelGGL(glm::k_glm_predict_finish,
                       dim3((unsigned)((count * nq + GLM_FIN_THREADS - 1) / GLM_FIN_THREADS)),
                       dim3(GLM_FIN_THREADS), 0, stream, part, S, ldw, count, nq, sums);
    return hipGetLastError();
}

} // namespace svgd_amd
