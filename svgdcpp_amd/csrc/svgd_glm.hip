// svgd_glm.hip -- grad log p of a Bayesian generalized linear model at every
// particle, CDNA4 (gfx950), fp64 (host_glm.cpp has the model):
//   z_im = a_m . theta_i
//   G_i  = s (M/B) sum_{m in window} r(y_m, z_im) a_m - lambda theta_i
//   r    = y - sigma(z) (logistic),  r = y - z (Gaussian link)
// Score = Gram product Theta A^T, an element-wise function, then a second
// product with A: the dataflow of the tile phi (k_phi<double, ...>) with the
// data rows on the column side and a sigmoid where the exp is.
//
// k_glm_pass<KP, LINK>   8 waves x 16 particle rows per work-group, theta as
//     the Gram MFMA's B operand in registers; the window's records
//     [a (KP) | y | 0 ...] stream through two LDS buffers in tiles of 64 (the
//     next tile is in flight in registers during this tile's arithmetic, one
//     barrier per tile).  Per 16(m) x 16(i) block: Z by KP/4
//     v_mfma_f64_16x16x4_f64 (A = records from LDS), r on the VALU (lane l:
//     i = l & 15, m = (l >> 4) + 4 reg -- already the A-operand map), then
//     acc += R A by ceil(d/16) MFMA blocks whose B operand is the same LDS
//     record.  A record past the window is stored to LDS as zeros (a = 0,
//     y = 0): r is finite for it and r * 0 = 0, so the loop masks nothing.
//     The grid is row groups x S ranges of the window's tiles -> part[S][rows][d].
// k_glm_finish           G = scale sum_s part[s] (s ascending) - lambda theta
// No floating-point atomics, every sum in a fixed order: two calls on the
// same state give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svgdcpp_amd/svgd_capi.h"
#include "dispatch.h"
#include "svgd_glm.h"

namespace svgd_amd {
namespace glm {

#include "svgd_exp_table.h" // EXP2_TAB4096 (this translation unit's copy)

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr double LOG2E = 0x1.71547652b82fep+0;
constexpr int EXP_TB = 4096; // exp table entries
constexpr int NT = 64 * GLM_WAVES;
// exponents below 2^-1100 give exactly 0 (the smallest subnormal is 2^-1074)
constexpr double U_MIN = -1100.0 * EXP_TB;

template <int KP, int LINK> struct Geom {
    static constexpr int RS = glm_rec_stride(KP);
    static constexpr int NCB = (KP + 15) / 16;
    static constexpr int TW = GLM_TILE * RS;        // doubles per tile
    static constexpr int NP = TW / 2;               // 16-byte pieces per tile
    static constexpr int NPRE = (NP + NT - 1) / NT; // per-thread prefetch registers
    static constexpr int TAB = LINK == SVGD_GLM_LOGISTIC ? EXP_TB : 0;
    static constexpr int LDS = (2 * TW + TAB) * 8;  // two tile buffers + the table
};

// 2^(f/4096), |f| <= 1/2: 1 + c1 f + c2 f^2 with the coefficients levelled
// over the interval (relative error <= 2.6e-14, tools/make_exp_table.py)
__device__ __forceinline__ double exp2_4096_poly(double f)
{
    return fma(fma(0x1.ebfbdff82c58fp-27, f, 0x1.62e42ff4f7b0ap-13), f, 1.0);
}

// sigma(z) from e = exp(-|z|) in both tails: 1 / (1 + e) or e / (1 + e); an
// underflowing e is exactly 0
__device__ __forceinline__ double sigmoid(double z, const double *__restrict__ tab)
{
    const double u = fmax(-fabs(z) * (EXP_TB * LOG2E), U_MIN);
    const double k = __builtin_rint(u);
    const double f = u - k;
    const int ki = (int)k;
    const double e = __builtin_ldexp(exp2_4096_poly(f) * tab[ki & (EXP_TB - 1)], ki >> 12);
    return (z >= 0.0 ? 1.0 : e) / (1.0 + e);
}

template <int KP, int LINK>
__global__ __launch_bounds__(NT) void k_glm_pass(const double *__restrict__ X, int d, int64_t nrows,
                                                 const double *__restrict__ rec, int64_t count, int S,
                                                 double *__restrict__ part, int64_t ldp)
{
    typedef Geom<KP, LINK> GM;
    constexpr int RS = GM::RS, NCB = GM::NCB, TW = GM::TW, NP = GM::NP, NPRE = GM::NPRE;
    __shared__ __attribute__((aligned(16))) double smem[GM::LDS / 8];
    const double *tab = smem + 2 * TW;
    if constexpr (LINK == SVGD_GLM_LOGISTIC)
        for (int m = threadIdx.x; m < EXP_TB; m += NT) smem[2 * TW + m] = EXP2_TAB4096[m];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lo = lane & 15, hi = lane >> 4;
    const int64_t grp = blockIdx.x / S;
    const int s = (int)(blockIdx.x - grp * S);
    const int64_t ibase = grp * GLM_ROWS_PER_WG + w * 16;
    // rows past the shard read its last row (valid memory; never stored)
    const int64_t il = ibase + lo < nrows ? ibase + lo : nrows - 1;
    // B operand of the Gram MFMA: Theta^T, lane holds theta[i = lo][k = 4kk + hi]
    double bI[KP / 4];
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) bI[kk] = 4 * kk + hi < d ? X[il * d + 4 * kk + hi] : 0.0;
    // B operand of the contraction: column cb 16 + lo of the record (columns
    // past the record read its last slot: those accumulators are not stored)
    int cidx[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) cidx[cb] = cb * 16 + lo < RS ? cb * 16 + lo : RS - 1;

    d4 acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[cb] = d4{0, 0, 0, 0};

    // this work-group's tiles [t0, t1) of the window; rec holds a tile of zero
    // records past the data, so whole tiles are copied
    const int64_t T = (count + GLM_TILE - 1) / GLM_TILE;
    const int64_t t0 = T * s / S, t1 = T * (s + 1) / S, nt = t1 - t0;
    const uint4 *gt = reinterpret_cast<const uint4 *>(rec + t0 * TW);
    uint4 pre[NPRE];
    auto fetch = [&](int64_t t) {
#pragma unroll
        for (int p = 0; p < NPRE; ++p) {
            const int e = p * NT + tid;
            if (NP % NT == 0 || e < NP) pre[p] = gt[t * NP + e];
        }
    };
    auto stash = [&](int64_t t) {
        uint4 *b = reinterpret_cast<uint4 *>(smem + (t & 1) * TW);
        const int64_t left = count - (t0 + t) * GLM_TILE; // window records from this tile on
#pragma unroll
        for (int p = 0; p < NPRE; ++p) {
            const int e = p * NT + tid;
            if (NP % NT == 0 || e < NP) b[e] = e / (RS / 2) < left ? pre[p] : make_uint4(0, 0, 0, 0);
        }
    };
    if (nt > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();
    for (int64_t t = 0; t < nt; ++t) {
        if (t + 1 < nt) fetch(t + 1); // in flight during this tile's arithmetic
        const double *sR = smem + (t & 1) * TW;
#pragma unroll
        for (int js = 0; js < 4; ++js) {
            d4 dot = {0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < KP / 4; ++kk)
                dot = __builtin_amdgcn_mfma_f64_16x16x4f64(sR[(js * 16 + lo) * RS + 4 * kk + hi], bI[kk],
                                                           dot, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double *q = sR + (js * 16 + hi + 4 * r) * RS;
                const double z = dot[r], yv = q[KP];
                const double rr = LINK == SVGD_GLM_LOGISTIC ? yv - sigmoid(z, tab) : yv - z;
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb)
                    acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(rr, q[cidx[cb]], acc[cb], 0, 0, 0);
            }
        }
        if (t + 1 < nt) stash(t + 1); // the buffer tile t - 1 was read from
        __syncthreads();
    }
    // acc lane map: row i = hi + 4q, column c = lo + 16 cb
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t li = ibase + hi + 4 * q;
            const int c = cb * 16 + lo;
            if (li < nrows && c < d) part[((int64_t)s * ldp + li) * d + c] = acc[cb][q];
        }
}

__global__ __launch_bounds__(GLM_FIN_THREADS) void k_glm_finish(const double *__restrict__ X,
                                                                int64_t tot, const double *__restrict__ part,
                                                                int S, int64_t lds, double scale,
                                                                double lambda, double *__restrict__ G)
{
    const int64_t e = (int64_t)blockIdx.x * GLM_FIN_THREADS + threadIdx.x;
    if (e >= tot) return;
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += part[(int64_t)s * lds + e];
    G[e] = scale * v - lambda * X[e];
}

typedef void (*PassFn)(const double *, int, int64_t, const double *, int64_t, int, double *, int64_t);

PassFn pass_fn(int kp, int link)
{
    // KP = 4, 8, .., 64
    PassFn f = nullptr;
    if (kp % 4 == 0)
        dispatch_range<1, 16>(kp / 4, [&](auto q) {
            constexpr int K = 4 * decltype(q)::value;
            f = link == SVGD_GLM_LOGISTIC ? &k_glm_pass<K, SVGD_GLM_LOGISTIC> : &k_glm_pass<K, SVGD_GLM_GAUSSIAN>;
        });
    return f;
}

} // namespace glm

int glm_blocks_per_cu(int d, int link)
{
    const glm::PassFn f = d >= 1 && d <= 64 ? glm::pass_fn(glm_kp(d), link) : nullptr;
    hipFuncAttributes fa;
    if (!f || hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(f)) != hipSuccess) return 1;
    // 8 waves per work-group on 4 SIMDs: two waves per SIMD each (512 VGPRs
    // per lane, allocated in eights), capped by the 160 KiB of LDS
    const int regs = (fa.numRegs > 0 ? fa.numRegs + 7 : 8) / 8 * 8;
    const int by_regs = 512 / regs / 2 < 4 ? 512 / regs / 2 : 4;
    const int by_lds = fa.sharedSizeBytes > 0 ? (int)(163840 / fa.sharedSizeBytes) : 4;
    const int b = by_regs < by_lds ? by_regs : by_lds;
    return b > 1 ? b : 1;
}

hipError_t launch_glm_pass(int d, int link, const double *X, int64_t nrows, const double *rec,
                           int64_t m0, int64_t count, int S, double *part, int64_t ldp,
                           hipStream_t stream)
{
    if (nrows <= 0) return hipSuccess;
    if (d < 1 || d > 64 || (link != SVGD_GLM_LOGISTIC && link != SVGD_GLM_GAUSSIAN) || m0 < 0 ||
        count < 1 || S < 1 || S > glm_tiles(count) || ldp < nrows)
        return hipErrorInvalidValue;
    const glm::PassFn f = glm::pass_fn(glm_kp(d), link);
    const int64_t grid = (nrows + GLM_ROWS_PER_WG - 1) / GLM_ROWS_PER_WG * S;
    if (!f || grid > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f, dim3((unsigned)grid), dim3(glm::NT), 0, stream, X, d, nrows,
                       rec + m0 * glm_rec_stride(d), count, S, part, ldp);
    return hipGetLastError();
}

hipError_t launch_glm_finish(int d, const double *X, int64_t nrows, const double *part, int S,
                             int64_t ldp, double scale, double lambda, double *G, hipStream_t stream)
{
    if (nrows <= 0) return hipSuccess;
    const int64_t tot = nrows * d;
    hipLaunchKernelGGL(glm::k_glm_finish, dim3((unsigned)((tot + GLM_FIN_THREADS - 1) / GLM_FIN_THREADS)),
                       dim3(GLM_FIN_THREADS), 0, stream, X, tot, part, S, ldp * d, scale, lambda, G);
    return hipGetLastError();
}

} // namespace svgd_amd
