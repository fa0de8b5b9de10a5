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

#include "svgd_glm_dev.h" // the table exponential's pieces, d4, NT, blocks_per_cu

template <int KP, int LINK> struct Geom {
    static constexpr int RS = glm_rec_stride(KP);
    static constexpr int NCB = (KP + 15) / 16;
    static constexpr int TW = GLM_TILE * RS;        // doubles per tile
    static constexpr int NP = TW / 2;               // 16-byte pieces per tile
    static constexpr int NPRE = (NP + NT - 1) / NT; // per-thread prefetch registers
    static constexpr int TAB = LINK == SVGD_GLM_LOGISTIC ? EXP_TB : 0;
    static constexpr int LDS = (2 * TW + TAB) * 8;  // two tile buffers + the table
};

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

// ------------------------------------------------- Hessian sum (logistic) --
// -sum_i hess log p(theta_i) = s (M/B) sum_m W_m a_m a_m^T + lambda nrows I,
// W_m = sum_i w(a_m . theta_i): the score's Gram product with the reduction
// turned round -- over the particles, per data record.
//
// k_glm_wpass<KP>   data-stationary: 8 waves x 16 records per work-group, the
//     records as the Gram MFMA's B operand in registers (lane (lo, hi):
//     record lo, coordinate 4kk + hi); the shard's particles stream through
//     two LDS buffers in tiles of 64 rows as the A operand (k_glm_pass's
//     pipeline: the next tile in registers during this tile's arithmetic,
//     one barrier per tile, the record stride of svgd_glm.h).  The MFMA
//     leaves lane (lo, hi) with z of record lo and rows hi + 4r, so the lane
//     adds its w into one register: no cross-lane operation in the loop.
//     Rows past the shard are masked by index in the tail tile only (w(0) =
//     1/4: a zero row is not neutral).  Grid: record groups x S ranges of
//     the particle tiles -> wpart[S][ldw], the 4 hi partials added in hi order.
// k_glm_wfinish     W_m = sum_s wpart[s][m] (s ascending)
// k_glm_wgram       one triangle of sum_m W_m a_m a_m^T over a contiguous
//     range of 64-record blocks (m ascending) -> hpart[block][tri]
// k_glm_hfinish     H = scale sum_b hpart[b] (b ascending) + lambda nrows I,
//     the triangle mirrored: exactly symmetric

// w = sigma (1 - sigma) = e / (1 + e)^2 with e = exp(-|z|): no cancelling
// 1 - sigma in the tail, an underflowing e gives exactly 0
__device__ __forceinline__ double logistic_weight(double z, const double *__restrict__ tab)
{
    const double u = fmax(-fabs(z) * (EXP_TB * LOG2E), U_MIN);
    const double k = __builtin_rint(u);
    const double f = u - k;
    const int ki = (int)k;
    const double e = __builtin_ldexp(exp2_4096_poly(f) * tab[ki & (EXP_TB - 1)], ki >> 12);
    const double q = 1.0 + e;
    return e / (q * q);
}

template <int KP> struct WGeom {
    static constexpr int RS = glm_rec_stride(KP);
    static constexpr int TW = GLM_TILE * RS;                    // doubles per LDS tile
    static constexpr int NPRE = (GLM_TILE * KP + NT - 1) / NT;  // per-thread prefetch registers
    static constexpr int LDS = (2 * TW + EXP_TB) * 8;           // two tile buffers + the table
};

template <int KP>
__global__ __launch_bounds__(NT) void k_glm_wpass(const double *__restrict__ X, int d, int64_t nrows,
                                                  const double *__restrict__ rec, int64_t count, int S,
                                                  double *__restrict__ wpart, int64_t ldw)
{
    typedef WGeom<KP> GM;
    constexpr int RS = GM::RS, TW = GM::TW, NPRE = GM::NPRE;
    __shared__ __attribute__((aligned(16))) double smem[GM::LDS / 8];
    const double *tab = smem + 2 * TW;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lo = lane & 15, hi = lane >> 4;
    for (int m = tid; m < EXP_TB; m += NT) smem[2 * TW + m] = EXP2_TAB4096[m];
    // the coordinates d .. RS of a row are never written again: they stay 0
    for (int m = tid; m < 2 * TW; m += NT) smem[m] = 0.0;

    const int64_t grp = blockIdx.x / S;
    const int s = (int)(blockIdx.x - grp * S);
    const int64_t mbase = grp * GLM_ROWS_PER_WG + w * 16;
    // records past the window read its last record (valid memory; never stored)
    const int64_t ml = mbase + lo < count ? mbase + lo : count - 1;
    // B operand of the Gram MFMA: A^T, lane holds a[m = lo][k = 4kk + hi]
    // (the record's slots d .. KP are zero)
    double bR[KP / 4];
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) bR[kk] = rec[ml * RS + 4 * kk + hi];

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
    double wacc = 0.0;
    auto tile = [&](int64_t t, auto masked) {
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
                const double wv = logistic_weight(dot[r], tab);
                if constexpr (decltype(masked)::value)
                    wacc += js * 16 + hi + 4 * r < left ? wv : 0.0;
                else
                    wacc += wv;
            }
        }
    };
    // only the shard's last tile can be partial
    const bool tail = nt > 0 && t1 == T && nrows % GLM_TILE != 0;
    const int64_t nfull = tail ? nt - 1 : nt;
    for (int64_t t = 0; t < nfull; ++t) {
        if (t + 1 < nt) fetch(t + 1); // in flight during this tile's arithmetic
        tile(t, std::false_type{});
        if (t + 1 < nt) stash(t + 1); // the buffer tile t - 1 was read from
        __syncthreads();
    }
    if (tail) tile(nt - 1, std::true_type{});
    // the 4 hi partials of record lo, added in hi order
    const double p0 = __shfl(wacc, lo), p1 = __shfl(wacc, lo + 16), p2 = __shfl(wacc, lo + 32),
                 p3 = __shfl(wacc, lo + 48);
    if (hi == 0 && mbase + lo < count) wpart[(int64_t)s * ldw + mbase + lo] = ((p0 + p1) + p2) + p3;
}

__global__ __launch_bounds__(GLM_FIN_THREADS) void k_glm_wfinish(const double *__restrict__ wpart, int S,
                                                                 int64_t ldw, int64_t count,
                                                                 double *__restrict__ W)
{
    const int64_t m = (int64_t)blockIdx.x * GLM_FIN_THREADS + threadIdx.x;
    if (m >= count) return;
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += wpart[(int64_t)s * ldw + m];
    W[m] = v;
}

// element e of the lower triangle -> (r, l), l <= r
__device__ __forceinline__ void tri_rl(int e, int *r, int *l)
{
    int rr = (int)((__builtin_sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
    while (rr * (rr + 1) / 2 > e) --rr;
    while ((rr + 1) * (rr + 2) / 2 <= e) ++rr;
    *r = rr;
    *l = e - rr * (rr + 1) / 2;
}

// W == nullptr: every weight is wconst (the Gaussian link's nrows)
__global__ __launch_bounds__(GLM_GRAM_THREADS) void k_glm_wgram(const double *__restrict__ rec, int RS,
                                                                int d, int64_t count,
                                                                const double *__restrict__ W,
                                                                double wconst, int64_t nblk,
                                                                double *__restrict__ hpart)
{
    // a chunk of 64 records [a (d) | weight] at a time
    __shared__ double sA[GLM_GRAM_CHUNK * (64 + 1)];
    const int tid = threadIdx.x, ntri = d * (d + 1) / 2, ld = d + 1;
    // this work-group's blocks of GLM_GRAM_BLOCK records [b0, b1): records [m_lo, m_hi)
    const int64_t b0 = nblk * blockIdx.x / gridDim.x, b1 = nblk * (blockIdx.x + 1) / gridDim.x;
    const int64_t m_lo = b0 * GLM_GRAM_BLOCK;
    const int64_t m_hi = b1 * GLM_GRAM_BLOCK < count ? b1 * GLM_GRAM_BLOCK : count;
    int er[GLM_GRAM_EPT], el[GLM_GRAM_EPT];
    double acc[GLM_GRAM_EPT];
#pragma unroll
    for (int q = 0; q < GLM_GRAM_EPT; ++q) {
        const int e = q * GLM_GRAM_THREADS + tid;
        tri_rl(e < ntri ? e : 0, &er[q], &el[q]);
        acc[q] = 0.0;
    }
    for (int64_t mc = m_lo; mc < m_hi; mc += GLM_GRAM_CHUNK) {
        const int nm = (int)(m_hi - mc < GLM_GRAM_CHUNK ? m_hi - mc : GLM_GRAM_CHUNK);
        __syncthreads(); // the last chunk has been read
        for (int e = tid; e < nm * ld; e += GLM_GRAM_THREADS) {
            const int m = e / ld, k = e - m * ld;
            sA[e] = k < d ? rec[(mc + m) * RS + k] : (W ? W[mc + m] : wconst);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < GLM_GRAM_EPT; ++q) {
            if (q * GLM_GRAM_THREADS + tid >= ntri) continue;
            double h = acc[q];
            for (int m = 0; m < nm; ++m) {
                const double *a = sA + m * ld;
                h = fma(a[d] * a[er[q]], a[el[q]], h);
            }
            acc[q] = h;
        }
    }
#pragma unroll
    for (int q = 0; q < GLM_GRAM_EPT; ++q) {
        const int e = q * GLM_GRAM_THREADS + tid;
        if (e < ntri) hpart[(int64_t)blockIdx.x * ntri + e] = acc[q];
    }
}

__global__ __launch_bounds__(GLM_FIN_THREADS) void k_glm_hfinish(const double *__restrict__ hpart, int nb,
                                                                 int d, double scale, double diag,
                                                                 double *__restrict__ H)
{
    const int ntri = d * (d + 1) / 2;
    const int e = blockIdx.x * GLM_FIN_THREADS + threadIdx.x;
    if (e >= ntri) return;
    int r, l;
    tri_rl(e, &r, &l);
    double v = 0.0;
    for (int b = 0; b < nb; ++b) v += hpart[(int64_t)b * ntri + e];
    const double h = scale * v + (r == l ? diag : 0.0);
    H[r * d + l] = h;
    H[l * d + r] = h;
}

typedef void (*WPassFn)(const double *, int, int64_t, const double *, int64_t, int, double *, int64_t);

WPassFn wpass_fn(int kp)
{
    // KP = 4, 8, .., 64
    WPassFn f = nullptr;
    if (kp % 4 == 0)
        dispatch_range<1, 16>(kp / 4, [&](auto q) { f = &k_glm_wpass<4 * decltype(q)::value>; });
    return f;
}

} // namespace glm

int glm_blocks_per_cu(int d, int link)
{
    const glm::PassFn f = d >= 1 && d <= 64 ? glm::pass_fn(glm_kp(d), link) : nullptr;
    return glm::blocks_per_cu(reinterpret_cast<const void *>(f));
}

int glm_wpass_blocks_per_cu(int d)
{
    const glm::WPassFn f = d >= 1 && d <= 64 ? glm::wpass_fn(glm_kp(d)) : nullptr;
    return glm::blocks_per_cu(reinterpret_cast<const void *>(f));
}

hipError_t launch_glm_weights(int d, const double *X, int64_t nrows, const double *rec, int64_t m0,
                              int64_t count, int S, double *wpart, double *W, hipStream_t stream)
{
    if (nrows <= 0) return hipSuccess;
    if (d < 1 || d > 64 || m0 < 0 || count < 1 || S < 1 || S > glm_tiles(nrows)) return hipErrorInvalidValue;
    const glm::WPassFn f = glm::wpass_fn(glm_kp(d));
    const int64_t groups = glm_wgroups(count), ldw = groups * GLM_ROWS_PER_WG;
    if (!f || groups * S > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f, dim3((unsigned)(groups * S)), dim3(glm::NT), 0, stream, X, d, nrows,
                       rec + m0 * glm_rec_stride(d), count, S, wpart, ldw);
    hipLaunchKernelGGL(glm::k_glm_wfinish, dim3((unsigned)((count + GLM_FIN_THREADS - 1) / GLM_FIN_THREADS)),
                       dim3(GLM_FIN_THREADS), 0, stream, wpart, S, ldw, count, W);
    return hipGetLastError();
}

hipError_t launch_glm_wgram(int d, const double *rec, int64_t m0, int64_t count, const double *W,
                            double wconst, double scale, double diag, double *hpart, double *H,
                            hipStream_t stream)
{
    if (d < 1 || d > 64 || m0 < 0 || count < 1) return hipErrorInvalidValue;
    const int64_t nblk = glm_gram_blocks(count);
    const int nb = glm_gram_grid(count), ntri = d * (d + 1) / 2;
    hipLaunchKernelGGL(glm::k_glm_wgram, dim3(nb), dim3(GLM_GRAM_THREADS), 0, stream,
                       rec + m0 * glm_rec_stride(d), glm_rec_stride(d), d, count, W, wconst, nblk, hpart);
    hipLaunchKernelGGL(glm::k_glm_hfinish, dim3((ntri + GLM_FIN_THREADS - 1) / GLM_FIN_THREADS),
                       dim3(GLM_FIN_THREADS), 0, stream, hpart, nb, d, scale, diag, H);
    return hipGetLastError();
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
