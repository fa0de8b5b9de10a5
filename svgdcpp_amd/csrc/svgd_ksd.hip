// svgd_ksd.hip -- kernelized Stein discrepancy (KSD) of the particle set with
// the isotropic RBF kernel k(x, y) = exp(-a |x - y|^2), CDNA4 (gfx950), fp64.
//
// For scores s_i = grad log p(x_i) and r = x_i - x_j the Stein kernel is
//   u_ij = k_ij [ s_i.s_j + 2a (s_i - s_j).r + 2ad - 4a^2 |r|^2 ]
// and KSD^2_V = (1/N^2) sum_ij u_ij,  KSD^2_U = (1/(N(N-1))) sum_{i != j} u_ij.
// On centred coordinates xc (svgd_ksd.h) it takes two Gram products and one
// exp per ordered pair:
//   u_ij = exp(-a max(n_i + n_j - 2 xc_i.xc_j, 0)) (v_i.v_j + 4a^2 xc_i.xc_j + c_i + c_j + 2ad)
// The diagonal u_ii = |s_i|^2 + 2ad is taken from its closed form (the Gram
// form would lose it to cancellation when a^2 |xc|^2 is large).
//
// Passes (one stream, no floating-point atomics, every sum in a fixed order,
// so two calls on the same state give the same bits):
//   k_ksd_colsum / k_ksd_mean   centre mu = mean of X
//   k_ksd_prep                  per-particle operands
//   k_ksd_rows<D> (d <= 16)     this rank's rows x all columns on the VALU:
//       the row operands of R rows per lane in registers, the column records
//       streamed through LDS in chunks of 64 (every lane reads the same
//       record: a broadcast), the k_phi_rows pattern; the grid splits the
//       columns S ways -> part[S][rows]
//   k_ksd_tile (d 17..64)       the same sums from 64 x 64 tiles, 4 x 4 pairs
//       per lane, operands k-major through LDS in slices of 16 coordinates
//   k_ksd_rowfin / k_ksd_final  row_i = (1/N) sum_s part[s][i]; the sums of
//       row_i and u_ii over this rank's rows
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dispatch.h"
#include "svgd_ksd.h"

namespace svgd_amd {
namespace ksd {

#include "svgd_exp_table.h" // EXP2_TAB4096 (this translation unit's copy)

constexpr double LOG2E = 0x1.71547652b82fep+0;
constexpr int CH = 64;       // columns per LDS chunk of k_ksd_rows
constexpr int EXP_TB = 4096; // exp table entries
// exponents below 2^-1100 give exactly 0 (the smallest subnormal is 2^-1074)
constexpr double U_MIN = -1100.0 * EXP_TB;

template <int D> struct Geom {
    static constexpr int R = ksd_rows_per_lane(D);
    static constexpr int RS = ksd_rec_stride(D);
    static constexpr int CHW = CH * RS;                // doubles per chunk
    static constexpr int NPRE = (CHW + 255) / 256;     // per-thread prefetch registers
    static constexpr int LDS = (2 * CHW + EXP_TB) * 8; // two chunk buffers + the table
};

// 2^(f/4096), |f| <= 1/2: 1 + c1 f + c2 f^2 with the coefficients levelled
// over the interval (relative error <= 2.6e-14, tools/make_exp_table.py)
__device__ __forceinline__ double exp2_4096_poly(double f)
{
    return fma(fma(0x1.ebfbdff82c58fp-27, f, 0x1.62e42ff4f7b0ap-13), f, 1.0);
}

// acc_r += u_ij for the lane's R rows against the column record q (LDS);
// CHK: column j may be one of the rows (the diagonal term from dg)
template <int D, int R, bool CHK>
__device__ __forceinline__ void rows_pair(const double *__restrict__ q, const double (&xs)[R][D],
                                          const double (&vs)[R][D], const double (&ei)[R],
                                          const double (&ci)[R], const double (&dg)[R],
                                          const int64_t (&gi)[R], int64_t j, double beta,
                                          double (&acc)[R], const double *__restrict__ tab)
{
    double g[R], w[R], u[R], f[R], T[R];
    int ki[R];
    const double qe = q[2 * D], qc = q[2 * D + 1];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        g[r] = xs[r][0] * q[0];
        w[r] = fma(vs[r][0], q[D], qc);
    }
#pragma unroll
    for (int k = 1; k < D; ++k)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            g[r] = fma(xs[r][k], q[k], g[r]);
            w[r] = fma(vs[r][k], q[D + k], w[r]);
        }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        // u = -4096 a log2e |xc_i - xc_j|^2 (<= 0 up to rounding)
        u[r] = fmax(fmin(g[r] + (ei[r] + qe), 0.0), U_MIN);
        const double k = __builtin_rint(u[r]);
        f[r] = u[r] - k;
        ki[r] = (int)k;
        T[r] = tab[ki[r] & (EXP_TB - 1)];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double K = __builtin_ldexp(exp2_4096_poly(f[r]) * T[r], ki[r] >> 12);
        double t = K * (fma(beta, g[r], w[r]) + ci[r]);
        if constexpr (CHK) t = gi[r] == j ? dg[r] : t;
        acc[r] += t;
    }
}

template <int D>
__global__ __launch_bounds__(256) void k_ksd_rows(const double *__restrict__ rec,
                                                  const double *__restrict__ cvec,
                                                  const double *__restrict__ diag, double a,
                                                  int64_t row0, int64_t nrows, int64_t n, int S,
                                                  double *__restrict__ part, int64_t ldp)
{
    typedef Geom<D> GM;
    constexpr int R = GM::R, RS = GM::RS, CHW = GM::CHW, NPRE = GM::NPRE;
    __shared__ __attribute__((aligned(16))) double smem[GM::LDS / 8];
    double *tab = smem + 2 * CHW;
    for (int m = threadIdx.x; m < EXP_TB; m += 256) tab[m] = EXP2_TAB4096[m];

    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t iblk = blockIdx.x / S;
    const int s = (int)(blockIdx.x - iblk * S);
    const int64_t rbase = iblk * (256 * R) + wv * (64 * R); // local row of this wave's lane 0
    // row coordinates pre-scaled: g = 8192 a log2e xc_i.xc_j, and
    // 4a^2 xc_i.xc_j = beta g
    const double alpha = 8192.0 * LOG2E * a, beta = a / (2048.0 * LOG2E);

    double xs[R][D], vs[R][D], ei[R], ci[R], dg[R], acc[R];
    int64_t gi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int64_t li = rbase + 64 * r + lane;
        if (li >= nrows) li = nrows - 1; // padding lanes recompute a valid row
        gi[r] = row0 + li;
        const double *ri = rec + gi[r] * RS;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            xs[r][k] = alpha * ri[k];
            vs[r][k] = ri[D + k];
        }
        ei[r] = ri[2 * D];
        ci[r] = cvec[gi[r]];
        dg[r] = diag[gi[r]];
        acc[r] = 0.0;
    }

    // this work-group's columns [j0, j1) in chunks of CH records; rec holds
    // >= CH padded records past n, so whole chunks are copied
    const int64_t j0 = n * s / S, j1 = n * (s + 1) / S;
    const int64_t nch = (j1 - j0 + CH - 1) / CH;
    const double *gcol = rec + j0 * RS;
    double pre[NPRE];
    auto fetch = [&](int64_t c) {
#pragma unroll
        for (int p = 0; p < NPRE; ++p) {
            const int e = p * 256 + threadIdx.x;
            pre[p] = e < CHW ? gcol[c * CHW + e] : 0.0;
        }
    };
    auto stash = [&](int64_t c) {
        double *b = smem + (c & 1) * CHW;
#pragma unroll
        for (int p = 0; p < NPRE; ++p) {
            const int e = p * 256 + threadIdx.x;
            if (e < CHW) b[e] = pre[p];
        }
    };
    if (nch > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();
    // the wave's rows as global indices: only a chunk that meets them needs
    // the diagonal test
    const int64_t w0 = row0 + rbase, w1 = w0 + 64 * R;
    for (int64_t c = 0; c < nch; ++c) {
        if (c + 1 < nch) fetch(c + 1); // in flight during this chunk's arithmetic
        const double *cb = smem + (c & 1) * CHW;
        const int64_t jb = j0 + c * CH;
        const int cnt = (int)min<int64_t>(CH, j1 - jb);
        if (jb < w1 && jb + cnt > w0) {
            for (int jj = 0; jj < cnt; ++jj)
                rows_pair<D, R, true>(cb + jj * RS, xs, vs, ei, ci, dg, gi, jb + jj, beta, acc, tab);
        } else {
            for (int jj = 0; jj < cnt; ++jj)
                rows_pair<D, R, false>(cb + jj * RS, xs, vs, ei, ci, dg, gi, jb + jj, beta, acc, tab);
        }
        if (c + 1 < nch) stash(c + 1); // the buffer chunk c - 1 was read from
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t li = rbase + 64 * r + lane;
        if (li < nrows) part[(int64_t)s * ldp + li] = acc[r];
    }
}

// d = 17..64: 64 rows x 64 columns per tile, lane (ty, tx) holds rows
// 4 ty .. 4 ty + 3 and columns 4 tx .. 4 tx + 3 of both Gram products
constexpr int KS = 16; // coordinates per LDS slice
__global__ __launch_bounds__(256) void k_ksd_tile(const double *__restrict__ xt,
                                                  const double *__restrict__ vt,
                                                  const double *__restrict__ nrm,
                                                  const double *__restrict__ cvec,
                                                  const double *__restrict__ diag, double a, int d,
                                                  int KP, int64_t row0, int64_t nrows, int64_t n,
                                                  int64_t np, int S, double *__restrict__ part,
                                                  int64_t ldp)
{
    constexpr int TL = KSD_TILE;
    __shared__ __attribute__((aligned(16))) double sXr[KS][TL], sVr[KS][TL], sXc[KS][TL], sVc[KS][TL];
    __shared__ double red[TL][17];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t iblk = blockIdx.x / S;
    const int s = (int)(blockIdx.x - iblk * S);
    const int64_t T = (n + TL - 1) / TL; // column tiles (the last one may hold padding: K = 0)
    const int64_t t0 = T * s / S, t1 = T * (s + 1) / S;
    const double c2ad = 2.0 * a * d, a4 = 4.0 * a * a;

    int64_t gi[4];
    double nr[4], cr[4], dg[4], racc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t li = min<int64_t>(iblk * TL + ty * 4 + r, nrows - 1);
        gi[r] = row0 + li;
        nr[r] = nrm[gi[r]];
        cr[r] = cvec[gi[r]] + c2ad;
        dg[r] = diag[gi[r]];
        racc[r] = 0.0;
    }
    // the slice element this thread copies: coordinate lk of particle lj (x 4 slices of 4)
    const int lj = tid & 63, lk = tid >> 6;
    const int64_t grow = row0 + min<int64_t>(iblk * TL + lj, nrows - 1);

    for (int64_t t = t0; t < t1; ++t) {
        double xx[4][4], vv[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) xx[r][c] = vv[r][c] = 0.0;
        const int64_t gcol = t * TL + lj; // < np: np >= T TL + TL
        for (int k0 = 0; k0 < KP; k0 += KS) {
            __syncthreads(); // the previous slice has been read
#pragma unroll
            for (int q = 0; q < KS / 4; ++q) {
                const int k = lk + 4 * q;
                const int64_t o = (int64_t)(k0 + k) * np;
                sXr[k][lj] = xt[o + grow];
                sVr[k][lj] = vt[o + grow];
                sXc[k][lj] = xt[o + gcol];
                sVc[k][lj] = vt[o + gcol];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                double xr[4], vr[4], xc[4], vc[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xr[e] = sXr[k][ty * 4 + e];
                    vr[e] = sVr[k][ty * 4 + e];
                    xc[e] = sXc[k][tx * 4 + e];
                    vc[e] = sVc[k][tx * 4 + e];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        xx[r][c] = fma(xr[r], xc[c], xx[r][c]);
                        vv[r][c] = fma(vr[r], vc[c], vv[r][c]);
                    }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t j = t * TL + tx * 4 + c;
            const double nj = nrm[j], cj = cvec[j]; // padding: +inf, 0
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double K = exp(-a * fmax(nr[r] + nj - 2.0 * xx[r][c], 0.0));
                const double u = K * (fma(a4, xx[r][c], vv[r][c]) + cr[r] + cj);
                racc[r] += gi[r] == j ? dg[r] : u;
            }
        }
    }
    // the 16 column groups' sums of each row, added in tx order
#pragma unroll
    for (int r = 0; r < 4; ++r) red[ty * 4 + r][tx] = racc[r];
    __syncthreads();
    if (tid < TL) {
        double v = red[tid][0];
        for (int q = 1; q < 16; ++q) v += red[tid][q];
        const int64_t li = iblk * TL + tid;
        if (li < nrows) part[(int64_t)s * ldp + li] = v;
    }
}

// column sums of rows [b RPB, (b + 1) RPB) -> partial[b][d]: thread (g, c)
// adds column c of every G-th row, the groups are added in g order
__global__ __launch_bounds__(256) void k_ksd_colsum(const double *__restrict__ X, int64_t n, int d,
                                                    int64_t rpb, double *__restrict__ partial)
{
    __shared__ double sh[256];
    const int G = 256 / d, tid = threadIdx.x;
    const int g = tid / d, c = tid - g * d;
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min<int64_t>(n, r0 + rpb);
    double v = 0.0;
    if (g < G)
        for (int64_t r = r0 + g; r < r1; r += G) v += X[r * d + c];
    sh[tid] = v;
    __syncthreads();
    if (tid < d) {
        double t = sh[tid];
        for (int q = 1; q < G; ++q) t += sh[q * d + tid];
        partial[(int64_t)blockIdx.x * d + tid] = t;
    }
}

__global__ __launch_bounds__(64) void k_ksd_mean(const double *__restrict__ partial, int nblk,
                                                 int d, int64_t n, double *__restrict__ mu)
{
    const int k = threadIdx.x;
    if (k >= d) return;
    double t = 0.0;
    for (int b = 0; b < nblk; ++b) t += partial[(int64_t)b * d + k];
    mu[k] = t / (double)n;
}

__global__ __launch_bounds__(256) void k_ksd_prep(const double *__restrict__ X,
                                                  const double *__restrict__ G,
                                                  const double *__restrict__ mu, double a, int64_t n,
                                                  int64_t np, int d, int KP, int RS,
                                                  double *__restrict__ rec, double *__restrict__ xt,
                                                  double *__restrict__ vt, double *__restrict__ nrm,
                                                  double *__restrict__ cvec, double *__restrict__ diag)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    const bool real = j < n;
    double nj = 0.0, sx = 0.0, ss = 0.0;
    for (int k = 0; k < d; ++k) {
        const double x = real ? X[j * d + k] - mu[k] : 0.0;
        const double sc = real ? G[j * d + k] : 0.0;
        const double v = sc - 2.0 * a * x;
        nj = fma(x, x, nj);
        sx = fma(sc, x, sx);
        ss = fma(sc, sc, ss);
        if (rec) {
            rec[j * RS + k] = x;
            rec[j * RS + d + k] = v;
        } else {
            xt[(int64_t)k * np + j] = x;
            vt[(int64_t)k * np + j] = v;
        }
    }
    const double c = 2.0 * a * sx - 4.0 * a * a * nj, c2ad = 2.0 * a * d;
    if (rec) {
        rec[j * RS + 2 * d] = real ? -4096.0 * LOG2E * a * nj : -INFINITY;
        rec[j * RS + 2 * d + 1] = real ? c + c2ad : 0.0;
    } else {
        for (int k = d; k < KP; ++k) xt[(int64_t)k * np + j] = vt[(int64_t)k * np + j] = 0.0;
    }
    nrm[j] = real ? nj : INFINITY;
    cvec[j] = real ? c : 0.0;
    diag[j] = real ? ss + c2ad : 0.0;
}

// fixed-order sum of the block's 256 values (a, b) -> thread 0
__device__ __forceinline__ void block_sum2(double *sa, double *sb, double &a, double &b)
{
    const int tid = threadIdx.x;
    sa[tid] = a;
    sb[tid] = b;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            sa[tid] += sa[tid + h];
            sb[tid] += sb[tid + h];
        }
        __syncthreads();
    }
    a = sa[0];
    b = sb[0];
}

__global__ __launch_bounds__(KSD_FIN_THREADS) void k_ksd_rowfin(const double *__restrict__ part, int S,
                                                                int64_t ldp, int64_t nrows, double inv_n,
                                                                const double *__restrict__ diag_rows,
                                                                double *__restrict__ rows,
                                                                double *__restrict__ bpart)
{
    __shared__ double sa[KSD_FIN_THREADS], sb[KSD_FIN_THREADS];
    const int64_t li = (int64_t)blockIdx.x * KSD_FIN_THREADS + threadIdx.x;
    double v = 0.0, dv = 0.0;
    if (li < nrows) {
        for (int s = 0; s < S; ++s) v += part[(int64_t)s * ldp + li];
        v *= inv_n;
        rows[li] = v;
        dv = diag_rows[li];
    }
    block_sum2(sa, sb, v, dv);
    if (threadIdx.x == 0) {
        bpart[2 * (int64_t)blockIdx.x] = v;
        bpart[2 * (int64_t)blockIdx.x + 1] = dv;
    }
}

__global__ __launch_bounds__(KSD_FIN_THREADS) void k_ksd_final(const double *__restrict__ bpart,
                                                               int64_t nblk, double *__restrict__ out)
{
    __shared__ double sa[KSD_FIN_THREADS], sb[KSD_FIN_THREADS];
    double v = 0.0, dv = 0.0;
    for (int64_t b = threadIdx.x; b < nblk; b += KSD_FIN_THREADS) {
        v += bpart[2 * b];
        dv += bpart[2 * b + 1];
    }
    block_sum2(sa, sb, v, dv);
    if (threadIdx.x == 0) {
        out[0] = v;
        out[1] = dv;
    }
}

} // namespace ksd

int ksd_blocks_per_cu(int d)
{
    const void *f = reinterpret_cast<const void *>(&ksd::k_ksd_tile);
    dispatch_range<1, 16>(d, [&](auto dc) {
        f = reinterpret_cast<const void *>(&ksd::k_ksd_rows<decltype(dc)::value>);
    });
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, f) != hipSuccess) return 2;
    // 4 waves per work-group on 4 SIMDs: work-groups per CU = waves per SIMD
    // (512 VGPRs per lane, allocated in eights), capped by the 160 KiB of LDS
    const int regs = (fa.numRegs > 0 ? fa.numRegs + 7 : 8) / 8 * 8;
    const int by_regs = 512 / regs < 8 ? 512 / regs : 8;
    const int by_lds = fa.sharedSizeBytes > 0 ? (int)(163840 / fa.sharedSizeBytes) : 8;
    const int b = by_regs < by_lds ? by_regs : by_lds;
    return b > 1 ? b : 1;
}

hipError_t launch_ksd_mean(const double *X, int64_t n, int d, double *partial, double *mu,
                           hipStream_t stream)
{
    if (n < 1 || d < 1 || d > 64) return hipErrorInvalidValue;
    const int64_t rpb = (n + KSD_MEAN_BLOCKS - 1) / KSD_MEAN_BLOCKS;
    const int nblk = (int)((n + rpb - 1) / rpb);
    hipLaunchKernelGGL(ksd::k_ksd_colsum, dim3(nblk), dim3(256), 0, stream, X, n, d, rpb, partial);
    hipLaunchKernelGGL(ksd::k_ksd_mean, dim3(1), dim3(64), 0, stream, partial, nblk, d, n, mu);
    return hipGetLastError();
}

hipError_t launch_ksd_prep(const double *X, const double *G, const double *mu, double a, int64_t n,
                           int64_t np, int d, double *rec, double *xt, double *vt, double *nrm,
                           double *cvec, double *diag, hipStream_t stream)
{
    if (n < 1 || np < ksd_padded(n) || d < 1 || d > 64) return hipErrorInvalidValue;
    const bool rows = d <= 16;
    if (rows ? !rec : (!xt || !vt)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ksd::k_ksd_prep, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream, X, G, mu,
                       a, n, np, d, ksd_kp(d), ksd_rec_stride(d), rows ? rec : nullptr, xt, vt, nrm,
                       cvec, diag);
    return hipGetLastError();
}

hipError_t launch_ksd_pairs(int d, double a, const double *rec, const double *xt, const double *vt,
                            const double *nrm, const double *cvec, const double *diag, int64_t row0,
                            int64_t nrows, int64_t n, int64_t np, int S, double *part, int64_t ldp,
                            hipStream_t stream)
{
    if (nrows <= 0) return hipSuccess;
    if (d < 1 || d > 64 || S < 1 || row0 < 0 || row0 + nrows > n || np < ksd_padded(n) || ldp < nrows)
        return hipErrorInvalidValue;
    const int64_t rwg = ksd_rows_per_wg(d);
    const int64_t grid = (nrows + rwg - 1) / rwg * S;
    if (grid > 0x7fffffff) return hipErrorInvalidValue;
    if (d > 16) {
        hipLaunchKernelGGL(ksd::k_ksd_tile, dim3((unsigned)grid), dim3(256), 0, stream, xt, vt, nrm, cvec,
                           diag, a, d, ksd_kp(d), row0, nrows, n, np, S, part, ldp);
        return hipGetLastError();
    }
    dispatch_range<1, 16>(d, [&](auto dc) {
        hipLaunchKernelGGL(ksd::k_ksd_rows<decltype(dc)::value>, dim3((unsigned)grid), dim3(256), 0, stream, rec,
                           cvec, diag, a, row0, nrows, n, S, part, ldp);
    });
    return hipGetLastError();
}

hipError_t launch_ksd_finish(const double *part, int S, int64_t ldp, int64_t nrows, double inv_n,
                             const double *diag_rows, double *rows, double *bpart, double *out,
                             hipStream_t stream)
{
    const int64_t nblk = nrows > 0 ? (nrows + KSD_FIN_THREADS - 1) / KSD_FIN_THREADS : 1;
    hipLaunchKernelGGL(ksd::k_ksd_rowfin, dim3((unsigned)nblk), dim3(KSD_FIN_THREADS), 0, stream, part, S,
                       ldp, nrows, inv_n, diag_rows, rows, bpart);
    hipLaunchKernelGGL(ksd::k_ksd_final, dim3(1), dim3(KSD_FIN_THREADS), 0, stream, bpart, nblk, out);
    return hipGetLastError();
}

} // namespace svgd_amd
