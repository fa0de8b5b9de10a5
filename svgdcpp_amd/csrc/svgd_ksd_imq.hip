// svgd_ksd_imq.hip -- the kernelized Stein discrepancy under the inverse
// multiquadric kernel, CDNA4 (gfx950), fp64 whatever the context's dtype.
// With centred coordinates xc, scores s, n = |xc|^2, p = s.xc:
//   r2   = max(n_i + n_j - 2 xc_i.xc_j, 0),  k = (1 + a r2)^(-1/2)
//   u_ij = k s_i.s_j + a k^3 (p_i + p_j - (s_i.xc_j + xc_i.s_j) + d) - 3 a^2 k^5 r2
//   u_ii = |s_i|^2 + a d
// (the diagonal is taken by index from diag[], so the Gram form's rounding of
// |xc_i - xc_i|^2, times a, never reaches k.)
// Gram-shaped, so on the fp64 matrix cores: the dataflow of k_imq_pass
// (svgd_imq.hip) with three Gram chains and no contraction.
//
// k_ksd_imq_prep      column records [xc | s | n | p] (svgd_ksd_imq.h) for the
//     n particles, all-zero records up to ksd_imq_padded(n); diag.
// k_ksd_imq_pass<KP>  8 waves x 16 particle rows per work-group, xc_i and s_i
//     as the MFMAs' B operands in registers; the records stream through two
//     LDS buffers in tiles of Geom::TILE (the next tile is in flight in
//     registers during this tile's arithmetic, one barrier per tile).  Per
//     16(j) x 16(i) block, from two LDS reads per 4 coordinates:
//       xx    = xc_j.xc_i                 KP/4 v_mfma_f64_16x16x4_f64
//       ss    = s_j.s_i                   KP/4
//       cross = xc_j.s_i + s_j.xc_i       2 KP/4 (one accumulator)
//     then u on the VALU (lane l: i = l & 15, j = (l >> 4) + 4 reg: all four
//     values of a lane belong to one row, so the row sum is a scalar per
//     lane).  The column j = i takes diag[i]; a padding column takes 0 by
//     index (its record is all zeros, but u_ij of a zero record is not 0).
//     At the end the four lane groups of a row are added in a fixed order.
//     The grid is row groups x S ranges of the tiles -> part[S][rows].
// The row finish and the two sums are launch_ksd_finish's (svgd_ksd.hip).
// No floating-point atomics, every sum in a fixed order: two calls on the
// same state give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dispatch.h"
#include "svgd_imq_dev.h"
#include "svgd_ksd_imq.h"

namespace svgd_amd {
namespace ksd_imq {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef unsigned int u4 __attribute__((ext_vector_type(4))); // a 16-byte piece of a tile
constexpr int NT = 64 * KSD_IMQ_WAVES;

// (the rule of svgd_imq.hip's tile_of, on the same stride)
constexpr int tile_of(int kp) { return 2 * 64 * ksd_imq_rec_stride(kp) * 8 <= 80 * 1024 ? 64 : 32; }

template <int KP> struct Geom {
    static constexpr int RS = ksd_imq_rec_stride(KP);
    static constexpr int TILE = tile_of(KP);
    static constexpr int TW = TILE * RS;            // doubles per tile
    static constexpr int NP = TW / 2;               // 16-byte pieces per tile
    static constexpr int NPRE = (NP + NT - 1) / NT; // per-thread prefetch registers
    static constexpr int LDS = 2 * TW * 8;          // two tile buffers
};

// one thread per record
__global__ __launch_bounds__(256) void k_ksd_imq_prep(const double *__restrict__ X,
                                                      const double *__restrict__ G,
                                                      const double *__restrict__ mu, double a, int d,
                                                      int KP, int RS, int64_t n, int64_t np,
                                                      double *__restrict__ rec, double *__restrict__ diag)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    const bool real = j < n;
    double *r = rec + j * RS;
    double nj = 0.0, pj = 0.0, ss = 0.0;
    for (int k = 0; k < d; ++k) {
        const double x = real ? X[j * d + k] - mu[k] : 0.0;
        const double sc = real ? G[j * d + k] : 0.0;
        nj = fma(x, x, nj);
        pj = fma(sc, x, pj);
        ss = fma(sc, sc, ss);
        r[k] = x;
        r[KP + k] = sc;
    }
    for (int k = d; k < KP; ++k) r[k] = r[KP + k] = 0.0;
    r[2 * KP] = nj;
    r[2 * KP + 1] = pj;
    for (int k = 2 * KP + 2; k < RS; ++k) r[k] = 0.0;
    diag[j] = real ? ss + a * (double)d : 0.0;
}

template <int KP>
__global__ __launch_bounds__(NT) void k_ksd_imq_pass(const double *__restrict__ rec,
                                                     const double *__restrict__ diag, double a, int d,
                                                     int64_t row0, int64_t nrows, int64_t n,
                                                     int64_t ntiles, int S, double *__restrict__ part,
                                                     int64_t ldp)
{
    typedef Geom<KP> GM;
    constexpr int RS = GM::RS, TILE = GM::TILE, TW = GM::TW, NP = GM::NP, NPRE = GM::NPRE;
    constexpr int OS = KP, ON = 2 * KP, OP = 2 * KP + 1;
    __shared__ __attribute__((aligned(16))) double smem[GM::LDS / 8];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lo = lane & 15, hi = lane >> 4;
    const int64_t grp = blockIdx.x / S;
    const int s = (int)(blockIdx.x - grp * S);
    const int64_t ibase = grp * KSD_IMQ_ROWS_PER_WG + w * 16;
    // rows past the shard read its last row (valid memory; never stored)
    const int64_t il = ibase + lo < nrows ? ibase + lo : nrows - 1;
    const double *ri = rec + (row0 + il) * RS;
    // B operands: Xc^T and S^T, lane holds xc / s [i = lo][k = 4kk + hi]
    // (the record's slots d .. KP are zero)
    double bX[KP / 4], bS[KP / 4];
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) {
        bX[kk] = ri[4 * kk + hi];
        bS[kk] = ri[OS + 4 * kk + hi];
    }
    const double ni = ri[ON];
    const double pid = ri[OP] + (double)d; // p_i + d
    const double dgi = diag[row0 + il];
    // this work-group's tiles [t0, t1); rec holds whole tiles (zero records
    // past the particles), so whole tiles are copied
    const int64_t t0 = ntiles * s / S, t1 = ntiles * (s + 1) / S, nt = t1 - t0;
    // among this work-group's columns: this lane's own particle (-1: not among
    // them) and the first padding column
    const int64_t jd64 = row0 + ibase + lo - t0 * TILE;
    const int jd = jd64 >= 0 && jd64 < 0x7fffffff ? (int)jd64 : -1;
    const int64_t je64 = n - t0 * TILE;
    const int je = je64 < 0 ? 0 : je64 < 0x7fffffff ? (int)je64 : 0x7fffffff;
    const double c3 = 3.0 * a * a;

    const u4 *gt = reinterpret_cast<const u4 *>(rec + t0 * TW);
    u4 pre[NPRE];
    auto fetch = [&](int64_t t) {
#pragma unroll
        for (int p = 0; p < NPRE; ++p) {
            const int e = p * NT + tid; // (pieces past the tile read its last one: not stored)
            pre[p] = gt[t * NP + (NP % NT == 0 || e < NP ? e : NP - 1)];
        }
    };
    auto stash = [&](int64_t t) {
        u4 *b = reinterpret_cast<u4 *>(smem + (t & 1) * TW);
#pragma unroll
        for (int p = 0; p < NPRE; ++p) {
            const int e = p * NT + tid;
            if (NP % NT == 0 || e < NP) b[e] = pre[p];
        }
    };
    if (nt > 0) {
        fetch(0);
        stash(0);
    }
    __syncthreads();
    double acc = 0.0; // this lane's share of row i = lo: the columns j = hi (mod 4)
    for (int64_t t = 0; t < nt; ++t) {
        if (t + 1 < nt) fetch(t + 1); // in flight during this tile's arithmetic
        const double *sR = smem + (t & 1) * TW;
#pragma unroll 1 // (as k_imq_pass: unrolled, the next block's LDS reads are hoisted into registers)
        for (int js = 0; js < TILE / 16; ++js) {
            d4 xx = {0, 0, 0, 0}, ss = {0, 0, 0, 0}, cr = {0, 0, 0, 0};
            const double *qa = sR + (js * 16 + lo) * RS + hi;
#pragma unroll
            for (int kk = 0; kk < KP / 4; ++kk) {
                const double ax = qa[4 * kk], as = qa[OS + 4 * kk];
                xx = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, bX[kk], xx, 0, 0, 0);
                ss = __builtin_amdgcn_mfma_f64_16x16x4f64(as, bS[kk], ss, 0, 0, 0);
                cr = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, bS[kk], cr, 0, 0, 0);
                cr = __builtin_amdgcn_mfma_f64_16x16x4f64(as, bX[kk], cr, 0, 0, 0);
            }
            // lane map of the three: column j = js 16 + hi + 4r, row i = lo
            const int jc = (int)t * TILE + js * 16 + hi;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double *q = sR + (js * 16 + hi + 4 * r) * RS;
                const double r2 = fmax(fma(-2.0, xx[r], ni + q[ON]), 0.0);
                const double k = imq::rsqrt_full(fmin(fma(a, r2, 1.0), 1e300));
                const double k2 = k * k, k3 = k2 * k;
                const double lin = a * ((pid + q[OP]) - cr[r]);
                double u = fma(k, ss[r], k3 * (lin - c3 * (k2 * r2)));
                u = jc + 4 * r == jd ? dgi : u;
                u = jc + 4 * r < je ? u : 0.0;
                acc += u;
            }
        }
        if (t + 1 < nt) stash(t + 1); // the buffer tile t - 1 was read from
        __syncthreads();
    }
    // the four lane groups of row lo, in a fixed order: (h0 + h1) + (h2 + h3)
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    const int64_t li = ibase + lo;
    if (hi == 0 && li < nrows) part[(int64_t)s * ldp + li] = acc;
}

typedef void (*PassFn)(const double *, const double *, double, int, int64_t, int64_t, int64_t, int64_t,
                       int, double *, int64_t);

PassFn pass_fn(int kp)
{
    // KP = 4, 8, .., 64
    PassFn f = nullptr;
    if (kp % 4 == 0)
        dispatch_range<1, 16>(kp / 4, [&](auto q) { f = &k_ksd_imq_pass<4 * decltype(q)::value>; });
    return f;
}

} // namespace ksd_imq

int ksd_imq_tile(int d) { return ksd_imq::tile_of(imq_kp(d)); }

// work-groups of 8 waves that one CU holds at a time: two waves per SIMD each
// (512 VGPRs per lane, allocated in eights), capped by the 160 KiB of LDS
int ksd_imq_blocks_per_cu(int d)
{
    const ksd_imq::PassFn f = d >= 1 && d <= 64 ? ksd_imq::pass_fn(imq_kp(d)) : nullptr;
    hipFuncAttributes fa;
    if (!f || hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(f)) != hipSuccess) return 1;
    const int regs = (fa.numRegs > 0 ? fa.numRegs + 7 : 8) / 8 * 8;
    const int by_regs = 512 / regs / 2 < 4 ? 512 / regs / 2 : 4;
    const int by_lds = fa.sharedSizeBytes > 0 ? (int)(163840 / fa.sharedSizeBytes) : 4;
    const int b = by_regs < by_lds ? by_regs : by_lds;
    return b > 1 ? b : 1;
}

hipError_t launch_ksd_imq_prep(int d, const double *X, const double *G, const double *mu, double a,
                               int64_t n, double *rec, double *diag, hipStream_t stream)
{
    if (d < 1 || d > 64 || n < 1) return hipErrorInvalidValue;
    const int64_t np = ksd_imq_padded(n), grid = (np + 255) / 256;
    if (grid > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ksd_imq::k_ksd_imq_prep, dim3((unsigned)grid), dim3(256), 0, stream, X, G, mu, a, d,
                       imq_kp(d), ksd_imq_rec_stride(d), n, np, rec, diag);
    return hipGetLastError();
}

hipError_t launch_ksd_imq_pass(int d, double a, const double *rec, const double *diag, int64_t row0,
                               int64_t nrows, int64_t n, int S, double *part, int64_t ldp,
                               hipStream_t stream)
{
    if (nrows <= 0) return hipSuccess;
    if (d < 1 || d > 64 || row0 < 0 || row0 + nrows > n || S < 1 || S > ksd_imq_tiles(d, n) || ldp < nrows)
        return hipErrorInvalidValue;
    const ksd_imq::PassFn f = ksd_imq::pass_fn(imq_kp(d));
    const int64_t grid = (nrows + KSD_IMQ_ROWS_PER_WG - 1) / KSD_IMQ_ROWS_PER_WG * S;
    if (!f || grid > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f, dim3((unsigned)grid), dim3(ksd_imq::NT), 0, stream, rec, diag, a, d, row0, nrows,
                       n, ksd_imq_tiles(d, n), S, part, ldp);
    return hipGetLastError();
}

} // namespace svgd_amd
