// svgd_mmd.hip -- the kernel sums behind the maximum mean discrepancy between
// the particles and a caller's sample, CDNA4 (gfx950), fp64 whatever the
// context's dtype.  With both sets centred on the particles' mean
// (z~ = z - mu), n = |z~|^2:
//   r2 = max(n_i + n_j - 2 x~_i.z~_j, 0)
//   RBF  k = exp(-a r2)            IMQ  k = (1 + a r2)^(-1/2)
// Gram-shaped, so on the fp64 matrix cores: the dataflow of k_ksd_imq_pass
// (svgd_ksd_imq.hip) with one Gram chain, and with rows and columns that may
// come from two different sets.
//
// k_mmd_prep            point records [z~ | n] (svgd_mmd.h) for the n points of
//     a set, all-zero records up to mmd_padded(n).
// k_mmd_pass<KP, KIND>  8 waves x 16 rows per work-group, x~_i as the MFMAs' B
//     operand in registers; the column records stream through two LDS buffers
//     in tiles of MMD_TILE (the next tile is in flight in registers during
//     this tile's arithmetic, one barrier per tile).  Per 16(j) x 16(i) block
//     KP/4 v_mfma_f64_16x16x4_f64 for z~_j.x~_i, then k on the VALU (lane l:
//     i = l & 15, j = (l >> 4) + 4 reg: all four values of a lane belong to one
//     row, so the row sum is a scalar per lane).  A padding column takes 0 by
//     index (k of a zero record is exp(-a n_i) or (1 + a n_i)^(-1/2), not 0);
//     in a same-set pass the column j = i takes exactly 1 by index (the Gram
//     form's rounding of |x~_i - x~_i|^2, times a, never reaches k).  At the
//     end the four lane groups of a row are added in a fixed order.  The grid
//     is row groups x S ranges of the column tiles -> part[S][rows].
// The row finish and the sums over rows are launch_ksd_finish's (svgd_ksd.hip).
// No floating-point atomics, every sum in a fixed order: two calls on the
// same state give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svgdcpp_amd/svgd_capi.h"
#include "dispatch.h"
#include "svgd_imq_dev.h"
#include "svgd_mmd.h"

namespace svgd_amd {
namespace mmd {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef unsigned int u4 __attribute__((ext_vector_type(4))); // a 16-byte piece of a tile
constexpr int NT = 64 * MMD_WAVES;

template <int KP> struct Geom {
    static constexpr int RS = mmd_rec_stride(KP);
    static constexpr int TILE = MMD_TILE;
    static constexpr int TW = TILE * RS;            // doubles per tile
    static constexpr int NP = TW / 2;               // 16-byte pieces per tile
    static constexpr int NPRE = (NP + NT - 1) / NT; // per-thread prefetch registers
    static constexpr int LDS = 2 * TW * 8;          // two tile buffers (at most 68 KiB: two work-groups per CU)
};

// one thread per record
__global__ __launch_bounds__(256) void k_mmd_prep(const double *__restrict__ Z,
                                                  const double *__restrict__ mu, int d, int KP, int RS,
                                                  int64_t n, int64_t np, double *__restrict__ rec)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    const bool real = j < n;
    double *r = rec + j * RS;
    double nj = 0.0;
    for (int k = 0; k < d; ++k) {
        const double z = real ? Z[j * d + k] - mu[k] : 0.0;
        nj = fma(z, z, nj);
        r[k] = z;
    }
    for (int k = d; k < KP; ++k) r[k] = 0.0;
    r[KP] = nj;
    for (int k = KP + 1; k < RS; ++k) r[k] = 0.0;
}

template <int KP, int KIND>
__global__ __launch_bounds__(NT) void k_mmd_pass(const double *__restrict__ rowrec,
                                                 const double *__restrict__ colrec, double a,
                                                 int64_t row0, int64_t nrows, int64_t ncol,
                                                 int64_t ntiles, int same, int S,
                                                 double *__restrict__ part, int64_t ldp)
{
    typedef Geom<KP> GM;
    constexpr int RS = GM::RS, TILE = GM::TILE, TW = GM::TW, NP = GM::NP, NPRE = GM::NPRE;
    constexpr int ON = KP;
    __shared__ __attribute__((aligned(16))) double smem[GM::LDS / 8];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lo = lane & 15, hi = lane >> 4;
    const int64_t grp = blockIdx.x / S;
    const int s = (int)(blockIdx.x - grp * S);
    const int64_t ibase = grp * MMD_ROWS_PER_WG + w * 16;
    // rows past the window read its last row (valid memory; never stored)
    const int64_t il = ibase + lo < nrows ? ibase + lo : nrows - 1;
    const double *ri = rowrec + (row0 + il) * RS;
    // B operand: X~^T, lane holds x~ [i = lo][k = 4kk + hi] (the record's
    // slots d .. KP are zero)
    double bX[KP / 4];
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) bX[kk] = ri[4 * kk + hi];
    const double ni = ri[ON];
    // this work-group's tiles [t0, t1); colrec holds whole tiles (zero records
    // past the points), so whole tiles are copied
    const int64_t t0 = ntiles * s / S, t1 = ntiles * (s + 1) / S, nt = t1 - t0;
    // among this work-group's columns: this lane's own point in a same-set
    // pass (-1: not among them) and the first padding column
    const int64_t jd64 = row0 + ibase + lo - t0 * TILE;
    const int jd = same && jd64 >= 0 && jd64 < 0x7fffffff ? (int)jd64 : -1;
    const int64_t je64 = ncol - t0 * TILE;
    const int je = je64 < 0 ? 0 : je64 < 0x7fffffff ? (int)je64 : 0x7fffffff;

    const u4 *gt = reinterpret_cast<const u4 *>(colrec + t0 * TW);
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
#pragma unroll 1 // (as k_ksd_imq_pass: unrolled, the next block's LDS reads are hoisted into registers)
        for (int js = 0; js < TILE / 16; ++js) {
            d4 xx = {0, 0, 0, 0};
            const double *qa = sR + (js * 16 + lo) * RS + hi;
#pragma unroll
            for (int kk = 0; kk < KP / 4; ++kk)
                xx = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[4 * kk], bX[kk], xx, 0, 0, 0);
            // lane map: column j = js 16 + hi + 4r, row i = lo
            const int jc = (int)t * TILE + js * 16 + hi;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double nj = sR[(js * 16 + hi + 4 * r) * RS + ON];
                const double r2 = fmax(fma(-2.0, xx[r], ni + nj), 0.0);
                double k;
                if (KIND == SVGD_KERNEL_IMQ)
                    k = imq::rsqrt_full(fmin(fma(a, r2, 1.0), 1e300));
                else
                    k = exp(-(a * r2)); // (an underflowing k is exactly 0 or a denormal)
                k = jc + 4 * r == jd ? 1.0 : k;
                k = jc + 4 * r < je ? k : 0.0;
                acc += k;
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

typedef void (*PassFn)(const double *, const double *, double, int64_t, int64_t, int64_t, int64_t, int, int,
                       double *, int64_t);

PassFn pass_fn(int kp, int kernel)
{
    // KP = 4, 8, .., 64
    PassFn f = nullptr;
    if (kp % 4 != 0) return f;
    if (kernel == SVGD_KERNEL_RBF)
        dispatch_range<1, 16>(kp / 4, [&](auto q) { f = &k_mmd_pass<4 * decltype(q)::value, SVGD_KERNEL_RBF>; });
    else if (kernel == SVGD_KERNEL_IMQ)
        dispatch_range<1, 16>(kp / 4, [&](auto q) { f = &k_mmd_pass<4 * decltype(q)::value, SVGD_KERNEL_IMQ>; });
    return f;
}

} // namespace mmd

// work-groups of 8 waves that one CU holds at a time: two waves per SIMD each
// (512 VGPRs per lane, allocated in eights), capped by the 160 KiB of LDS
int mmd_blocks_per_cu(int d, int kernel)
{
    const mmd::PassFn f = d >= 1 && d <= 64 ? mmd::pass_fn(imq_kp(d), kernel) : nullptr;
    hipFuncAttributes fa;
    if (!f || hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(f)) != hipSuccess) return 1;
    const int regs = (fa.numRegs > 0 ? fa.numRegs + 7 : 8) / 8 * 8;
    const int by_regs = 512 / regs / 2 < 4 ? 512 / regs / 2 : 4;
    const int by_lds = fa.sharedSizeBytes > 0 ? (int)(163840 / fa.sharedSizeBytes) : 4;
    const int b = by_regs < by_lds ? by_regs : by_lds;
    return b > 1 ? b : 1;
}

hipError_t launch_mmd_prep(int d, const double *Z, const double *mu, int64_t n, double *rec,
                           hipStream_t stream)
{
    if (d < 1 || d > 64 || n < 1) return hipErrorInvalidValue;
    const int64_t np = mmd_padded(n), grid = (np + 255) / 256;
    if (grid > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mmd::k_mmd_prep, dim3((unsigned)grid), dim3(256), 0, stream, Z, mu, d, imq_kp(d),
                       mmd_rec_stride(d), n, np, rec);
    return hipGetLastError();
}

hipError_t launch_mmd_pass(int d, int kernel, double a, const double *rowrec, int64_t row0, int64_t nrows,
                           const double *colrec, int64_t ncol, bool same, int S, double *part,
                           int64_t ldp, hipStream_t stream)
{
    if (nrows <= 0) return hipSuccess;
    if (d < 1 || d > 64 || row0 < 0 || ncol < 1 || (same && row0 + nrows > ncol) || S < 1 ||
        S > mmd_tiles(ncol) || ldp < nrows)
        return hipErrorInvalidValue;
    const mmd::PassFn f = mmd::pass_fn(imq_kp(d), kernel);
    const int64_t grid = (nrows + MMD_ROWS_PER_WG - 1) / MMD_ROWS_PER_WG * S;
    if (!f || grid > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f, dim3((unsigned)grid), dim3(mmd::NT), 0, stream, rowrec, colrec, a, row0, nrows,
                       ncol, mmd_tiles(ncol), same ? 1 : 0, S, part, ldp);
    return hipGetLastError();
}

} // namespace svgd_amd
