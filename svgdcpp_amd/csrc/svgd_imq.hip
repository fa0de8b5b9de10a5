// svgd_imq.hip -- phi_hat of the SVGD step under the inverse multiquadric
// kernel, CDNA4 (gfx950), fp64 whatever the context's dtype:
//   k_ij  = (1 + a |xc_i - xc_j|^2)^(-1/2)
//   phi_i = (1/N) [ G_i + sum_{j != i} k_ij G_j
//                   + a ( xc_i sum_{j != i} k_ij^3 - sum_{j != i} k_ij^3 xc_j ) ]
// (k_ii = 1 and its repulsion term is 0 by definition: the pass leaves the
// diagonal out by index and the finish adds G_i, so the Gram form's rounding
// of |xc_i - xc_i|^2, times a, never reaches phi -- at a = 1e6 it would be
// 1e-8 of G_i.)
// Gram-shaped, so on the fp64 matrix cores: the dataflow of k_glm_pass
// (svgd_glm.hip) with a reciprocal square root where the sigmoid is and two
// contractions instead of one.
//
// k_imq_prep        column records [xc | w = 1 | G | n = |xc|^2] (svgd_imq.h)
//     for the n particles, all-zero records up to imq_padded(n).
// k_imq_pass<KP>    8 waves x 16 particle rows per work-group, xc_i as the
//     Gram MFMA's B operand in registers; the records stream through two LDS
//     buffers in tiles of Geom::TILE (the next tile is in flight in registers
//     during this tile's arithmetic, one barrier per tile).  Per 16(j) x 16(i)
//     block: dot by KP/4 v_mfma_f64_16x16x4_f64 (A = records from LDS),
//     s = 1 + a max(n_i + n_j - 2 dot, 0), k = s^(-1/2), k = 0 at j = i, on
//     the VALU (lane l: i = l & 15, j = (l >> 4) + 4 reg -- already the
//     A-operand map), then
//     accG += K G_J by ceil(d/16) blocks and accX += K^3 [xc_J | w_J] by
//     KP/16 + 1 blocks whose B operands are the same LDS record.
//     A padding record is all zeros: k is finite for it (s >= 1) and
//     k * 0 = 0, k^3 * 0 = 0 in every sum, the row sum of k^3 included (its
//     column is w), so the loop masks nothing.
//     The grid is row groups x S ranges of the tiles -> part[S][rows][2d+1].
// k_imq_finish      sums s ascending, adds the diagonal's G_i and forms phi_i.
// No floating-point atomics, every sum in a fixed order: two calls on the
// same state give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dispatch.h"
#include "svgd_imq.h"
#include "svgd_imq_dev.h" // rsqrt_full

namespace svgd_amd {
namespace imq {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef unsigned int u4 __attribute__((ext_vector_type(4))); // a 16-byte piece of a tile
constexpr int NT = 64 * IMQ_WAVES;

constexpr int tile_of(int kp) { return 2 * 64 * imq_rec_stride(kp) * 8 <= 80 * 1024 ? 64 : 32; }

template <int KP> struct Geom {
    static constexpr int RS = imq_rec_stride(KP);
    static constexpr int TILE = tile_of(KP);
    static constexpr int NCBG = (KP + 15) / 16;     // blocks of K G (= ceil(d/16) at every d of this KP)
    // blocks of K^3 [xc | w]: ceil((d+1)/16), but for d = KP - 3 .. KP - 1 at KP % 16 == 0, which
    // run one block more than they need (a branch in the MFMA chain made KP >= 48 spill)
    static constexpr int NCBX = KP / 16 + 1;
    static constexpr int TW = TILE * RS;            // doubles per tile
    static constexpr int NP = TW / 2;               // 16-byte pieces per tile
    static constexpr int NPRE = (NP + NT - 1) / NT; // per-thread prefetch registers
    static constexpr int LDS = 2 * TW * 8;          // two tile buffers
};

__global__ __launch_bounds__(256) void k_imq_prep(const double *__restrict__ xc, int xs,
                                                  const double *__restrict__ G, int d, int KP, int RS,
                                                  int64_t n, int64_t tot, double *__restrict__ rec)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= tot) return;
    const int64_t j = e / RS;
    const int k = (int)(e - j * RS);
    double v = 0.0;
    if (j < n) {
        if (k < d)
            v = xc[j * xs + k];
        else if (k == KP)
            v = 1.0;
        else if (k > KP && k - KP - 1 < d)
            v = G[j * d + (k - KP - 1)];
        else if (k == 2 * KP + 1) {
            for (int q = 0; q < d; ++q) v = fma(xc[j * xs + q], xc[j * xs + q], v);
        }
    }
    rec[e] = v;
}

template <int KP>
__global__ __launch_bounds__(NT) void k_imq_pass(const double *__restrict__ rec,
                                                 const double *__restrict__ a_ptr, int d, int64_t row0,
                                                 int64_t nrows, int64_t ntiles, int S,
                                                 double *__restrict__ part, int64_t ldp)
{
    typedef Geom<KP> GM;
    constexpr int RS = GM::RS, TILE = GM::TILE, NCBG = GM::NCBG, NCBX = GM::NCBX, TW = GM::TW,
                  NP = GM::NP, NPRE = GM::NPRE;
    constexpr int OW = KP, OG = KP + 1, ON = 2 * KP + 1;
    __shared__ __attribute__((aligned(16))) double smem[GM::LDS / 8];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lo = lane & 15, hi = lane >> 4;
    const int64_t grp = blockIdx.x / S;
    const int s = (int)(blockIdx.x - grp * S);
    const int64_t ibase = grp * IMQ_ROWS_PER_WG + w * 16;
    // rows past the shard read its last row (valid memory; never stored)
    const int64_t il = ibase + lo < nrows ? ibase + lo : nrows - 1;
    const double *ri = rec + (row0 + il) * RS;
    // B operand of the Gram MFMA: Xc^T, lane holds xc[i = lo][k = 4kk + hi]
    // (the record's slots d .. KP are zero)
    double bI[KP / 4];
#pragma unroll
    for (int kk = 0; kk < KP / 4; ++kk) bI[kk] = ri[4 * kk + hi];
    const double ni = ri[ON];
    // this lane's own particle as a column of this work-group's tiles (-1: not among them)
    const int64_t jd64 = row0 + ibase + lo - (ntiles * s / S) * TILE;
    const int jd = jd64 >= 0 && jd64 < 0x7fffffff ? (int)jd64 : -1;
    const double a = a_ptr[0];
    // B operands of the contractions: column cb 16 + lo of G, and of [xc | w]
    // (columns past d read a valid slot: those accumulators are not stored)
    int gidx[NCBG], xidx[NCBX];
#pragma unroll
    for (int cb = 0; cb < NCBG; ++cb) gidx[cb] = cb * 16 + lo < d ? OG + cb * 16 + lo : OG;
#pragma unroll
    for (int cb = 0; cb < NCBX; ++cb) xidx[cb] = cb * 16 + lo < d ? cb * 16 + lo : OW;

    d4 accG[NCBG], accX[NCBX];
#pragma unroll
    for (int cb = 0; cb < NCBG; ++cb) accG[cb] = d4{0, 0, 0, 0};
#pragma unroll
    for (int cb = 0; cb < NCBX; ++cb) accX[cb] = d4{0, 0, 0, 0};

    // this work-group's tiles [t0, t1); rec holds whole tiles (zero records
    // past the particles), so whole tiles are copied
    const int64_t t0 = ntiles * s / S, t1 = ntiles * (s + 1) / S, nt = t1 - t0;
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
    for (int64_t t = 0; t < nt; ++t) {
        if (t + 1 < nt) fetch(t + 1); // in flight during this tile's arithmetic
        const double *sR = smem + (t & 1) * TW;
#pragma unroll 1 // (unrolled, the scheduler hoists the next block's LDS reads and KP >= 48 spills)
        for (int js = 0; js < TILE / 16; ++js) {
            d4 dot = {0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < KP / 4; ++kk)
                dot = __builtin_amdgcn_mfma_f64_16x16x4f64(sR[(js * 16 + lo) * RS + 4 * kk + hi], bI[kk],
                                                           dot, 0, 0, 0);
            // dot lane map: column j = js 16 + hi + 4r, row i = lo
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double *q = sR + (js * 16 + hi + 4 * r) * RS;
                const double r2 = fmax(fma(-2.0, dot[r], ni + q[ON]), 0.0);
                const double kf = rsqrt_full(fmin(fma(a, r2, 1.0), 1e300));
                const double k = (int)t * TILE + js * 16 + hi + 4 * r == jd ? 0.0 : kf; // (the finish adds j = i)
                const double k3 = k * k * k;
#pragma unroll
                for (int cb = 0; cb < NCBG; ++cb)
                    accG[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(k, q[gidx[cb]], accG[cb], 0, 0, 0);
#pragma unroll
                for (int cb = 0; cb < NCBX; ++cb)
                        accX[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(k3, q[xidx[cb]], accX[cb], 0, 0, 0);
            }
        }
        if (t + 1 < nt) stash(t + 1); // the buffer tile t - 1 was read from
        __syncthreads();
    }
    // acc lane map: row i = hi + 4q, column c = lo + 16 cb
    const int W = imq_part_width(d);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t li = ibase + hi + 4 * q;
        if (li >= nrows) continue;
        double *o = part + ((int64_t)s * ldp + li) * W;
#pragma unroll
        for (int cb = 0; cb < NCBG; ++cb) {
            const int c = cb * 16 + lo;
            if (c < d) o[c] = accG[cb][q];
        }
#pragma unroll
        for (int cb = 0; cb < NCBX; ++cb) {
            const int c = cb * 16 + lo;
            if (c <= d) o[d + c] = accX[cb][q];
        }
    }
}

__global__ __launch_bounds__(IMQ_FIN_THREADS) void k_imq_finish(const double *__restrict__ rec, int RS,
                                                                const double *__restrict__ a_ptr, int d,
                                                                int64_t row0, int64_t tot,
                                                                const double *__restrict__ part, int S,
                                                                int64_t ldp, double inv_n,
                                                                double *__restrict__ phi)
{
    const int64_t e = (int64_t)blockIdx.x * IMQ_FIN_THREADS + threadIdx.x;
    if (e >= tot) return;
    const int64_t li = e / d;
    const int c = (int)(e - li * d);
    const int W = imq_part_width(d);
    double sg = 0.0, sx = 0.0, s3 = 0.0;
    for (int s = 0; s < S; ++s) {
        const double *p = part + ((int64_t)s * ldp + li) * W;
        sg += p[c];
        sx += p[d + c];
        s3 += p[2 * d];
    }
    const double *ri = rec + (row0 + li) * RS;
    // (j = i: k = 1, no repulsion)
    phi[e] = inv_n * (ri[imq_off_g(d) + c] + sg + a_ptr[0] * (ri[c] * s3 - sx));
}

typedef void (*PassFn)(const double *, const double *, int, int64_t, int64_t, int64_t, int, double *,
                       int64_t);

PassFn pass_fn(int kp)
{
    // KP = 4, 8, .., 64
    PassFn f = nullptr;
    if (kp % 4 == 0)
        dispatch_range<1, 16>(kp / 4, [&](auto q) { f = &k_imq_pass<4 * decltype(q)::value>; });
    return f;
}

// work-groups of 8 waves that one CU holds at a time: two waves per SIMD each
// (512 VGPRs per lane, allocated in eights), capped by the 160 KiB of LDS
int blocks_per_cu(const void *f)
{
    hipFuncAttributes fa;
    if (!f || hipFuncGetAttributes(&fa, f) != hipSuccess) return 1;
    const int regs = (fa.numRegs > 0 ? fa.numRegs + 7 : 8) / 8 * 8;
    const int by_regs = 512 / regs / 2 < 4 ? 512 / regs / 2 : 4;
    const int by_lds = fa.sharedSizeBytes > 0 ? (int)(163840 / fa.sharedSizeBytes) : 4;
    const int b = by_regs < by_lds ? by_regs : by_lds;
    return b > 1 ? b : 1;
}

} // namespace imq

int imq_tile(int d) { return imq::tile_of(imq_kp(d)); }

int imq_blocks_per_cu(int d)
{
    const imq::PassFn f = d >= 1 && d <= 64 ? imq::pass_fn(imq_kp(d)) : nullptr;
    return imq::blocks_per_cu(reinterpret_cast<const void *>(f));
}

hipError_t launch_imq_prep(int d, const double *xc, int xs, const double *G, int64_t n, double *rec,
                           hipStream_t stream)
{
    if (d < 1 || d > 64 || xs < d || n < 1) return hipErrorInvalidValue;
    const int RS = imq_rec_stride(d);
    const int64_t tot = imq_padded(n) * RS, grid = (tot + 255) / 256;
    if (grid > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(imq::k_imq_prep, dim3((unsigned)grid), dim3(256), 0, stream, xc, xs, G, d,
                       imq_kp(d), RS, n, tot, rec);
    return hipGetLastError();
}

hipError_t launch_imq_pass(int d, const double *rec, const double *a_ptr, int64_t row0, int64_t nrows,
                           int64_t n, int S, double *part, int64_t ldp, hipStream_t stream)
{
    if (nrows <= 0) return hipSuccess;
    if (d < 1 || d > 64 || row0 < 0 || row0 + nrows > n || S < 1 || S > imq_tiles(d, n) || ldp < nrows)
        return hipErrorInvalidValue;
    const imq::PassFn f = imq::pass_fn(imq_kp(d));
    const int64_t grid = (nrows + IMQ_ROWS_PER_WG - 1) / IMQ_ROWS_PER_WG * S;
    if (!f || grid > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f, dim3((unsigned)grid), dim3(imq::NT), 0, stream, rec, a_ptr, d, row0, nrows,
                       imq_tiles(d, n), S, part, ldp);
    return hipGetLastError();
}

hipError_t launch_imq_finish(int d, const double *rec, const double *a_ptr, int64_t row0, int64_t nrows,
                             const double *part, int S, int64_t ldp, double inv_n, double *phi,
                             hipStream_t stream)
{
    if (nrows <= 0) return hipSuccess;
    const int64_t tot = nrows * d;
    hipLaunchKernelGGL(imq::k_imq_finish, dim3((unsigned)((tot + IMQ_FIN_THREADS - 1) / IMQ_FIN_THREADS)),
                       dim3(IMQ_FIN_THREADS), 0, stream, rec, imq_rec_stride(d), a_ptr, d, row0, tot, part,
                       S, ldp, inv_n, phi);
    return hipGetLastError();
}

} // namespace svgd_amd
