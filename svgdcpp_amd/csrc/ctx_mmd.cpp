// ctx_mmd.cpp -- svgd_mmd: the maximum mean discrepancy between the particles
// and a caller's sample under the RBF or the inverse multiquadric kernel, an
// observer with work arrays of its own (the particles' side allocated by the
// first call, the sample's side grown when a later call brings more points).
#include "ctx.h"
#include <algorithm>
#include <cmath>
#include "svgd_ksd.h"
#include "svgd_mmd.h"

using namespace svgd_amd;

namespace svgd_amd {
namespace {

int mmd_alloc(svgd_ctx *c, int64_t m)
{
    svgd_ctx::Mmd &k = c->mmd;
    const int d = c->dim;
    if (!k.ready) {
        HIPCHK(c, hipDeviceGetAttribute(&k.cus, hipDeviceAttributeMultiprocessorCount, c->device));
        k.bpc[SVGD_KERNEL_RBF] = mmd_blocks_per_cu(d, SVGD_KERNEL_RBF);
        k.bpc[SVGD_KERNEL_IMQ] = mmd_blocks_per_cu(d, SVGD_KERNEL_IMQ);
        CHK(dalloc(c, &k.mu, 64));
        CHK(dalloc(c, &k.mpart, (int64_t)KSD_MEAN_BLOCKS * d));
        CHK(dalloc(c, &k.xrec, mmd_padded(c->n) * mmd_rec_stride(d)));
        CHK(dalloc(c, &k.out, 4));
        k.ready = true;
    }
    if (m > k.m_cap) {
        k.m_cap = 0; // (set again only when every array below is in place)
        // (this rank's rows of Y are at most ceil(m / world))
        const int64_t yrows = (m + c->world - 1) / c->world;
        k.ldp = (std::max<int64_t>(1, std::max(c->nrows, yrows)) + 63) / 64 * 64;
        CHK(dalloc(c, &k.Y, m * d));
        CHK(dalloc(c, &k.yrec, mmd_padded(m) * mmd_rec_stride(d)));
        CHK(dalloc(c, &k.rxx, k.ldp));
        CHK(dalloc(c, &k.rxy, k.ldp));
        CHK(dalloc(c, &k.ryy, k.ldp));
        CHK(dalloc(c, &k.bpart, 2 * ((k.ldp + KSD_FIN_THREADS - 1) / KSD_FIN_THREADS)));
        k.m_cap = m;
    }
    return SVGD_OK;
}

// column splits of one pass (the rule of ksd_imq_alloc): the grid (row groups
// x S) fills the resident work-group slots at most twice; each split at least
// one tile wide
int mmd_splits(const svgd_ctx *c, int kernel, int64_t nrows, int64_t ncol)
{
    const int64_t groups = std::max<int64_t>(1, (nrows + MMD_ROWS_PER_WG - 1) / MMD_ROWS_PER_WG);
    const int64_t resident = (int64_t)std::max(1, c->mmd.cus) * c->mmd.bpc[kernel];
    return (int)std::min<int64_t>(std::max<int64_t>(1, 2 * resident / groups), mmd_tiles(ncol));
}

} // namespace
} // namespace svgd_amd

extern "C" {

int svgd_mmd(svgd_ctx *c, int kernel, const double *Y, int64_t m, double a, double *mmd2_v, double *mmd2_u,
             double *means3_out, double *witness_shard_out)
{
    CHK(check_results(c));
    if (kernel != SVGD_KERNEL_RBF && kernel != SVGD_KERNEL_IMQ)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Unknown MMD kernel.");
    if (!Y) return fail(c, SVGD_ERR_ARG, "[Argument Error] Null MMD sample.");
    if (m < 1) return fail(c, SVGD_ERR_DIM, "[Dimension Error] The MMD sample needs at least one point.");
    if (!std::isfinite(a) || !(a > 0.0))
        return fail(c, SVGD_ERR_ARG, "[Argument Error] The MMD kernel scale must be finite and positive.");
    const int d = c->dim;
    for (int64_t e = 0; e < m * d; ++e)
        if (!std::isfinite(Y[e]))
            return fail(c, SVGD_ERR_ARG, "[Argument Error] The MMD sample holds a non-finite value.");
    CHK(resolve_pending(c));
    HIPCHK(c, hipSetDevice(c->device));
    svgd_ctx::Mmd &k = c->mmd;
    CHK(mmd_alloc(c, m));
    // this rank's rows of the YY sum
    int64_t y0 = 0, y1 = m;
    svgd_plan_rows(m, c->world, c->rank, &y0, &y1);
    const int64_t yrows = y1 - y0;
    const int sxx = mmd_splits(c, kernel, c->nrows, c->n), sxy = mmd_splits(c, kernel, c->nrows, m),
              syy = mmd_splits(c, kernel, yrows, m);
    const int64_t need = (int64_t)std::max(sxx, std::max(sxy, syy)) * k.ldp;
    if (need > k.part_cap) {
        k.part_cap = 0;
        CHK(dalloc(c, &k.part, need));
        k.part_cap = need;
    }
    // work is queued behind the step's marks: they no longer end the stream
    c->mark = c->phi_end = c->last_phi_end = nullptr;
    HIPCHK(c, hipMemcpyAsync(k.Y, Y, sizeof(double) * (size_t)m * d, hipMemcpyHostToDevice, c->stream));
    // One pass at a time through part.  launch_ksd_finish with weight 1: rows =
    // the row sums (s ascending), out[0] = their sum by its fixed tree; its
    // second sum (of the `diag' argument: part here, any valid array) lands in
    // out[1] and is overwritten by the next pass's first -- XX, XY, YY in this
    // order leave out[0..2] = [Sxx, Sxy, Syy] of this rank's rows.
    auto pass = [&](const double *rowrec, int64_t row0, int64_t nrows, const double *colrec, int64_t ncol,
                    bool same, int S, double *rows, double *out) {
        hipError_t e = launch_mmd_pass(d, kernel, a, rowrec, row0, nrows, colrec, ncol, same, S, k.part, k.ldp,
                                       c->stream);
        if (e == hipSuccess)
            e = launch_ksd_finish(k.part, S, k.ldp, nrows, 1.0, k.part, rows, k.bpart, out, c->stream);
        return e;
    };
    hipError_t e = launch_ksd_mean(c->X, c->n, d, k.mpart, k.mu, c->stream);
    if (e == hipSuccess) e = launch_mmd_prep(d, c->X, k.mu, c->n, k.xrec, c->stream);
    if (e == hipSuccess) e = launch_mmd_prep(d, k.Y, k.mu, m, k.yrec, c->stream);
    if (e == hipSuccess) e = pass(k.xrec, c->row0, c->nrows, k.xrec, c->n, true, sxx, k.rxx, k.out);
    if (e == hipSuccess) e = pass(k.xrec, c->row0, c->nrows, k.yrec, m, false, sxy, k.rxy, k.out + 1);
    if (e == hipSuccess) e = pass(k.yrec, y0, yrows, k.yrec, m, true, syy, k.ryy, k.out + 2);
    if (e != hipSuccess) return fail(c, SVGD_ERR_HIP, std::string("[HIP Error] MMD pass: ") + hipGetErrorString(e));
    // the observer's collective stays out of the step's collective hash and
    // of the level-2 diagnostic spans
    const uint64_t sig = c->co.coll_sig;
    const int tlevel = c->tm.tlevel;
    c->tm.tlevel = 0;
    const int rc = allreduce_f64(c, k.out, 3);
    c->tm.tlevel = tlevel;
    c->co.coll_sig = sig;
    CHK(rc);
    double sums[3] = {0.0, 0.0, 0.0};
    HIPCHK(c, hipMemcpyAsync(sums, k.out, sizeof(sums), hipMemcpyDeviceToHost, c->stream));
    std::vector<double> rxy;
    if (witness_shard_out && c->nrows > 0) {
        rxy.resize((size_t)c->nrows);
        HIPCHK(c, hipMemcpyAsync(witness_shard_out, k.rxx, sizeof(double) * (size_t)c->nrows,
                                 hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(rxy.data(), k.rxy, sizeof(double) * (size_t)c->nrows, hipMemcpyDeviceToHost,
                                 c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // sums = [Sxx, Sxy, Syy] over all ranks; the definition's order
    const double N = (double)c->n, M = (double)m;
    const double mxx = sums[0] / (N * N), myy = sums[2] / (M * M), mxy = sums[1] / (N * M);
    if (mmd2_v) *mmd2_v = mxx + myy - 2.0 * mxy;
    if (mmd2_u)
        *mmd2_u = c->n < 2 || m < 2
                      ? NAN
                      : (sums[0] - N) / (N * (N - 1.0)) + (sums[2] - M) / (M * (M - 1.0)) - 2.0 * mxy;
    if (means3_out) {
        means3_out[0] = mxx;
        means3_out[1] = myy;
        means3_out[2] = mxy;
    }
    if (witness_shard_out)
        for (int64_t i = 0; i < c->nrows; ++i) witness_shard_out[i] = witness_shard_out[i] / N - rxy[(size_t)i] / M;
    return SVGD_OK;
}

} // extern "C"
