// ctx_ksd.cpp -- svgd_ksd / svgd_ksd_kernel: the kernelized Stein discrepancy of
// the particles under the RBF or the inverse multiquadric kernel, an observer
// with work arrays of its own (one set per kernel, allocated by that kernel's
// first call).
#include "ctx.h"
#include <cmath>
#include "svgd_ksd.h"
#include "svgd_ksd_imq.h"

using namespace svgd_amd;

namespace svgd_amd {
namespace {

int ksd_alloc(svgd_ctx *c)
{
    svgd_ctx::Ksd &k = c->ksd;
    if (k.ready) return SVGD_OK;
    const int d = c->dim;
    k.np = ksd_padded(c->n);
    // column splits: the work-groups take equal time, so the grid (row groups
    // x S) should fill the device's resident slots a whole number of times
    // -- at most twice here -- and not spill a few work-groups into one more
    // round; each split at least 128 columns (d <= 16) or one tile wide
    const int64_t rwg = ksd_rows_per_wg(d);
    const int64_t groups = std::max<int64_t>(1, (c->nrows + rwg - 1) / rwg);
    const int64_t smax = d <= 16 ? std::max<int64_t>(1, c->n / 128) : (c->n + KSD_TILE - 1) / KSD_TILE;
    int cus = 0;
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const int64_t resident = (int64_t)std::max(1, cus) * ksd_blocks_per_cu(d);
    k.S = (int)std::min<int64_t>(std::max<int64_t>(1, 2 * resident / groups), smax);
    k.ldp = (std::max<int64_t>(1, c->nrows) + 63) / 64 * 64;
    CHK(dalloc(c, &k.G, (int64_t)c->world * c->chunk * d));
    CHK(dalloc(c, &k.mu, 64));
    CHK(dalloc(c, &k.mpart, (int64_t)KSD_MEAN_BLOCKS * d));
    if (d <= 16) {
        CHK(dalloc(c, &k.rec, k.np * ksd_rec_stride(d)));
    } else {
        CHK(dalloc(c, &k.xt, k.np * ksd_kp(d)));
        CHK(dalloc(c, &k.vt, k.np * ksd_kp(d)));
    }
    CHK(dalloc(c, &k.nrm, k.np));
    CHK(dalloc(c, &k.cvec, k.np));
    CHK(dalloc(c, &k.diag, k.np));
    CHK(dalloc(c, &k.part, (int64_t)k.S * k.ldp));
    CHK(dalloc(c, &k.rows, k.ldp));
    CHK(dalloc(c, &k.bpart, 2 * ((k.ldp + KSD_FIN_THREADS - 1) / KSD_FIN_THREADS)));
    CHK(dalloc(c, &k.out, 2));
    k.ready = true;
    return SVGD_OK;
}

int ksd_imq_alloc(svgd_ctx *c)
{
    svgd_ctx::KsdImq &k = c->ksdq;
    if (k.ready) return SVGD_OK;
    const int d = c->dim;
    // column splits as above: the grid fills the resident slots at most twice
    const int64_t groups = std::max<int64_t>(1, (c->nrows + KSD_IMQ_ROWS_PER_WG - 1) / KSD_IMQ_ROWS_PER_WG);
    int cus = 0;
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const int64_t resident = (int64_t)std::max(1, cus) * ksd_imq_blocks_per_cu(d);
    k.S = (int)std::min<int64_t>(std::max<int64_t>(1, 2 * resident / groups), ksd_imq_tiles(d, c->n));
    k.ldp = (std::max<int64_t>(1, c->nrows) + 63) / 64 * 64;
    const int64_t np = ksd_imq_padded(c->n);
    CHK(dalloc(c, &k.G, (int64_t)c->world * c->chunk * d));
    CHK(dalloc(c, &k.mu, 64));
    CHK(dalloc(c, &k.mpart, (int64_t)KSD_MEAN_BLOCKS * d));
    CHK(dalloc(c, &k.rec, np * ksd_imq_rec_stride(d)));
    CHK(dalloc(c, &k.diag, np));
    CHK(dalloc(c, &k.part, (int64_t)k.S * k.ldp));
    CHK(dalloc(c, &k.rows, k.ldp));
    CHK(dalloc(c, &k.bpart, 2 * ((k.ldp + KSD_FIN_THREADS - 1) / KSD_FIN_THREADS)));
    CHK(dalloc(c, &k.out, 2));
    k.ready = true;
    return SVGD_OK;
}

int ksd_check(svgd_ctx *c, const double *G_shard, double a)
{
    CHK(check_results(c));
    if (!std::isfinite(a) || !(a > 0.0))
        return fail(c, SVGD_ERR_ARG, "[Argument Error] The KSD kernel scale must be finite and positive.");
    if (!G_shard && !has_device_model(c))
        return fail(c, SVGD_ERR_ARG,
                    "[Argument Error] Null log-gradient buffer and no device model set.");
    return SVGD_OK;
}

// What the two statistics share: the scores of this rank's rows into G (from
// the host or the device model) and their all-gather, passes() (centre, prep,
// pairs, finish: rows, and out = [sum_i row_i, sum_i u_ii] of this rank), the
// all-reduce of out and the results.
template <class Passes>
int ksd_run(svgd_ctx *c, const double *G_shard, double *G, const double *rows, double *out,
            double *ksd2_v, double *ksd2_u, double *rows_shard_out, Passes passes)
{
    const int d = c->dim;
    const size_t off = (size_t)c->row0 * d, bytes = sizeof(double) * (size_t)c->nrows * d;
    // work is queued behind the step's marks: they no longer end the stream
    c->mark = c->phi_end = c->last_phi_end = nullptr;
    if (G_shard) {
        if (c->nrows > 0)
            HIPCHK(c, hipMemcpyAsync(G + off, G_shard, bytes, hipMemcpyHostToDevice, c->stream));
    } else {
        CHK(launch_device_model_grad(c, c->X + off, c->nrows, G + off));
    }
    // the observer's collectives stay out of the step's collective hash and
    // of the level-2 diagnostic spans
    const uint64_t sig = c->co.coll_sig;
    const int tlevel = c->tm.tlevel;
    c->tm.tlevel = 0;
    int rc = allgather_rows(c, G);
    if (rc == SVGD_OK) {
        const hipError_t e = passes();
        if (e != hipSuccess)
            rc = fail(c, SVGD_ERR_HIP, std::string("[HIP Error] KSD pass: ") + hipGetErrorString(e));
    }
    if (rc == SVGD_OK) rc = allreduce_f64(c, out, 2);
    c->tm.tlevel = tlevel;
    c->co.coll_sig = sig;
    CHK(rc);
    double sums[2] = {0.0, 0.0};
    HIPCHK(c, hipMemcpyAsync(sums, out, sizeof(sums), hipMemcpyDeviceToHost, c->stream));
    if (rows_shard_out && c->nrows > 0)
        HIPCHK(c, hipMemcpyAsync(rows_shard_out, rows, sizeof(double) * (size_t)c->nrows,
                                 hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // sums = [sum_i row_i, sum_i u_ii] over all ranks
    const double N = (double)c->n;
    if (ksd2_v) *ksd2_v = sums[0] / N;
    if (ksd2_u) *ksd2_u = c->n < 2 ? NAN : (N * sums[0] - sums[1]) / (N * (N - 1.0));
    return SVGD_OK;
}

int ksd_imq(svgd_ctx *c, const double *G_shard, double a, double *ksd2_v, double *ksd2_u,
            double *rows_shard_out)
{
    CHK(ksd_check(c, G_shard, a));
    if (c->dim > 64)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] The inverse multiquadric kernel supports d <= 64.");
    CHK(resolve_pending(c));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ksd_imq_alloc(c));
    svgd_ctx::KsdImq &k = c->ksdq;
    const int d = c->dim;
    return ksd_run(c, G_shard, k.G, k.rows, k.out, ksd2_v, ksd2_u, rows_shard_out, [&]() {
        hipError_t e = launch_ksd_mean(c->X, c->n, d, k.mpart, k.mu, c->stream);
        if (e == hipSuccess) e = launch_ksd_imq_prep(d, c->X, k.G, k.mu, a, c->n, k.rec, k.diag, c->stream);
        if (e == hipSuccess)
            e = launch_ksd_imq_pass(d, a, k.rec, k.diag, c->row0, c->nrows, c->n, k.S, k.part, k.ldp,
                                    c->stream);
        if (e == hipSuccess)
            e = launch_ksd_finish(k.part, k.S, k.ldp, c->nrows, 1.0 / (double)c->n, k.diag + c->row0,
                                  k.rows, k.bpart, k.out, c->stream);
        return e;
    });
}

} // namespace

} // namespace svgd_amd

extern "C" {

int svgd_ksd(svgd_ctx *c, const double *G_shard, double a, double *ksd2_v, double *ksd2_u,
             double *rows_shard_out)
{
    CHK(ksd_check(c, G_shard, a));
    CHK(resolve_pending(c));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ksd_alloc(c));
    svgd_ctx::Ksd &k = c->ksd;
    const int d = c->dim;
    return ksd_run(c, G_shard, k.G, k.rows, k.out, ksd2_v, ksd2_u, rows_shard_out, [&]() {
        hipError_t e = launch_ksd_mean(c->X, c->n, d, k.mpart, k.mu, c->stream);
        if (e == hipSuccess)
            e = launch_ksd_prep(c->X, k.G, k.mu, a, c->n, k.np, d, k.rec, k.xt, k.vt, k.nrm, k.cvec,
                                k.diag, c->stream);
        if (e == hipSuccess)
            e = launch_ksd_pairs(d, a, k.rec, k.xt, k.vt, k.nrm, k.cvec, k.diag, c->row0, c->nrows, c->n,
                                 k.np, k.S, k.part, k.ldp, c->stream);
        if (e == hipSuccess)
            e = launch_ksd_finish(k.part, k.S, k.ldp, c->nrows, 1.0 / (double)c->n, k.diag + c->row0,
                                  k.rows, k.bpart, k.out, c->stream);
        return e;
    });
}

int svgd_ksd_kernel(svgd_ctx *c, int kernel, const double *G_shard, double a, double *ksd2_v,
                    double *ksd2_u, double *rows_shard_out)
{
    if (kernel == SVGD_KERNEL_RBF) return svgd_ksd(c, G_shard, a, ksd2_v, ksd2_u, rows_shard_out);
    if (kernel == SVGD_KERNEL_IMQ) return ksd_imq(c, G_shard, a, ksd2_v, ksd2_u, rows_shard_out);
    if (!c) return SVGD_ERR_ARG;
    return fail(c, SVGD_ERR_ARG, "[Argument Error] Unknown KSD kernel.");
}

} // extern "C"
