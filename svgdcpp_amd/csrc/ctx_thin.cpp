// ctx_thin.cpp -- svgd_stein_thin: Stein thinning of the current particles
// (svgd_thin.hip), an observer with work arrays of its own in the standing of
// svgd_ksd_kernel (ctx_ksd.cpp): the same front -- this rank's scores into G
// from the host or the device model, their all-gather -- then the whole
// selection on every rank, redundantly, on the full X and G.
#include "ctx.h"
#include <cmath>
#include <vector>
#include "svgd_thin.h"

using namespace svgd_amd;

namespace svgd_amd {
namespace {

int thin_alloc(svgd_ctx *c, int64_t m)
{
    svgd_ctx::Thin &k = c->thin;
    const int d = c->dim;
    if (!k.ready) {
        const int64_t np = thin_padded(c->n);
        CHK(dalloc(c, &k.G, (int64_t)c->world * c->chunk * d));
        CHK(dalloc(c, &k.xs, 2 * d * np));
        CHK(dalloc(c, &k.diag, np));
        CHK(dalloc(c, &k.acc, np));
        CHK(dalloc(c, &k.pval, thin_part_slots(c->n)));
        CHK(dalloc(c, &k.pidx, thin_part_slots(c->n)));
        k.ready = true;
    }
    if (m > k.m_cap) {
        // (the stream's earlier picks no longer read the old arrays)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        CHK(dalloc(c, &k.idx, m));
        CHK(dalloc(c, &k.S, m));
        k.m_cap = m;
    }
    return SVGD_OK;
}

} // namespace
} // namespace svgd_amd

extern "C" int svgd_stein_thin(svgd_ctx *c, int kernel, const double *G_shard, double a, int64_t m,
                               int64_t *idx_out, double *ksd2_out)
{
    CHK(check_results(c));
    if (kernel != SVGD_KERNEL_RBF && kernel != SVGD_KERNEL_IMQ)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Unknown Stein thinning kernel.");
    if (!std::isfinite(a) || !(a > 0.0))
        return fail(c, SVGD_ERR_ARG, "[Argument Error] The Stein thinning kernel scale must be finite and positive.");
    if (m < 1) return fail(c, SVGD_ERR_ARG, "[Argument Error] Stein thinning needs at least one pick.");
    if (!G_shard && !has_device_model(c))
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Null log-gradient buffer and no device model set.");
    if (c->dim > 64) return fail(c, SVGD_ERR_ARG, "[Argument Error] Stein thinning supports d <= 64.");
    if (c->n > THIN_MAX_N)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Stein thinning supports fewer than 2^31 - 256 particles.");
    CHK(resolve_pending(c));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(thin_alloc(c, m));
    svgd_ctx::Thin &k = c->thin;
    const int d = c->dim;
    const size_t off = (size_t)c->row0 * d, bytes = sizeof(double) * (size_t)c->nrows * d;
    // work is queued behind the step's marks: they no longer end the stream
    c->mark = c->phi_end = c->last_phi_end = nullptr;
    if (G_shard) {
        if (c->nrows > 0)
            HIPCHK(c, hipMemcpyAsync(k.G + off, G_shard, bytes, hipMemcpyHostToDevice, c->stream));
    } else {
        CHK(launch_device_model_grad(c, c->X + off, c->nrows, k.G + off));
    }
    // the observer's collective stays out of the step's collective hash and of
    // the level-2 diagnostic spans
    const uint64_t sig = c->co.coll_sig;
    const int tlevel = c->tm.tlevel;
    c->tm.tlevel = 0;
    const int rc = allgather_rows(c, k.G);
    c->tm.tlevel = tlevel;
    c->co.coll_sig = sig;
    CHK(rc);
    const bool imq = kernel == SVGD_KERNEL_IMQ;
    const ThinArgs w{c->X, k.G, k.xs, k.diag, k.acc, k.pval, k.pidx, k.idx, k.S};
    hipError_t e = launch_thin_prep(imq, d, c->n, a, w, c->stream);
    if (e == hipSuccess) e = launch_thin_picks(imq, d, c->n, a, m, c->knobs.thin_select.or_(0) != 0, w, c->stream);
    if (e != hipSuccess)
        return fail(c, SVGD_ERR_HIP, std::string("[HIP Error] Stein thinning: ") + hipGetErrorString(e));
    std::vector<int64_t> idx((size_t)m);
    std::vector<double> S((size_t)m);
    HIPCHK(c, hipMemcpyAsync(idx.data(), k.idx, sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.data(), k.S, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bool finite = true;
    for (int64_t t = 1; t <= m; ++t) {
        const double ksd2 = S[(size_t)t - 1] / ((double)t * (double)t);
        finite = finite && std::isfinite(ksd2);
        if (idx_out) idx_out[t - 1] = idx[(size_t)t - 1];
        if (ksd2_out) ksd2_out[t - 1] = ksd2;
    }
    if (!finite) return fail(c, SVGD_ERR_RUNTIME, "[Runtime Error] Stein thinning: a KSD value is not finite.");
    return SVGD_OK;
}
