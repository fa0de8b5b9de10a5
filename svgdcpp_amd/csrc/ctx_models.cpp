// ctx_models.cpp -- the device models (Gaussian sum, GLM): their mirrors, gradient
// and Hessian-sum launches and entry points.
#include "ctx.h"
#include <algorithm>
#include <new>
#include "svgd_glm.h"
#include "svgd_gauss_hess.h"
#include "host_models.h"
#include "host_glm.h"

using namespace svgd_amd;

namespace svgd_amd {

// grad log p of the device model -- the Gaussian sum or the GLM, whichever is
// set -- at `rows` particles X (stride d) -> G, fp64, on the context's stream
int launch_device_model_grad(svgd_ctx *c, const double *X, int64_t rows, double *G)
{
    if (c->dm.glm.m > 0) {
        const svgd_ctx::DeviceModels::Glm &g = c->dm.glm;
        const int S = (int)std::min<int64_t>(g.smax, glm_tiles(g.count));
        HIPCHK(c, launch_glm_pass(c->dim, g.link, X, rows, g.rec, g.m0, g.count, S, g.part, g.ldp,
                                  c->stream));
        HIPCHK(c, launch_glm_finish(c->dim, X, rows, g.part, S, g.ldp,
                                    g.lik_scale * ((double)g.m / (double)g.count), g.prior_prec, G,
                                    c->stream));
        return SVGD_OK;
    }
    HIPCHK(c, launch_gauss_grad(X, rows, c->dim, c->dm.k, c->dm.mu, c->dm.prec, G, c->stream));
    return SVGD_OK;
}

// sum_i -hess log p(x_i) of the device model over `rows` particles X (stride
// d) -> H (d x d, device), fp64, on the context's stream; rows == 0: zeros
int launch_device_model_hess(svgd_ctx *c, const double *X, int64_t rows, double *H)
{
    const int d = c->dim;
    if (c->dm.glm.m > 0) {
        const svgd_ctx::DeviceModels::Glm &g = c->dm.glm;
        if (rows <= 0) {
            HIPCHK(c, hipMemsetAsync(H, 0, sizeof(double) * (size_t)d * d, c->stream));
            return SVGD_OK;
        }
        const bool logistic = g.link == SVGD_GLM_LOGISTIC;
        if (logistic) {
            // particle splits: record groups x S fills the resident slots at
            // most twice (as svgd_set_device_glm sizes the score's splits)
            const int64_t groups = glm_wgroups(g.count);
            const int S = (int)std::min<int64_t>(std::max<int64_t>(1, 2 * c->dm.hess.resident / groups),
                                                 glm_tiles(rows));
            HIPCHK(c, launch_glm_weights(d, X, rows, g.rec, g.m0, g.count, S, c->dm.hess.wpart, c->dm.hess.W,
                                         c->stream));
        }
        HIPCHK(c, launch_glm_wgram(d, g.rec, g.m0, g.count, logistic ? c->dm.hess.W : nullptr, (double)rows,
                                   g.lik_scale * ((double)g.m / (double)g.count),
                                   g.prior_prec * (double)rows, c->dm.hess.part, H, c->stream));
        return SVGD_OK;
    }
    HIPCHK(c, launch_gauss_hess_sum(X, rows, d, c->dm.k, c->dm.mu, c->dm.prec, c->dm.hess.part, H, c->stream));
    return SVGD_OK;
}

} // namespace svgd_amd

extern "C" {

int svgd_set_device_model(svgd_ctx *c, const void *model)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    if (!model) {
        c->dm.k = 0;
        return SVGD_OK;
    }
    const HostModel *m = static_cast<const HostModel *>(model);
    if (m->d != c->dim)
        return fail(c, SVGD_ERR_DIM, "[Dimension Error] Model dimension does not match the particles.");
    if (m->d > 64)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Device model supports d <= 64.");
    CHK(dalloc(c, &c->dm.mu, (int64_t)m->k * m->d));
    CHK(dalloc(c, &c->dm.prec, (int64_t)m->k * m->d * m->d));
    HIPCHK(c, hipMemcpyAsync(c->dm.mu, m->mu.data(), sizeof(double) * m->mu.size(),
                             hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dm.prec, m->prec.data(), sizeof(double) * m->prec.size(),
                             hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    CHK(dalloc(c, &c->dm.hess.part, (int64_t)gauss_hess_grid(c->nrows) * m->d * m->d));
    CHK(dalloc(c, &c->dm.hess.out, (int64_t)m->d * m->d));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->dm.k = m->k;
    c->dm.glm.m = 0; // the two device models exclude each other
    return SVGD_OK;
}

int svgd_set_device_glm(svgd_ctx *c, const void *glm)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    if (!glm) {
        c->dm.glm.m = 0;
        return SVGD_OK;
    }
    const HostGlm *m = static_cast<const HostGlm *>(glm);
    if (m->d != c->dim)
        return fail(c, SVGD_ERR_DIM, "[Dimension Error] Model dimension does not match the particles.");
    if (m->d > 64)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Device model supports d <= 64.");
    HIPCHK(c, hipSetDevice(c->device));
    svgd_ctx::DeviceModels::Glm &g = c->dm.glm;
    g.m = 0;
    const int d = m->d, RS = glm_rec_stride(d), KP = glm_kp(d);
    // padded records [a | 0 .. | y | 0 ..]; the tile past the data stays zero
    std::vector<double> rec;
    try {
        rec.assign((size_t)glm_padded(m->m) * RS, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(c, SVGD_ERR_RUNTIME, "[Runtime Error] Device GLM records: out of memory.");
    }
    for (int64_t j = 0; j < m->m; ++j) {
        std::copy(m->A.data() + (size_t)j * d, m->A.data() + (size_t)(j + 1) * d, rec.data() + (size_t)j * RS);
        rec[(size_t)j * RS + KP] = m->y[(size_t)j];
    }
    // data splits: the work-groups take equal time, so the grid (row groups x
    // S) should fill the device's resident slots a whole number of times, at
    // most twice (as ksd_alloc sizes its column splits); a launch uses
    // min(smax, tiles of its window)
    const int64_t groups = std::max<int64_t>(1, (c->nrows + GLM_ROWS_PER_WG - 1) / GLM_ROWS_PER_WG);
    int cus = 0;
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const int64_t resident = (int64_t)std::max(1, cus) * glm_blocks_per_cu(d, m->link);
    g.smax = (int)std::min<int64_t>(std::max<int64_t>(1, 2 * resident / groups), glm_tiles(m->m));
    g.ldp = std::max<int64_t>(1, c->nrows);
    CHK(dalloc(c, &g.rec, (int64_t)rec.size()));
    CHK(dalloc(c, &g.part, (int64_t)g.smax * g.ldp * d));
    // the Hessian sum's work areas, for any window of these data: the weight
    // pass launches record groups x S <= max(2 resident, groups) work-groups
    c->dm.hess.resident = (int64_t)std::max(1, cus) * glm_wpass_blocks_per_cu(d);
    CHK(dalloc(c, &c->dm.hess.wpart,
               std::max<int64_t>(2 * c->dm.hess.resident, glm_wgroups(m->m)) * GLM_ROWS_PER_WG));
    CHK(dalloc(c, &c->dm.hess.W, glm_wgroups(m->m) * GLM_ROWS_PER_WG));
    CHK(dalloc(c, &c->dm.hess.part, (int64_t)glm_gram_grid(m->m) * (d * (d + 1) / 2)));
    CHK(dalloc(c, &c->dm.hess.out, (int64_t)d * d));
    HIPCHK(c, hipMemcpyAsync(g.rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    g.link = m->link;
    g.lik_scale = m->lik_scale;
    g.prior_prec = m->prior_prec;
    g.m0 = m->m0;
    g.count = m->count;
    g.m = m->m;
    c->dm.k = 0; // the two device models exclude each other
    return SVGD_OK;
}

int svgd_set_device_glm_batch(svgd_ctx *c, int64_t m0, int64_t count)
{
    if (!c) return SVGD_ERR_ARG;
    if (c->dm.glm.m == 0) return fail(c, SVGD_ERR_UNSET, "[Unset Error] No device GLM set.");
    if (m0 < 0 || count < 1 || m0 > c->dm.glm.m || count > c->dm.glm.m - m0)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Batch window outside the data.");
    CHK(resolve_pending(c));
    c->dm.glm.m0 = m0;
    c->dm.glm.count = count;
    return SVGD_OK;
}

int svgd_device_logp_grad(svgd_ctx *c, double *G_shard_out)
{
    CHK(check_ready(c));
    CHK(resolve_pending(c));
    if (!has_device_model(c)) return fail(c, SVGD_ERR_UNSET, "[Unset Error] No device model set.");
    if (!G_shard_out) return fail(c, SVGD_ERR_ARG, "[Argument Error] Null output buffer.");
    CHK(launch_device_model_grad(c, c->X + (size_t)c->row0 * c->dim, c->nrows, c->phi));
    HIPCHK(c, hipMemcpyAsync(G_shard_out, c->phi, sizeof(double) * (size_t)c->nrows * c->dim,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SVGD_OK;
}

int svgd_device_neg_hess_sum(svgd_ctx *c, double *H_shard_out)
{
    CHK(check_ready(c));
    CHK(resolve_pending(c));
    if (!has_device_model(c)) return fail(c, SVGD_ERR_UNSET, "[Unset Error] No device model set.");
    if (!H_shard_out) return fail(c, SVGD_ERR_ARG, "[Argument Error] Null output buffer.");
    HIPCHK(c, hipSetDevice(c->device));
    // work is queued behind the step's marks: they no longer end the stream
    c->mark = c->phi_end = c->last_phi_end = nullptr;
    CHK(launch_device_model_hess(c, c->X + (size_t)c->row0 * c->dim, c->nrows, c->dm.hess.out));
    HIPCHK(c, hipMemcpyAsync(H_shard_out, c->dm.hess.out, sizeof(double) * (size_t)c->dim * c->dim,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SVGD_OK;
}

int svgd_set_device_hessian(svgd_ctx *c, int on)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    c->dm.hess.on = on != 0;
    return SVGD_OK;
}

} // extern "C"
