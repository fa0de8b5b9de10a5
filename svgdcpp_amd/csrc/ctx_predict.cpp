// ctx_predict.cpp -- svgd_glm_predict: the posterior predictive of a generalized
// linear model on held-out records at the context's particles, an observer
// with work arrays of its own.
#include "ctx.h"
#include <algorithm>
#include <new>
#include "svgd_ksd.h"
#include "svgd_glm_predict.h"
#include "host_glm.h"

using namespace svgd_amd;

namespace svgd_amd {
namespace {

// the work arrays for m records in S splits: allocated on first use, grown
// when a call needs more
int predict_alloc(svgd_ctx *c, int64_t m, int64_t part_need)
{
    svgd_ctx::Predict &p = c->pred;
    const int d = c->dim;
    if (!p.mu) {
        CHK(dalloc(c, &p.mu, 64));
        CHK(dalloc(c, &p.mpart, (int64_t)KSD_MEAN_BLOCKS * d));
    }
    const int64_t rec_need = glm_padded(m) * glm_rec_stride(d);
    if (rec_need > p.rec_cap) {
        CHK(dalloc(c, &p.rec, rec_need));
        p.rec_cap = rec_need;
    }
    if (m > p.m_cap) {
        CHK(dalloc(c, &p.cvec, m));
        CHK(dalloc(c, &p.sums, 3 * m));
        p.m_cap = m;
    }
    if (part_need > p.part_cap) {
        CHK(dalloc(c, &p.part, part_need));
        p.part_cap = part_need;
    }
    return SVGD_OK;
}

} // namespace
} // namespace svgd_amd

extern "C" {

int svgd_glm_predict(svgd_ctx *c, int link, double lik_scale, const double *A, const double *y, int64_t m,
                     double *mean_out, double *var_out, double *lpd_out)
{
    CHK(check_results(c));
    const int d = c->dim;
    if (lpd_out && !y)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] The log predictive density needs labels.");
    const int ok = glm_predict_check(link, lik_scale, d, A, y, m, lpd_out);
    if (ok == SVGD_ERR_DIM)
        return fail(c, SVGD_ERR_DIM, "[Dimension Error] Prediction needs at least one test row.");
    if (ok != SVGD_OK)
        return fail(c, ok,
                    "[Argument Error] Prediction: the test data must be finite, logistic labels in [0, 1], "
                    "the link known and lik_scale > 0.");
    if (d > 64) return fail(c, SVGD_ERR_ARG, "[Argument Error] Device prediction supports d <= 64.");
    CHK(resolve_pending(c));
    HIPCHK(c, hipSetDevice(c->device));
    svgd_ctx::Predict &p = c->pred;
    const int has_y = y ? 1 : 0, nq = 2 + has_y;
    const int RS = glm_rec_stride(d), KP = glm_kp(d);
    // padded records [a | 0 .. | y | 0 ..]; the tile past the data stays zero
    std::vector<double> rec, down;
    try {
        rec.assign((size_t)glm_padded(m) * RS, 0.0);
        down.assign((size_t)(nq + 1) * m, 0.0);
    } catch (const std::bad_alloc &) {
        return fail(c, SVGD_ERR_RUNTIME, "[Runtime Error] Prediction records: out of memory.");
    }
    for (int64_t j = 0; j < m; ++j) {
        std::copy(A + (size_t)j * d, A + (size_t)(j + 1) * d, rec.data() + (size_t)j * RS);
        if (y) rec[(size_t)j * RS + KP] = y[j];
    }
    // particle splits: record groups x S fills the resident slots at most
    // twice (as launch_device_model_hess sizes the weight pass)
    if (p.cus == 0) {
        HIPCHK(c, hipDeviceGetAttribute(&p.cus, hipDeviceAttributeMultiprocessorCount, c->device));
        p.cus = std::max(1, p.cus);
    }
    const int64_t resident = (int64_t)p.cus * glm_predict_blocks_per_cu(d, link, has_y);
    const int64_t groups = glm_wgroups(m);
    const int S = (int)std::min<int64_t>(std::max<int64_t>(1, 2 * resident / groups),
                                         std::max<int64_t>(1, glm_tiles(c->nrows)));
    CHK(predict_alloc(c, m, (int64_t)S * 3 * groups * GLM_ROWS_PER_WG));
    // work is queued behind the step's marks: they no longer end the stream
    c->mark = c->phi_end = c->last_phi_end = nullptr;
    HIPCHK(c, hipMemcpyAsync(p.rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice, c->stream));
    // the centre: the mean of all N particles in a fixed order (X is the full
    // matrix on every rank, so every rank forms the same bits)
    hipError_t e = launch_ksd_mean(c->X, c->n, d, p.mpart, p.mu, c->stream);
    if (e == hipSuccess) e = launch_glm_predict_center(d, link, p.rec, m, p.mu, p.cvec, c->stream);
    // an empty shard launches nothing and contributes zeros
    if (e == hipSuccess)
        e = launch_glm_predict(d, link, has_y, 0.5 * lik_scale, c->X + (size_t)c->row0 * d, c->nrows, p.rec,
                               p.cvec, m, S, p.part, p.sums, c->stream);
    if (e != hipSuccess)
        return fail(c, SVGD_ERR_HIP, std::string("[HIP Error] GLM prediction: ") + hipGetErrorString(e));
    // the observer's collective stays out of the step's collective hash and
    // of the level-2 diagnostic spans
    const uint64_t sig = c->co.coll_sig;
    const int tlevel = c->tm.tlevel;
    c->tm.tlevel = 0;
    const int rc = allreduce_f64(c, p.sums, (size_t)nq * m);
    c->tm.tlevel = tlevel;
    c->co.coll_sig = sig;
    CHK(rc);
    HIPCHK(c, hipMemcpyAsync(down.data(), p.sums, sizeof(double) * (size_t)nq * m, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(down.data() + (size_t)nq * m, p.cvec, sizeof(double) * (size_t)m,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the formulas after the all-reduce: every rank ends with the same bits
    const double N = (double)c->n, lconst = glm_predict_lconst(link, lik_scale);
    const double *sa = down.data(), *sb = sa + m, *sl = has_y ? sb + m : nullptr, *cv = down.data() + (size_t)nq * m;
    for (int64_t j = 0; j < m; ++j)
        glm_predict_finalize(cv[j], sa[j], sb[j], sl ? sl[j] : 0.0, N, lconst, mean_out ? mean_out + j : nullptr,
                             var_out ? var_out + j : nullptr, lpd_out ? lpd_out + j : nullptr);
    return SVGD_OK;
}

} // extern "C"
