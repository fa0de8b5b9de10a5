// ctx_phi.cpp -- G's upload and all-gather, phi_hat on the planned path (with the
// fused optimizer update) and the kernel scale's setters and getters.
#include "ctx.h"
#include "svgd_imq.h"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace svgd_amd;

namespace svgd_amd {
namespace {

// This step's optimizer arguments (advances t: call once per step).
int opt_args(svgd_ctx *c, OptArgs *o)
{
    if (c->opt_kind < 0)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Invalid Optimizer object pointer.");
    c->t += 1;
    double c1 = 1.0, c2 = 1.0;
    if (c->opt_kind == SVGD_OPT_ADAM) {
        c1 = 1.0 - std::pow(c->b1, (double)c->t);
        c2 = 1.0 - std::pow(c->b2, (double)c->t);
    }
    const size_t off = (size_t)c->row0 * c->dim;
    *o = OptArgs{c->opt_kind, c->dim, c->nrows * c->dim, c->m, c->v, c->X + off, c->lr, c->b1,
                 c->b2, c->eps, c1, c2, c->bounded ? c->lower : nullptr,
                 c->bounded ? c->upper : nullptr,
                 // X_t, m_t, v_t of this rank's rows for a redo if the device plan failed
                 c->spec_step ? c->bak : nullptr,
                 // the next host gradient's X_{t+1}
                 c->hs.in_host_step && c->hs.xmirror ? c->hs.h_xm_dev : nullptr};
    return SVGD_OK;
}

int alloc_matrix_scale(svgd_ctx *c)
{
    if (c->ms.M) return SVGD_OK;
    const int64_t dd = (int64_t)c->dim * c->dim;
    CHK(dalloc(c, &c->ms.src, dd));
    CHK(dalloc(c, &c->ms.M, dd));
    CHK(dalloc(c, &c->ms.L, dd));
    CHK(dalloc(c, &c->ms.sgn, c->dim));
    CHK(dalloc(c, &c->ms.work, 2 * dd));
    CHK(dalloc(c, &c->ms.wv, c->np * c->dim));
    if (!c->rowpath) CHK(dalloc(c, &c->ms.zc, c->np * c->plan.KP));
    if (c->dtype == SVGD_F32) CHK(dalloc(c, &c->ms.zcf, c->np * c->plan.KP));
    CHK(dalloc(c, &c->ms.err, 1));
    HIPCHK(c, c->ms.h_err.alloc(1, hipHostMallocDefault));
    *c->ms.h_err = 0;
    return SVGD_OK;
}

const char *const IMQ_SCALE_MSG =
    "[Argument Error] The inverse multiquadric kernel takes a scalar scale (median or fixed), not a "
    "Hessian or matrix scale.";

// The IMQ pass's records and partials (the first svgd_set_kernel(IMQ)).
// Column splits: the work-groups take equal time, so the grid (row groups x
// S) should fill the device's resident slots a whole number of times, at most
// twice (as svgd_set_device_glm sizes the score's splits).
int alloc_imq(svgd_ctx *c)
{
    svgd_ctx::Imq &q = c->imq;
    if (q.ready) return SVGD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const int d = c->dim;
    const int64_t groups = std::max<int64_t>(1, (c->nrows + IMQ_ROWS_PER_WG - 1) / IMQ_ROWS_PER_WG);
    int cus = 0;
    HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const int64_t resident = (int64_t)std::max(1, cus) * imq_blocks_per_cu(d);
    q.S = (int)std::min<int64_t>(std::max<int64_t>(1, 2 * resident / groups), imq_tiles(d, c->n));
    q.ldp = std::max<int64_t>(1, c->nrows);
    CHK(dalloc(c, &q.rec, imq_padded(c->n) * imq_rec_stride(d)));
    CHK(dalloc(c, &q.part, (int64_t)q.S * q.ldp * imq_part_width(d)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    q.ready = true;
    return SVGD_OK;
}

} // namespace

// G shard -> device on the copy stream (ready at ev_g) ...
int upload_g_begin(svgd_ctx *c, const double *G_shard)
{
    const size_t bytes = sizeof(double) * (size_t)c->nrows * c->dim;
    if (!G_shard) return fail(c, SVGD_ERR_ARG, "[Argument Error] Null log-gradient buffer.");
    if (c->nrows > 0) {
        if (G_shard != c->h_g) {
            HIPCHK(c, hipEventSynchronize(c->ev_g)); // the previous upload left h_g
            std::memcpy(c->h_g, G_shard, bytes);
        }
        // the last phi chain may still read G on the compute stream: a step
        // returns with it queued, and a redo (resolve_pending) inside this
        // very call has just queued one that needs the failed step's G
        hipEvent_t xev = c->ev_xready_use ? c->ev_xready_use : c->ev_xready;
        if (hipEventQuery(xev) != hipSuccess) HIPCHK(c, hipStreamWaitEvent(c->cstream, xev, 0));
        HIPCHK(c, hipMemcpyAsync(c->G + (size_t)c->row0 * c->dim, c->h_g, bytes,
                                 hipMemcpyHostToDevice, c->cstream));
    }
    HIPCHK(c, hipEventRecord(c->ev_g, c->cstream));
    return SVGD_OK;
}

// ... and the all-gather of the shards.  With a G communicator (P > 1 over
// RCCL) it runs on its own stream as soon as the shard has landed, beside the
// median chain, and the phi chain waits for it (run_phi); otherwise on the
// compute stream once it needs G.
int upload_g_finish(svgd_ctx *c)
{
    if (c->co.gcomm) {
        // the issue-order invariant (svgd_ctx): with a median pending, every
        // comm call of scale_begin precedes this gcomm call on every rank
        if (c->median_pending && c->co.coll_phase != 1)
            return fail(c, SVGD_ERR_RUNTIME,
                        "[Runtime Error] G all-gather issued before the median's collectives "
                        "(cross-communicator issue order).");
        c->co.coll_phase = 2;
        if (hipEventQuery(c->ev_g) != hipSuccess) HIPCHK(c, hipStreamWaitEvent(c->co.gstream, c->ev_g, 0));
        CHK(allgather_rows_on(c, c->G, c->co.gcomm, c->co.gstream, DG_GATHER_G));
        HIPCHK(c, hipEventRecord(c->co.ev_gg, c->co.gstream));
        c->co.gg_pending = true;
        return SVGD_OK;
    }
    // a G copy that has already landed needs no cross-queue barrier (a wait
    // on the copy stream's signal cost a ~25 us dispatch gap before the
    // record prep even when the copy had finished long before)
    if (hipEventQuery(c->ev_g) != hipSuccess) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_g, 0));
    CHK(allgather_rows(c, c->G));
    return SVGD_OK;
}

int upload_g(svgd_ctx *c, const double *G_shard)
{
    CHK(upload_g_begin(c, G_shard));
    return upload_g_finish(c);
}

int run_phi(svgd_ctx *c, const OptArgs *opt)
{
    // phi phase: the record preparation (V = G - 2a xc, part of the
    // reference's ComputePhi) through the reduce (+ the fused update); the
    // start event goes before the preparation -- an event between two
    // kernels costs a dispatch gap
    EvPair ev{};
    if (c->tm.timing) {
        ev = take_pair(c);
        if (c->mark) { // the median's end event, nothing queued since
            ev.spare = ev.a;
            ev.a = c->mark;
        } else {
            HIPCHK(c, hipEventRecord(ev.a, c->stream));
        }
    }
    // level 2: the device's wait between the median's end and the phi chain
    // (the host gradient, the G copies and, P > 1, the G all-gather)
    hipEvent_t med_end = c->tm.tlevel >= 2 ? c->tm.med_end_ev : nullptr;
    c->tm.med_end_ev = nullptr;
    c->mark = nullptr;
    if (c->co.gg_pending) {
        if (hipEventQuery(c->co.ev_gg) != hipSuccess) HIPCHK(c, hipStreamWaitEvent(c->stream, c->co.ev_gg, 0));
        c->co.gg_pending = false;
    }
    if (med_end) diag_end(c, c->stream, med_end, DG_PHI_WAIT, true);
    // The inverse multiquadric kernel, chosen after the plan was made like a
    // matrix scale, replaces the planned chain per call: records from this
    // step's xc and the all-gathered G, the fp64 MFMA pass over this rank's
    // rows against all N columns, the finish.  Nothing keyed on the planned
    // path runs (no row halves, no symmetric exchange); the update is
    // k_opt_update's (run_phi_opt).
    if (imq_kernel(c)) {
        c->hs.xhalf_ready = false;
        const svgd_ctx::Imq &q = c->imq;
        HIPCHK(c, launch_imq_prep(c->dim, c->xc, c->plan.KP, c->G, c->n, q.rec, c->stream));
        hipEvent_t k0 = diag_begin(c, c->stream);
        HIPCHK(c, launch_imq_pass(c->dim, q.rec, c->scal, c->row0, c->nrows, c->n, q.S, q.part, q.ldp,
                                  c->stream));
        diag_end(c, c->stream, k0, DG_PHI_KERNEL, true);
        HIPCHK(c, launch_imq_finish(c->dim, q.rec, c->scal, c->row0, c->nrows, q.part, q.S, q.ldp,
                                    1.0 / (double)c->n, c->phi, c->stream));
        if (c->tm.timing) {
            HIPCHK(c, hipEventRecord(ev.b, c->stream));
            c->tm.ev_phi.push_back(ev);
            c->phi_end = c->last_phi_end = ev.b;
        }
        return SVGD_OK;
    }
    // A matrix scale, chosen after the plan was made, modifies the planned
    // launch per call (matrix_scale_plan): no symmetric pass, the 4-wave row
    // kernel (signature rows, sc_sgn), zc / zcf = L^T xc for xc / xcf, wv = 2 M xc.
    const bool mat = matrix_scale(c);
    const PhiPlan p = mat ? matrix_scale_plan(c->plan) : c->plan;
    const PhiPath path = p.path;
    const RowsKind rows_kind = p.rows_kind;
    if (mat) {
        // M = factor * src, L = chol(M), a_eff = 1 (GaussianRBFKernel.hpp:189-210)
        const double factor = c->scale_method == SVGD_SCALE_HESSIAN
                                  ? 1.0 / (2.0 * (double)c->dim * (double)c->n)
                                  : 1.0;
        HIPCHK(c, launch_scale_factor(c->ms.src, factor, c->dim, c->ms.M, c->ms.L, c->ms.sgn,
                                      c->ms.work, c->scal, c->ms.err, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->ms.h_err, c->ms.err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (!p.rows()) {
            // the MFMA tile kernels need M positive definite: check before phi
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (*c->ms.h_err == 2)
                return fail(c, SVGD_ERR_RUNTIME,
                            "[Runtime Error] The kernel scale matrix is indefinite; the device "
                            "path supports indefinite matrices for fp64 particles with d <= 16 only.");
        }
        if (*c->ms.h_err == 1 && !p.rows())
            return fail(c, SVGD_ERR_RUNTIME, "[Runtime Error] The kernel scale matrix is not finite.");
        if (p.rows())
            HIPCHK(c, launch_prep_rec_mat(c->xc, c->G, c->ms.M, c->ms.L, c->ms.sgn, c->n, c->np,
                                          c->dim, p.KP, c->RS, c->rec, c->ms.wv, c->stream));
        else
            HIPCHK(c, launch_prep_v_mat(c->xc, c->G, c->ms.M, c->ms.L, c->n, c->np, c->dim, p.KP,
                                        p.VW, c->ms.zc, c->V, c->cvec, c->ms.wv, c->stream));
    } else if (path == PHI_ROWS) // (the symmetric pass's prep writes these when it does not apply)
        HIPCHK(c, launch_prep_rec(c->xc, c->G, c->nrm, c->scal, c->n, c->np, c->dim, p.KP, c->RS,
                                  c->rec, c->stream));
    else if (!p.rows())
        HIPCHK(c, launch_prep_v(c->xc, c->G, c->nrm, c->scal, c->n, c->np, c->dim, p.KP, p.VW,
                                c->V, c->cvec, c->stream));
    // F32: the streamed kernels' operand-ordered column copies (k_swz_b3 /
    // k_swz_f32), or the row-major fp32 copies of the generic tile kernel
    const int64_t ntl = (c->n + TBJ_COLS - 1) / TBJ_COLS;
    if (c->dtype == SVGD_F32) {
        if (path == PHI_B3)
            HIPCHK(c, launch_swz_b3(mat ? c->ms.zc : c->xc, p.KP, c->V, p.VW, c->cvec, c->n, ntl, c->B3,
                                    c->stream));
        else if (path == PHI_F32S)
            HIPCHK(c, launch_swz_f32(mat ? c->ms.zc : c->xc, p.KP, c->V, p.VW, c->cvec, ntl, c->XS,
                                     c->VS, c->stream));
        else
            HIPCHK(c, launch_cvt_f32(c->V, c->np * p.VW, c->Vf, c->stream));
        HIPCHK(c, launch_cvt_f32(c->cvec, c->np, c->cvf, c->stream));
        if (mat) HIPCHK(c, launch_cvt_f32(c->ms.zc, c->np * p.KP, c->ms.zcf, c->stream));
    }
    // level 2: the phi kernel alone (k_phi_rows before its reduce, k_phi_sym,
    // or the tile kernel)
    const bool sym = path == PHI_SYM;
    const bool split = path == PHI_ROWS && c->hs.split_rows && c->hs.in_host_step && !mat && opt;
    c->hs.xhalf_ready = split;
    c->n_split += split ? 1 : 0;
    hipEvent_t k0 = sym ? (c->tm.tlevel >= 2 ? take_ev(c) : nullptr) : diag_begin(c, c->stream);
    hipEvent_t k1 = k0 ? take_ev(c) : nullptr;
    const double inv_n = 1.0 / (double)c->n;
    switch (path) {
    case PHI_SYM: {
        clear_marks(c);
        SymArgs sa{c->dim,    c->xc,        p.KP,           c->G,        c->nrm,       c->scal,
                   nmax_cur(c),   c->n,         c->sym.nb,      c->sym.u0,   c->sym.u1,    c->sym.srec,
                   c->sym.ok,  c->sym.rowpart,   c->sym.colpart,     c->sym.grid, c->row0,
                   c->nrows,  inv_n, c->phi, c->rec, c->RS, c->sym.contrib,
                   c->sym.tab, c->sym.tab + 2 * c->sym.nb,
                   c->sym.SM, c->sym.Ia, c->sym.Ib, c->part, c->sym.fS, c->ldp,
                   c->sym.tab + 3 * c->sym.nb, c->sym.qlast, c->sym.tab8k};
        // (when the records' flag says the symmetric form would leave its
        // range, symok = 0, the same launch runs the row stream's work-groups
        // instead; their partials are summed by the finish / k_sym_apply)
        HIPCHK(c, launch_phi_sym(sa, k0, k1, c->stream));
        HIPCHK(c, launch_sym_finish(sa, opt, c->stream));
        if (c->sym.contrib) {
            // every rank's sums of its rows (issued whether or not symok: the
            // ranks' collective sequences must not depend on device data)
            CHK(sym_exchange(c));
            HIPCHK(c, launch_sym_apply(sa, c->sym.contrib + (size_t)c->row0 * (c->dim + 1), c->sym.xrecv_buf, c->sym.xtab_d,
                                       c->sym.xtab_d ? c->world : 1, c->sym.xtab_d ? c->rank : 0, opt, c->stream));
        }
        break;
    }
    case PHI_ROWS:
        if (split) {
            // two row halves: the first half's X_{t+1} is final at ev_xhalf, while
            // the second half's phi runs (svgd_step_host_model copies it down and
            // starts its gradient there)
            const int64_t h = c->hs.split_h, d = c->dim;
            OptArgs o1 = *opt, o2 = *opt;
            o2.X += h * d;
            o2.m += h * d;
            o2.v += h * d;
            if (o2.bak) o2.bak += h * d;
            if (o2.xh) o2.xh += h * d;
            HIPCHK(c, launch_phi_rows(c->dim, rows_kind, c->rec, c->scal, c->row0, h, c->n, c->hs.S2, c->part, h,
                                      inv_n, nullptr, nullptr, nmax_cur(c), c->phi, &o1, c->stream, k1));
            HIPCHK(c, hipEventRecord(c->hs.ev_xhalf, c->stream));
            hipEvent_t k2 = diag_begin(c, c->stream);
            hipEvent_t k3 = k2 ? take_ev(c) : nullptr;
            HIPCHK(c, launch_phi_rows(c->dim, rows_kind, c->rec, c->scal, c->row0 + h, c->nrows - h, c->n, c->hs.S2b,
                                      c->part, c->nrows - h, inv_n, nullptr, nullptr, nmax_cur(c),
                                      c->phi + h * d, &o2, c->stream, k3));
            if (k2) c->tm.ev_diag.push_back({k2, k3, DG_PHI_KERNEL, true});
        } else {
            HIPCHK(c, launch_phi_rows(c->dim, rows_kind, c->rec, c->scal, c->row0, c->nrows, c->n, c->S, c->part,
                                      c->ldp, inv_n, mat ? c->ms.wv : nullptr, mat ? c->ms.sgn : nullptr,
                                      mat ? nullptr : nmax_cur(c), c->phi, opt, c->stream, k1));
        }
        break;
    case PHI_B3:
        HIPCHK(c, launch_phi_b3(p.KP, p.NCB, p.s1v, c->B3, c->cvf, c->scal, c->row0, c->nrows, ntl, c->dim, inv_n,
                                mat ? c->ms.wv : nullptr, c->xc, p.KP, c->phi, opt, p.b3_rg, c->stream));
        break;
    case PHI_F32S:
        HIPCHK(c, launch_phi_f32s(p.KP, p.NCB, c->XS, c->VS, mat ? c->ms.zcf : c->xcf, c->cvf, c->scal,
                                  c->row0, c->nrows, ntl, c->dim, inv_n, mat ? c->ms.wv : nullptr, c->xc,
                                  p.KP, c->phi, opt, c->stream));
        break;
    case PHI_TILE_F32:
        HIPCHK(c, launch_phi<float>(p.KP, p.NCB, p.s1v, mat ? c->ms.zcf : c->xcf, c->cvf, c->Vf, c->scal, c->row0,
                                    c->nrows, (c->n + TB - 1) / TB, c->n, c->dim, inv_n,
                                    mat ? c->ms.wv : nullptr, c->xc, c->phi, c->stream));
        break;
    case PHI_TILE_F64: {
        const double *x = mat ? c->ms.zc : c->xc; // (the kernel's columns and its epilogue's rows)
        HIPCHK(c, launch_phi<double>(p.KP, p.NCB, p.s1v, x, c->cvec, c->V, c->scal, c->row0, c->nrows,
                                     (c->n + TB - 1) / TB, c->n, c->dim, inv_n, mat ? c->ms.wv : nullptr, x,
                                     c->phi, c->stream));
        break;
    }
    }
    if (k0) {
        if (!c->rowpath) HIPCHK(c, hipEventRecord(k1, c->stream));
        c->tm.ev_diag.push_back({k0, k1, DG_PHI_KERNEL, true});
    }
    if (sym) clear_marks(c);
    if (c->tm.timing) {
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        c->tm.ev_phi.push_back(ev);
        c->phi_end = c->last_phi_end = ev.b;
    }
    return SVGD_OK;
}

// The step's phi and optimizer update: on the row path and the streamed F32
// tile path the phi kernel's epilogue applies it (one launch fewer, no phi
// re-read), else k_opt_update.
int run_phi_opt(svgd_ctx *c)
{
    if (c->opt_kind < 0)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Invalid Optimizer object pointer.");
    OptArgs o;
    CHK(opt_args(c, &o));
    const bool fused = c->plan.fused() && !imq_kernel(c); // (the IMQ finish writes phi alone)
    c->phi_end = nullptr;
    c->hs.xh_valid = false;
    CHK(run_phi(c, fused ? &o : nullptr));
    if (!fused) {
        HIPCHK(c, launch_opt_update(o, c->phi, c->stream));
        c->phi_end = nullptr;
    }
    c->hs.xh_valid = o.xh != nullptr;
    c->xver += 1; // X_{t+1} (the centring fold's version)
    // this rank's rows of X_{t+1} are final here: the next step's X_t copy
    // down (host gradient) need not wait for the X all-gather (P > 1)
    if (c->phi_end) {
        c->ev_xready_use = c->phi_end;
    } else {
        HIPCHK(c, hipEventRecord(c->ev_xready, c->stream));
        c->ev_xready_use = c->ev_xready;
    }
    CHK(allgather_rows(c, c->X));
    c->phi_end = nullptr;
    return coll_check_step(c);
}

} // namespace svgd_amd

extern "C" {

int svgd_set_scale(svgd_ctx *c, int method, double fixed_a)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    if (method != SVGD_SCALE_MEDIAN && method != SVGD_SCALE_FIXED && method != SVGD_SCALE_HESSIAN)
        return fail(c, SVGD_ERR_ARG, "[Argument error] Invalid scale method Enum provided.");
    if (method == SVGD_SCALE_HESSIAN && imq_kernel(c)) return fail(c, SVGD_ERR_ARG, IMQ_SCALE_MSG);
    if (method == SVGD_SCALE_HESSIAN) CHK(alloc_matrix_scale(c));
    c->scale_method = method;
    c->fixed_a = fixed_a;
    c->ms.hess_ready = false;
    return SVGD_OK;
}

int svgd_set_scale_matrix(svgd_ctx *c, const double *M)
{
    if (!c || !M) return c ? fail(c, SVGD_ERR_ARG, "[Argument Error] Null scale matrix.") : SVGD_ERR_ARG;
    const int d = c->dim;
    for (int r = 0; r < d; ++r)
        for (int q = 0; q < r; ++q)
            if (M[r * d + q] != M[q * d + r])
                return fail(c, SVGD_ERR_ARG, "[Argument Error] The kernel scale matrix must be symmetric.");
    if (imq_kernel(c)) return fail(c, SVGD_ERR_ARG, IMQ_SCALE_MSG);
    CHK(resolve_pending(c));
    CHK(alloc_matrix_scale(c));
    HIPCHK(c, hipMemcpyAsync(c->ms.src, M, sizeof(double) * (size_t)d * d, hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->scale_method = SVGD_SCALE_MATRIX;
    return SVGD_OK;
}

int svgd_set_kernel(svgd_ctx *c, int kind)
{
    if (!c) return SVGD_ERR_ARG;
    if (kind != SVGD_KERNEL_RBF && kind != SVGD_KERNEL_IMQ)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Invalid kernel kind.");
    CHK(resolve_pending(c));
    if (kind == SVGD_KERNEL_IMQ) {
        if (matrix_scale(c)) return fail(c, SVGD_ERR_ARG, IMQ_SCALE_MSG);
        if (c->dim > 64)
            return fail(c, SVGD_ERR_ARG, "[Argument Error] The inverse multiquadric kernel supports d <= 64.");
        CHK(alloc_imq(c));
    }
    c->imq.kind = kind;
    return SVGD_OK;
}

int svgd_get_kernel(const svgd_ctx *c, int *kind)
{
    if (!c || !kind) return SVGD_ERR_ARG;
    *kind = c->imq.kind;
    return SVGD_OK;
}

int svgd_set_step_hessian_sum(svgd_ctx *c, const double *H_shard_sum)
{
    if (!c || !H_shard_sum) return c ? fail(c, SVGD_ERR_ARG, "[Argument Error] Null Hessian sum.") : SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    if (c->scale_method != SVGD_SCALE_HESSIAN)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] The kernel scale method is not Hessian.");
    const size_t dd = (size_t)c->dim * c->dim;
    c->ms.h_mat.assign(H_shard_sum, H_shard_sum + dd);
    HIPCHK(c, hipMemcpyAsync(c->ms.src, c->ms.h_mat.data(), sizeof(double) * dd, hipMemcpyHostToDevice,
                             c->stream));
    CHK(allreduce_f64(c, c->ms.src, dd));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // h_mat may be reused
    c->ms.hess_ready = true;
    return SVGD_OK;
}

int svgd_get_scale_matrix(svgd_ctx *c, double *M_out)
{
    if (!c || !M_out) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int d = c->dim;
    if (matrix_scale(c)) {
        if (*c->ms.h_err == 1)
            return fail(c, SVGD_ERR_RUNTIME, "[Runtime Error] The kernel scale matrix is not finite.");
        if (*c->ms.h_err == 2 && !c->rowpath)
            return fail(c, SVGD_ERR_RUNTIME,
                        "[Runtime Error] The kernel scale matrix is indefinite; the device path "
                        "supports indefinite matrices for fp64 particles with d <= 16 only.");
        HIPCHK(c, hipMemcpy(M_out, c->ms.M, sizeof(double) * (size_t)d * d, hipMemcpyDeviceToHost));
        return SVGD_OK;
    }
    CHK(fetch_scale(c));
    const double a = c->scale_method == SVGD_SCALE_FIXED ? c->fixed_a : c->h_scal[0];
    for (int r = 0; r < d; ++r)
        for (int q = 0; q < d; ++q) M_out[r * d + q] = r == q ? a : 0.0;
    return SVGD_OK;
}

} // extern "C"
