// svgd_capi.cpp -- C-ABI implementation: optimizer, particles, step orchestration.
//
// One context = one GPU (one process per GPU in multi-GPU runs).  The step
// follows SVGD::Step (reference include/SVGDCpp/SVGD.hpp:373-400):
//   kernel->Step()  -> median scale (GaussianRBFKernel.hpp:141-188)
//   ComputePhi()    -> phi_hat      (SVGD.hpp:407-454)
//   X += opt.Step() -> optimizer + clamp (SVGD.hpp:393-399)
// with X device-resident and only G (host model gradients, Model.hpp:335)
// crossing PCIe each step.
// The context and its units: ctx.h.
#include "ctx.h"
#include <cmath>
#include <cstdio>
#include <cstring>

using namespace svgd_amd;

namespace svgd_amd {

int check_ready(svgd_ctx *c)
{
    if (!c) return SVGD_ERR_ARG;
    if (!c->have_particles)
        return fail(c, SVGD_ERR_UNSET, "[Unset Error] Particle coordinates are unset.");
    return SVGD_OK;
}

// Calls that hand results back refuse a measurement context (svgd_create_sim):
// its particles, phi and scale are one rank's share computed without the
// other ranks' data, not the step's.
int check_results(svgd_ctx *c)
{
    CHK(check_ready(c));
    if (c->sim_world > 1)
        return fail(c, SVGD_ERR_RUNTIME,
                    "[Runtime Error] measurement context (svgd_create_sim, world " +
                        std::to_string(c->sim_world) + "): its results are not the step's.");
    return SVGD_OK;
}

} // namespace svgd_amd

extern "C" {

const char *svgd_last_error(const svgd_ctx *c) { return c ? c->err.c_str() : "SVGDCpp: null context"; }

int svgd_shard(const svgd_ctx *c, int64_t *row0, int64_t *row1)
{
    if (!c) return SVGD_ERR_ARG;
    if (row0) *row0 = c->row0;
    if (row1) *row1 = c->row1;
    return SVGD_OK;
}

int svgd_set_optimizer(svgd_ctx *c, int kind, double lr, double beta1, double beta2, double eps)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    if (kind == SVGD_OPT_ADAM && (beta1 >= 1.0 || beta1 < 0.0 || beta2 >= 1.0 || beta2 < 0.0))
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Invalid value for decay parameter beta.");
    if (kind == SVGD_OPT_RMSPROP && (beta1 > 1.0 || beta1 < 0.0))
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Invalid value for decay parameter beta.");
    if (kind < SVGD_OPT_ADAM || kind > SVGD_OPT_RMSPROP)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Invalid Optimizer object pointer.");
    c->opt_kind = kind;
    c->lr = lr;
    c->b1 = beta1;
    c->b2 = beta2;
    c->eps = eps;
    return svgd_reset_optimizer(c);
}

int svgd_reset_optimizer(svgd_ctx *c)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(1, c->nrows) * c->dim;
    HIPCHK(c, hipMemsetAsync(c->m, 0, bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(c->v, 0, bytes, c->stream));
    c->t = 0;
    return SVGD_OK;
}

int svgd_set_bounds(svgd_ctx *c, const double *lower, const double *upper)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    if (!lower && !upper) {
        c->bounded = false;
        return SVGD_OK;
    }
    if (!lower || !upper)
        return fail(c, SVGD_ERR_DIM, "[Dimension Error] The provided bounds have incorrect dimensions.");
    // the step just issued may not have read its bounds yet (its chain runs
    // on c->stream, which the null stream does not wait for): drain it, then
    // upload in stream order like every other setter
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpyAsync(c->lower, lower, sizeof(double) * c->dim, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->upper, upper, sizeof(double) * c->dim, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream)); // the caller's arrays may be reused
    c->bounded = true;
    return SVGD_OK;
}

int svgd_set_particles(svgd_ctx *c, const double *X)
{
    if (!c || !X) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->X, X, sizeof(double) * (size_t)c->n * c->dim,
                             hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_xready, c->stream));
    c->ev_xready_use = c->ev_xready;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_particles = true;
    c->hs.xhalf_ready = false;
    c->hs.xh_valid = false;
    c->xver += 1;
    c->cpart_ver[0] = c->cpart_ver[1] = -1; // new particles: centred on their own mean
    c->trk.restart(true); // new particles: the median history restarts
    return SVGD_OK;
}

int svgd_get_particles(svgd_ctx *c, double *X)
{
    CHK(check_results(c));
    CHK(resolve_pending(c));
    if (!X) return fail(c, SVGD_ERR_ARG, "[Argument Error] Null output buffer.");
    HIPCHK(c, hipMemcpyAsync(X, c->X, sizeof(double) * (size_t)c->n * c->dim,
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SVGD_OK;
}

int svgd_get_shard(svgd_ctx *c, double *X_shard)
{
    CHK(check_results(c));
    CHK(resolve_pending(c));
    if (c->nrows == 0) return SVGD_OK;
    HIPCHK(c, hipMemcpyAsync(X_shard, c->X + (size_t)c->row0 * c->dim,
                             sizeof(double) * (size_t)c->nrows * c->dim, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SVGD_OK;
}

int svgd_phi(svgd_ctx *c, const double *G_shard, double a, double *phi_out)
{
    CHK(check_results(c));
    CHK(resolve_pending(c));
    c->spec_step = false;
    if (hipEventQuery(c->ev_scal) != hipSuccess) // the last [a, med] copy has read scal
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_scal, 0));
    CHK(center(c));
    HIPCHK(c, launch_set_scal(a, NAN, c->scal, c->stream));
    // the host copy of [a, med] follows (svgd_last_scale after svgd_phi)
    HIPCHK(c, hipEventSynchronize(c->ev_scal)); // no D2H into h_scal pending
    c->h_scal[0] = a;
    c->h_scal[1] = NAN;
    c->scal_fresh = true;
    CHK(upload_g(c, G_shard));
    CHK(run_phi(c, nullptr));
    if (phi_out && c->nrows > 0) {
        HIPCHK(c, hipMemcpyAsync(phi_out, c->phi, sizeof(double) * (size_t)c->nrows * c->dim,
                                 hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SVGD_OK;
}

int svgd_begin_step(svgd_ctx *c, double *X_shard_out)
{
    CHK(check_ready(c));
    CHK(resolve_pending(c));
    if (c->opt_kind < 0)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Invalid Optimizer object pointer.");
    const size_t bytes = sizeof(double) * (size_t)c->nrows * c->dim;
    if (X_shard_out && c->nrows > 0) {
        // X_t is final once the previous step's update (and all-gather) ran
        HIPCHK(c, hipStreamWaitEvent(c->cstream, c->ev_xready_use ? c->ev_xready_use : c->ev_xready, 0));
        HIPCHK(c, hipMemcpyAsync(c->h_x, c->X + (size_t)c->row0 * c->dim, bytes,
                                 hipMemcpyDeviceToHost, c->cstream));
        HIPCHK(c, hipEventRecord(c->ev_x, c->cstream));
    }
    CHK(plan_step(c));
    CHK(scale_begin(c));
    if (X_shard_out && c->nrows > 0) {
        HIPCHK(c, hipEventSynchronize(c->ev_x));
        if (X_shard_out != c->h_x) std::memcpy(X_shard_out, c->h_x, bytes);
    }
    return SVGD_OK;
}

int svgd_finish_step(svgd_ctx *c, const double *G_shard)
{
    CHK(check_ready(c));
    if (c->co.coll_phase != 1) // (also keeps the collectives in their order, svgd_ctx)
        return fail(c, SVGD_ERR_RUNTIME, "[Runtime Error] svgd_finish_step without svgd_begin_step.");
    CHK(upload_g_begin(c, G_shard));
    // the G all-gather is queued before the host waits for the median counts
    // (scale_finish), so the device runs it during that round trip
    CHK(upload_g_finish(c));
    CHK(scale_finish(c));
    CHK(run_phi_opt(c));
    return SVGD_OK;
}

int svgd_step(svgd_ctx *c, const double *G_shard)
{
    if (G_shard) {
        CHK(svgd_begin_step(c, nullptr));
        return svgd_finish_step(c, G_shard);
    }
    // fully device-resident step: grad log p from the device model
    CHK(check_ready(c));
    if (!has_device_model(c))
        return fail(c, SVGD_ERR_ARG,
                    "[Argument Error] Null log-gradient buffer and no device model set.");
    CHK(svgd_begin_step(c, nullptr));
    if (c->scale_method == SVGD_SCALE_HESSIAN && c->dm.hess.on && !c->ms.hess_ready) {
        // the device model's Hessian sum, where svgd_set_step_hessian_sum
        // would upload the caller's (a sum supplied for this step wins)
        CHK(launch_device_model_hess(c, c->X + (size_t)c->row0 * c->dim, c->nrows, c->ms.src));
        CHK(allreduce_f64(c, c->ms.src, (size_t)c->dim * c->dim));
        c->ms.hess_ready = true;
    }
    CHK(launch_device_model_grad(c, c->X + (size_t)c->row0 * c->dim, c->nrows,
                                 c->G + (size_t)c->row0 * c->dim));
    c->mark = nullptr; // (the gradient kernel runs after the median's end event)
    CHK(scale_finish(c));
    CHK(allgather_rows(c, c->G));
    CHK(run_phi_opt(c));
    return SVGD_OK;
}

int svgd_host_buffers(svgd_ctx *c, double **x_shard, double **g_shard)
{
    if (!c) return SVGD_ERR_ARG;
    if (x_shard) *x_shard = c->h_x;
    if (g_shard) *g_shard = c->h_g;
    return SVGD_OK;
}

int svgd_sync(svgd_ctx *c)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SVGD_OK;
}

// (The plan is made at creation and a matrix scale is chosen afterwards, so
// the name stays the isotropic-scale kernel's: under a matrix scale a row
// stream or symmetric-pass context launches matrix_scale_plan's kernel, the
// row stream in its 4-wave geometry.)
int svgd_phi_kernel_name(const svgd_ctx *c, char *buf, int cap)
{
    if (!c || !buf || cap <= 0) return SVGD_ERR_ARG;
    if (imq_kernel(c)) { // (chosen after the plan too, but a kernel of its own)
        std::snprintf(buf, (size_t)cap, "k_imq_pass<%d>", (c->dim + 3) / 4 * 4);
        return SVGD_OK;
    }
    phi_plan_name(c->plan, built_caps(c->dim, c->dtype), buf, cap);
    return SVGD_OK;
}

int svgd_plan_phi_name(int dim, int64_t n, int dtype, int world, int rank, char *buf, int cap)
{
    if (!buf || cap <= 0 || n <= 0 || world < 1 || rank < 0 || rank >= world ||
        (dtype != SVGD_F64 && dtype != SVGD_F32))
        return SVGD_ERR_ARG;
    int64_t row0 = 0, row1 = 0;
    svgd_plan_rows(n, world, rank, &row0, &row1);
    PhiPlan p;
    const PhiCaps caps = built_caps(dim, dtype);
    if (!plan_phi(dim, n, dtype, world, row0, read_knobs(), caps, &p)) return SVGD_ERR_DIM;
    phi_plan_name(p, caps, buf, cap);
    return SVGD_OK;
}

} // extern "C"
