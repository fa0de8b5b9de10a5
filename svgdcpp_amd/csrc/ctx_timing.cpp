// ctx_timing.cpp -- the pooled timing events, the level-2 diagnostic spans and
// the calls that read them (svgd_set_timing, svgd_get_timing, svgd_get_diagnostics).
#include "ctx.h"

using namespace svgd_amd;

namespace svgd_amd {

EvPair take_pair(svgd_ctx *c)
{
    EvPair p;
    p.a = c->tm.pool.take();
    p.b = c->tm.pool.take();
    return p;
}

hipEvent_t take_ev(svgd_ctx *c) { return c->tm.pool.take(); }

// level-2 diagnostic span on stream s: begin records a pooled event, end its
// partner; begin returns nullptr below level 2 and end then does nothing
hipEvent_t diag_begin(svgd_ctx *c, hipStream_t s)
{
    if (c->tm.tlevel < 2) return nullptr;
    hipEvent_t e = take_ev(c);
    (void)hipEventRecord(e, s);
    clear_marks(c); // work (an event) queued after those marks
    return e;
}
void diag_end(svgd_ctx *c, hipStream_t s, hipEvent_t a, int kind, bool own_a)
{
    if (!a) return;
    hipEvent_t b = take_ev(c);
    (void)hipEventRecord(b, s);
    c->tm.ev_diag.push_back({a, b, kind, own_a});
    clear_marks(c);
}

// Level 2: the start of the phi-wait span (run_phi) -- a pooled event of its
// own, recorded where the median ends (the phase events go back to the pool
// in svgd_get_timing; a diagnostic span must not share one of them)
int mark_median_end(svgd_ctx *c)
{
    if (c->tm.tlevel < 2) return SVGD_OK;
    if (c->tm.med_end_ev) c->tm.pool.give(c->tm.med_end_ev); // (never consumed)
    c->tm.med_end_ev = take_ev(c);
    HIPCHK(c, hipEventRecord(c->tm.med_end_ev, c->stream));
    c->mark = nullptr; // work (an event) queued after the median's end
    return SVGD_OK;
}

} // namespace svgd_amd

extern "C" {

int svgd_set_timing(svgd_ctx *c, int enable)
{
    if (!c) return SVGD_ERR_ARG;
    c->tm.timing = enable != 0;
    c->tm.tlevel = enable < 0 ? 0 : enable;
    c->last_phi_end = nullptr;
    return SVGD_OK;
}

int svgd_get_diagnostics(svgd_ctx *c, double *out, int cap)
{
    if (!c || (!out && cap > 0)) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->co.gstream) HIPCHK(c, hipStreamSynchronize(c->co.gstream));
    for (auto &e : c->tm.ev_diag) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, e.a, e.b));
        c->tm.dg_ms[e.kind] += ms;
        c->tm.dg_cnt[e.kind] += 1;
        if (e.own_a) c->tm.pool.give(e.a);
        c->tm.pool.give(e.b);
    }
    c->tm.ev_diag.clear();
    int ranks = 1;
    if (c->co.comm) (void)ncclCommCount(c->co.comm, &ranks);
    else if (c->co.hcomm) ranks = c->world;
    const double v[SVGD_DIAG_LEN] = {(double)c->hs.h_steps,
                                     c->tm.dg_ms[DG_PHI_KERNEL],
                                     (double)c->tm.dg_cnt[DG_PHI_KERNEL],
                                     c->tm.dg_ms[DG_PHI_WAIT],
                                     (double)c->tm.dg_cnt[DG_PHI_WAIT],
                                     c->tm.dg_ms[DG_COLL],
                                     (double)c->tm.dg_cnt[DG_COLL],
                                     c->tm.dg_ms[DG_GATHER_G],
                                     (double)c->tm.dg_cnt[DG_GATHER_G],
                                     c->hs.h_grad_ms,
                                     c->hs.h_xwait_ms,
                                     c->hs.h_job_ms,
                                     c->hs.h_wait_ms,
                                     (double)ranks,
                                     (double)c->hs.host_threads,
                                     (double)c->trk.steps,
                                     (double)c->trk.miss,
                                     (double)c->sim_world,
                                     (double)c->cpu_quota,
                                     (double)c->n_split,
                                     (double)c->n_mirror,
                                     (double)c->n_spec,
                                     c->co.gcomm ? 1.0 : 0.0,
                                     c->trk.band_sum};
    for (int i = 0; i < cap && i < SVGD_DIAG_LEN; ++i) out[i] = v[i];
    for (int k = 0; k < 4; ++k) c->tm.dg_ms[k] = 0, c->tm.dg_cnt[k] = 0;
    c->hs.h_grad_ms = c->hs.h_xwait_ms = c->hs.h_job_ms = c->hs.h_wait_ms = 0;
    c->hs.h_steps = 0;
    c->trk.steps = c->trk.miss = 0;
    c->trk.band_sum = 0;
    c->n_split = c->n_mirror = c->n_spec = 0;
    return cap < SVGD_DIAG_LEN ? cap : SVGD_DIAG_LEN;
}

int svgd_get_timing(svgd_ctx *c, double *phi_ms, double *median_ms, int64_t *count)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the events go back to the pool: the status / scale-final marks may be
    // among them (everything they mark is complete now)
    c->ev_status_use = c->ev_fin_use = c->mark = c->phi_end = c->ev_xready_use = nullptr;
    c->last_phi_end = nullptr;
    for (auto &e : c->tm.ev_phi) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, e.a, e.b));
        c->tm.phi_ms += ms;
        c->tm.tcount += 1;
        c->tm.pool.give(e.spare ? e.spare : e.a); // (a shared a is ev_med's b: given back there)
        c->tm.pool.give(e.b);
    }
    c->tm.ev_phi.clear();
    for (auto &e : c->tm.ev_med) {
        float ms = 0;
        HIPCHK(c, hipEventElapsedTime(&ms, e.a, e.b));
        c->tm.med_ms += ms;
        c->tm.pool.give(e.spare ? e.spare : e.a);
        c->tm.pool.give(e.b);
    }
    c->tm.ev_med.clear();
    if (phi_ms) *phi_ms = c->tm.phi_ms;
    if (median_ms) *median_ms = c->tm.med_ms;
    if (count) *count = c->tm.tcount;
    c->tm.phi_ms = c->tm.med_ms = 0;
    c->tm.tcount = 0;
    return SVGD_OK;
}

} // extern "C"
