// ctx_median.cpp -- the centring and the median scale of a step: bracket (sampled
// or tracked), collect pass, selection (synchronous or speculative) and its redo.
#include "ctx.h"
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>

using namespace svgd_amd;

namespace svgd_amd {
namespace {

int allreduce_cnt3(svgd_ctx *c)
{
    // below, candidate and overflowed-region totals and the bucket counts are
    // sums; the bracket (CNT_LO, CNT_HI) is identical on every rank and stays local
    return allreduce_u64(c, c->cnt3, 3 + NBK);
}

// A fresh select state (make_state) from the host to the device.
int upload_state(svgd_ctx *c, const SelState &s)
{
    HIPCHK(c, launch_set_state(s, c->st, c->stream));
    return SVGD_OK;
}

// One sweep over this rank's median pair tiles (mode 0 collect, 1 radix
// histogram, 2 debug dump) on the row-stream (d <= 16) or MFMA tile kernel.
// (the collect pass, mode 0, also histograms its candidates in key-range
// buckets: c->bpart, which the other modes' launchers leave alone)
PairArgs pair_args(svgd_ctx *c, uint64_t *regions, int64_t cap, double *dbg)
{
    return PairArgs{c->n,      c->pnb,   c->tile0, c->tile0 + c->own_tiles, regions, cap,
                    c->counts, c->below, c->st,    c->ghist,                c->bpart, dbg};
}

hipError_t pair_pass(svgd_ctx *c, int mode, int grid, uint64_t *regions, int64_t cap, double *dbg)
{
    const PairArgs a = pair_args(c, regions, cap, dbg);
    if (c->rowpath)
        return launch_pair_rows(c->dim, c->plan.KP, mode, grid, c->xc, c->nrm, c->xf, nmax_cur(c), a, c->stream);
    if (c->dtype == SVGD_F32)
        return launch_pair_tiles<float>(c->plan.KP, mode, grid, c->xcf, c->nrmf, c->XK, a, c->stream);
    return launch_pair_tiles<double>(c->plan.KP, mode, grid, c->xc, c->nrm, nullptr, a, c->stream);
}

constexpr double WIDE_SIGMA = 8.0; // re-bracket after a miss
// k_pair_mcol stages ~4096 x band pairs per 16-column block and wave (512
// slots): wider brackets (tiny samples, tests) take k_pair_rows' collect
constexpr double MCOL_MAX_BAND = 0.02;

SelState sample_state(svgd_ctx *c, double sigma);
int sample_bracket(svgd_ctx *c);
int collect_counts(svgd_ctx *c);
int median_finish_spec(svgd_ctx *c, double logn);

// This step's bracket, decided before the centring launch (which then also
// writes the predicted select state): predicted on speculative steps (row
// and tile paths: keys are D^2 as doubles on both) when the tracker allows
// it, else sampled in median_begin -- by the one sample plan both read.
void trk_plan(svgd_ctx *c)
{
    c->trk_go = false;
    c->trk.begin_step();
    const int64_t M = upper_pairs(c->n);
    if (M <= c->direct_max_pairs) return; // every key is a candidate: no bracket
    c->samp = plan_sample(M, !c->rowpath && c->n / TB >= 2, c->sample_size,
                          c->co.any() || c->sim_world > 1, c->shard_sample, c->sim_world,
                          c->bracket_sigma);
    if (!c->spec_step || c->sample_size > 0 || c->cand_capacity > 0) return;
    const double Mq = c->sim_world > 1 ? (double)c->sim_pairs : (double)M;
    c->trk_go = c->trk.predict(Mq, c->samp.band_samp, &c->trk_lo, &c->trk_hi, &c->trk_band);
}

// The collect pass's candidate regions (and the compaction buffer beside
// them) hold reg_cap keys each.
int grow_regions(svgd_ctx *c)
{
    const int64_t need = c->reg_cap * c->nregions;
    if (c->regions_alloc < need) {
        CHK(dalloc(c, &c->regions, need));
        CHK(dalloc(c, &c->cbuf, need));
        c->regions_alloc = need;
    }
    return SVGD_OK;
}

// Phase 1 of the median: candidate bracket + collect pass + counts.
// Leaves the reduced counts in c->h_cnt (ready at c->ev_cnt).
int median_begin(svgd_ctx *c)
{
    c->trk_keys = false;
    const int64_t n = c->n;
    c->sel = plan_ranks(n, c->sim_world, c->sim_pairs);
    c->median_pending = true;
    if (c->sel.nsel == 0) { // med = 0 (n <= 1 or all diagonal)
        c->med_path = SVGD_MEDIAN_DIRECT;
        return SVGD_OK;
    }

    const int64_t M = upper_pairs(n);
    const int64_t tiles = c->own_tiles;
    c->collect_grid = (int)std::max<int64_t>(1, std::min<int64_t>(tiles, c->collect_blocks));
    c->nregions = c->rowpath ? 4 * (int64_t)c->collect_grid : c->collect_grid;
    const int64_t tiles_per_blk = (tiles + c->nregions - 1) / c->nregions;
    const int64_t pairs_own = tiles * c->pblock * c->pblock;

    if (M <= c->direct_max_pairs) {
        // every key is a candidate: bracket [0, ~0)
        c->med_path = SVGD_MEDIAN_DIRECT;
        c->reg_cap = tiles_per_blk * c->pblock * c->pblock;
        uint64_t z[2] = {0, 0};
        CHK(upload_state(c, make_state(1, z, 0, ~0ull)));
    } else if (c->trk_go) {
        // predicted bracket (trk_plan; its select state was written by the
        // centring launch): no sample, no radix passes (k_center zeroed the
        // bucket counts); regions sized for 4x the band
        c->med_path = SVGD_MEDIAN_BRACKET;
        c->band_est = c->trk_band;
        c->reg_cap = region_cap_predicted(c->trk_band, pairs_own, c->nregions);
    } else {
        c->med_path = SVGD_MEDIAN_BRACKET;
        SamplePlan &sp = c->samp;
        const int64_t S = sp.S;
        if (c->sample_alloc < S) {
            CHK(dalloc(c, &c->sample_keys, S));
            c->sample_alloc = S;
        }
        if (sp.tile_sample)
            HIPCHK(c, launch_sample_tiles(c->plan.KP, c->xc, c->nrm, c->xcf, c->nrmf, c->XK, n,
                                          S / (TB * TB), c->sample_keys, c->stream));
        // sharded (P > 1, scattered pairs): rank r draws pairs [S r/P, S (r+1)/P)
        // of the one counter-based sequence and the bracket's histograms are
        // all-reduced -- the same sample, hence the same bracket, as on one rank
        sp.shard = !sp.tile_sample && (c->co.any()) && c->shard_sample;
        const int64_t g0 = sp.shard ? S * c->rank / c->world : 0;
        sp.local = sp.shard ? S * (c->rank + 1) / c->world - g0 : S;
        const double Mq = c->sim_world > 1 ? (double)c->sim_pairs : (double)M;
        sp.qlo = (double)c->sel.sel_rank[0] / Mq;
        sp.qhi = (double)c->sel.sel_rank[c->sel.nsel - 1] / Mq;
        const SelState init = sample_state(c, sp.sigma);
        if (!sp.tile_sample)
            HIPCHK(c, launch_sample_keys(c->xc, c->nrm, c->xf, n, c->dim, c->plan.KP, g0, sp.local,
                                         c->sample_keys, init, c->st, c->stream));
        else
            HIPCHK(c, launch_set_state(init, c->st, c->stream));
        CHK(sample_bracket(c));
        c->reg_cap = region_cap_sampled(sp, c->cand_capacity, pairs_own, c->nregions);
    }
    CHK(grow_regions(c));
    return collect_counts(c);
}

// The select state of the bracket passes: the sample ranks sigma
// sample-quantile standard deviations either side of the target quantiles.
SelState sample_state(svgd_ctx *c, double sigma)
{
    const SampleRanks r = sample_ranks(c->samp.S, c->samp.qlo, c->samp.qhi, sigma);
    const uint64_t sr[2] = {r.slo, r.shi};
    c->band_est = r.band_est;
    return make_state(2, sr, 0, ~0ull);
}

// The two radix passes over the sample from that state (on the device: the
// sampler or an upload wrote it) -> bracket [lo_key, hi_key), which stays on
// the device (read by the collect pass).  Per pass: one histogram launch
// (atomics into ghist), the all-reduce if the sample is sharded, one scan
// launch; the last scan also sets the bracket.
int sample_bracket(svgd_ctx *c)
{
    for (int p = 0; p < 2; ++p) {
        HIPCHK(c, launch_hist_regions(c->sample_keys, nullptr, 1, c->samp.local, 0, c->st, c->ghist,
                                      c->stream));
        if (c->samp.shard) CHK(allreduce_u64(c, c->ghist, 2 * RADIX));
        HIPCHK(c, launch_select_scan(c->st, c->ghist, p == 1, c->cnt3 + 3, c->stream));
    }
    return SVGD_OK;
}

// Collect pass over this rank's pair tiles, then the all-reduced counts to the
// host (ready at ev_cnt).
int collect_counts(svgd_ctx *c)
{
    const PairArgs a = pair_args(c, c->regions, c->reg_cap, nullptr);
    if (c->rowpath && c->mcol && c->med_path != SVGD_MEDIAN_DIRECT && c->band_est <= MCOL_MAX_BAND)
        // bracket collect: fp32 MFMA classification, exact keys for the band
        // (a thin band only: each band pair is staged and finished one by one)
        HIPCHK(c, launch_pair_mcol(c->dim, c->collect_grid, c->xc, c->xf, nmax_cur(c), c->xsplit, a, c->stream));
    else if (!c->rowpath && c->dtype == SVGD_F32 && c->mcol)
        // fp32 tile path: k_pair_tiles' keys, rows held in VGPRs, no LDS
        HIPCHK(c, launch_pair_tcol(c->plan.KP, c->collect_grid, c->xcf, c->nrmf, c->XK, a, c->stream));
    else
        HIPCHK(c, pair_pass(c, 0, c->collect_grid, c->regions, c->reg_cap, nullptr));
    HIPCHK(c, launch_counts_reduce(c->below, c->counts, c->nregions, c->reg_cap, c->st, c->bpart,
                                   c->collect_grid, c->cnt3, c->stream,
                                   c->spec_step ? c->gseg + (size_t)c->rank * (c->spec_cap + 1) : nullptr));
    CHK(allreduce_cnt3(c));
    // speculative: the device plan and the selection are queued right behind
    // the counts (while the device still runs the collect pass), not when the
    // host comes back from the gradient -- no launch gaps between them
    if (c->spec_step) return median_finish_spec(c, std::log((double)c->n));
    HIPCHK(c, hipMemcpyAsync(c->h_cnt, c->cnt3, CNT_LEN * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_cnt, c->stream));
    return SVGD_OK;
}

// Speculative phase 2: plan, compact, gather and select on the device; the
// plan's status goes to the host on the copy stream (resolve_pending).
int median_finish_spec(svgd_ctx *c, double logn)
{
    const int64_t cap = c->spec_cap;
    uint64_t *seg = c->gseg + (size_t)c->rank * (cap + 1);
    // the plan also stores its status straight into pinned host memory: no
    // copy on the copy stream (a small copy there turned the X shard copies
    // into blit kernels competing with the median kernels)
    // (the compaction's blocks derive the bucket plan themselves: no plan launch)
    const RankPlan &r = c->sel;
    const PlanArgs pa{c->cnt3, r.nsel, (uint64_t)r.sel_rank[0], (uint64_t)r.sel_rank[r.nsel - 1],
                      cap, c->d_status, c->h_status_dev,
                      c->sim_world > 1 ? 1 : 0, c->h_trk_dev};
    HIPCHK(c, launch_compact_buckets(c->regions, c->counts, c->nregions, c->reg_cap, c->st, seg, cap,
                                     c->d_status, c->stream, &pa));
    CHK(allgather_u64(c, c->gseg, (size_t)cap + 1));
    // the plan's status is final once the selection completes.  Timing off
    // (the product path): no event at all -- the selection stores a sequence
    // number into pinned memory after its last store and resolve_pending
    // polls it (an event between two kernels costs a ~6 us dispatch gap,
    // profiles/r06_step_timeline_*); with phase timing the phase event there
    // serves.  (c->pending -- the plan's status to check -- is set when the
    // step is complete, by median_finish: resolve_pending never redoes half a
    // step.)
    const bool by_seq = !c->tm.timing && c->tm.tlevel < 2;
    c->status_seq = by_seq ? ++c->seq_ctr : 0;
    HIPCHK(c, launch_select_small(c->st, c->gseg, c->world, cap, r.navg, r.src_lo, r.src_hi, logn,
                                  c->scal, c->d_status, c->stream, c->h_trk_dev, c->status_seq));
    c->trk_keys = true;
    if (by_seq) {
        c->ev_status_use = nullptr;
        c->med_ev_done = true; // (no scale-final event either: fetch_scale syncs the stream)
        c->mark = nullptr;
        return SVGD_OK;
    }
    if (c->tm.timing && !c->tm.ev_med.empty()) {
        c->ev_status_use = c->tm.ev_med.back().b; // also the median phase's end
        c->med_ev_done = true;
        c->mark = c->ev_status_use;
    } else {
        c->ev_status_use = c->ev_status;
    }
    HIPCHK(c, hipEventRecord(c->ev_status_use, c->stream));
    CHK(mark_median_end(c));
    return SVGD_OK;
}

// Phase 2: exact selection among candidates (or streamed fallback), then a.
int median_finish(svgd_ctx *c)
{
    if (!c->median_pending) return fail(c, SVGD_ERR_RUNTIME, "[Runtime Error] median not begun.");
    c->median_pending = false;
    const double logn = std::log((double)c->n);
    if (c->sel.nsel == 0) {
        // every averaged order statistic is a diagonal zero
        uint64_t z[2] = {0, 0};
        CHK(upload_state(c, make_state(1, z, 0, 0)));
        HIPCHK(c, launch_finalize(c->st, c->sel.navg, -1, -1, logn, c->scal, c->scal + 1, c->stream));
        c->last_path = SVGD_MEDIAN_DIRECT;
        return SVGD_OK;
    }
    if (c->spec_step) { // queued by collect_counts
        c->pending = true;
        c->last_path = c->med_path;
        return SVGD_OK;
    }
    c->last_fast = false;
    HIPCHK(c, hipEventSynchronize(c->ev_cnt));
    if (c->sim_world > 1 && !c->h_cnt[2] && c->h_cnt[1] > 0) {
        // measurement mode: the share is selected alone -- re-anchor the
        // ranks inside its candidates (the device plan does the same)
        const int64_t dr = c->sel.sel_rank[c->sel.nsel - 1] - c->sel.sel_rank[0];
        c->sel.sel_rank[0] = (int64_t)(c->h_cnt[0] + c->h_cnt[1] / 2);
        if (c->sel.nsel > 1) c->sel.sel_rank[1] = c->sel.sel_rank[0] + dr;
    }
    const uint64_t r0 = (uint64_t)c->sel.sel_rank[0], r1 = (uint64_t)c->sel.sel_rank[c->sel.nsel - 1];
    auto in_bracket = [&]() {
        return !c->h_cnt[2] && r0 >= c->h_cnt[0] && r1 < c->h_cnt[0] + c->h_cnt[1];
    };
    int path = c->med_path;
    if (!in_bracket() && path == SVGD_MEDIAN_BRACKET && !c->h_cnt[2]) {
        // the order statistics fell outside the sampled bracket (probability
        // ~2e-3 per step at the default 3 sigma): bracket again from the same
        // sample at WIDE_SIGMA and repeat the collect pass (one more pass)
        // instead of the streamed radix select (one pass per 11-bit digit)
        CHK(upload_state(c, sample_state(c, std::max(c->bracket_sigma, WIDE_SIGMA))));
        CHK(sample_bracket(c));
        CHK(collect_counts(c));
        HIPCHK(c, hipEventSynchronize(c->ev_cnt));
        path = SVGD_MEDIAN_REBRACKET;
    }
    const unsigned long long below = c->h_cnt[0];
    const uint64_t lo_key = c->h_cnt[CNT_LO], hi_key = c->h_cnt[CNT_HI];
    bool ok = in_bracket();
    uint64_t ranks[2];
    if (ok) {
        ranks[0] = c->sel.sel_rank[0] - below;
        ranks[1] = c->sel.sel_rank[c->sel.nsel - 1] - below;
    } else {
        path = SVGD_MEDIAN_FALLBACK;
        ranks[0] = c->sel.sel_rank[0];
        ranks[1] = c->sel.sel_rank[c->sel.nsel - 1];
    }
    // Bucket select: the collect pass histogrammed the candidates in NBK
    // key-range buckets (all-reduced with the counts), so the bucket holding
    // each order statistic is known here.  If those buckets are small, every
    // rank compacts its keys in them, the compacted keys are all-gathered once
    // and one work-group selects exactly -- no per-digit all-reduces.
    if (ok && c->bucket_cap > 0) {
        const int64_t rr[2] = {(int64_t)ranks[0], (int64_t)ranks[1]};
        int bsel[2];
        int64_t rin[2], tot = 0;
        const int ns = (c->sel.nsel > 1 && ranks[1] != ranks[0]) ? 2 : 1;
        if (svgd_plan_bucket_select(c->h_cnt + 3, NBK, ns, rr, bsel, rin, &tot) == 0 &&
            tot <= std::min<int64_t>(c->bucket_cap, CAPG)) {
            // one segment per rank, sized for the selected buckets' total (a
            // rank holds at most that many): the all-gather moves tot keys per
            // rank, not the CAPG capacity
            const int64_t scap = std::max<int64_t>(1, tot);
            uint64_t *seg = c->gseg + (size_t)c->rank * (scap + 1);
            HIPCHK(c, launch_set_sel(c->st, c->sel.nsel, (uint64_t)rin[0],
                                     (uint64_t)(c->sel.nsel > 1 ? rin[ns - 1] : rin[0]), bsel[0],
                                     bsel[ns - 1], seg, c->stream));
            HIPCHK(c, launch_compact_buckets(c->regions, c->counts, c->nregions, c->reg_cap, c->st,
                                             seg, scap, nullptr, c->stream));
            CHK(allgather_u64(c, c->gseg, (size_t)scap + 1));
            HIPCHK(c, launch_select_small(c->st, c->gseg, c->world, scap, c->sel.navg, c->sel.src_lo,
                                          c->sel.src_hi, logn, c->scal, nullptr, c->stream, c->h_trk_dev));
            c->trk_keys = true;
            c->last_path = path;
            // the next step may take the device plan if this one would have
            c->last_fast = (path == SVGD_MEDIAN_BRACKET || path == SVGD_MEDIAN_DIRECT) &&
                           tot <= std::min<int64_t>(c->bucket_cap, CAPG);
            c->last_tot = tot;
            return SVGD_OK;
        }
    }
    // every candidate key lies in [lo_key, hi_key): their common leading bits
    // are known, so the radix passes start below them (bracket path only)
    const bool bracketed = path == SVGD_MEDIAN_BRACKET || path == SVGD_MEDIAN_REBRACKET;
    const int known = bracketed ? known_from(lo_key, hi_key) : 63;
    CHK(upload_state(c, make_state(c->sel.nsel, ranks, 0, ~0ull, known, lo_key)));
    const int passes = (known + RADIX_BITS - 1) / RADIX_BITS;
    if (path == SVGD_MEDIAN_FALLBACK) {
        // streamed radix select over every pair (rare: the bracket missed)
        for (int p = 0; p < passes; ++p) {
            const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(c->own_tiles, 2048));
            HIPCHK(c, pair_pass(c, 1, grid, nullptr, 0, nullptr));
            CHK(allreduce_u64(c, c->ghist, 2 * RADIX));
            HIPCHK(c, launch_select_scan(c->st, c->ghist, 0, nullptr, c->stream));
        }
    } else if (passes > 0) {
        // first digit over every candidate, then only the keys in the chosen
        // bucket(s) are kept (compacted) for the remaining digits
        HIPCHK(c, launch_hist_regions(c->regions, c->counts, c->nregions, c->reg_cap, 0, c->st,
                                      c->ghist, c->stream));
        CHK(allreduce_u64(c, c->ghist, 2 * RADIX));
        HIPCHK(c, launch_select_scan(c->st, c->ghist, 0, nullptr, c->stream));
        if (passes > 1) {
            HIPCHK(c, launch_compact(c->regions, c->counts, c->nregions, c->reg_cap, c->st, c->cbuf,
                                     c->ccount, c->stream));
            if (!c->co.any()) {
                // remaining digits in one work-group, no launches in between
                HIPCHK(c, launch_select_tail(c->st, c->cbuf, c->ccount, passes - 1, c->stream));
            } else {
                for (int p = 1; p < passes; ++p) {
                    HIPCHK(c, launch_hist_count(c->cbuf, c->ccount, c->regions_alloc, c->st,
                                                c->ghist, c->stream));
                    CHK(allreduce_u64(c, c->ghist, 2 * RADIX));
                    HIPCHK(c, launch_select_scan(c->st, c->ghist, 0, nullptr, c->stream));
                }
            }
        }
    }
    HIPCHK(c, launch_finalize(c->st, c->sel.navg, c->sel.src_lo, c->sel.src_hi, logn, c->scal, c->scal + 1,
                              c->stream));
    c->last_path = path;
    return SVGD_OK;
}

// A resolved selection (its keys and error flag in h_trk) and the bracket it
// was taken from -> the tracking history.
void trk_record(svgd_ctx *c, uint64_t lo_key, uint64_t hi_key, uint64_t cand)
{
    c->trk.record(c->h_trk[TRK_KEY0], c->h_trk[TRK_KEY1], c->h_trk[TRK_ERR], lo_key, hi_key, cand);
}

// A synchronous step's selection into the tracking history (its keys are in
// h_trk once the step's scale is final; its bracket counts in h_cnt), or a
// restart of the history when that step selected another way.
int trk_resolve_sync(svgd_ctx *c)
{
    const int s = c->trk_sync;
    c->trk_sync = 0;
    if (s == 0) return SVGD_OK;
    if (s == 2 || !c->trk.allowed) {
        c->trk.restart();
        return SVGD_OK;
    }
    HIPCHK(c, hipEventSynchronize(c->ev_fin_use ? c->ev_fin_use : c->ev_fin));
    trk_record(c, c->h_cnt[CNT_LO], c->h_cnt[CNT_HI], c->h_cnt[1]);
    return SVGD_OK;
}

} // namespace

// st_init (optional): the predicted bracket's select state, written by the
// centring launch itself (no launch of its own)
int center(svgd_ctx *c, const SelState *st_init)
{
    // the fold (svgd_ctx::cpart): the previous version's partials as the centre
    const int64_t v = c->xver;
    const int ps = (int)((v - 1) & 1), cs = (int)(v & 1);
    const bool have = c->cpart && c->cpart_ver[ps] == v - 1;
    // F32 at KP 32 / 64: the centring writes the fp32 copies itself
    const bool fused = c->dtype == SVGD_F32 && !c->rowpath && (c->plan.KP == 32 || c->plan.KP == 64);
    HIPCHK(c, launch_mean_center(c->X, c->n, c->dim, c->plan.KP, c->np, c->partial, c->nparts, c->xc, c->nrm,
                                 c->rowpath ? 1 : 0, c->xf, nmax_cur(c), c->cnt3 + 3, c->stream, c->st,
                                 st_init, have ? c->cpart + ps * c->cpart_stride : nullptr,
                                 have ? c->cpart_n[ps] : 0, c->cpart ? c->cpart + cs * c->cpart_stride : nullptr,
                                 c->nmax ? c->nmax + (1 - cs) : nullptr, fused ? c->xcf : nullptr,
                                 fused ? c->nrmf : nullptr, c->xsplit));
    if (c->cpart) {
        c->cpart_ver[cs] = v;
        c->cpart_n[cs] = center_fold_grid(c->dim, c->np);
    }
    if (c->dtype == SVGD_F32) {
        if (!fused) {
            HIPCHK(c, launch_cvt_f32(c->xc, c->np * c->plan.KP, c->xcf, c->stream));
            HIPCHK(c, launch_cvt_nrm_f32(c->nrm, c->n, c->np, c->nrmf, c->stream));
        }
        if (c->XK) HIPCHK(c, launch_swz_keys_b3(c->xcf, c->plan.KP, c->np, c->XK, c->stream));
    }
    return SVGD_OK;
}

int scale_begin(svgd_ctx *c)
{
    if (hipEventQuery(c->ev_scal) != hipSuccess) // the last [a, med] copy has read scal
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_scal, 0));
    const bool med = !(c->scale_method == SVGD_SCALE_FIXED || matrix_scale(c));
    // the median phase's start event goes before the centring (which it
    // needs): an event between two kernels costs a dispatch gap, so the last
    // step's phi end (a timing event) serves when there is one -- the phase
    // then also holds the gap between steps (a diagnostic only: these events
    // feed svgd_get_timing and nothing else)
    if (c->tm.timing && med) {
        EvPair ev = take_pair(c);
        if (c->last_phi_end) {
            ev.spare = ev.a;
            ev.a = c->last_phi_end;
        } else {
            HIPCHK(c, hipEventRecord(ev.a, c->stream));
        }
        c->tm.ev_med.push_back(ev);
    }
    c->last_phi_end = nullptr;
    c->trk_go = false;
    if (med) trk_plan(c);
    if (c->trk_go) {
        const SelState st = make_state(1, &c->trk_lo, c->trk_lo, c->trk_hi);
        CHK(center(c, &st));
    } else {
        CHK(center(c));
    }
    if (med) CHK(median_begin(c));
    c->co.coll_phase = 1; // every comm call of this phase is issued (upload_g_finish)
    return SVGD_OK;
}

int scale_finish(svgd_ctx *c)
{
    if (c->scale_method == SVGD_SCALE_HESSIAN && !c->ms.hess_ready)
        return fail(c, SVGD_ERR_UNSET,
                    "[Unset Error] Hessian scale: svgd_set_step_hessian_sum was not called this step.");
    if (matrix_scale(c)) {
        c->ms.hess_ready = false;
        return SVGD_OK;
    }
    if (c->scale_method == SVGD_SCALE_FIXED) {
        HIPCHK(c, launch_set_scal(c->fixed_a, NAN, c->scal, c->stream));
        HIPCHK(c, hipEventSynchronize(c->ev_scal)); // no D2H into h_scal pending
        c->h_scal[0] = c->fixed_a;
        c->h_scal[1] = NAN;
        c->scal_fresh = true;
        return SVGD_OK;
    }
    CHK(median_finish(c));
    // a synchronous selection joins the tracking history when resolved
    // (the speculative ones in resolve_pending)
    if (!c->spec_step) c->trk_sync = c->trk_keys ? 1 : 2;
    // [a, med] reach the host only when asked (fetch_scale): no copy on the
    // step's path; the event marks where this step's scale is final (on the
    // speculative path the status event, recorded right after the selection)
    if (c->med_ev_done) {
        c->ev_fin_use = c->ev_status_use;
    } else {
        if (c->tm.timing && !c->tm.ev_med.empty()) HIPCHK(c, hipEventRecord(c->tm.ev_med.back().b, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_fin, c->stream));
        c->ev_fin_use = c->ev_fin;
        c->mark = nullptr;
        CHK(mark_median_end(c));
    }
    c->med_ev_done = false;
    c->scal_fresh = false;
    return SVGD_OK;
}

// [a, med] of the last scale to h_scal (waits for the step's scale only).
int fetch_scale(svgd_ctx *c)
{
    if (c->scal_fresh) return SVGD_OK;
    if (c->status_seq && !c->ev_fin_use) HIPCHK(c, hipStreamSynchronize(c->stream)); // (no scale-final event)
    else HIPCHK(c, hipStreamWaitEvent(c->cstream, c->ev_fin_use ? c->ev_fin_use : c->ev_fin, 0));
    HIPCHK(c, hipMemcpyAsync(c->h_scal, c->scal, 2 * sizeof(double), hipMemcpyDeviceToHost,
                             c->cstream));
    HIPCHK(c, hipEventRecord(c->ev_scal, c->cstream));
    HIPCHK(c, hipEventSynchronize(c->ev_scal));
    c->scal_fresh = true;
    return SVGD_OK;
}

// Check the pending speculative step; on a failed device plan restore X_t,
// m_t, v_t, t and redo the step on the synchronous path (G_t is still on the
// device).  Every rank sees the same status (it derives from all-reduced
// counts), so the redo's collectives match across ranks.
int resolve_pending(svgd_ctx *c)
{
    CHK(trk_resolve_sync(c));
    if (!c->pending) return SVGD_OK;
    c->pending = false;
    if (c->status_seq) {
        // the selection's sequence number in pinned memory (median_finish_spec)
        // Polling: yields for the first 100 us, then 20 us sleeps (the
        // host-gradient threads share the CPUs), and the HIP runtime is asked
        // whether the stream drained at most once per ms, not per iteration
        // (it takes the runtime's locks the gradient worker's HIP calls need;
        // same-box A/B: equal at cfg3 / cfg2, cfg5 6.74-6.92 vs 6.78-7.77 ms
        // with the host gradient's spread 1.58-1.65 vs 1.60-1.97 ms)
        volatile uint64_t *sq = c->h_trk + TRK_SEQ;
        const auto t0 = std::chrono::steady_clock::now();
        auto t_idle = t0, t_query = t0;
        bool idle = false;
        while (*sq != c->status_seq) {
            const auto now = std::chrono::steady_clock::now();
            // the stream has drained and the number is still not there (a
            // bounded grace for the store's visibility): an error, not a hang
            if (!idle && now - t_query > std::chrono::milliseconds(1)) {
                t_query = now;
                if (hipStreamQuery(c->stream) == hipSuccess) {
                    idle = true;
                    t_idle = now;
                }
            }
            if (idle && now - t_idle > std::chrono::milliseconds(200))
                return fail(c, SVGD_ERR_RUNTIME, "[Runtime Error] the selection did not publish its status.");
            if (now - t0 > std::chrono::seconds(300))
                return fail(c, SVGD_ERR_RUNTIME, "[Runtime Error] timed out waiting for the median's status.");
            if (now - t0 < std::chrono::microseconds(100))
                std::this_thread::yield();
            else
                std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    } else {
        HIPCHK(c, hipEventSynchronize(c->ev_status_use ? c->ev_status_use : c->ev_status));
    }
    if (*c->h_status == 0) {
        c->last_tot = (int64_t)c->h_trk[TRK_TOT];
        if (c->trk.allowed) trk_record(c, c->h_trk[TRK_LO], c->h_trk[TRK_HI], c->h_trk[TRK_CAND]);
        return SVGD_OK;
    }
    c->trk.failed();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->cstream));
    // this rank's rows of X_t, m_t, v_t back, then X_t all-gathered again
    const size_t sb = sizeof(double) * (size_t)c->nrows * c->dim;
    const size_t cnt = (size_t)c->nrows * c->dim;
    if (c->nrows > 0) {
        HIPCHK(c, hipMemcpyAsync(c->X + (size_t)c->row0 * c->dim, c->bak, sb, hipMemcpyDeviceToDevice,
                                 c->stream));
        HIPCHK(c, hipMemcpyAsync(c->m, c->bak + cnt, sb, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->v, c->bak + 2 * cnt, sb, hipMemcpyDeviceToDevice, c->stream));
    }
    CHK(allgather_rows(c, c->X));
    c->t -= 1;
    c->spec_step = false;
    c->last_fast = false;
    c->xver -= 1; // X_t is back (its centre's partials were never overwritten)
    CHK(scale_begin(c));
    CHK(scale_finish(c));
    CHK(run_phi_opt(c));
    // the redo's selection (synchronous path) continues the tracking history
    return trk_resolve_sync(c);
}

// Speculate this step's median when the last one would have allowed it.
int plan_step(svgd_ctx *c)
{
    // (a step whose buckets outgrow the segment capacity fails its plan and
    // is redone synchronously)
    c->spec_cap = spec_segment_cap(c->last_tot);
    c->spec_step = c->knobs.speculate.or_(1) && c->last_fast && c->scale_method == SVGD_SCALE_MEDIAN &&
                   c->bucket_cap >= c->spec_cap;
    if (c->spec_step && !c->bak) CHK(dalloc(c, &c->bak, 3 * std::max<int64_t>(1, c->nrows) * c->dim));
    c->n_spec += c->spec_step ? 1 : 0;
    return SVGD_OK;
}

} // namespace svgd_amd

extern "C" {

int svgd_median_scale(svgd_ctx *c, double *a_out, double *med_out)
{
    CHK(check_results(c));
    CHK(resolve_pending(c));
    c->spec_step = false;
    const int keep = c->scale_method;
    c->scale_method = SVGD_SCALE_MEDIAN;
    int rc = scale_begin(c);
    if (rc == SVGD_OK) rc = scale_finish(c);
    c->scale_method = keep;
    c->trk_sync = 0; // not a step: X_t's median would enter the history twice
    c->co.coll_phase = 0;
    CHK(rc);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    CHK(fetch_scale(c));
    if (a_out) *a_out = c->h_scal[0];
    if (med_out) *med_out = c->h_scal[1];
    return SVGD_OK;
}

int svgd_last_scale(const svgd_ctx *c, double *a_out, double *med_out, int *path)
{
    if (!c) return SVGD_ERR_ARG;
    svgd_ctx *m = const_cast<svgd_ctx *>(c);
    CHK(resolve_pending(m));
    CHK(fetch_scale(m));
    if (a_out) *a_out = c->h_scal[0];
    if (med_out) *med_out = c->h_scal[1];
    if (path) *path = c->last_path;
    return SVGD_OK;
}

int svgd_last_median_keys(svgd_ctx *c, double *sq_lo, double *sq_hi, int64_t *rank_lo,
                          int64_t *rank_hi)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    SelState s;
    HIPCHK(c, hipMemcpy(&s, c->st, sizeof(SelState), hipMemcpyDeviceToHost));
    int64_t rlo, rhi;
    svgd_plan_median_ranks(c->n, &rlo, &rhi);
    auto val = [&](int src) {
        if (src < 0) return 0.0;
        double v;
        std::memcpy(&v, &s.prefix[src], sizeof(v));
        return v;
    };
    if (sq_lo) *sq_lo = val(c->sel.src_lo);
    if (sq_hi) *sq_hi = val(c->sel.src_hi);
    if (rank_lo) *rank_lo = rlo;
    if (rank_hi) *rank_hi = rhi;
    return SVGD_OK;
}

int svgd_set_median_tuning(svgd_ctx *c, int64_t direct_max_pairs, int64_t sample_size,
                           int64_t candidate_capacity)
{
    if (!c) return SVGD_ERR_ARG;
    CHK(resolve_pending(c));
    if (direct_max_pairs >= 0) c->direct_max_pairs = direct_max_pairs;
    if (sample_size > 0) c->sample_size = sample_size;
    if (candidate_capacity >= 0) c->cand_capacity = candidate_capacity;
    return SVGD_OK;
}

int svgd_debug_pair_keys(svgd_ctx *c, double *out, int64_t capacity)
{
    CHK(check_ready(c));
    CHK(resolve_pending(c));
    const int64_t M = upper_pairs(c->n);
    if (capacity < M) return fail(c, SVGD_ERR_ARG, "[Argument Error] Output buffer too small.");
    if (c->world != 1)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Debug keys are single-GPU only.");
    CHK(center(c));
    DevBuf<double> &d = c->dbg_keys; // (held for the call only)
    HIPCHK(c, d.alloc((size_t)std::max<int64_t>(1, M)));
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(c->own_tiles, 1024));
    hipError_t e = pair_pass(c, 2, grid, nullptr, 0, d);
    if (e == hipSuccess)
        e = hipMemcpyAsync(out, d, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    d.reset();
    HIPCHK(c, e);
    return SVGD_OK;
}

} // extern "C"
