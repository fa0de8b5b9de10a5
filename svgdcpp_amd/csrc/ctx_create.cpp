// ctx_create.cpp -- a context's creation (knobs, row and tile plan, buffers, host
// policy) and its destruction.
#include "ctx.h"
#include <omp.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "host_models.h"

using namespace svgd_amd;

namespace svgd_amd {
namespace {

// CPUs the cgroup (v2 cpu.max "quota period", v1 cfs files) allows this
// process, rounded down; 0 = no quota or unreadable
int cgroup_cpus()
{
    long long quota = -1, period = 0;
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0)
            quota = std::atoll(q);
        std::fclose(f);
    } else {
        if (FILE *f1 = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
            if (std::fscanf(f1, "%lld", &quota) != 1) quota = -1;
            std::fclose(f1);
        }
        if (FILE *f2 = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
            if (std::fscanf(f2, "%lld", &period) != 1) period = 0;
            std::fclose(f2);
        }
    }
    return (quota > 0 && period > 0) ? (int)(quota / period) : 0;
}

// Step 1: this rank's rows and its range of the median's pair tiles.
void plan_rows_tiles(svgd_ctx *c, int sim_world)
{
    const int64_t n = c->n;
    c->nb = (n + TB - 1) / TB;
    c->np = c->nb * TB + TB;
    c->chunk = (n + c->world - 1) / c->world;
    // svgd_create_sim (measurement only, one rank): run rank 0's share of a
    // P-rank step -- its rows of phi and the optimizer, 1/P of the median's
    // pair tiles with the order statistics' ranks scaled to that share, the
    // host gradient on the threads a rank of P gets -- on one GPU without
    // collectives, to time the per-rank work of a P-GPU run.  The results are
    // NOT the step's (no data from the other ranks): result calls refuse it.
    const int plan_world = c->world == 1 && sim_world > 1 ? sim_world : c->world;
    c->sim_world = plan_world != c->world ? plan_world : 1;
    c->plan_world = plan_world;
    svgd_plan_rows(n, plan_world, c->rank, &c->row0, &c->row1);
    c->nrows = c->row1 - c->row0;
    c->pblock = SVGD_PAIR_BLOCK_DT(c->dim, c->dtype);
    c->pnb = (n + c->pblock - 1) / c->pblock;
    c->own_tiles = svgd_plan_pair_tiles(n, c->pblock, plan_world, c->rank);
    c->tile0 = c->pnb * (c->pnb + 1) / 2 * c->rank / plan_world;
    if (c->sim_world > 1) { // real pairs of the share's tiles (diagonal tiles: upper half)
        for (int64_t t = 0; t < c->own_tiles; ++t) {
            int64_t I, J;
            svgd_plan_pair_tile(n, c->pblock, plan_world, c->rank, t, &I, &J);
            const int64_t ri = std::min<int64_t>(c->pblock, n - I * c->pblock);
            const int64_t rj = std::min<int64_t>(c->pblock, n - J * c->pblock);
            c->sim_pairs += I == J ? ri * (ri - 1) / 2 : ri * rj;
        }
    }
}

// The symmetric pass (plan.path == PHI_SYM): this rank's units, its tables and buffers.
int setup_sym(svgd_ctx *c, int ncu)
{
    const int dim = c->dim;
    const int64_t n = c->n;
    if (!phi_sym_geom(dim, &c->sym.B, &c->sym.SRS, &c->sym.NSUB))
        return fail(c, SVGD_ERR_DIM, "[Dimension Error] The symmetric phi pass has no geometry for this dimension.");
    const int64_t B = c->sym.B;
    c->sym.nb = (n + B - 1) / B;
    c->sym.units = svgd_plan_sym_total(n, (int)B, c->sym.NSUB); // (no padding-only sub-tiles)
    const int64_t Pw = c->plan_world, r = c->sim_world > 1 ? 0 : c->rank;
    const int64_t slots = (int64_t)phi_sym_blocks_per_cu(dim) * ncu;
    const int64_t Vr = c->sym.units * (r + 1) / Pw - c->sym.units * r / Pw;
    c->sym.grid = (int)std::max<int64_t>(1, std::min<int64_t>(Vr, slots));
    // the rank's units, the row blocks each work-group's contiguous run
    // visits and each row block's contiguous row-sum records (plan.cpp)
    const int64_t nbs = c->sym.nb;
    std::vector<int> tab(3 * (size_t)nbs + 2 * (size_t)c->sym.grid);
    int *blkg = tab.data(), *rbase = blkg + 2 * nbs, *wst = rbase + nbs;
    const int64_t nrec = svgd_plan_sym_units(n, (int)B, c->sym.NSUB, (int)Pw, (int)r, c->sym.grid,
                                             &c->sym.u0, &c->sym.u1, blkg, rbase, &c->sym.Ia, &c->sym.Ib);
    // each work-group's first unit (the kernel advances from there)
    for (int g = 0; g < c->sym.grid; ++g) {
        const int64_t V = c->sym.u1 - c->sym.u0;
        int64_t t = 0, q = 0;
        svgd_plan_sym_unit(n, (int)B, c->sym.NSUB, c->sym.u0 + V * g / c->sym.grid, &t, &q);
        wst[2 * g] = (int)t;
        wst[2 * g + 1] = (int)q;
    }
    {
        const int64_t sub = B / c->sym.NSUB, valid = n - (nbs - 1) * B;
        c->sym.qlast = (int)((valid + sub - 1) / sub);
    }
    c->sym.SM = (nbs - 1) / 2 + 2;
    // the row stream's hand-over inside k_phi_sym (symok = 0): its
    // 8-wave work-groups, one wave of them (<= c->S, the part buffer's splits)
    {
        const int64_t rows_wg = rows_geom(ROWS_8W).rows_per_wg(phi_rows_per_lane(dim));
        const int64_t ib = std::max<int64_t>(1, (c->nrows + rows_wg - 1) / rows_wg);
        c->sym.fS = (int)std::max<int64_t>(1, std::min<int64_t>(c->S, ncu / ib));
    }
    CHK(dalloc(c, &c->sym.tab, (int64_t)tab.size()));
    HIPCHK(c, hipMemcpyAsync(c->sym.tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice,
                             c->stream)); // (after dalloc's memset on the same stream)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    CHK(dalloc(c, &c->sym.srec, c->sym.nb * B * c->sym.SRS));
    CHK(dalloc(c, &c->sym.rowpart, nrec * B * (dim + 1)));
    // zeroed here once: entries no unit of this rank writes stay zero
    CHK(dalloc(c, &c->sym.colpart, nbs * c->sym.SM * B * (dim + 1)));
    CHK(dalloc(c, &c->sym.ok, 1));
    CHK(dalloc(c, &c->sym.tab8k, 8192));
    HIPCHK(c, launch_fill_tab8k(c->sym.tab8k, c->stream));
    // (SVGD_PHI_SYM=2, a test knob: the P > 1 form -- sums, exchange call site, apply -- at any P)
    if (Pw > 1 || c->knobs.phi_sym.or_(-1) == 2)
        CHK(dalloc(c, &c->sym.contrib, std::max<int64_t>(c->np, c->world * c->chunk) * (dim + 1)));
    if (c->world > 1) {
        // the exchange plan: the same ranges on both sides of every pair of ranks
        c->sym.xsend.assign(2 * (size_t)c->world, 0);
        c->sym.xrecv.assign(3 * (size_t)c->world, 0);
        for (int q = 0; q < c->world; ++q) {
            int64_t a, b;
            svgd_plan_sym_exchange(n, (int)B, c->sym.NSUB, c->world, c->rank, q, &a, &b);
            c->sym.xsend[2 * q] = a;
            c->sym.xsend[2 * q + 1] = q == c->rank ? a : b; // (its own rows: not sent)
            svgd_plan_sym_exchange(n, (int)B, c->sym.NSUB, c->world, q, c->rank, &a, &b);
            if (q != c->rank && b > a) {
                c->sym.xrecv[3 * q] = a;
                c->sym.xrecv[3 * q + 1] = b;
                c->sym.xrecv[3 * q + 2] = c->sym.xrecv_rows;
                c->sym.xrecv_rows += b - a;
            }
        }
        CHK(dalloc(c, &c->sym.xrecv_buf, std::max<int64_t>(1, c->sym.xrecv_rows) * (dim + 1)));
        HIPCHK(c, c->sym.xtab_d.alloc(c->sym.xrecv.size()));
        HIPCHK(c, hipMemcpy(c->sym.xtab_d, c->sym.xrecv.data(), c->sym.xrecv.size() * sizeof(int64_t),
                            hipMemcpyHostToDevice));
    }
    return SVGD_OK;
}

// The row stream's records, column splits and partials (+ the symmetric pass).
int alloc_phi_rows(svgd_ctx *c)
{
    const PhiPlan &p = c->plan;
    const int dim = c->dim;
    const int64_t n = c->n;
    int ncu = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess) ncu = prop.multiProcessorCount;
    // column splits of a launch over `rows` rows: enough work-groups to fill
    // every CU at the kernel's occupancy, 2 blocks per resident slot: one
    // block wave per slot left a tail of idle CUs (measured at cfg3, phi
    // launch: S x1 4.00 ms, x2 3.83-3.93, x4 3.81-3.90, x8 3.91-3.95 -- x2
    // and x4 tie, x2 has half the partials)
    const int64_t resident = (int64_t)phi_rows_blocks_per_cu(dim, p.rows_kind) * ncu;
    const int64_t rows_wg = rows_geom(p.rows_kind).rows_per_wg(p.R);
    auto splits = [&](int64_t rows) {
        constexpr int split_mult = 2;
        const int64_t ib = std::max<int64_t>(1, (rows + rows_wg - 1) / rows_wg);
        const int64_t s = std::max<int64_t>(1, (resident + ib - 1) / ib) * split_mult;
        return (int)std::min<int64_t>(s, std::max<int64_t>(1, n / 256));
    };
    c->S = splits(c->nrows);
    c->RS = phi_rec_stride(dim);
    c->ldp = std::max<int64_t>(1, c->nrows);
    // two row parts (svgd_step_host_model at P > 1, split_rows policy in
    // host_policy): the first part's rows get their X_{t+1} while the second
    // part's phi still runs; the second part's gradient has to fit in the
    // next step's median phase.  Each launch takes its own column splits.
    // First part SVGD_PHI_SPLIT_FRAC percent of the rows, default 50
    // (cfg3 8-rank share, profiles/r04_sim_world.jsonl: 50 % 0.632 ms,
    // 62 % 0.783, 72 % 0.765 -- uneven parts made phi itself 40 % slower)
    c->hs.split_h = (c->nrows * c->knobs.phi_split_frac.or_(50) / 100) / rows_wg * rows_wg;
    if (c->hs.split_h >= c->nrows) c->hs.split_h = 0;
    if (c->hs.split_h > 0) {
        c->hs.S2 = splits(c->hs.split_h);
        c->hs.S2b = splits(c->nrows - c->hs.split_h);
    }
    CHK(dalloc(c, &c->rec, c->np * c->RS));
    CHK(dalloc(c, &c->xf, c->np * med_f32_stride(dim)));
    CHK(dalloc(c, &c->nmax, 2)); // one slot per X version parity (center)
    CHK(dalloc(c, &c->part, std::max({(int64_t)c->S * c->ldp, (int64_t)c->hs.S2 * c->hs.split_h,
                                      (int64_t)c->hs.S2b * (c->nrows - c->hs.split_h)}) * (dim + 1)));
    if (p.path == PHI_SYM) CHK(setup_sym(c, ncu));
    // the centring fold (svgd_ctx::cpart)
    c->cpart_stride = (int64_t)center_fold_grid(dim, c->np) * dim;
    CHK(dalloc(c, &c->cpart, 2 * c->cpart_stride));
    return SVGD_OK;
}

// Step 3: the particles, their centred copies and the planned phi path's operands.
int alloc_phi(svgd_ctx *c)
{
    const PhiPlan &p = c->plan;
    const int dim = c->dim;
    const int64_t rows_all = c->chunk * c->world;
    CHK(dalloc(c, &c->X, rows_all * dim));
    CHK(dalloc(c, &c->G, rows_all * dim));
    CHK(dalloc(c, &c->xc, c->np * p.KP));
    CHK(dalloc(c, &c->nrm, c->np));
    CHK(dalloc(c, &c->cvec, c->np));
    if (c->dtype == SVGD_F32) {
        CHK(dalloc(c, &c->xcf, c->np * p.KP));
        CHK(dalloc(c, &c->nrmf, c->np));
        CHK(dalloc(c, &c->cvf, c->np));
        // KP 32 / 64: the median keys on the bf16 matrix cores (their parts)
        if (const int64_t w = median_key_part_words(p.KP, c->np)) CHK(dalloc(c, &c->XK, w));
    }
    if (!p.rows()) CHK(dalloc(c, &c->V, c->np * p.VW));
    switch (p.path) {
    case PHI_SYM:
    case PHI_ROWS:
        CHK(alloc_phi_rows(c));
        break;
    case PHI_B3: // np is a multiple of 2 TBJ_COLS: ceil(n / TBJ_COLS) tiles fit
        CHK(dalloc(c, &c->B3, (c->np / TBJ_COLS) * phi_b3_tile_words(p.KP, p.NCB)));
        break;
    case PHI_F32S:
        CHK(dalloc(c, &c->XS, c->np * p.KP));
        CHK(dalloc(c, &c->VS, c->np * 16 * (p.NCB + 1)));
        break;
    case PHI_TILE_F32: // the row-major fp32 copy of V
        CHK(dalloc(c, &c->Vf, c->np * p.VW));
        break;
    case PHI_TILE_F64:
        break;
    }
    CHK(dalloc(c, &c->phi, std::max<int64_t>(1, c->nrows) * dim));
    CHK(dalloc(c, &c->m, std::max<int64_t>(1, c->nrows) * dim));
    CHK(dalloc(c, &c->v, std::max<int64_t>(1, c->nrows) * dim));
    CHK(dalloc(c, &c->lower, dim));
    CHK(dalloc(c, &c->upper, dim));
    CHK(dalloc(c, &c->partial, (int64_t)c->nparts * dim));
    CHK(dalloc(c, &c->scal, 2));
    return SVGD_OK;
}

// Step 4: the median's buffers and its knobs.
int alloc_median(svgd_ctx *c)
{
    const Knobs &k = c->knobs;
    CHK(dalloc(c, &c->counts, 4 * MAX_COLLECT_BLOCKS)); // <= 4 regions per collect block
    CHK(dalloc(c, &c->below, 4 * MAX_COLLECT_BLOCKS));
    CHK(dalloc(c, &c->cnt3, CNT_LEN + 3));
    CHK(dalloc(c, &c->bpart, (int64_t)MAX_COLLECT_BLOCKS * NBK));
    CHK(dalloc(c, &c->gseg, (int64_t)c->world * (CAPG + 1)));
    c->bucket_cap = k.bucket_cap.or_(c->bucket_cap);
    c->sample_size = k.median_sample.or_(c->sample_size);
    c->bracket_sigma = k.median_sigma.or_(c->bracket_sigma);
    // A/B and test knob (SVGD_COLLECT_FP64=1): the reference collect passes
    // (k_pair_rows / k_pair_tiles MODE 0) instead of the matrix-core ones
    // (k_pair_mcol / k_pair_tcol)
    c->mcol = k.mcol.or_(c->mcol);
    // k_pair_mcol's Gram as split bf16 (d <= 8; SVGD_MCOL_BF16=0: f32): its operands (center)
    if (c->xf && c->mcol && k.mcol_bf16.or_(1) && c->dim <= 8) {
        CHK(dalloc(c, &c->xsplit, c->np * 8));
        c->collect_blocks = 1280; // k_pair_mcol<D, true>: 5 work-groups per CU (31 KiB LDS, <= 96 VGPRs)
    }
    CHK(dalloc(c, &c->st, 1));
    CHK(dalloc(c, &c->ghist, 2 * RADIX));
    CHK(dalloc(c, &c->ccount, 1));
    CHK(dalloc(c, &c->d_status, 1));
    c->trk.allowed = k.track_bracket.or_(c->trk.allowed);
    c->trk.min_width = k.track_min_width.or_(c->trk.min_width);
    // A miss redoes the step; the band it saves is collect-pass work, which
    // outweighs the misses' cost only when the collect is large: 2.5 x the
    // recent error from N = 32768 up (cfg3: median phase 0.550 -> 0.513 ms,
    // 86 instead of 72 of 90 steps tracked, no miss in 360), 4 below (cfg2
    // at 2.5: 3 misses in 180 steps, slower) -- profiles/r04_track_mult_ab.txt
    c->trk.err_mult = k.track_err_mult.or_(c->n >= 32768 ? 2.5 : 4.0);
    return SVGD_OK;
}

// Step 5: pinned host memory and the events.
int alloc_host(svgd_ctx *c)
{
    const size_t hn = (size_t)std::max<int64_t>(1, c->nrows) * c->dim, hb = sizeof(double) * hn;
    HIPCHK(c, c->h_x.alloc(hn, hipHostMallocDefault));
    HIPCHK(c, c->h_g.alloc(hn, hipHostMallocDefault));
    c->hs.xmirror = c->knobs.x_mirror.or_(hb <= XMIRROR_MAX);
    if (c->hs.xmirror) {
        // coherent: the update epilogue writes it uncached (the host reads it
        // once the step's end event has passed); only a mirroring context pins it
        HIPCHK(c, c->hs.h_xm.alloc(hn, hipHostMallocCoherent));
        HIPCHK(c, hipHostGetDevicePointer((void **)&c->hs.h_xm_dev, c->hs.h_xm, 0));
    }
    HIPCHK(c, c->h_cnt.alloc(CNT_LEN + 3, hipHostMallocDefault));
    HIPCHK(c, c->h_scal.alloc(2, hipHostMallocDefault));
    for (Event *e : {&c->ev_x, &c->ev_xready, &c->ev_g, &c->ev_cnt, &c->ev_scal, &c->ev_fin,
                     &c->ev_status, &c->hs.ev_xhalf})
        HIPCHK(c, e->create(hipEventDisableTiming));
    for (Event &e : c->hs.ev_xch) HIPCHK(c, e.create(hipEventDisableTiming));
    HIPCHK(c, c->h_status.alloc(1, hipHostMallocCoherent));
    *c->h_status = 0;
    HIPCHK(c, hipHostGetDevicePointer((void **)&c->h_status_dev, c->h_status, 0));
    HIPCHK(c, c->h_trk.alloc(TRK_LEN, hipHostMallocCoherent));
    std::memset(c->h_trk, 0, TRK_LEN * sizeof(uint64_t));
    HIPCHK(c, hipHostGetDevicePointer((void **)&c->h_trk_dev, c->h_trk, 0));
    return SVGD_OK;
}

// Step 6: the host gradient's threads and whether phi runs in two row parts.
void host_policy(svgd_ctx *c)
{
    // half the OpenMP threads, but no more than this rank's share of the
    // cgroup CPU quota (ranks of one node share it; OpenMP sees the affinity
    // mask, not the quota) and at most 32 (the gradient of a 65536-row share
    // takes 0.4 ms on 8 threads, hidden behind the device median).  A
    // measurement context (svgd_create_sim) models rank 0 of a P-GPU node:
    // the pool leases CPUs per GPU (16 with each MI355X), so that rank's
    // share of the node's quota is this one-GPU box's whole quota
    // (SVGD_HOST_THREADS=2 reproduces the 16-CPU box split 8 ways, the
    // pessimistic bound of rounds 3-5).
    int t = std::max(1, omp_get_max_threads() / 2);
    c->cpu_quota = cgroup_cpus();
    const int sharing = c->sim_world > 1 ? 1 : std::max(1, c->plan_world);
    if (c->cpu_quota > 0) t = std::min(t, std::max(1, c->cpu_quota / sharing));
    c->hs.host_threads = c->knobs.host_threads.or_(std::min(t, 32));
    // phi in row halves when a rank of 4 or more has more rows per gradient
    // thread than the device's median phase hides: then phi waited for G;
    // with halves the first half's gradient runs beside the second half's
    // phi (cost: a second phi launch and reduce, ~20 us at P = 8).  AVX2
    // gradient block (~18 us per 1000 rows and thread at cfg3's GMM): split
    // above 2048 rows per thread (profiles/r04_sim_world: P = 8 at 2 threads
    // 0.714 -> 0.656 ms).  AVX-512 block (~7 us per 1000 rows and thread on
    // the EPYC 9575F): the whole-rows step wins at P = 8 and 4
    // (profiles/r05_sim_split_ab.txt: 0.580 vs 0.598 ms, 1.052 vs 1.077 ms),
    // split above 8192 rows per thread.  SVGD_PHI_SPLIT replaces the policy,
    // not the need for a row stream with a first part.
    const int64_t per_thread = svgd_amd::host_grad_avx512() ? 8192 : 2048;
    const bool policy = c->plan_world >= 4 && c->nrows > per_thread * (int64_t)std::max(1, c->hs.host_threads);
    c->hs.split_rows = c->rowpath && c->hs.split_h > 0 && c->knobs.phi_split.or_(policy);
}

// A context's creation, after its knobs, world and rank are set.
int init_ctx(svgd_ctx *c, int dim, int64_t n, int dtype, int device, int sim_world = 1)
{
    if (dim <= 0 || n <= 0)
        return fail(c, SVGD_ERR_DIM, "[Dimension Error] Particle count and dimension must be positive.");
    if (dtype != SVGD_F64 && dtype != SVGD_F32)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] dtype must be SVGD_F64 or SVGD_F32.");
    c->dim = dim;
    c->n = n;
    c->dtype = dtype;
    c->device = device;
    plan_rows_tiles(c, sim_world);
    if (!plan_phi(dim, n, dtype, c->plan_world, c->row0, c->knobs, built_caps(dim, dtype), &c->plan))
        return fail(c, SVGD_ERR_DIM, "[Dimension Error] Device path supports dimension <= 64.");
    c->rowpath = c->plan.rows();
    HIPCHK(c, hipSetDevice(device));
    HIPCHK(c, c->stream.create());
    HIPCHK(c, c->cstream.create());
    CHK(alloc_phi(c));
    CHK(alloc_median(c));
    CHK(alloc_host(c));
    host_policy(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SVGD_OK;
}

} // namespace

// ------------------------------------------------------------- creation --

// The environment, read once per context: every SVGD_* variable the library
// knows is named here, next to its Knobs field, and nowhere else.  Parsing
// only -- what an unset knob defaults to is decided where it is used.
Knobs read_knobs()
{
    auto get = [](const char *name, auto parse, auto *knob) {
        if (const char *e = std::getenv(name)) {
            knob->set = true;
            knob->v = parse(e);
        }
    };
    auto onoff = [](const char *e) { return (int)(std::atoi(e) != 0); };
    auto real = [](const char *e) { return std::atof(e); };
    Knobs k;
    k.phi_tile_generic = std::getenv("SVGD_PHI_TILE_GENERIC") != nullptr;
    get("SVGD_PHI_B3", onoff, &k.phi_b3);
    get("SVGD_PHI_S1V", onoff, &k.phi_s1v);
    get("SVGD_PHI_B3_RG", [](const char *e) { return std::atoi(e) == 2 ? 2 : 1; }, &k.phi_b3_rg);
    get("SVGD_PHI_SYM", [](const char *e) { return std::atoi(e); }, &k.phi_sym);
    get("SVGD_PHI_SPLIT", onoff, &k.phi_split);
    get("SVGD_PHI_SPLIT_FRAC", [](const char *e) { return std::min(90, std::max(10, std::atoi(e))); },
        &k.phi_split_frac);
    get("SVGD_X_MIRROR", onoff, &k.x_mirror);
    get("SVGD_BUCKET_CAP", [](const char *e) { return (int64_t)std::atoll(e); }, &k.bucket_cap);
    get("SVGD_MEDIAN_SAMPLE", [](const char *e) { return std::max<int64_t>(1, std::atoll(e)); },
        &k.median_sample);
    get("SVGD_MEDIAN_SIGMA", [](const char *e) { return std::max(0.0, std::atof(e)); }, &k.median_sigma);
    get("SVGD_COLLECT_FP64", [](const char *e) { return (int)(std::atoi(e) == 0); }, &k.mcol);
    get("SVGD_MCOL_BF16", onoff, &k.mcol_bf16);
    get("SVGD_SPECULATE", onoff, &k.speculate);
    get("SVGD_TRACK_BRACKET", onoff, &k.track_bracket);
    get("SVGD_TRACK_MIN_WIDTH", real, &k.track_min_width);
    get("SVGD_TRACK_ERR_MULT", real, &k.track_err_mult);
    get("SVGD_HOST_THREADS", [](const char *e) { return std::max(1, std::atoi(e)); }, &k.host_threads);
    get("SVGD_DEBUG_COLL", onoff, &k.debug_coll);
    get("SVGD_G_COMM", onoff, &k.g_comm);
    get("SVGD_HOSTCOMM", [](const char *e) { return std::string(e); }, &k.hostcomm);
    get("SVGD_THIN_SELECT", onoff, &k.thin_select);
    return k;
}

// What the kernel translation unit has built for (dim, dtype): the lists of
// built.h, with the wave counts of this build
PhiCaps built_caps(int dim, int dtype) { return phi_caps(dim, dtype == SVGD_F32, phi_build()); }

} // namespace svgd_amd

extern "C" {

int svgd_create(svgd_ctx **out, int dim, int64_t n, int dtype, int device)
{
    return svgd_create_sim(out, dim, n, dtype, device, 1); // (a world of one: nothing simulated)
}

int svgd_create_sim(svgd_ctx **out, int dim, int64_t n, int dtype, int device, int sim_world)
{
    if (!out) return SVGD_ERR_ARG;
    svgd_ctx *c = new svgd_ctx();
    *out = c;
    c->knobs = read_knobs();
    if (sim_world < 1) return fail(c, SVGD_ERR_ARG, "[Argument Error] Invalid simulated world size.");
    return init_ctx(c, dim, n, dtype, device, sim_world);
}

int svgd_create_dist(svgd_ctx **out, int dim, int64_t n, int dtype, int device, int world,
                     int rank, const void *unique_id128)
{
    if (!out) return SVGD_ERR_ARG;
    svgd_ctx *c = new svgd_ctx();
    *out = c;
    c->knobs = read_knobs();
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && !unique_id128 && !c->knobs.hostcomm.set))
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Invalid world/rank.");
    c->world = world;
    c->rank = rank;
    CHK(init_ctx(c, dim, n, dtype, device));
    return comm_create(c, unique_id128);
}

// A context, however far its creation got: the owning members free what was
// allocated when the context is deleted.
int svgd_destroy(svgd_ctx *c)
{
    if (!c) return SVGD_OK;
    c->hs.join(); // idle between steps: joins the gradient thread
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->cstream) (void)hipStreamSynchronize(c->cstream);
    if (c->co.gstream) (void)hipStreamSynchronize(c->co.gstream);
    comm_destroy(c); // gcomm, comm, the host communicator
    delete c;
    return SVGD_OK;
}

} // extern "C"
