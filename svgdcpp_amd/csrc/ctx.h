// ctx.h -- the runtime's context (svgd_ctx) and what its units share.
//
// One context = one GPU (one process per GPU in multi-GPU runs).  The context
// owns every resource it allocates (resource.h): deleting it frees them all.
// State that one unit alone reads or writes sits in that unit's group (co,
// sym, ms, hs, tm, dm, ksd, ksdq, mmd, thin, pred, imq); what several units share stays flat.  The units
// (ctx_*.cpp, svgd_capi.cpp) call each other through the functions declared
// at the end, per unit.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/svgdcpp_amd/svgd_capi.h"
#include "svgd_kernels.h"
#include "plan.h"
#include "median_plan.h"
#include "hostcomm.h"
#include "resource.h"

namespace svgd_amd {

constexpr int64_t TB = 64;
constexpr int XCH = 8; // row chunks of the pipelined host-gradient step
constexpr int64_t TBJ_COLS = 32; // column tile of k_phi_f32s (TBJ in svgd_kernels.hip)
constexpr int64_t MAX_COLLECT_BLOCKS = 2048; // collect-pass grid limit (buffer sizes)
constexpr size_t XMIRROR_MAX = size_t(1) << 20; // shard bytes for the host mirror / G host read

struct EvPair {
    hipEvent_t a, b;
    hipEvent_t spare = nullptr; // a's own event when a is a shared mark (back to the pool)
};

// diagnostic event kinds (svgd_set_timing level 2; svgd_get_diagnostics)
enum { DG_PHI_KERNEL = 0, DG_PHI_WAIT = 1, DG_COLL = 2, DG_GATHER_G = 3 };

class HostWorker; // svgd_step_host_model's gradient thread (ctx_host_step.cpp)

} // namespace svgd_amd

struct svgd_ctx {
    int dim = 0;
    int64_t n = 0;
    int dtype = SVGD_F64;
    int device = 0;
    int world = 1, rank = 0;
    // svgd_create_sim (measurement only): rank 0's share of a P-rank step on
    // one GPU; every result-returning call refuses such a context
    int sim_world = 1;
    int64_t sim_pairs = 0; // the unordered pairs in that share's tiles
    int plan_world = 1;    // ranks the rows and pair tiles are planned for (world or sim_world)
    int cpu_quota = 0;     // the cgroup's CPUs (0: no quota), shared by plan_world ranks
    // the communicators and their step-order bookkeeping (ctx_comm.cpp)
    struct Comm {
        ncclComm_t comm = nullptr;
        // a second communicator (ncclCommSplit of comm) for the G all-gather on
        // its own stream: it overlaps the median chain's kernels and collectives
        // (one communicator's operations would run in issue order behind them).
        // On by default for P >= 2 over RCCL since round 6 (SVGD_G_COMM=0 on
        // every rank keeps the G all-gather on comm; =1 also splits a one-rank
        // communicator, the test form); the split's outcome is agreed across
        // ranks.
        //
        // Cross-communicator issue order (the invariant both communicators rely
        // on): within a step every rank issues
        //   comm:  the counts all-reduce [+ the keys all-gather when speculative]
        //          (scale_begin, all of it before returning)
        //   gcomm: the G all-gather                   (upload_g_finish)
        //   comm:  [the keys all-gather when synchronous] + the X all-gather
        // -- the same sequence on every rank because every branch in it depends on
        // all-reduced state only.  upload_g_finish checks that scale_begin has
        // issued its comm calls (coll_phase); SVGD_DEBUG_COLL=1 also all-gathers a
        // hash of each step's collective sequence and fails on any mismatch.
        ncclComm_t gcomm = nullptr;
        int coll_phase = 0;      // 0 step not begun, 1 scale_begin's comm calls issued, 2 G gathered
        uint64_t coll_sig = 0;   // FNV hash of this step's collectives (communicator, op, count)
        svgd_amd::DevBuf<uint64_t> sig_buf; // world u64 (the debug all-gather)
        svgd_amd::DevBuf<int> d_ok;         // the G communicator's agreed split outcome (creation)
        svgd_amd::Stream gstream;
        svgd_amd::Event ev_gg;        // G all-gathered (gstream)
        bool gg_pending = false;      // phi must wait for ev_gg
        svgd_amd::HostComm *hcomm = nullptr; // SVGD_HOSTCOMM rehearsal backend (ranks sharing one GPU)
        bool any() const { return comm || hcomm; } // more than this rank's data in a collective
    } co;
    // the device models (ctx_models.cpp); has_device_model is the one test
    // for which is set
    struct DeviceModels {
        // device mirror of a built-in Gaussian-sum model (svgd_set_device_model)
        int k = 0;
        svgd_amd::DevBuf<double> mu, prec;
        // device mirror of a generalized linear model (svgd_set_device_glm); at
        // most one of the two device models is set (k > 0 or glm.m > 0)
        struct Glm {
            int64_t m = 0;                // data rows (0: no device GLM)
            int link = 0;
            double lik_scale = 1, prior_prec = 0;
            int64_t m0 = 0, count = 0;    // batch window
            svgd_amd::DevBuf<double> rec;  // glm_padded(m) records of glm_rec_stride(d) doubles
            svgd_amd::DevBuf<double> part; // smax x ldp x d partial sums
            int smax = 1;                 // data splits that fill the device at most twice
            int64_t ldp = 0;
        } glm;
        // device Hessian sum of the device model (svgd_device_neg_hess_sum, and
        // the Hessian-scale step's when `on`: svgd_set_device_hessian)
        struct Hess {
            bool on = false;
            int64_t resident = 1;           // work-group slots of the GLM weight pass
            svgd_amd::DevBuf<double> wpart; // GLM: per-split weight sums
            svgd_amd::DevBuf<double> W;     // GLM: W_m of the window
            svgd_amd::DevBuf<double> part;  // per-block d x d (GLM: triangle) partial sums
            svgd_amd::DevBuf<double> out;   // d x d, the observer's result
        } hess;
    } dm;
    int64_t row0 = 0, row1 = 0, nrows = 0, chunk = 0;
    svgd_amd::Knobs knobs;  // the environment, read once at creation (read_knobs)
    svgd_amd::PhiPlan plan; // the phi kernel of this context and its launch parameters (plan_phi)
    int64_t nb = 0, np = 0; // row blocks; padded rows of the work arrays
    svgd_amd::Stream stream;

    // device buffers
    svgd_amd::DevBuf<double> X;   // world*chunk x d (first n rows are the particles)
    svgd_amd::DevBuf<double> G;   // world*chunk x d
    svgd_amd::DevBuf<double> xc;  // np x KP
    svgd_amd::DevBuf<double> nrm; // np
    svgd_amd::DevBuf<double> cvec;
    svgd_amd::DevBuf<double> V;   // np x VW
    svgd_amd::DevBuf<double> phi; // nrows x d
    svgd_amd::DevBuf<double> m, v;
    svgd_amd::DevBuf<double> lower, upper;
    svgd_amd::DevBuf<double> partial;
    int nparts = 64;
    svgd_amd::DevBuf<double> scal; // [0] a, [1] med
    // SVGD_F32: fp32 copies feeding the tile kernels
    svgd_amd::DevBuf<float> xcf, nrmf, cvf, Vf;
    svgd_amd::DevBuf<float> XS, VS; // operand-ordered column copies (k_phi_f32s)
    svgd_amd::DevBuf<uint32_t> B3;  // operand-ordered bf16 parts (k_phi_b3), replaces XS / VS
    svgd_amd::DevBuf<uint32_t> XK;  // F32 median key parts, KP 32 / 64 (svgd_device.h)

    // row-stream path (d <= ROWS_MAX_D): plan.rows(), which the median's
    // kernels follow too
    bool rowpath = false;
    int RS = 0;                         // record stride 2d+2
    svgd_amd::DevBuf<double> rec;       // np x RS particle records
    svgd_amd::DevBuf<double> part;      // S x ldp x (d+1) phi partials
    svgd_amd::DevBuf<float> xf;         // np x med_f32_stride(d) fp32 median records
    svgd_amd::DevBuf<unsigned long long> nmax; // max |xc|^2 (double bits)
    int S = 1;
    int64_t ldp = 0;
    // symmetric phi pass (k_phi_sym, d <= 8; plan.path == PHI_SYM): geometry and buffers
    struct Sym {
        int B = 0, SRS = 0, NSUB = 0, grid = 0;
        int64_t nb = 0, units = 0, u0 = 0, u1 = 0; // all units, this rank's [u0, u1)
        int fS = 1; // the row stream's column splits when it takes the step (ok = 0)
        int64_t SM = 0, Ia = 0, Ib = 0; // colpart slots per column block; units' row-block span
        int qlast = 0; // real sub-tiles of the last column block
        svgd_amd::DevBuf<double> srec, rowpart, colpart, tab8k;
        svgd_amd::DevBuf<double> contrib; // P > 1: every particle's sums from this rank's units (exchanged)
        // P > 1 over a communicator: the point-to-point exchange of those sums
        // (svgd_plan_sym_exchange): per rank q the rows [xsend[2q], xsend[2q+1])
        // sent to q, the rows [xrecv[3q], xrecv[3q+1]) of this rank received from
        // q into xrecv_buf + xrecv[3q+2] rows (xtab_d: xrecv on the device)
        std::vector<int64_t> xsend, xrecv;
        int64_t xrecv_rows = 0;
        svgd_amd::DevBuf<double> xrecv_buf;
        svgd_amd::DevBuf<int64_t> xtab_d;
        svgd_amd::DevBuf<int> tab;    // the symmetric pass tables (SymArgs::blkg | rbase | wst)
        svgd_amd::DevBuf<int> ok;
    } sym;

    // median
    int64_t direct_max_pairs = int64_t(1) << 24;
    int64_t sample_size = 0; // 0: auto, clamp(M / 256, 2^18, 2^22) for M pairs
    double bracket_sigma = 3.0; // sample-quantile standard deviations either side
    // P > 1: every rank draws the whole (smaller, <= 2^20) bracket sample of
    // the one counter-based sequence and derives the same bracket locally --
    // no histogram all-reduces in the step (two RCCL calls cost more than
    // sampling 2^20 pairs).  (shard_sample: round 2's protocol, ranks drew
    // disjoint parts of a full-size sample and all-reduced its two radix
    // histograms; kept off -- tests/test_multirank_cpu.py pins it on CPU)
    bool shard_sample = false;
    int64_t collect_blocks = 1024; // collect-pass work-groups (4 per CU resident; 5 for the bf16-split mcol)
    bool mcol = true;              // bracket collect on the matrix cores (k_pair_mcol / _tcol)
    svgd_amd::DevBuf<uint32_t> xsplit; // its operands, [hi | lo] bf16 x 8 per particle (the centring writes them)
    double band_est = 1.0;         // this step's bracket (sampled or predicted): expected share of the pairs
    svgd_amd::SamplePlan samp;     // this step's bracket sample (trk_plan; its draw: median_begin)
    int64_t cand_capacity = 0; // 0 = automatic
    svgd_amd::DevBuf<uint64_t> sample_keys;
    int64_t sample_alloc = 0;
    svgd_amd::DevBuf<uint64_t> regions;
    int64_t regions_alloc = 0;
    svgd_amd::DevBuf<uint64_t> cbuf;          // compacted candidates (regions_alloc keys)
    svgd_amd::DevBuf<unsigned long long> ccount;
    svgd_amd::DevBuf<uint32_t> bpart;         // collect blocks' key-range bucket histograms (max blocks x NBK)
    svgd_amd::DevBuf<uint64_t> gseg;          // world x (CAPG + 1): compacted selected-bucket keys
    int64_t bucket_cap = svgd_amd::CAPG;      // bucket select path if the selected buckets hold <= this
    int64_t last_tot = 0;              // the last selection's selected-bucket keys (all ranks)
    int64_t spec_cap = svgd_amd::CAPR_MIN;    // this speculative step's segment capacity (spec_segment_cap)
    svgd_amd::DevBuf<uint32_t> counts;
    svgd_amd::DevBuf<unsigned long long> below;
    int collect_grid = 0;
    int64_t nregions = 0; // candidate regions: one per wave (row-stream) or per block (tiles)
    svgd_amd::DevBuf<unsigned long long> cnt3;
    svgd_amd::DevBuf<svgd_amd::SelState> st;
    svgd_amd::DevBuf<unsigned long long> ghist; // [2][RADIX] radix histograms (64-bit counts)
    svgd_amd::DevBuf<double> dbg_keys;          // svgd_debug_pair_keys: every pair's key
    int64_t own_tiles = 0, tile0 = 0; // this rank's range of the median tile plan
    int pblock = 64;                  // median tile block (SVGD_PAIR_BLOCK)
    int64_t pnb = 0;                  // median row blocks

    // per-step median plan (set in begin, consumed in finish)
    int med_path = SVGD_MEDIAN_DIRECT;
    int64_t reg_cap = 0;
    svgd_amd::RankPlan sel; // the ranks to select and the statistics averaged (plan_ranks)
    bool median_pending = false;

    // pinned host
    svgd_amd::HostBuf<double> h_x, h_g;
    // The centring fold (row path, d <= 16): X version xver (+1 per update,
    // -1 for a redo's restore, +1 and the history cleared by
    // svgd_set_particles) is centred on the mean of version xver - 1 when its
    // column partials are at hand -- the ones that version's centring left in
    // cpart[(xver - 1) & 1] -- so the centring is one launch at any P (else
    // k_mean_partial's exact mean first).  Every rank centres the same
    // all-gathered X the same way; a repeated centring of one version (a phi
    // or scale call, a redo) finds the same partials, so it forms the same
    // centre.  nmax (max |xc|^2) has a slot per version parity: a centring
    // fills its own and zeroes the other for the next.
    int64_t xver = 0;
    svgd_amd::DevBuf<double> cpart; // 2 x cpart_stride
    int64_t cpart_stride = 0;
    int cpart_n[2] = {0, 0};
    int64_t cpart_ver[2] = {-1, -1};
    svgd_amd::HostBuf<unsigned long long> h_cnt;
    svgd_amd::HostBuf<double> h_scal;
    svgd_amd::Event ev_x, ev_cnt, ev_scal, ev_fin;
    // host<->device copies of the X / G shards run on their own stream so
    // they overlap the median kernels; RCCL calls stay on `stream` (one
    // communicator, one issue order on every rank)
    svgd_amd::Stream cstream;
    svgd_amd::Event ev_xready, ev_g;

    // svgd_step_host_model's state (ctx_host_step.cpp) and what the update
    // does for it: phi in two row parts, X_{t+1} mirrored to the host
    struct HostStep {
        HostStep();
        ~HostStep();
        void join(); // idle between steps: joins the gradient thread
        // OpenMP threads of the host gradient inside svgd_step_host_model: half the
        // host's CPUs, leaving room for this thread and the HIP runtime's -- on a
        // box whose CPU quota equals OMP_NUM_THREADS, all of them tripped the
        // cgroup throttle in ~1 of 3 runs (+0.45 ms/step at cfg3)
        int host_threads = 0;
        std::unique_ptr<svgd_amd::HostWorker> worker; // svgd_step_host_model's gradient thread
        svgd_amd::Event ev_xch[svgd_amd::XCH]; // X_t row chunks on the host (svgd_step_host_model)
        // svgd_step_host_model on a small shard (<= XMIRROR_MAX bytes): the update
        // epilogue also stores X_{t+1} into h_xm (xmirror; xh_valid while X has not
        // changed otherwise since; a buffer of its own: h_x, the caller's, is
        // never written by the device behind its back) -- no D2H copy-engine round
        // trip and cross-queue wait on the host gradient's path
        bool xmirror = false, xh_valid = false;
        svgd_amd::HostBuf<double> h_xm;
        double *h_xm_dev = nullptr; // (h_xm as seen by kernels)
        // phi in two row parts (svgd_step_host_model when split_rows): rows
        // [0, split_h) with S2 column splits, then [split_h, nrows) with S2b
        bool split_rows = false;      // policy (init_ctx)
        bool in_host_step = false;    // run_phi_opt called by svgd_step_host_model
        bool xhalf_ready = false;     // the last step's ev_xhalf marks its first half's X_{t+1}
        int64_t split_h = 0;
        int S2 = 0, S2b = 0;
        svgd_amd::Event ev_xhalf;
        // host-side wall clocks of svgd_step_host_model (always on: steady_clock)
        double h_grad_ms = 0, h_xwait_ms = 0, h_job_ms = 0, h_wait_ms = 0;
        int64_t h_steps = 0;
    } hs;

    // optimizer
    int opt_kind = -1;
    double lr = 0, b1 = 0, b2 = 0, eps = 1e-8;
    int64_t t = 0;
    bool bounded = false;
    int scale_method = SVGD_SCALE_MEDIAN;
    double fixed_a = 1.0;
    // full-matrix scale (SVGD_SCALE_MATRIX / SVGD_SCALE_HESSIAN): device M, its
    // Cholesky factor L, the (rank-summed) Hessian sum, wv = 2 M xc, zc = L^T xc
    struct MatrixScale {
        svgd_amd::DevBuf<double> src, M, L, wv, zc;
        svgd_amd::DevBuf<float> zcf; // SVGD_F32: zc's fp32 copy
        svgd_amd::DevBuf<double> sgn, work; // M = L diag(sgn) L^T; Jacobi scratch
        svgd_amd::DevBuf<int> err;
        svgd_amd::HostBuf<int> h_err;
        bool hess_ready = false; // Hessian sum supplied for the current step
        std::vector<double> h_mat;
    } ms;
    bool have_particles = false;
    // the kernel of phi (svgd_set_kernel) and the inverse multiquadric pass's
    // work arrays (svgd_imq.h), allocated by the first svgd_set_kernel(IMQ): a
    // context that never asks for it allocates and launches nothing of this
    struct Imq {
        int kind = SVGD_KERNEL_RBF;
        bool ready = false;
        int S = 1;                      // column-tile ranges of the pass
        int64_t ldp = 0;
        svgd_amd::DevBuf<double> rec;   // imq_padded(n) records of imq_rec_stride(d) doubles
        svgd_amd::DevBuf<double> part;  // S x ldp x (2d+1) partial sums
    } imq;

    // timing (svgd_set_timing): level 1 = phase events at the phase
    // boundaries only; level 2 adds the diagnostic events (phi kernel alone,
    // the wait for G before the phi chain, every collective) -- each one a
    // dispatch gap, so a diagnostic pass, never the timed one
    struct Timing {
        bool timing = false;
        int tlevel = 0;
        svgd_amd::EventPool pool; // every event below is the pool's; these hold handles
        std::vector<svgd_amd::EvPair> ev_phi, ev_med;
        double phi_ms = 0, med_ms = 0;
        int64_t tcount = 0;
        struct DiagEv {
            hipEvent_t a, b;
            int kind;    // DG_* (ctx.h)
            bool own_a;  // a came from the pool (else it is a phase event)
        };
        std::vector<DiagEv> ev_diag;
        hipEvent_t med_end_ev = nullptr;    // this step's median-end phase event
        double dg_ms[4] = {0, 0, 0, 0};
        int64_t dg_cnt[4] = {0, 0, 0, 0};
    } tm;

    int last_path = SVGD_MEDIAN_DIRECT;
    std::string err;

    // Speculative step (device-side bucket plan, no mid-step host round trip):
    // taken when the last synchronous median found the bucket path with the
    // selected buckets under CAPR.  The plan's status is copied back and
    // checked before the next call that depends on the step; a failed plan
    // (bracket miss, overflow, big buckets) restores X, m, v, t from the
    // backups and redoes the step on the synchronous path.
    bool spec_step = false;    // this step's median is speculative
    bool med_ev_done = false;  // this step's median end event is recorded
    bool last_fast = false;    // the last resolved median could have been speculative
    bool pending = false;      // a speculative step awaits its status
    bool scal_fresh = true;    // h_scal holds the last scale (fetch_scale)
    svgd_amd::DevBuf<int> d_status;
    svgd_amd::HostBuf<int> h_status;
    int *h_status_dev = nullptr; // (h_status as seen by kernels)
    svgd_amd::Event ev_status;
    // Every event record between two kernels costs a ~5 us dispatch gap, so
    // the end of the median records ONE event that serves as the plan status
    // (ev_status_use), the scale-final mark (ev_fin_use), the median phase's
    // end and -- while no work was queued after it (mark) -- the phi phase's
    // start.
    hipEvent_t ev_status_use = nullptr, ev_fin_use = nullptr, mark = nullptr;
    // timing off: the speculative step's status is known from this sequence
    // number, stored by the selection into h_trk[TRK_SEQ] (no event); 0: by event
    uint64_t status_seq = 0, seq_ctr = 0;
    // likewise at the step's end: the phi phase's end event (timing) doubles
    // as X_t-final for the copy stream (ev_xready_use) when nothing follows it
    hipEvent_t phi_end = nullptr, ev_xready_use = nullptr;
    hipEvent_t last_phi_end = nullptr; // the last phi phase's end (timing): the next median's start
    svgd_amd::DevBuf<double> bak; // [X_t | m_t | v_t] of this rank's rows for the pending step

    // Bracket tracking (median_plan.h): the history, this step's prediction
    // and the counters; what follows is the step's bookkeeping around it
    svgd_amd::BracketTracker trk;
    svgd_amd::HostBuf<uint64_t> h_trk; // pinned, TRK_LEN slots (select_state.h TrkSlot)
    uint64_t *h_trk_dev = nullptr;     // (h_trk as seen by kernels)
    bool trk_go = false;        // this step's bracket is the predicted one (trk_plan)
    uint64_t trk_lo = 0, trk_hi = 0;
    double trk_band = 0;        // its expected share of the pairs
    bool trk_keys = false;      // this step's k_select_small writes h_trk
    // a synchronous step's selection to add to the history (resolve_pending):
    // 1 its keys are in h_trk / h_cnt, 2 it took another path (history restarts)
    int trk_sync = 0;
    // path counters (svgd_get_diagnostics): steps whose phi ran in two row
    // parts, host-model steps whose gradient read the update's pinned mirror,
    // speculative steps
    int64_t n_split = 0, n_mirror = 0, n_spec = 0;

    // svgd_ksd's own work arrays (allocated by its first call): it reads X
    // and nothing else of the step's state
    struct Ksd {
        bool ready = false;
        int64_t np = 0, ldp = 0;
        int S = 1;
        svgd_amd::DevBuf<double> G;                  // world*chunk x d (all-gathered scores)
        svgd_amd::DevBuf<double> mu, mpart;          // centre, its column-sum partials
        svgd_amd::DevBuf<double> rec, xt, vt;        // d <= 16 records / d > 16 k-major copies
        svgd_amd::DevBuf<double> nrm, cvec, diag;
        svgd_amd::DevBuf<double> part, rows, bpart, out;
    } ksd;

    // svgd_ksd_kernel(SVGD_KERNEL_IMQ)'s own work arrays (allocated by its
    // first call): the same observer under the inverse multiquadric kernel;
    // nothing of the imq group (the phi records) is read or written
    struct KsdImq {
        bool ready = false;
        int64_t ldp = 0;
        int S = 1;                                   // column-tile ranges of the pass
        svgd_amd::DevBuf<double> G;                  // world*chunk x d (all-gathered scores)
        svgd_amd::DevBuf<double> mu, mpart;          // centre, its column-sum partials
        svgd_amd::DevBuf<double> rec, diag;          // ksd_imq_padded(n) records, |s|^2 + ad
        svgd_amd::DevBuf<double> part, rows, bpart, out;
    } ksdq;

    // svgd_mmd's own work arrays (allocated by its first call, the sample's
    // side grown when a later call brings more points): it reads X and
    // nothing else of the step's state
    struct Mmd {
        bool ready = false;
        int cus = 0;                        // the device's CUs
        int bpc[2] = {1, 1};                // work-groups of the pass one CU holds, per kernel (mmd_blocks_per_cu)
        int64_t m_cap = 0;                  // sample points the Y side holds
        int64_t ldp = 0;                    // partial stride: rows of X's shard or of Y's, whichever is more
        int64_t part_cap = 0;               // doubles of part
        svgd_amd::DevBuf<double> mu, mpart; // the particles' mean, its column-sum partials
        svgd_amd::DevBuf<double> xrec;      // mmd_padded(n) records of mmd_rec_stride(d) doubles
        svgd_amd::DevBuf<double> Y, yrec;   // the sample (m_cap x d) and its mmd_padded(m_cap) records
        svgd_amd::DevBuf<double> part;      // S x ldp partial row sums (one pass at a time)
        svgd_amd::DevBuf<double> rxx, rxy, ryy; // ldp row sums of each pass
        svgd_amd::DevBuf<double> bpart, out;    // the finish's block partials; [Sxx, Sxy, Syy, -]
    } mmd;

    // svgd_stein_thin's own work arrays (allocated by its first call, idx and S
    // grown when a call asks for more picks): the selection reads X and
    // nothing else of the step's state
    struct Thin {
        bool ready = false;
        int64_t m_cap = 0;
        svgd_amd::DevBuf<double> G;          // world*chunk x d (all-gathered scores)
        svgd_amd::DevBuf<double> xs;         // 2d x thin_padded(n): x and s, coordinate-major
        svgd_amd::DevBuf<double> diag, acc;  // thin_padded(n)
        svgd_amd::DevBuf<double> pval;       // thin_part_slots(n) work-group minima ...
        svgd_amd::DevBuf<int> pidx;          // ... and their indices
        svgd_amd::DevBuf<int64_t> idx;       // m_cap picks
        svgd_amd::DevBuf<double> S;          // m_cap running sums
    } thin;

    // svgd_glm_predict's own work arrays (allocated by its first call, grown
    // when a call brings more records): it reads X and nothing else of the
    // step's state
    struct Predict {
        int cus = 0;                      // the device's CUs (0: not asked yet)
        int64_t rec_cap = 0, m_cap = 0, part_cap = 0;
        svgd_amd::DevBuf<double> mu, mpart; // the particles' mean, its column-sum partials
        svgd_amd::DevBuf<double> rec;       // glm_padded(m) test records of glm_rec_stride(d) doubles
        svgd_amd::DevBuf<double> cvec;      // m centres
        svgd_amd::DevBuf<double> sums;      // 3 x m: A, B, L (all-reduced)
        svgd_amd::DevBuf<double> part;      // S x 3 x ldw per-split sums
    } pred;
};

namespace svgd_amd {

inline int fail(svgd_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = "SVGDCpp: " + msg;
    return code;
}

#define HIPCHK(c, expr)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail((c), SVGD_ERR_HIP,                                                      \
                        std::string("[HIP Error] ") + #expr + ": " + hipGetErrorString(e_));    \
    } while (0)

#define NCCLCHK(c, expr)                                                                        \
    do {                                                                                        \
        ncclResult_t r_ = (expr);                                                               \
        if (r_ != ncclSuccess)                                                                  \
            return fail((c), SVGD_ERR_RCCL,                                                     \
                        std::string("[RCCL Error] ") + #expr + ": " + ncclGetErrorString(r_));  \
    } while (0)

#define CHK(expr)                                                                               \
    do {                                                                                        \
        int rc_ = (expr);                                                                       \
        if (rc_ != SVGD_OK) return rc_;                                                         \
    } while (0)

// (Re)allocate an owning member: the old allocation freed, at least one
// element, zeroed on c->stream.
template <class T> int dalloc(svgd_ctx *c, DevBuf<T> *p, int64_t count)
{
    if (count <= 0) count = 1;
    HIPCHK(c, p->alloc((size_t)count));
    HIPCHK(c, hipMemsetAsync(*p, 0, sizeof(T) * (size_t)count, c->stream));
    return SVGD_OK;
}

// work was queued after the median's / phi's end event: those marks no
// longer end the stream
inline void clear_marks(svgd_ctx *c) { c->mark = c->phi_end = nullptr; }

// max |xc|^2 of the current X version (its parity slot)
inline unsigned long long *nmax_cur(const svgd_ctx *c) { return c->nmax ? c->nmax + (c->xver & 1) : nullptr; }

inline bool matrix_scale(const svgd_ctx *c)
{
    return c->scale_method == SVGD_SCALE_MATRIX || c->scale_method == SVGD_SCALE_HESSIAN;
}

inline bool imq_kernel(const svgd_ctx *c) { return c->imq.kind == SVGD_KERNEL_IMQ; }

inline bool has_device_model(const svgd_ctx *c) { return c->dm.k > 0 || c->dm.glm.m > 0; }

// ---- svgd_capi.cpp: the checks every entry point starts with
int check_ready(svgd_ctx *c);
int check_results(svgd_ctx *c);

// ---- ctx_comm.cpp: collectives over comm / gcomm / the host communicator
int comm_create(svgd_ctx *c, const void *unique_id128);
void comm_destroy(svgd_ctx *c);
int allgather_rows_on(svgd_ctx *c, double *buf, ncclComm_t comm, hipStream_t s, int kind);
int allgather_rows(svgd_ctx *c, double *buf);
int allreduce_u64(svgd_ctx *c, unsigned long long *buf, size_t cnt);
int allgather_u64(svgd_ctx *c, uint64_t *buf, size_t cnt);
int allreduce_f64(svgd_ctx *c, double *buf, size_t cnt);
int sym_exchange(svgd_ctx *c);
int coll_check_step(svgd_ctx *c);

// ---- ctx_timing.cpp: pooled events, level-2 diagnostic spans
EvPair take_pair(svgd_ctx *c);
hipEvent_t take_ev(svgd_ctx *c);
hipEvent_t diag_begin(svgd_ctx *c, hipStream_t s);
void diag_end(svgd_ctx *c, hipStream_t s, hipEvent_t a, int kind, bool own_a = true);
int mark_median_end(svgd_ctx *c);

// ---- ctx_median.cpp: the centring and the median scale of a step
int center(svgd_ctx *c, const SelState *st_init = nullptr);
int scale_begin(svgd_ctx *c);
int scale_finish(svgd_ctx *c);
int fetch_scale(svgd_ctx *c);
int resolve_pending(svgd_ctx *c);
int plan_step(svgd_ctx *c);

// ---- ctx_phi.cpp: G's upload, phi and the update
int upload_g_begin(svgd_ctx *c, const double *G_shard);
int upload_g_finish(svgd_ctx *c);
int upload_g(svgd_ctx *c, const double *G_shard);
int run_phi(svgd_ctx *c, const OptArgs *opt);
int run_phi_opt(svgd_ctx *c);

// ---- ctx_create.cpp: what a context is created from
Knobs read_knobs();
PhiCaps built_caps(int dim, int dtype);

// ---- ctx_models.cpp: the device model's gradient and Hessian sum
int launch_device_model_grad(svgd_ctx *c, const double *X, int64_t rows, double *G);
int launch_device_model_hess(svgd_ctx *c, const double *X, int64_t rows, double *H);

} // namespace svgd_amd
