// ctx_host_step.cpp -- svgd_step_host_model: the host gradient of a built-in model
// on a thread of its own, pipelined in row chunks beside the step's median chain.
#include "ctx.h"
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include "host_models.h"

using namespace svgd_amd;

namespace svgd_amd {

// One persistent host thread per context that runs the host-gradient half of
// svgd_step_host_model (X_t chunks down -> grad log p -> G chunks up) while
// the calling thread enqueues the step's median chain: the ~14 launches
// (~5 us each) no longer sit in front of the gradient on one thread.  The
// worker spins ~1 ms after a job (the next step usually follows within it),
// then sleeps on the condition variable.
class HostWorker {
  public:
    ~HostWorker()
    {
        if (!th_.joinable()) return;
        {
            std::lock_guard<std::mutex> g(mu_);
            quit_ = true;
        }
        cv_.notify_one();
        th_.join();
    }
    void post(std::function<int(std::string &)> job)
    {
        if (!th_.joinable()) th_ = std::thread([this] { loop(); });
        {
            std::lock_guard<std::mutex> g(mu_);
            job_ = std::move(job);
            state_.store(1, std::memory_order_release);
        }
        cv_.notify_one();
    }
    // wait for the posted job; its return code (and message in err on failure)
    int wait(std::string &err)
    {
        for (int spin = 0; state_.load(std::memory_order_acquire) != 2; ++spin)
            if (spin > 64) std::this_thread::yield();
        state_.store(0, std::memory_order_relaxed);
        if (rc_) err = msg_;
        return rc_;
    }

  private:
    void loop()
    {
        for (;;) {
            const auto t0 = std::chrono::steady_clock::now();
            while (state_.load(std::memory_order_acquire) != 1 &&
                   std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(1))
                std::this_thread::yield();
            std::function<int(std::string &)> job;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [this] { return quit_ || state_.load() == 1; });
                if (quit_) return;
                job = std::move(job_);
            }
            msg_.clear();
            rc_ = job(msg_);
            state_.store(2, std::memory_order_release);
        }
    }
    std::thread th_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::function<int(std::string &)> job_;
    std::atomic<int> state_{0}; // 0 idle, 1 posted, 2 done
    int rc_ = 0;
    std::string msg_;
    bool quit_ = false;
};

} // namespace svgd_amd

// (defined where HostWorker is complete)
svgd_ctx::HostStep::HostStep() = default;
svgd_ctx::HostStep::~HostStep() = default;
void svgd_ctx::HostStep::join() { worker.reset(); }

extern "C" {

int svgd_step_host_model(svgd_ctx *c, const void *model)
{
    CHK(check_ready(c));
    const svgd_amd::HostModel *m = static_cast<const svgd_amd::HostModel *>(model);
    if (!m || m->d != c->dim)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Host model missing or of another dimension.");
    if (c->scale_method == SVGD_SCALE_HESSIAN) // (the split calls carry the caller's sum)
        return fail(c, SVGD_ERR_UNSET,
                    "[Unset Error] Hessian scale: svgd_set_step_hessian_sum was not called this step "
                    "(svgd_step_host_model does not supply it; use svgd_begin_step / "
                    "svgd_set_step_hessian_sum / svgd_finish_step).");
    CHK(resolve_pending(c));
    if (c->opt_kind < 0)
        return fail(c, SVGD_ERR_ARG, "[Argument Error] Invalid Optimizer object pointer.");
    const int d = c->dim;
    const int64_t rows = c->nrows;
    // row chunks of >= 1 MiB (a chunk's copy, event and OpenMP region cost
    // ~10 us: smaller chunks lose more than they overlap), at most XCH
    const int64_t min_rows = std::max<int64_t>(1, (int64_t(1) << 20) / (8 * d));
    // the last step ran phi in row halves: the first half's chunks wait for
    // its X_{t+1} only (ev_xhalf), so their gradient starts while the second
    // half's phi still runs; chunks never straddle the halves
    const int64_t hsplit = c->hs.xhalf_ready ? c->hs.split_h : 0;
    const int nh = hsplit > 0 ? (int)std::max<int64_t>(1, std::min<int64_t>(XCH / 2, hsplit / min_rows)) : 0;
    const int nch = hsplit > 0 ? 2 * nh
                               : (int)std::max<int64_t>(1, std::min<int64_t>(XCH, rows / min_rows));
    auto chunk = [hsplit, nh, nch, rows](int q, int64_t *r0, int64_t *r1) {
        if (hsplit > 0) {
            const int64_t b = q < nh ? 0 : hsplit, len = q < nh ? hsplit : rows - hsplit;
            const int qq = q < nh ? q : q - nh;
            *r0 = b + len * qq / nh;
            *r1 = b + len * (qq + 1) / nh;
            return;
        }
        *r0 = rows * q / nch;
        *r1 = rows * (q + 1) / nch;
    };
    HIPCHK(c, hipEventSynchronize(c->ev_g)); // the previous step's upload has left h_g
    // the event chunk q's X_t waits for: its copy's, or -- when the last
    // update stored X_t into h_x (xh_valid) -- that update's own end
    hipEvent_t xwait[XCH];
    if (rows > 0) {
        // X_t is final once the previous step's update (and all-gather) ran
        hipEvent_t xev = c->ev_xready_use ? c->ev_xready_use : c->ev_xready;
        if (c->hs.xh_valid) {
            for (int q = 0; q < nch; ++q) xwait[q] = hsplit > 0 && q < nh ? c->hs.ev_xhalf : xev;
        } else {
            HIPCHK(c, hipStreamWaitEvent(c->cstream, hsplit > 0 ? c->hs.ev_xhalf : xev, 0));
            for (int q = 0; q < nch; ++q) {
                int64_t r0, r1;
                chunk(q, &r0, &r1);
                if (hsplit > 0 && q == nh) HIPCHK(c, hipStreamWaitEvent(c->cstream, xev, 0));
                HIPCHK(c, hipMemcpyAsync(c->h_x + r0 * d, c->X + (size_t)(c->row0 + r0) * d,
                                         sizeof(double) * (size_t)(r1 - r0) * d, hipMemcpyDeviceToHost,
                                         c->cstream));
                HIPCHK(c, hipEventRecord(c->hs.ev_xch[q], c->cstream));
                xwait[q] = c->hs.ev_xch[q];
            }
        }
    }
    // the gradient's input: X_t from the last update's mirror, or its copy
    const double *hx = c->hs.xh_valid ? c->hs.h_xm : c->h_x;
    c->n_mirror += c->hs.xh_valid && rows > 0 ? 1 : 0;
    // the gradient thread: each chunk waits for its X_t copy, evaluates the
    // model and queues its G copy on the copy stream (the calling thread only
    // touches `stream` until it waits for this job)
    if (!c->hs.worker) c->hs.worker.reset(new HostWorker());
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0, clk::time_point t1) {
        return std::chrono::duration<double, std::milli>(t1 - t0).count();
    };
    const clk::time_point t_post = clk::now();
    std::array<hipEvent_t, XCH> xw;
    std::copy(xwait, xwait + (rows > 0 ? nch : 0), xw.begin());
    c->hs.worker->post([c, m, d, rows, nch, chunk, ms_since, t_post, xw, hx](std::string &msg) -> int {
        for (int q = 0; q < nch && rows > 0; ++q) {
            int64_t r0, r1;
            chunk(q, &r0, &r1);
            const clk::time_point tw = clk::now();
            hipError_t e = hipEventSynchronize(xw[q]);
            if (e != hipSuccess) {
                msg = std::string("SVGDCpp: [HIP Error] X_t chunk copy: ") + hipGetErrorString(e);
                return SVGD_ERR_HIP;
            }
            const clk::time_point tg = clk::now();
            if (const int rc = model_logp_grad_threads(m, hx + r0 * d, r1 - r0, c->h_g + r0 * d,
                                                       c->hs.host_threads)) {
                msg = rc == SVGD_ERR_RUNTIME ? "SVGDCpp: [Runtime Error] Host model evaluation: out of memory."
                                             : "SVGDCpp: [Argument Error] Host model evaluation failed.";
                return rc;
            }
            c->hs.h_xwait_ms += ms_since(tw, tg);
            c->hs.h_grad_ms += ms_since(tg, clk::now());
            e = hipMemcpyAsync(c->G + (size_t)(c->row0 + r0) * d, c->h_g + r0 * d,
                               sizeof(double) * (size_t)(r1 - r0) * d, hipMemcpyHostToDevice,
                               c->cstream);
            if (e != hipSuccess) {
                msg = std::string("SVGDCpp: [HIP Error] G chunk copy: ") + hipGetErrorString(e);
                return SVGD_ERR_HIP;
            }
        }
        hipError_t e = hipEventRecord(c->ev_g, c->cstream);
        // the gradient thread waits for its copies to land (the device is
        // still in the median): the compute stream then needs no barrier on
        // the copy stream (upload_g_finish)
        if (e == hipSuccess) e = hipEventSynchronize(c->ev_g);
        if (e != hipSuccess) {
            msg = std::string("SVGDCpp: [HIP Error] G event: ") + hipGetErrorString(e);
            return SVGD_ERR_HIP;
        }
        c->hs.h_job_ms += ms_since(t_post, clk::now());
        return SVGD_OK;
    });
    int rc = plan_step(c);
    if (rc == SVGD_OK) rc = scale_begin(c);
    std::string wmsg;
    const clk::time_point tw0 = clk::now();
    const int wrc = c->hs.worker->wait(wmsg); // always joined before returning
    c->hs.h_wait_ms += ms_since(tw0, clk::now());
    c->hs.h_steps += 1;
    CHK(rc);
    if (wrc != SVGD_OK) {
        c->err = wmsg;
        return wrc;
    }
    CHK(upload_g_finish(c));
    CHK(scale_finish(c));
    c->hs.in_host_step = true;
    rc = run_phi_opt(c);
    c->hs.in_host_step = false;
    return rc;
}

} // extern "C"
