// ctx_comm.cpp -- the communicators: their set-up and teardown, every collective
// of the step (RCCL or the host-shm rehearsal backend) and the issue-order check.
#include "ctx.h"
#include <algorithm>
#include <cstring>
#include <vector>

using namespace svgd_amd;

namespace svgd_amd {
namespace {

// Every collective this rank issues goes into the step's sequence hash (the
// SVGD_DEBUG_COLL cross-rank check of the issue-order invariant, svgd_ctx).
enum { CO_GATHER_ROWS = 1, CO_REDUCE_U64 = 2, CO_GATHER_U64 = 3, CO_REDUCE_F64 = 4, CO_XCHG = 6, CO_GCOMM = 16 };
void coll_note(svgd_ctx *c, int op, size_t cnt)
{
    uint64_t h = c->co.coll_sig ? c->co.coll_sig : 0xcbf29ce484222325ull;
    for (uint64_t v : {(uint64_t)op, (uint64_t)cnt}) {
        h ^= v;
        h *= 0x100000001b3ull;
    }
    c->co.coll_sig = h;
}

} // namespace

int allgather_rows_on(svgd_ctx *c, double *buf, ncclComm_t comm, hipStream_t s, int kind)
{
    if (!c->co.any()) return SVGD_OK; // one rank, no communicator
    clear_marks(c); // work queued after the median's / phi's end event
    const size_t cnt = (size_t)c->chunk * c->dim;
    coll_note(c, CO_GATHER_ROWS | (comm && comm == c->co.gcomm ? CO_GCOMM : 0), cnt);
    hipEvent_t d0 = diag_begin(c, s);
    if (c->co.hcomm) {
        if (hostcomm_allgather(c->co.hcomm, reinterpret_cast<char *>(buf), cnt * sizeof(double), s))
            return fail(c, SVGD_ERR_RCCL, "[RCCL Error] host all-gather failed.");
    } else {
        NCCLCHK(c, ncclAllGather(buf + (size_t)c->rank * cnt, buf, cnt, ncclDouble, comm, s));
    }
    diag_end(c, s, d0, kind);
    return SVGD_OK;
}

int allgather_rows(svgd_ctx *c, double *buf)
{
    return allgather_rows_on(c, buf, c->co.comm, c->stream, DG_COLL);
}

int allreduce_u64(svgd_ctx *c, unsigned long long *buf, size_t cnt)
{
    if (!c->co.any()) return SVGD_OK; // one rank, no communicator
    coll_note(c, CO_REDUCE_U64, cnt);
    hipEvent_t d0 = diag_begin(c, c->stream);
    if (c->co.hcomm) {
        if (hostcomm_allreduce_u64(c->co.hcomm, buf, cnt, c->stream))
            return fail(c, SVGD_ERR_RCCL, "[RCCL Error] host all-reduce failed.");
    } else {
        NCCLCHK(c, ncclAllReduce(buf, buf, cnt, ncclUint64, ncclSum, c->co.comm, c->stream));
    }
    diag_end(c, c->stream, d0, DG_COLL);
    return SVGD_OK;
}

// In-place all-gather of `cnt` u64 per rank (rank r's part at buf + r * cnt).
int allgather_u64(svgd_ctx *c, uint64_t *buf, size_t cnt)
{
    if (!c->co.any()) return SVGD_OK; // one rank, no communicator
    coll_note(c, CO_GATHER_U64, cnt);
    hipEvent_t d0 = diag_begin(c, c->stream);
    if (c->co.hcomm) {
        if (hostcomm_allgather(c->co.hcomm, reinterpret_cast<char *>(buf), cnt * sizeof(uint64_t),
                               c->stream))
            return fail(c, SVGD_ERR_RCCL, "[RCCL Error] host all-gather failed.");
    } else {
        NCCLCHK(c, ncclAllGather(buf + (size_t)c->rank * cnt, buf, cnt, ncclUint64, c->co.comm,
                                 c->stream));
    }
    diag_end(c, c->stream, d0, DG_COLL);
    return SVGD_OK;
}

// The sharded symmetric pass's exchange (the parallel branch of
// SVGD.hpp:410-432): one group of point-to-point sends and receives -- to
// each rank the range of its rows this rank's units touched, from each rank
// the range of this rank's rows its units touched (svgd_plan_sym_exchange;
// at P = 8, cfg3: ~2.5 MB per rank to ~5 peers over their direct links,
// against 4.1 MB per GPU in 7 ring steps for a reduce-scatter of all N
// sums).  k_sym_apply adds the pieces in rank order.  The host-shm
// rehearsal backend runs the same plan, and a receiver sees only what its
// senders sent (NaN elsewhere).
int sym_exchange(svgd_ctx *c)
{
    if (!c->co.any()) return SVGD_OK; // one rank / simulated world: no exchange
    clear_marks(c);
    const size_t w = (size_t)c->dim + 1;
    coll_note(c, CO_XCHG, (size_t)c->n * w); // (the pieces differ by rank; the call is the same)
    hipEvent_t d0 = diag_begin(c, c->stream);
    if (c->co.hcomm) {
        if (hostcomm_exchange_f64(c->co.hcomm, c->sym.contrib, (size_t)c->n, w, c->sym.xsend.data(), c->sym.xrecv_buf,
                                  (size_t)c->sym.xrecv_rows, c->sym.xrecv.data(), c->row0, c->row0 + c->nrows,
                                  c->stream))
            return fail(c, SVGD_ERR_RCCL, "[RCCL Error] host point-to-point exchange failed.");
    } else {
        NCCLCHK(c, ncclGroupStart());
        for (int q = 0; q < c->world; ++q) {
            if (q == c->rank) continue;
            const int64_t a = c->sym.xsend[2 * q], b = c->sym.xsend[2 * q + 1];
            if (b > a) NCCLCHK(c, ncclSend(c->sym.contrib + a * w, (size_t)(b - a) * w, ncclDouble, q, c->co.comm, c->stream));
            const int64_t ra = c->sym.xrecv[3 * q], rb = c->sym.xrecv[3 * q + 1], off = c->sym.xrecv[3 * q + 2];
            if (rb > ra)
                NCCLCHK(c, ncclRecv(c->sym.xrecv_buf + off * w, (size_t)(rb - ra) * w, ncclDouble, q, c->co.comm,
                                    c->stream));
        }
        NCCLCHK(c, ncclGroupEnd());
    }
    diag_end(c, c->stream, d0, DG_COLL);
    return SVGD_OK;
}

int allreduce_f64(svgd_ctx *c, double *buf, size_t cnt)
{
    if (!c->co.any()) return SVGD_OK; // one rank, no communicator
    coll_note(c, CO_REDUCE_F64, cnt);
    if (c->co.hcomm) {
        if (hostcomm_allreduce_f64(c->co.hcomm, buf, cnt, c->stream))
            return fail(c, SVGD_ERR_RCCL, "[RCCL Error] host all-reduce failed.");
        return SVGD_OK;
    }
    NCCLCHK(c, ncclAllReduce(buf, buf, cnt, ncclDouble, ncclSum, c->co.comm, c->stream));
    return SVGD_OK;
}

// End of a step's collectives: SVGD_DEBUG_COLL=1 all-gathers every rank's
// hash of the step's collective sequence (communicator, op, count, in issue
// order) and fails unless all are equal -- the cross-rank check of the issue
// order both communicators rely on (svgd_ctx).  Off by default (a blocking
// all-gather per step).
int coll_check_step(svgd_ctx *c)
{
    const uint64_t mine = c->co.coll_sig;
    c->co.coll_sig = 0;
    c->co.coll_phase = 0;
    if (!c->knobs.debug_coll.or_(0) || !c->co.any()) return SVGD_OK;
    if (!c->co.sig_buf) HIPCHK(c, c->co.sig_buf.alloc((size_t)c->world));
    HIPCHK(c, hipMemcpyAsync(c->co.sig_buf + c->rank, &mine, sizeof(uint64_t), hipMemcpyHostToDevice,
                             c->stream));
    if (c->co.hcomm) {
        if (hostcomm_allgather(c->co.hcomm, reinterpret_cast<char *>((uint64_t *)c->co.sig_buf), sizeof(uint64_t),
                               c->stream))
            return fail(c, SVGD_ERR_RCCL, "[RCCL Error] host all-gather failed.");
    } else {
        NCCLCHK(c, ncclAllGather(c->co.sig_buf + c->rank, c->co.sig_buf, 1, ncclUint64, c->co.comm, c->stream));
    }
    std::vector<uint64_t> all((size_t)c->world);
    HIPCHK(c, hipMemcpyAsync(all.data(), c->co.sig_buf, sizeof(uint64_t) * all.size(),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    clear_marks(c);
    for (uint64_t s : all)
        if (s != mine)
            return fail(c, SVGD_ERR_RCCL,
                        "[RCCL Error] ranks issued different collective sequences this step.");
    return SVGD_OK;
}

// The communicator of a context created with world and rank set (after its
// buffers: the host backend's slots are sized from them).
int comm_create(svgd_ctx *c, const void *unique_id128)
{
    const Knobs &k = c->knobs;
    const int world = c->world, rank = c->rank;
    if (world > 1 && k.hostcomm.set) {
        // rehearsal backend: ranks sharing one GPU, collectives through host shm
        const size_t slot = std::max<size_t>(
            std::max<size_t>(
                std::max<size_t>((size_t)c->chunk * c->dim, (size_t)c->dim * c->dim) * sizeof(double),
                2 * RADIX * sizeof(unsigned long long)),
            std::max<size_t>((CAPG + 1) * sizeof(uint64_t), (3 + NBK) * sizeof(uint64_t)));
        const size_t slot_rs = c->sym.contrib ? 2 * sizeof(int64_t) * (size_t)world +
                                                    (size_t)c->n * (c->dim + 1) * sizeof(double)
                                              : 0;
        if (hostcomm_create(&c->co.hcomm, k.hostcomm.v.c_str(), world, rank, std::max(slot, slot_rs)))
            return fail(c, SVGD_ERR_RCCL, "[RCCL Error] host communicator setup failed.");
        return SVGD_OK;
    }
    // world == 1 with a unique id: a one-rank RCCL communicator, so every
    // collective of the sharded step runs through RCCL on a single GPU
    if (unique_id128) {
        ncclUniqueId id;
        std::memcpy(&id, unique_id128, sizeof(id));
        NCCLCHK(c, ncclCommInitRank(&c->co.comm, world, id, rank));
        // the G all-gather's own communicator and stream (upload_g_finish):
        // by default at P >= 2, so the all-gather of G runs beside the median
        // (15-30 us off the P = 8 critical path); SVGD_G_COMM=0 /
        // 1 on every rank forces it off / on (the split is collective).
        // Every rank learns whether every split succeeded (a min all-reduce
        // over comm): one rank gathering G on gcomm while another gathers it
        // on comm would hang both, so any failure drops gcomm everywhere and
        // the G all-gather stays on the compute stream.
        if (k.g_comm.or_(world > 1)) {
            int ok = ncclCommSplit(c->co.comm, 0, rank, &c->co.gcomm, nullptr) == ncclSuccess && c->co.gcomm;
            if (ok && c->co.gstream.create() != hipSuccess) ok = 0;
            if (ok && c->co.ev_gg.create(hipEventDisableTiming) != hipSuccess) ok = 0;
            HIPCHK(c, c->co.d_ok.alloc(1));
            HIPCHK(c, hipMemcpy(c->co.d_ok, &ok, sizeof(int), hipMemcpyHostToDevice));
            NCCLCHK(c, ncclAllReduce(c->co.d_ok, c->co.d_ok, 1, ncclInt32, ncclMin, c->co.comm, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipMemcpy(&ok, c->co.d_ok, sizeof(int), hipMemcpyDeviceToHost));
            c->co.d_ok.reset();
            if (!ok) {
                if (c->co.gcomm) (void)ncclCommDestroy(c->co.gcomm);
                c->co.gcomm = nullptr;
            }
        }
    }
    return SVGD_OK;
}

// gcomm, then comm, then the host communicator (their streams are idle)
void comm_destroy(svgd_ctx *c)
{
    if (c->co.gcomm) (void)ncclCommDestroy(c->co.gcomm);
    if (c->co.comm) (void)ncclCommDestroy(c->co.comm);
    if (c->co.hcomm) hostcomm_destroy(c->co.hcomm);
    c->co.gcomm = c->co.comm = nullptr;
    c->co.hcomm = nullptr;
}

} // namespace svgd_amd

extern "C" {

int svgd_get_unique_id(void *unique_id128)
{
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return SVGD_ERR_RCCL;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    std::memcpy(unique_id128, &id, sizeof(id));
    return SVGD_OK;
}

} // extern "C"
