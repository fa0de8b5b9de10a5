"""Rank body of tests/test_multirank_cpu.py (gloo, one process per rank).

Re-enacts, step after step, the sharded step protocol the library runs over
RCCL (svgd_capi.cpp scale_begin / median_begin / collect_counts /
median_finish(_spec) / upload_g_finish / run_phi_opt), with the
library's own host planners (libsvgdcpp_amd.so: the row and tile plans of
plan.cpp and the median policy of median_plan.cpp -- the bracket tracker
through its handle, the sample plan, the sample ranks, the speculative
capacity -- so nothing of the policy is restated here) and numpy + the
oracle as the arithmetic.  Per step:

  1. rows [row0, row1) = svgd_plan_rows; G for own rows;
  2. median (GaussianRBFKernel.hpp:164-188, 222-254), exact:
     a. bracket, decided before the collect (trk_plan):
        - tracked (the shipped default on speculative steps): the last
          selected medians extrapolated, half-width a multiple of the largest
          recent prediction error (svgd_plan_tracker_predict / _record); no
          sample, no collective;
        - else sampled: protocol "shipped" -- EVERY rank draws the whole
          sample (<= 2^20 pairs of one counter-based sequence) and runs the
          two 11-bit radix passes locally: the same bracket everywhere with
          no collective; protocol "shard" (SVGD_SAMPLE_SHARD=1, round 2's) --
          rank r draws pairs [S r/P, S (r+1)/P) and each radix pass
          all-reduces its histograms;
     b. collect over this rank's svgd_plan_pair_tiles tiles: keys below lo
        counted, keys in [lo, hi) kept and histogrammed in NBK buckets; ONE
        all-reduce of [below, candidates, NBK bucket counts] (comm);
     c. bracket hit: svgd_plan_bucket_select names the bucket(s), ONE
        all-gather of the compacted keys (comm), every rank selects the same
        keys; a tracked bracket that misses = a failed device plan: the step
        is redone with a sampled bracket; a sampled one that misses -> the
        streamed radix select over every key (one all-reduce per digit);
  3. the G all-gather on the G communicator (a second gloo group standing
     for the ncclCommSplit one, or the main group when gcomm is off), issued
     where upload_g_finish issues it: after every comm call of the median's
     first phase -- so on speculative steps after the keys all-gather, on
     synchronous ones before it (the cross-communicator issue order of
     svgd_ctx);
  4. phi_hat, Adam and clamp for own rows; the X all-gather (comm).

Every collective is logged as (group, op); the test checks the sequence.
"""
import ctypes
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

RADIX = 11
NBK = 2048  # select_state.h
CAPG = 262144  # select_state.h: the selected buckets' key cap of the bucket path
M64 = (1 << 64) - 1


def _sqdist_keys(X, I, J, block):
    """u64 keys (bit patterns of D^2) of the unordered pairs of tile (I, J)."""
    n = X.shape[0]
    r0, r1 = I * block, min(n, (I + 1) * block)
    c0, c1 = J * block, min(n, (J + 1) * block)
    diff = X[r0:r1, None, :] - X[None, c0:c1, :]
    D2 = np.einsum("ijk,ijk->ij", diff, diff)
    if I == J:
        D2 = D2[np.triu_indices(r1 - r0, k=1)]
    return D2.ravel().astype(np.float64).view(np.uint64)


def _mix64(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _sample_keys(X, g0, g1):
    """Keys of sample slots [g0, g1) of the counter-based pair sequence
    (k_sample_keys_f32: pair (i, j != i) from mix64(2 g + 1))."""
    n = X.shape[0]
    g = np.arange(g0, g1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = _mix64(g * np.uint64(2) + np.uint64(1))
    i = ((h >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)
    j = i + np.uint64(1) + (((h & np.uint64(0xFFFFFFFF)) * np.uint64(n - 1)) >> np.uint64(32))
    j = np.where(j >= n, j - np.uint64(n), j)
    diff = X[i.astype(np.int64)] - X[j.astype(np.int64)]
    return np.einsum("ij,ij->i", diff, diff).view(np.uint64)


class Comms:
    """The main communicator and the G one; every call logged as (group, op)."""

    def __init__(self, dist, torch, gcomm):
        self.dist, self.torch = dist, torch
        self.g = dist.new_group() if gcomm else None
        self.log = []

    def allreduce(self, arr):
        t = self.torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64))
        self.dist.all_reduce(t)
        self.log.append(("comm", "allreduce"))
        return t.numpy()

    def allgather(self, arr, group="comm", what="allgather"):
        t = self.torch.from_numpy(np.ascontiguousarray(arr))
        parts = [self.torch.zeros_like(t) for _ in range(self.dist.get_world_size())]
        self.dist.all_gather(parts, t, group=self.g if group == "gcomm" and self.g is not None else None)
        self.log.append(("gcomm" if group == "gcomm" and self.g is not None else "comm", what))
        return [p.numpy() for p in parts]


def _radix_select(reduce, keys, ranks, passes):
    """Dual radix select from bit 63 down, `passes` digits of RADIX bits;
    `reduce` combines the histograms (an all-reduce, or the identity when
    every rank holds the whole key set).  Returns the resolved prefixes and
    the bit below them."""
    prefix = [0, 0]
    rank = list(ranks)
    hi_bit = 63
    for _ in range(passes):
        lo_bit = max(0, hi_bit - RADIX)
        width = hi_bit - lo_bit
        hists = []
        for s in range(2):
            sel = keys[(keys >> np.uint64(hi_bit)) == np.uint64(prefix[s] >> hi_bit)]
            digit = ((sel >> np.uint64(lo_bit)) & np.uint64((1 << width) - 1)).astype(np.int64)
            hists.append(np.bincount(digit, minlength=1 << RADIX))
        h = reduce(np.concatenate(hists))
        for s in range(2):
            cum = np.cumsum(h[s * (1 << RADIX):(s + 1) * (1 << RADIX)])
            b = int(np.searchsorted(cum, rank[s], side="right"))
            rank[s] -= int(cum[b - 1]) if b > 0 else 0
            prefix[s] |= b << lo_bit
        hi_bit = lo_bit
        if hi_bit == 0:
            break
    return prefix, hi_bit


class Tracker:
    """The library's bracket tracker (median_plan.cpp BracketTracker) through
    its handle, with the creation defaults below N = 32768."""

    def __init__(self, lib):
        self.lib = lib
        self.h = lib.svgd_plan_tracker_new(4.0, 2e-5)
        assert self.h

    def close(self):
        self.lib.svgd_plan_tracker_free(self.h)

    def begin_step(self):
        self.lib.svgd_plan_tracker_begin_step(self.h)

    def predict(self, Mq, band_samp):
        lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
        band, pred, w = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        if not self.lib.svgd_plan_tracker_predict(self.h, Mq, band_samp, ctypes.byref(lo), ctypes.byref(hi),
                                                  ctypes.byref(band), ctypes.byref(pred), ctypes.byref(w)):
            return None
        return lo.value, hi.value

    def record(self, k_lo, k_hi, lo_key, hi_key, cand):
        self.lib.svgd_plan_tracker_record(self.h, int(k_lo), int(k_hi), 0, int(lo_key), int(hi_key), int(cand))

    def lost(self):
        """A selection by another path left no keys: the history restarts
        (trk_resolve_sync), as after a flagged record."""
        self.lib.svgd_plan_tracker_record(self.h, 0, 0, 1, 0, 0, 0)


def _bucket_of(keys, lo, binv):
    t = (keys - np.uint64(lo)).astype(np.float64) * binv
    return np.where(t < NBK - 1, np.where(t > 0, t, 0).astype(np.int64), NBK - 1)


def _median(cm, lib, X, keys, protocol, sigma, shift, trk, spec, on_g, cap=CAPG):
    """One step's exact median; on_g() issues the G all-gather where
    upload_g_finish would.  Returns (med, path, bracket kind, selected D^2
    keys, fast, bracket record for the tracker)."""
    n = X.shape[0]
    world, rank = cm.dist.get_world_size(), cm.dist.get_rank()
    M = n * (n - 1) // 2
    lo_r, hi_r = ctypes.c_int64(), ctypes.c_int64()
    navg = lib.svgd_plan_median_ranks(n, ctypes.byref(lo_r), ctypes.byref(hi_r))
    sel = sorted({r for r in (lo_r.value, hi_r.value) if r >= 0})
    r0, r1 = sel[0], sel[-1]
    # the sample every rank would draw (scattered pairs) and its bracket's share
    band_samp = ctypes.c_double()
    S = lib.svgd_plan_median_sample(n, 0, 0, int(world > 1), int(protocol == "shard"), 1, sigma,
                                    ctypes.byref(band_samp))
    band_samp = band_samp.value
    # a. bracket: tracked (speculative steps only), else sampled
    br = trk.predict(float(M), band_samp) if (spec and protocol == "shipped" and not shift) else None
    kind = "tracked" if br is not None else "sampled"
    if br is not None:
        lo, hi = br
    else:
        if protocol == "shipped":  # every rank draws the whole sample: no collective
            g0, g1 = 0, S
            reduce = lambda h: h  # noqa: E731
        else:  # round 2's sharded sample: histograms all-reduced per pass
            g0, g1 = S * rank // world, S * (rank + 1) // world
            reduce = cm.allreduce
        skeys = _sample_keys(X, g0, g1)
        slo, shi = ctypes.c_int64(), ctypes.c_int64()
        lib.svgd_plan_sample_ranks(S, r0 / M, r1 / M, sigma, ctypes.byref(slo), ctypes.byref(shi), None)
        slo, shi = float(slo.value), float(shi.value)
        if shift:  # tests: a bracket displaced off the median forces the fallback
            sh = shift * (np.sqrt(S * 0.25) + 1)
            slo, shi = min(S - 1.0, slo + sh), min(S - 1.0, shi + sh)
        (p_lo, p_hi), below_bit = _radix_select(reduce, skeys, (int(slo), int(shi)), 2)
        lo = p_lo
        hi = min(M64, p_hi + (1 << below_bit))
    # b. collect: counts + key-range buckets, ONE all-reduce
    below = int(np.count_nonzero(keys < np.uint64(lo)))
    cand = keys[(keys >= np.uint64(lo)) & (keys < np.uint64(hi))] if hi < M64 else keys[keys >= np.uint64(lo)]
    binv = NBK / float(hi - lo)
    bk = _bucket_of(cand, lo, binv)
    cnt = cm.allreduce(np.concatenate([[below, cand.size], np.bincount(bk, minlength=NBK)]))
    below_all, cand_all, buckets = int(cnt[0]), int(cnt[1]), cnt[2:]
    hit = r0 >= below_all and r1 < below_all + cand_all
    if not spec:
        on_g()  # synchronous step: the G all-gather precedes the keys all-gather
    if hit:
        ranks = (ctypes.c_int64 * 2)(r0 - below_all, r1 - below_all)
        bsel, rin, tot = (ctypes.c_int * 2)(), (ctypes.c_int64 * 2)(), ctypes.c_int64()
        bc = (ctypes.c_ulonglong * NBK)(*[int(x) for x in buckets])
        ns = 2 if r1 != r0 else 1
        assert lib.svgd_plan_bucket_select(bc, NBK, ns, ranks, bsel, rin, ctypes.byref(tot)) == 0
        if spec and tot.value > cap:
            hit = False  # the device plan fails on oversized buckets (redo)
    if spec and not hit:
        # failed device plan: the speculative chain still ran (its keys
        # all-gather, the G all-gather); the caller redoes the step
        cm.allgather(np.zeros(cap + 1, dtype=np.int64), what="keys")
        on_g()
        return None
    if hit:
        # c. bucket select: ONE all-gather of the compacted keys
        mine = cand[np.isin(bk, [bsel[0], bsel[ns - 1]])]
        seg = np.zeros(tot.value + 1, dtype=np.int64)
        seg[0] = mine.size
        seg[1:1 + mine.size] = mine.view(np.int64)
        parts = cm.allgather(seg, what="keys")
        gathered = np.concatenate([p[1:1 + p[0]] for p in parts]).view(np.uint64)
        gb = _bucket_of(gathered, lo, binv)
        pool = {s: np.sort(gathered[gb == bsel[s]])[rin[s]] for s in range(ns)}
        vals = {r0: pool[0], r1: pool[ns - 1]}
        path = "bracket"
        fast = tot.value <= CAPG
    else:
        # fallback: streamed radix select over every key, all 64 bits
        (k0, k1), _ = _radix_select(cm.allreduce, keys, (r0, r1), 6)
        vals = {r0: np.uint64(k0), r1: np.uint64(k1)}
        path = "fallback"
        fast = False
    if spec:
        on_g()  # speculative step: every comm call of the median first
    out = [0.0 if kr < 0 else float(np.sqrt(np.uint64(vals[kr]).view(np.float64)))
           for kr in [lo_r.value, hi_r.value][:navg]]
    rec = (int(vals[r0]), int(vals[r1]), lo, hi, cand_all) if path == "bracket" else None
    return sum(out) / len(out), path, kind, fast, rec, (tot.value if hit else 0)


def run(rank, world, port, n, d, block, q, sigma=3.0, shift=0.0, steps=1, protocol="shipped",
        gcomm=True, lr=0.1, bound=2.0):
    try:
        import torch
        import torch.distributed as dist

        import oracle as O
        from svgdcpp_amd import _capi as C

        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        cm = Comms(dist, torch, gcomm)
        lib = C.lib()
        X = O.splitmix((n, d), 3.0, 21)
        mus = O.splitmix((3, d), 3.0, 22)
        covs = np.stack([np.eye(d) * (1.0 + 0.25 * c) for c in range(3)])

        r0, r1 = ctypes.c_int64(), ctypes.c_int64()
        lib.svgd_plan_rows(n, world, rank, ctypes.byref(r0), ctypes.byref(r1))
        row0, row1 = r0.value, r1.value
        chunk = -(-n // world)

        def gather_rows(shard, group="comm", what="rows"):
            buf = np.zeros((chunk, d))
            buf[: shard.shape[0]] = shard
            return np.concatenate(cm.allgather(buf, group=group, what=what))[:n]

        T = lib.svgd_plan_pair_tiles(n, block, world, rank)
        I, J = ctypes.c_int64(), ctypes.c_int64()
        tiles = []
        for t in range(T):
            lib.svgd_plan_pair_tile(n, block, world, rank, t, ctypes.byref(I), ctypes.byref(J))
            tiles.append((I.value, J.value))
        opt = O.Adam((row1 - row0, d), lr, 0.9, 0.999)
        lower, upper = -np.full(d, bound), np.full(d, bound)
        trk = Tracker(lib)
        last_fast = False
        last_tot = 0
        hist = []
        for _ in range(steps):
            Xt = X.copy()
            # 1. G for own rows (the host gradient)
            G_own = O.logp_grad_gmm(X[row0:row1], mus, covs)
            keys = np.concatenate([np.zeros(0, dtype=np.uint64)] +
                                  [_sqdist_keys(X, a, b, block) for a, b in tiles])
            total = int(cm.allreduce(np.array([keys.size]))[0])
            cm.log.pop()  # (the pair-count check is the test's, not the protocol's)
            mark = len(cm.log)
            box = {}

            def on_g():  # (a redo reuses the step's G: gathered once)
                if "G" not in box:
                    box["G"] = gather_rows(G_own, group="gcomm", what="G")

            # 2. the median: speculative when the last selection allowed it
            spec = last_fast
            trk.begin_step()
            res = _median(cm, lib, X, keys, protocol, sigma, shift, trk, spec, on_g,
                          lib.svgd_plan_spec_cap(last_tot))
            redo = res is None
            if redo:
                # a failed device plan (resolve_pending): the speculative
                # step's update and X all-gather ran; X_t, m_t, v_t are
                # restored and all-gathered, and the step is redone
                # synchronously with a sampled bracket
                gather_rows(X[row0:row1], what="X")
                gather_rows(X[row0:row1], what="X_restore")
                trk.begin_step()
                res = _median(cm, lib, X, keys, protocol, sigma, shift, trk, False, on_g)
            med, path, kind, fast, rec, last_tot = res
            if rec is not None:
                trk.record(*rec)
            else:
                trk.lost()
            last_fast = fast
            a = np.log(n) / med ** 2
            # 4. phi_hat + Adam + clamp for own rows, X all-gathered
            ph = O.phi(X, box["G"], a, rows=(row0, row1))
            Xs = X[row0:row1].copy()
            O.apply_update(Xs, opt.step(ph), lower, upper)
            X = gather_rows(Xs, what="X")
            hist.append(dict(X=Xt, X_new=X.copy(), G_all=box["G"], a=a, med=med, path=path,
                             bracket=kind, spec=spec, redo=redo, total=total,
                             colls=list(cm.log[mark:])))
        trk.close()
        if rank == 0:
            q.put(("ok", dict(steps=hist, mus=mus, covs=covs, lr=lr, bound=bound)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put(("err", traceback.format_exc()))
