"""The sharded step on the fp64 tile path and on every F32 phi path, at
row0 != 0: the cases of tests/_shard_cases.py, one process per rank on device
0 (tests/_gpu_shard_rank_worker.py; host collectives, SVGD_DEBUG_COLL=1).
GPU only.

run_phi hands row0 / nrows to k_phi<double> (+ k_opt_update), k_phi_f32s,
k_phi_b3 (their fused epilogues update X + row0 d and the rank-local m, v
through (i - row0) d + c and read wv / xc with the global i) and the generic
k_phi<float>, which an F32 rank whose shard starts at no multiple of 16 runs
while rank 0 keeps the streamed kernel -- at d = 32, 48, 64 in its S1V form
(padded columns masked by c_j = -inf), which no one-rank run reaches.

  a. each rank's first phi rows against oracle.phi(X0, G, a)[row0:row1]:
     max-abs 1e-10 (fp64), REL max|ref| (F32, tests/test_gpu_f32.py); an empty
     rank returns (0, d) and the others pass
  b. the update bit for bit: the ranks' phi rows assembled, the oracle's
     optimizer and clamp applied -> every rank's all-gathered X after each of
     three steps, zero differing elements; per-dimension bounds exercised
  c. a fixed SPD matrix scale sharded: phi against oracle.phi_matrix (same
     bars), the same bit-exact update
  d. four median steps of a Gaussian sum, with the direct pass and with the
     bracket passes: med against the oracle from the device's own X_t (rel
     1e-12 fp64, 1e-5 F32), scale and path code identical on all ranks, one X
     on all ranks, the first scale bit-identical to one rank's; fp64: positions
     against the oracle step 1e-9 and against one rank 1e-10 (the bars of
     tests/test_gpu_update_paths.py and tests/test_gpu_multirank.py); F32 on
     aligned shards: against one rank 1e-10 as well.  F32 on unaligned shards
     is not compared with one rank: rank 1 runs another kernel than the
     one-rank run does, whose phi differs at the F32 bar.
  e. sharded equals one rank bit for bit (X and (a, med), every step) with an
     elementwise model, on the fp64 tiles and on the aligned F32 shards: k_phi
     sweeps all column tiles in one order for every row, its S1V shuffles do
     not depend on where the row sits, the update is elementwise, the median
     exact.

Every rank of every run must report the kernel the table names for it.  Each
test prints what it observed ("shard_paths ...": error, bar, and the worst
ratio to the bar of the kernel family so far).
"""
import functools
import multiprocessing as mp
import uuid

import numpy as np
import pytest

import _gpu_shard_rank_worker as W
import _shard_cases as T
import _update_cases as U
from _dispatch import KNOBS
from test_gpu_f32 import REL

pytestmark = pytest.mark.gpu

WORST = {}  # kernel family / group -> worst observed ratio to its bar


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _family(name):
    for f in ("k_phi<double", "k_phi<float", "k_phi_f32s", "k_phi_b3"):
        if name.startswith(f):
            return f + (">" if "<" in f else "")
    return name


def _report(group, what, err, bar):
    WORST[group] = max(WORST.get(group, 0.0), err / bar)
    print("shard_paths %s %s: err %.3g bar %.3g (worst ratio of %s so far %.3g)"
          % (group, what, err, bar, group, WORST[group]))


def _ranks(world, cfg):
    assert world <= 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "svgd_" + uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=W.run, args=(r, world, name, cfg, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in range(world):
            status, rank, res = q.get(timeout=300)
            assert status == "ok", res
            out[rank] = res
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return out


_RUNS = {}


def _run(case, world, mode, **kw):
    """The ranks' results of one configuration, run once (a failed run fails
    every test that needs it, without running again)."""
    key = (case.id, world, mode, tuple(sorted(kw.items())))
    if key not in _RUNS:
        cfg = dict(n=case.n, d=case.d, dtype=case.dtype, env=case.env, opt=T.opt_of(case), mode=mode, **kw)
        try:
            _RUNS[key] = _ranks(world, cfg)
        except BaseException as e:  # (kept: the next test of this run re-raises it)
            _RUNS[key] = e
    if isinstance(_RUNS[key], BaseException):
        raise _RUNS[key]
    return _RUNS[key]


@functools.lru_cache(maxsize=None)
def _inputs(n, d):
    X, G, a = W.inputs(n, d)
    for arr in (X, G):
        arr.setflags(write=False)
    return X, G, a


@functools.lru_cache(maxsize=None)
def _ref_phi(n, d):
    import oracle
    X, G, a = _inputs(n, d)
    ref = oracle.phi(X, G, a)
    ref.setflags(write=False)
    return ref


def _oracle_opt(oracle, name, shape):
    if name == "adam":
        return oracle.Adam(shape, 0.1, 0.9, 0.999)
    if name == "adagrad":
        return oracle.AdaGrad(shape, 0.1)
    return oracle.RMSProp(shape, 0.1, 0.9)


def _check_names_and_shards(case, run, world=None):
    """Every rank ran the kernel the table names for it, on the planned rows."""
    world = case.world if world is None else world
    shards = [run[r]["shard"] for r in range(world)]
    assert shards[0][0] == 0 and shards[-1][1] == case.n
    assert all(a[1] == b[0] for a, b in zip(shards, shards[1:]))
    for r in range(world):
        prefix = case.names[r] if world == case.world else case.names[0]
        assert all(nm.startswith(prefix) for nm in run[r]["names"]), (case.id, r, run[r]["names"], prefix)
    return shards


def _assemble(run, world, key, t):
    return np.concatenate([run[r][key][t] for r in range(world)])


def _bar(case, ref):
    return 1e-10 if case.dtype == "f64" else REL * float(np.max(np.abs(ref)))


# ------------------------------------------------- a. phi against the oracle ----
@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_phi_rows_match_oracle(oracle, case):
    run = _run(case, case.world, "update")
    shards = _check_names_and_shards(case, run)
    ref = _ref_phi(case.n, case.d)
    bar = _bar(case, ref)
    bad = []
    for r, (r0, r1) in enumerate(shards):
        ph = run[r]["phi"][0]
        assert ph.shape == (r1 - r0, case.d), (r, ph.shape)
        if r1 == r0:
            assert case.shards == "empty" and r == case.world - 1
            print("shard_paths phi %s rank %d: no rows" % (case.id, r))
            continue
        assert np.all(np.isfinite(ph)), r
        err = float(np.max(np.abs(ph - ref[r0:r1])))
        name = run[r]["names"][0]
        _report(_family(name), "phi %s rank %d rows [%d, %d) %s" % (case.id, r, r0, r1, name), err, bar)
        if err > bar:
            bad.append((r, name, err, bar))
    # (an error on rank 1 only is the signature of a wrong row base)
    assert not bad, bad


# ------------------------------------------------ b. the update, bit for bit ----
def _bit_exact(oracle, case, run, phi_check=None):
    """The oracle's optimizer and clamp on the ranks' assembled phi rows give
    every rank's all-gathered X after each step, bit for bit.  phi_check(t,
    X_t, phi_t) runs before the step's update."""
    X0 = _inputs(case.n, case.d)[0]
    lo, up = U.bounds(case.d)
    o_opt = _oracle_opt(oracle, T.opt_of(case), X0.shape)
    Xo = X0.copy()
    for t in range(W.UPDATE_STEPS):
        ph = _assemble(run, case.world, "phi", t)
        assert ph.shape == X0.shape and np.all(np.isfinite(ph))
        if phi_check is not None:
            phi_check(t, Xo, ph)
        delta = o_opt.step(ph)
        Xpre = Xo + delta
        oracle.apply_update(Xo, delta, lo, up)
        for r in range(case.world):
            Xd = run[r]["X"][t]
            bad = np.flatnonzero((Xd != Xo).ravel())
            assert bad.size == 0, ("%s rank %d step %d: %d elements differ, first at %s, max |diff| %.3g"
                                   % (case.id, r, t, bad.size, np.unravel_index(bad[0], Xd.shape),
                                      np.max(np.abs(Xd - Xo))))
    # (two particles cannot sit on a bound of every dimension)
    n_lo, n_up = U.assert_bounds_exercised(Xo, lo, up, Xpre, every_dim=case.n > 2)
    print("shard_paths update %s %s: bit-identical over %d steps on %d ranks; dimensions on a lower / upper "
          "bound %d / %d" % (case.id, T.opt_of(case), W.UPDATE_STEPS, case.world, n_lo, n_up))


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_update_bit_exact(oracle, case):
    run = _run(case, case.world, "update")
    _check_names_and_shards(case, run)
    _bit_exact(oracle, case, run)


# ------------------------------------------- c. the matrix scale, sharded ----
@pytest.mark.parametrize("case_id", T.MATRIX_CASES)
def test_matrix_scale_sharded(oracle, case_id):
    case = T.BY_ID[case_id]
    run = _run(case, case.world, "update", matrix=True)
    shards = _check_names_and_shards(case, run)
    G = _inputs(case.n, case.d)[1]
    M = W.matrix(case.d)
    bad = []

    def phi_check(t, Xt, ph):
        # (the reference follows the oracle's -- bit for bit the device's -- trajectory)
        for r, (r0, r1) in enumerate(shards):
            ref = oracle.phi_matrix(Xt, G, M, rows=(r0, r1))
            bar = _bar(case, ref)
            err = float(np.max(np.abs(ph[r0:r1] - ref)))
            name = run[r]["names"][t]
            _report(_family(name) + " matrix", "%s step %d rank %d %s" % (case.id, t, r, name), err, bar)
            if err > bar:
                bad.append((t, r, name, err, bar))

    _bit_exact(oracle, case, run, phi_check)
    assert not bad, bad


# ---------------------------------------------- d. median steps, sharded ----
@pytest.mark.parametrize("bracket", [False, True], ids=["direct", "bracket"])
@pytest.mark.parametrize("case_id", T.STEP_CASES)
def test_median_steps_sharded(oracle, case_id, bracket):
    case = T.BY_ID[case_id]
    multi = _run(case, case.world, "steps", model="gmm", bracket=bracket)
    one = _run(case, 1, "steps", model="gmm", bracket=bracket)[0]
    _check_names_and_shards(case, multi)
    assert all(nm.startswith(case.names[0]) for nm in one["names"]), one["names"]
    f64 = case.dtype == "f64"
    X0 = _inputs(case.n, case.d)[0]
    mus, covs = W.gmm(case.d)
    lo, up = U.bounds(case.d)
    o_opt = _oracle_opt(oracle, T.opt_of(case), X0.shape)
    med_bar = 1e-12 if f64 else 1e-5
    tag = "%s %s" % (case.id, "bracket" if bracket else "direct")
    fam = "k_phi<double>" if f64 else "F32"
    for t in range(W.MODEL_STEPS):
        Xt = X0 if t == 0 else multi[0]["X"][t - 1]
        a_ref, med_ref = oracle.median_scale(Xt)
        s0 = multi[0]["scales"][t]
        for r in range(case.world):
            # one scale, one path code and one X on all ranks
            assert multi[r]["scales"][t] == s0, (t, r, multi[r]["scales"][t], s0)
            assert np.array_equal(multi[r]["X"][t], multi[0]["X"][t]), (t, r)
        _report(fam + " median", "%s step %d med (path %d)" % (tag, t, s0[2]), abs(s0[1] - med_ref) / med_ref,
                med_bar)
        assert s0[1] == pytest.approx(med_ref, rel=med_bar), (t, s0, med_ref)
        Xd = multi[0]["X"][t]
        assert np.all(np.isfinite(Xd))
        if f64:
            ph_ref = oracle.phi(Xt, oracle.logp_grad_gmm(Xt, mus, covs), a_ref)
            Xref = Xt.copy()
            oracle.apply_update(Xref, o_opt.step(ph_ref), lo, up)
            err = float(np.max(np.abs(Xd - Xref)))
            _report(fam + " step", "%s step %d positions vs the oracle step" % (tag, t), err, 1e-9)
            assert err <= 1e-9, (t, err)
        err1 = float(np.max(np.abs(Xd - one["X"][t])))
        if f64 or case.shards == "aligned":
            _report(fam + " vs one rank", "%s step %d positions" % (tag, t), err1, 1e-10)
            assert err1 <= 1e-10, (t, err1)
        else:
            print("shard_paths F32 vs one rank %s step %d: positions differ by %.3g (rank 1 runs %s, one rank %s: "
                  "not compared)" % (tag, t, err1, multi[1]["names"][t], one["names"][t]))
    # the first step's scale is an exact order statistic of the same keys
    assert multi[0]["scales"][0][:2] == one["scales"][0][:2], (multi[0]["scales"][0], one["scales"][0])
    if bracket:
        assert all(s[2] != 0 for s in multi[0]["scales"]), multi[0]["scales"]  # (not the direct pass)


# --------------------- e. sharded equals one rank, bit for bit (elementwise) ----
@pytest.mark.parametrize("case_id", T.BITWISE_CASES)
def test_sharded_equals_one_rank_bitwise(case_id):
    case = T.BY_ID[case_id]
    multi = _run(case, case.world, "steps", model="elem")
    one = _run(case, 1, "steps", model="elem")[0]
    _check_names_and_shards(case, multi)
    assert all(nm.startswith(case.names[0]) for nm in one["names"]), one["names"]
    for t in range(W.MODEL_STEPS):
        for r in range(case.world):
            Xd = multi[r]["X"][t]
            bad = np.flatnonzero((Xd != one["X"][t]).ravel())
            assert bad.size == 0, ("%s rank %d step %d: %d elements differ from one rank's, first at %s, max |diff| %.3g"
                                   % (case.id, r, t, bad.size, np.unravel_index(bad[0], Xd.shape),
                                      np.max(np.abs(Xd - one["X"][t]))))
            assert multi[r]["scales"][t][:2] == one["scales"][t][:2], (t, r, multi[r]["scales"][t], one["scales"][t])
    print("shard_paths bitwise %s: X and (a, med) of %d ranks equal one rank's over %d steps (%s)"
          % (case.id, case.world, W.MODEL_STEPS, multi[case.world - 1]["names"][0]))
