"""The restore and redo of a failed speculative step on every path that can
speculate.  GPU only.

Twins: context A at the defaults, context B with SVGD_SPECULATE=0 and
SVGD_TRACK_BRACKET=0; both receive the same calls.  The schedule
(tests/_gpu_redo_rank_worker.py): the bracket path from the first step, nine
steps, a one-key candidate capacity before steps 3 and 6.  After every step
the particles and [a, med] are bit-identical; at steps 3 and 6 A's spec_steps
rose by exactly one over the step and the scale came from the streamed
fallback -- a speculative step whose device plan failed, restored from bak
(X_t, m_t, v_t, t, xver) and redone.  Steps 4, 5, 7, 8 carry the restored
m, v, t forward: their bit identity is what catches a wrong restore.  fp64
cases also compare steps 3 and 6 with the oracle step from A's own X_t (1e-9).

n per case: N below, the smallest tried at which steps 3 and 6 speculate and
are redone -- the starting sizes (2049; 3100 for the symmetric pass) except on
the F32 paths, where at n = 2049 every step's selection took the streamed
fallback (no step speculated at d = 6, 14 or 64) and n = 3100 does.
"""
import multiprocessing as mp
import uuid

import numpy as np
import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

import _glm as R
import _gpu_redo_rank_worker as W
import _update_cases as U
from _dispatch import KNOBS

pytestmark = pytest.mark.gpu

FALLBACK = C.SVGD_MEDIAN_FALLBACK
SPEC_KNOBS = ("SVGD_SPECULATE", "SVGD_TRACK_BRACKET", "SVGD_TRACK_ERR_MULT", "SVGD_TRACK_MIN_WIDTH")
# the n each family settled on
N = {"rows": 2049, "sym": 3100, "t64": 2049, "f32": 3100, "imq": 2049, "gmm": 2049, "glm": 2049,
     "resolve": 2049, "world3": 2049, "world2": 3100, "miss": 6000}


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS + SPEC_KNOBS:
        monkeypatch.delenv(k, raising=False)


def _twins(monkeypatch, n, d, opt, bnd, env=None, dtype=None, kernel="rbf", prefix=None, X0=None, tune=True):
    """(A, B, X_0, (lo, up)): A at the defaults, B synchronous; same particles,
    optimizer, bounds and tuning."""
    X = W.problem(n, d)[0] if X0 is None else X0
    lo, up = U.BOUNDS[bnd](d)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    ctxs = []
    for sync in (False, True):
        if sync:
            for k, v in W.SYNC_ENV.items():
                monkeypatch.setenv(k, v)
        c = S.Context(d, n, dtype=dtype)
        c.set_particles(X)
        if kernel == "imq":
            c.set_kernel("imq")
        W.set_optimizer(c, opt)
        if lo is not None:
            c.set_bounds(lo, up)
        if tune:
            W.tune_bracket(c)
        if prefix is not None:
            assert c.phi_kernel_name().startswith(prefix), c.phi_kernel_name()
        ctxs.append(c)
    return ctxs[0], ctxs[1], X, (lo, up)


def _oracle_opt(oracle, opt, shape):
    if opt == "adam":
        return oracle.Adam(shape, 0.1, 0.9, 0.999)
    if opt == "adagrad":
        return oracle.AdaGrad(shape, 0.1)
    return oracle.RMSProp(shape, 0.1, 0.9)


def _same(ra, rb):
    """Returned values of the twins, bit for bit (NaN equal to NaN)."""
    if ra is None and rb is None:
        return
    ra = ra if isinstance(ra, tuple) else (ra,)
    rb = rb if isinstance(rb, tuple) else (rb,)
    assert len(ra) == len(rb)
    for x, y in zip(ra, rb):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), (x, y)


def _scale_eq(sa, sb):
    """[a, med] of two last_scale() results, bit for bit (med is NaN behind a
    fixed-scale call such as svgd_phi)."""
    return np.array_equal(np.array(sa[:2]), np.array(sb[:2]), equal_nan=True)


def _run(a, b, X0, do_step, ref=None, after=None, label=""):
    """The schedule on both twins.  do_step(c, t, X_t); ref(t, X_t, a_t) -> the
    oracle's X_{t+1} (compared at the failed steps); after[t](c) -> a call
    that meets the pending step t before anything else does."""
    a.diagnostics()
    b.diagnostics()
    X = X0
    worst = 0.0
    for t in range(W.STEPS):
        for c in (a, b):
            W.tune_step(c, t)
        assert a.diagnostics()["spec_steps"] == 0  # (read before the step: the read resets it)
        for c in (a, b):
            do_step(c, t, X)
        if after is not None and t in after:
            _same(after[t](a), after[t](b))
        Xa, Xb = a.get_particles(), b.get_particles()
        assert np.array_equal(Xa, Xb), (label, t, float(np.max(np.abs(Xa - Xb))))
        sa, sb = a.last_scale(), b.last_scale()
        assert _scale_eq(sa, sb), (label, t, sa, sb)
        rose = a.diagnostics()["spec_steps"]
        if t in W.FAIL:
            # one speculative step was planned over this step, and the scale
            # it ended with is the redo's (the one-key capacity overflows)
            assert rose == 1, (label, t, rose)
            assert sa[2] == FALLBACK and sb[2] == FALLBACK, (label, t, sa, sb)
        if ref is not None:
            Xr = ref(t, X, sa[0])
            if Xr is not None:
                err = float(np.max(np.abs(Xa - Xr)))
                if t in W.FAIL:
                    worst = max(worst, err)
                    assert err <= 1e-9, (label, t, err)
        X = Xa
    assert b.diagnostics()["spec_steps"] == 0
    if ref is not None:
        print("spec_redo %s n=%d: worst position err at the redone steps %.3g (bar 1e-9)"
              % (label, X0.shape[0], worst))
    a.close()
    b.close()
    return X, getattr(ref, "Xpre", None)


def _check_bounds(XT, Xpre, bounds):
    """(model-driven particles; Xpre is the oracle's, within 1e-9 of the device's)"""
    U.assert_bounds_exercised(XT, *bounds, Xpre=Xpre, every_dim=False, margin=1e-6)


def _ref(oracle, opt, shape, bounds, grad, phi=None):
    """The oracle's trajectory of optimizer states along A's own X_t: per step
    phi of (X_t, grad(t, X_t), A's scale), the optimizer step, the clamp."""
    o_opt = _oracle_opt(oracle, opt, shape)
    phi = oracle.phi if phi is None else phi

    def step(t, Xt, a_t):
        Xr = Xt.copy()
        delta = o_opt.step(phi(Xt, grad(t, Xt), a_t))
        step.Xpre = Xt + delta  # (the last step's positions before the clamp)
        oracle.apply_update(Xr, delta, *bounds)
        return Xr
    return step


def _model(n, d):
    _, mus, covs = W.problem(n, d)
    return S.GaussianSum(list(mus), list(covs)), mus, covs


def _imq_phi_host(X, G, a):
    """The library's host IMQ phi by direct differences (checked against the
    long-double definition on the CPU, tests/test_imq_cpu.py)."""
    n, d = X.shape
    out = np.empty((n, d))
    X, G = np.ascontiguousarray(X), np.ascontiguousarray(G)
    assert C.lib().svgd_imq_phi_host(d, n, C.dptr(X), C.dptr(G), float(a), 0, n, C.dptr(out)) == 0
    return out


def _steppers(model):
    cache = {}

    def caller_g(c, t, X):
        if t not in cache:
            cache.clear()
            cache[t] = model.log_model_grad(X)
        c.check(c.lib.svgd_step(c.h, C.dptr(cache[t])))
    return {"pipelined": lambda c, t, X: c.step_with_model(model),
            "split": lambda c, t, X: c.step_with_model(model, pipelined=False),
            "caller-g": caller_g}


# --------------------------------------------------------- 1. row stream ----
@pytest.mark.parametrize("mode", ["pipelined", "split", "caller-g"])
@pytest.mark.parametrize("opt", ["adam", "adagrad", "rmsprop"])
@pytest.mark.parametrize("d", [5, 12])
def test_row_stream_redo(oracle, monkeypatch, d, opt, mode):
    """k_phi_reduce's bak (R = 4 and R = 2), through svgd_step_host_model
    (mirror and row halves at their defaults), the split begin / finish calls
    and svgd_step with a caller's G; per-dimension bounds except on the
    pipelined Adam runs (the earlier tests' configuration, at this n)."""
    n = N["rows"]
    bnd = "none" if (mode, opt) == ("pipelined", "adam") else "perdim"
    a, b, X, bounds = _twins(monkeypatch, n, d, opt, bnd, prefix="k_phi_rows<%d," % d)
    model, mus, covs = _model(n, d)
    ref = _ref(oracle, opt, X.shape, bounds, lambda t, Xt: oracle.logp_grad_gmm(Xt, mus, covs))
    XT, Xpre = _run(a, b, X, _steppers(model)[mode], ref, label="rows d=%d %s %s" % (d, opt, mode))
    if bounds[0] is not None:
        _check_bounds(XT, Xpre, bounds)


# ------------------------------------------------------ 2. symmetric pass ----
@pytest.mark.parametrize("sym,opt", [("1", "rmsprop"), ("2", "adagrad")])
def test_symmetric_pass_redo(oracle, monkeypatch, sym, opt):
    """bak written by k_sym_finish (SVGD_PHI_SYM=1) and k_sym_apply (=2), d = 8."""
    n, d = N["sym"], 8
    a, b, X, bounds = _twins(monkeypatch, n, d, opt, "perdim", env={"SVGD_PHI_SYM": sym}, prefix="k_phi_sym<8>")
    model, mus, covs = _model(n, d)
    ref = _ref(oracle, opt, X.shape, bounds, lambda t, Xt: oracle.logp_grad_gmm(Xt, mus, covs))
    XT, Xpre = _run(a, b, X, _steppers(model)["pipelined"], ref, label="sym=%s %s" % (sym, opt))
    _check_bounds(XT, Xpre, bounds)


# ----------------------------------------------------------- 3. fp64 tiles ----
@pytest.mark.parametrize("d,opt", [(24, "adagrad"), (64, "adam"), (64, "rmsprop")])
def test_f64_tiles_redo(oracle, monkeypatch, d, opt):
    """bak written by k_opt_update behind k_phi<double>."""
    n = N["t64"]
    a, b, X, bounds = _twins(monkeypatch, n, d, opt, "perdim", prefix="k_phi<double,")
    model, mus, covs = _model(n, d)
    ref = _ref(oracle, opt, X.shape, bounds, lambda t, Xt: oracle.logp_grad_gmm(Xt, mus, covs))
    XT, Xpre = _run(a, b, X, _steppers(model)["pipelined"], ref, label="t64 d=%d %s" % (d, opt))
    _check_bounds(XT, Xpre, bounds)


# ------------------------------------------------------------------ 4. F32 ----
@pytest.mark.parametrize("d,opt,prefix", [(64, "adam", "k_phi_b3<64,"), (14, "adagrad", "k_phi_f32s<16,"),
                                          (6, "rmsprop", "k_phi<float, 8,")])
def test_f32_redo(monkeypatch, d, opt, prefix):
    """bak written by the fused epilogues of k_phi_b3 and k_phi_f32s and by
    k_opt_update behind the generic fp32 tiles; twins only.  n = 3100: at 2049
    no step of these paths speculates."""
    n = N["f32"]
    a, b, X, bounds = _twins(monkeypatch, n, d, opt, "perdim", dtype=C.SVGD_F32, prefix=prefix)
    model, _, _ = _model(n, d)
    XT, Xpre = _run(a, b, X, _steppers(model)["pipelined"], label="f32 d=%d %s" % (d, opt))
    _check_bounds(XT, Xpre, bounds)


# ------------------------------------------------------------------ 5. IMQ ----
@pytest.mark.parametrize("d,opt,prefix", [(8, "adam", "k_imq_pass<8>"), (8, "rmsprop", "k_imq_pass<8>"),
                                          (33, "adagrad", "k_imq_pass<36>")])
def test_imq_redo(oracle, monkeypatch, d, opt, prefix):
    """The IMQ chain (records, pass, finish, k_opt_update) restored and redone."""
    n = N["imq"]
    a, b, X, bounds = _twins(monkeypatch, n, d, opt, "perdim", kernel="imq", prefix=prefix)
    model, mus, covs = _model(n, d)
    ref = _ref(oracle, opt, X.shape, bounds, lambda t, Xt: oracle.logp_grad_gmm(Xt, mus, covs), _imq_phi_host)
    XT, Xpre = _run(a, b, X, _steppers(model)["pipelined"], ref, label="imq d=%d %s" % (d, opt))
    _check_bounds(XT, Xpre, bounds)


# -------------------------------------------------------- 6. device models ----
@pytest.mark.parametrize("opt", ["rmsprop", "adagrad"])
def test_device_gaussian_sum_redo(oracle, monkeypatch, opt):
    """step_device() with a three-component Gaussian sum at d = 8: the redo
    reuses the G the device model wrote for the failed step."""
    n, d = N["gmm"], 8
    a, b, X, bounds = _twins(monkeypatch, n, d, opt, "perdim")
    model, mus, covs = _model(n, d)
    for c in (a, b):
        c.set_device_model(model)
    ref = _ref(oracle, opt, X.shape, bounds, lambda t, Xt: oracle.logp_grad_gmm(Xt, mus, covs))
    XT, Xpre = _run(a, b, X, lambda c, t, Xt: c.step_device(), ref, label="device gmm %s" % opt)
    _check_bounds(XT, Xpre, bounds)


def _window(t, M):
    return (37 * t) % (M - 120), 100 + t


def test_device_glm_redo_inside_the_batch_setter(oracle, monkeypatch):
    """A device GLM (logistic, d = 17, M = 200) whose window moves before every
    step: the window of step t + 1 is set right behind step t, so the pending
    redo of a failed step runs inside svgd_set_device_glm_batch and must use
    the G of the old window (still on the device), not the new window's."""
    n, d, M = N["glm"], 17, 200
    A, y, X0 = R.case(d, M, n, "logistic")
    X0 = np.ascontiguousarray(X0 * 0.25)
    a, b, X, bounds = _twins(monkeypatch, n, d, "adam", "perdim", X0=X0)
    model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
    for c in (a, b):
        c.set_device_model(model)
        c.set_device_batch(*_window(0, M))

    def step(c, t, Xt):
        c.step_device()
        c.set_device_batch(*_window(t + 1, M))

    def grad(t, Xt):
        model.set_batch(*_window(t, M))
        return model.log_model_grad(Xt)
    ref = _ref(oracle, "adam", X.shape, bounds, grad)
    XT, Xpre = _run(a, b, X, step, ref, label="device glm")
    _check_bounds(XT, Xpre, bounds)


# ------------------------------- 7. resolved by something other than a step ----
def _resolvers(n, d):
    import oracle as O
    G = O.splitmix((n, d), 1.0, 91)
    At = O.splitmix((40, d), 1.0, 92)
    yt = (O.splitmix((40,), 1.0, 93) > 0).astype(np.float64)
    lo, up = U.inverted_bounds(d)
    return {"ksd": lambda c: c.ksd(G, 0.3),
            "glm_predict": lambda c: c.glm_predict(At, yt, "logistic", 1.0),
            "phi": lambda c: c.phi(G, 0.3),
            "median_scale": lambda c: c.median_scale(),
            "set_bounds": lambda c: c.set_bounds(lo, up),
            "set_optimizer": lambda c: c.set_optimizer(C.SVGD_OPT_RMSPROP, 0.1, 0.9, 0.0, 1e-8),
            "sync": lambda c: c.sync()}


@pytest.mark.parametrize("first,second", [("ksd", "glm_predict"), ("phi", "median_scale"),
                                          ("set_bounds", "sync"), ("set_optimizer", "ksd"),
                                          ("glm_predict", "set_optimizer"), ("median_scale", "phi"),
                                          ("sync", "set_bounds")])
def test_pending_failed_step_resolved_by_another_call(monkeypatch, first, second):
    """The failed step 3 (6) is pending when `first` (`second`) is called: the
    observer or setter runs the redo itself, then its own work on the redone
    X_{t+1}.  Returned values and the trajectory stay bit-identical
    (set_optimizer resets both twins to equal state)."""
    n, d = N["resolve"], 5
    a, b, X, _ = _twins(monkeypatch, n, d, "adam", "perdim", prefix="k_phi_rows<5,")
    model, _, _ = _model(n, d)
    res = _resolvers(n, d)
    _run(a, b, X, _steppers(model)["pipelined"], after={3: res[first], 6: res[second]},
         label="resolve %s/%s" % (first, second))


# ------------------------------------------------------------ 8. sharded ----
def _ranks(world, cfg):
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


@pytest.mark.parametrize("world,d,opt,env,key,prefix",
                         [(3, 5, "rmsprop", {}, "world3", "k_phi_rows<5,"),
                          (2, 8, "adam", {"SVGD_PHI_SYM": "1"}, "world2", "k_phi_sym<8>")])
def test_sharded_redo(world, d, opt, env, key, prefix):
    """The restore all-gathers X_t again and the redo's collectives match
    across ranks (SVGD_DEBUG_COLL=1 hashes every step's sequence).  The
    sharded speculative run against the sharded synchronous twin: bit for
    bit, every rank.  Against the one-rank synchronous twin the sharded phi
    sums are grouped differently (column splits, the symmetric exchange), so
    that bar is 1e-10 on positions and 1e-13 relative on later scales, the
    first scale bit-exact -- the bars of tests/test_gpu_multirank.py."""
    n = N[key]
    cfg = {"n": n, "d": d, "opt": opt, "env": dict(env, SVGD_DEBUG_COLL="1")}
    spec = _ranks(world, cfg)
    sync = _ranks(world, dict(cfg, env=dict(cfg["env"], **W.SYNC_ENV)))
    one = _ranks(1, dict(cfg, env=dict(cfg["env"], **W.SYNC_ENV)))[0]
    for rank in range(world):
        ra, rb = spec[rank], sync[rank]
        assert ra["phi_kernel"].startswith(prefix), ra["phi_kernel"]
        assert rb["spec"] == [0] * W.STEPS
        for t in range(W.STEPS):
            assert np.array_equal(ra["X"][t], rb["X"][t]), (rank, t)
            assert ra["scales"][t][:2] == rb["scales"][t][:2], (rank, t)
            np.testing.assert_allclose(ra["X"][t], one["X"][t], rtol=0, atol=1e-10)
            np.testing.assert_allclose(ra["scales"][t][0], one["scales"][t][0], rtol=1e-13)
        assert ra["scales"][0][0] == one["scales"][0][0]
        for t in W.FAIL:
            assert ra["spec"][t] == 1, (rank, ra["spec"])
            assert ra["scales"][t][2] == FALLBACK and rb["scales"][t][2] == FALLBACK
    # the ranks' trajectories are one trajectory
    for rank in range(1, world):
        assert all(np.array_equal(x, y) for x, y in zip(spec[0]["X"], spec[rank]["X"]))
    lo, up = U.bounds(d)
    U.assert_bounds_exercised(spec[0]["X"][-1], lo, up, every_dim=False)


# ------------------------------------------------------- 9. tracker miss ----
def test_tracker_miss_redo_with_rmsprop_and_bounds(monkeypatch):
    """A predicted bracket that always misses (instead of an overflow): every
    tracked step is restored and redone with a sampled bracket; RMSProp (bak
    reads m for a kind that never loads it) and per-dimension bounds.
    n = 6000: the tracker needs more pairs than direct_max_pairs with no
    tuning set."""
    n, d = N["miss"], 8
    env = {"SVGD_TRACK_ERR_MULT": "0", "SVGD_TRACK_MIN_WIDTH": "1e-14"}
    a, b, X, bounds = _twins(monkeypatch, n, d, "rmsprop", "perdim", env=env, tune=False)
    model, _, _ = _model(n, d)
    a.diagnostics()
    for t in range(10):
        for c in (a, b):
            c.step_with_model(model)
        assert np.array_equal(a.get_particles(), b.get_particles()), t
        assert _scale_eq(a.last_scale(), b.last_scale()), t
    da = a.diagnostics()
    assert da["trk_miss"] == da["trk_steps"] >= 3, da
    U.assert_bounds_exercised(a.get_particles(), *bounds, every_dim=False)
    a.close()
    b.close()
