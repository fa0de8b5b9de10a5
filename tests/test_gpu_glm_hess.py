"""Device Hessian sum (svgd_device_neg_hess_sum; k_glm_wpass / k_glm_wgram
of svgd_glm.hip, k_gauss_hess_sum of svgd_gauss_hess.hip) and the
Hessian-scale step that takes it from the device model
(svgd_set_device_hessian).

GLM bar (tests/test_glm_cpu.py): per element
    hbar = 1e-13 (s (M/B) nrows |A|^T |A| + lambda nrows I)
against the np.longdouble definition tests/_glm.py::ref_neg_hess_sum; a scale
matrix M = H / (2 d N) against hbar / (2 d N).  Each test prints its worst
error as a fraction of the bar ("glm hess ...").  Gaussian sum: the oracle at
rtol = atol = 1e-11, the tolerance tests/test_capi_cpu.py gives the host sum."""
import multiprocessing as mp
import uuid

import numpy as np
import pytest

import _glm as R
import _gpu_glm_hess_worker as W
import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

pytestmark = pytest.mark.gpu

LINKS = ["logistic", "gaussian"]
S_LIK, LAM = 0.7, 1.3
BASE_D, BASE_N, BASE_M = 8, 129, 1000
# each axis crossed with the base case: every kind of KP/4 remainder and the
# 16-column edges in d; a partial 16-row group, a partial tile and several
# splits in N; windows off a tile boundary, one record, and counts around one
# 64-record block of the Gram and of many blocks, from a nonzero start
CASES = [(d, BASE_N, BASE_M, 0, BASE_M) for d in (1, 3, 4, 5, 8, 16, 17, 33, 55, 64)] + \
        [(BASE_D, n, BASE_M, 0, BASE_M) for n in (1, 15, 1000)] + \
        [(BASE_D, BASE_N, BASE_M, 3, 61), (BASE_D, BASE_N, BASE_M, BASE_M - 1, 1)] + \
        [(BASE_D, BASE_N, 4200, 5, cnt) for cnt in (63, 64, 65, 4097)]


def _hbar(A, n, m0, cnt, s=S_LIK, lam=LAM):
    Aw = np.abs(A[m0:m0 + cnt])
    return R.BAR * (s * A.shape[0] / cnt * n * (Aw.T @ Aw) + lam * n * np.eye(A.shape[1]))


def _device_sum(X, model, dtype=None):
    c = S.Context(X.shape[1], X.shape[0], dtype=dtype)
    c.set_particles(X)
    c.set_device_model(model)
    return c, c.device_neg_hess_sum()


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d,n,M,m0,cnt", CASES)
def test_device_hessian_sum_matches_definition(d, n, M, m0, cnt, link):
    A, y, X = R.case(d, M, n, link)
    model = S.GeneralizedLinearModel(A, y, link, S_LIK, LAM)
    model.set_batch(m0, cnt)
    c, H = _device_sum(X, model)
    H2 = c.device_neg_hess_sum()
    c.close()
    c32, H3 = _device_sum(X, model, dtype=C.SVGD_F32)
    c32.close()
    ref = R.ref_neg_hess_sum(A, y, X, link, s=S_LIK, lam=LAM, m0=m0, count=cnt)
    ex = R.excess(H, ref, _hbar(A, n, m0, cnt))
    print("glm hess %s d=%d n=%d M=%d window=(%d, %d): %.3g of the bar" % (link, d, n, M, m0, cnt, ex))
    assert np.all(np.isfinite(H))
    assert ex <= 1.0
    assert np.array_equal(H, H.T)   # exactly symmetric
    assert np.array_equal(H, H2)    # a repeat returns the same bits
    assert np.array_equal(H, H3)    # fp64 whatever the context's dtype


def test_range_and_edges():
    """theta x 100 (|z| >= 800: e underflows, w = 0 exactly), all-zero data
    (exactly lambda N I), no prior, and a shard of a single row."""
    d, n, M = 8, 129, 1000
    A, y, X = R.case(d, M, n, "logistic")
    Xw = X * 100.0
    assert np.max(np.abs(Xw @ A.T)) >= 800.0
    model = S.GeneralizedLinearModel(A, y, "logistic", S_LIK, LAM)
    c, H = _device_sum(Xw, model)
    c.close()
    assert np.all(np.isfinite(H))
    ex = R.excess(H, R.ref_neg_hess_sum(A, y, Xw, "logistic", s=S_LIK, lam=LAM), _hbar(A, n, 0, M))
    print("glm hess wide: %.3g of the bar, max |z| = %.3g" % (ex, np.max(np.abs(Xw @ A.T))))
    assert ex <= 1.0
    for link in LINKS:
        zero = S.GeneralizedLinearModel(np.zeros_like(A), y, link, S_LIK, LAM)
        c, H = _device_sum(X, zero)
        c.close()
        assert np.array_equal(H, LAM * n * np.eye(d)), link
        free = S.GeneralizedLinearModel(A, y, link, S_LIK, 0.0)
        c, H = _device_sum(X, free)
        c.close()
        ex = R.excess(H, R.ref_neg_hess_sum(A, y, X, link, s=S_LIK, lam=0.0), _hbar(A, n, 0, M, lam=0.0))
        print("glm hess no prior %s: %.3g of the bar" % (link, ex))
        assert ex <= 1.0
        one = S.GeneralizedLinearModel(A, y, link, S_LIK, LAM)
        c, H = _device_sum(X[:1], one)
        c.close()
        ex = R.excess(H, R.ref_neg_hess_sum(A, y, X[:1], link, s=S_LIK, lam=LAM), _hbar(A, 1, 0, M))
        assert ex <= 1.0 and np.array_equal(H, H.T)


def test_switch_and_errors():
    d, n = 4, 256  # 2 d N a power of two: the supplied sum's scale matrix is exact
    A, y, X = R.case(d, 65, n, "logistic")
    glm = S.GeneralizedLinearModel(A, y, "logistic", S_LIK, LAM)
    c = S.Context(d, n)
    c.set_particles(X)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    with pytest.raises(S.UnsetException, match=r"^SVGDCpp: \[Unset Error\] No device model set\.$"):
        c.device_neg_hess_sum()
    assert c.lib.svgd_device_neg_hess_sum(c.h, None) == C.SVGD_ERR_UNSET
    c.set_device_hessian(True)  # harmless without the Hessian scale
    c.set_device_model(glm)
    assert c.lib.svgd_device_neg_hess_sum(c.h, None) == C.SVGD_ERR_ARG
    c.step_device()
    c.set_device_hessian(False)
    c.set_scale(C.SVGD_SCALE_HESSIAN, 0.0)
    # off: the Unset Error as before
    with pytest.raises(S.UnsetException,
                       match=r"^SVGDCpp: \[Unset Error\] Hessian scale: svgd_set_step_hessian_sum was not "
                             r"called this step\.$"):
        c.step_device()
    c.close()
    # on: the step runs, and the scale is the device model's
    c = S.Context(d, n)
    c.set_particles(X)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    c.set_scale(C.SVGD_SCALE_HESSIAN, 0.0)
    c.set_device_hessian(True)
    c.set_device_model(glm)  # leaves the switch alone
    c.step_device()
    ref = R.ref_neg_hess_sum(A, y, X, "logistic", s=S_LIK, lam=LAM) / (2 * d * n)
    assert R.excess(c.get_scale_matrix(), ref, _hbar(A, n, 0, 65) / (2 * d * n)) <= 1.0
    # a sum the caller supplied for the step wins
    cc = 0.375
    c.set_step_hessian_sum(2.0 * d * n * cc * np.eye(d))
    c.step_device()
    assert np.array_equal(c.get_scale_matrix(), cc * np.eye(d))
    # ... for that step only
    Xt = c.get_particles()
    c.step_device()
    ref = R.ref_neg_hess_sum(A, y, Xt, "logistic", s=S_LIK, lam=LAM) / (2 * d * n)
    assert R.excess(c.get_scale_matrix(), ref, _hbar(A, n, 0, 65) / (2 * d * n)) <= 1.0
    c.close()


def _window(t, M):
    return (37 * t) % (M - 120), 100 + t


@pytest.mark.parametrize("d", [3, 8, 24])
def test_device_hessian_step_follows_split_call_step(d):
    """Five Adam steps with a window that moves every step, the Hessian sum
    and the score from the device against host sum and host gradient: both
    scale matrices within hbar / (2 d N) of the definition at their own X_t,
    positions within 1e-9 (the bar tests/test_gpu_matrix_scale.py gives
    Hessian-scale steps).  d = 24 takes the tile path of phi."""
    n, M = 300, 300
    A, y, X0 = R.case(d, M, n, "logistic")
    X0 = X0 * 0.25
    ctxs = []
    for device in (True, False):
        c = S.Context(d, n)
        c.set_particles(X0)
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
        c.set_scale(C.SVGD_SCALE_HESSIAN, 0.0)
        model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
        if device:
            c.set_device_model(model)
            c.set_device_hessian(True)
        ctxs.append((c, model))
    worst_m, worst_x = 0.0, 0.0
    for t in range(5):
        m0, cnt = _window(t, M)
        for device, (c, model) in zip((True, False), ctxs):
            Xt = c.get_particles()
            if device:
                c.set_device_batch(m0, cnt)
                c.step_device()
            else:
                model.set_batch(m0, cnt)
                c.step_with_model(model, hessian=True)
            ref = R.ref_neg_hess_sum(A, y, Xt, "logistic", s=1.0, lam=1.0, m0=m0, count=cnt) / (2 * d * n)
            ex = R.excess(c.get_scale_matrix(), ref, _hbar(A, n, m0, cnt, s=1.0, lam=1.0) / (2 * d * n))
            worst_m = max(worst_m, ex)
            assert ex <= 1.0, (t, device, ex)
        err = float(np.max(np.abs(ctxs[0][0].get_particles() - ctxs[1][0].get_particles())))
        worst_x = max(worst_x, err)
        assert err <= 1e-9, (t, err)
    print("glm hess step d=%d: scale matrix %.3g of the bar, positions %.3g" % (d, worst_m, worst_x))
    for c, _ in ctxs:
        c.close()


def _run_ranks(world, n, d):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "svgd_" + uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=W.run, args=(r, world, name, n, d, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in range(world):
            res = q.get(timeout=300)
            assert res[0] == "ok", res[2]
            out[res[1]] = res[2]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return out


def test_sharded_matches_one_rank():
    """World 3 on one GPU over the host shared-memory collectives, three
    device Hessian steps: every rank's scale matrix within hbar / (2 d N) of
    the definition at its X_t, X within 1e-9 of one rank's."""
    n, d, world = 1000, 5, 3
    ranks = _run_ranks(world, n, d)
    model, A, y, X0 = W.problem(n, d)
    c = S.Context(d, n)
    one = W.steps(c, model, X0)
    c.close()
    worst = 0.0
    for res in [one] + [ranks[r] for r in range(world)]:
        for t, (m0, cnt) in enumerate(W.WINDOWS):
            ref = R.ref_neg_hess_sum(A, y, res["before"][t], "logistic", m0=m0, count=cnt) / (2 * d * n)
            ex = R.excess(res["mats"][t], ref, _hbar(A, n, m0, cnt, s=1.0, lam=1.0) / (2 * d * n))
            worst = max(worst, ex)
            assert ex <= 1.0, (t, ex)
    err = max(float(np.max(np.abs(ranks[r]["X"] - one["X"]))) for r in range(world))
    print("glm hess sharded world=%d n=%d: scale matrix %.3g of the bar, X err %.3g" % (world, n, worst, err))
    assert err <= 1e-9
    assert sorted(ranks[r]["shard"] for r in range(world))[0][0] == 0


def _spd(d, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d)) * 0.4
    return A @ A.T + np.eye(d) * 0.3


def _gmm(oracle, d, k):
    mus = oracle.splitmix((k, d), 2.0, 32 + d)
    covs = np.stack([_spd(d, 40 + i) + np.eye(d) for i in range(k)])
    return mus, covs, S.GaussianSum(list(mus), list(covs))


@pytest.mark.parametrize("n", [1, 255, 1200])
@pytest.mark.parametrize("d,k", [(1, 1), (3, 2), (8, 4), (17, 3), (64, 2)])
def test_gaussian_sum_hessian_matches_oracle(oracle, d, k, n):
    mus, covs, model = _gmm(oracle, d, k)
    X = oracle.splitmix((n, d), 3.0, 31 + d)
    c, H = _device_sum(X, model)
    H2 = c.device_neg_hess_sum()
    c.close()
    assert np.array_equal(H, H2)
    np.testing.assert_allclose(H, oracle.neg_hess_sum_gmm(X, mus, covs), rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("d,k", [(3, 2), (8, 4)])
def test_gaussian_sum_device_hessian_step_matches_oracle(oracle, d, k):
    """The loop of test_gpu_matrix_scale.py::test_hessian_scale_step_matches_oracle
    with the step wholly on the device, at the same bars."""
    n = 1200
    X = oracle.splitmix((n, d), 3.0, 31)
    mus = oracle.splitmix((k, d), 2.0, 32)
    covs = np.stack([_spd(d, 40 + i) + np.eye(d) for i in range(k)])
    model = S.GaussianSum(list(mus), list(covs))
    c = S.Context(d, n)
    c.set_particles(X)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    c.set_scale(C.SVGD_SCALE_HESSIAN, 0.0)
    c.set_device_model(model)
    c.set_device_hessian(True)
    o_opt = oracle.Adam((n, d), 0.05, 0.9, 0.999)
    for _ in range(3):
        Xt = c.get_particles()
        M = oracle.hessian_scale(Xt, mus, covs)
        G = oracle.logp_grad_gmm(Xt, mus, covs)
        ph = oracle.phi_matrix(Xt, G, M)
        c.step_device()
        np.testing.assert_allclose(c.get_scale_matrix(), M, rtol=1e-12, atol=1e-15)
        Xref = Xt.copy()
        oracle.apply_update(Xref, o_opt.step(ph))
        assert np.max(np.abs(c.get_particles() - Xref)) <= 1e-9
    c.close()


def test_svgd_class_takes_the_device_hessian_step():
    n, d, M, iters = 300, 5, 200, 4
    A, y, X0 = R.case(d, M, n, "logistic")
    X0 = np.ascontiguousarray((X0 * 0.25).T)  # (d, n)
    model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
    model.set_batch(5, 150)
    coord = X0.copy()
    kernel = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Hessian, model)
    sv = S.SVGD(d, iters, coord, kernel, model, S.Adam(d, n, 0.05, 0.9, 0.999))
    sv.Initialize()
    assert sv.UsesDeviceModelStep()
    sv.Run()
    # the manual split loop: host Hessian sum and host gradient
    host = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
    host.set_batch(5, 150)
    c = S.Context(d, n)
    c.set_particles(np.ascontiguousarray(X0.T))
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    c.set_scale(C.SVGD_SCALE_HESSIAN, 0.0)
    for _ in range(iters):
        c.step_with_model(host, hessian=True)
    Xm = c.get_particles().T
    c.close()
    err = float(np.max(np.abs(coord - Xm)))
    print("glm hess SVGD class: Run vs the manual split loop %.3g" % err)
    assert err <= 1e-9
    # a kernel whose target model is another object keeps the split calls,
    # and so does a subclass
    other = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
    k2 = S.GaussianRBFKernel(X0.copy(), S.GaussianRBFKernel.ScaleMethod.Hessian, other)
    sv2 = S.SVGD(d, 1, X0.copy(), k2, model, S.Adam(d, n, 0.05, 0.9, 0.999))
    assert not sv2.UsesDeviceModelStep()
    sv2.Initialize()
    sv2.Run()  # the split calls, with the kernel's own model's sum

    class Sub(S.GeneralizedLinearModel):
        pass
    sub = Sub(A, y)
    k3 = S.GaussianRBFKernel(X0.copy(), S.GaussianRBFKernel.ScaleMethod.Hessian, sub)
    assert not S.SVGD(d, 1, X0.copy(), k3, sub, S.Adam(d, n, 0.05, 0.9, 0.999)).UsesDeviceModelStep()
