"""Device GLM score (svgd_glm.hip: svgd_set_device_glm, k_glm_pass /
k_glm_finish) against the np.longdouble definition of tests/_glm.py.

Bar (tests/_glm.py): |device - reference| <= 1e-13 * scale per element, and
|device - host| <= 2e-13 * scale; each test prints its worst error as a
fraction of the bar ("glm ...").  The shapes are the smallest at which the
tile code can go wrong: every KP/4 remainder and 16-column block edge in d,
fewer rows than a wave's 16 and ragged work-groups in N, windows below one
64-record tile, exactly one, ragged, and many (S > 1 data splits)."""
import multiprocessing as mp
import uuid

import numpy as np
import pytest

import _glm as R
import _gpu_glm_worker as W
import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

pytestmark = pytest.mark.gpu

LINKS = ["logistic", "gaussian"]
DIMS = [1, 2, 3, 4, 5, 8, 15, 16, 17, 32, 33, 48, 49, 63, 64]
NS = [1, 15, 129, 1000]
BATCHES = [1, 15, 17, 64, 65, 1000, 4097]
# every d once, cycling through N and the batch; then the pairings the cycle
# misses: d = 4 with a ragged batch, S > 1 at d = 64 and at a ragged d with
# 8 row groups
GRID = [(d, NS[i % 4], BATCHES[i % 7]) for i, d in enumerate(DIMS)] + \
       [(4, 129, 17), (64, 1000, 1000), (55, 1000, 65), (16, 15, 4097)]
S_LIK, LAM = 0.7, 1.3


def _device_grad(X, model, dtype=None):
    c = S.Context(X.shape[1], X.shape[0], dtype=dtype)
    c.set_particles(X)
    c.set_device_model(model)
    G = c.device_logp_grad()
    return c, G


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d,n,batch", GRID)
def test_device_gradient_matches_definition_and_host(d, n, batch, link):
    A, y, X = R.case(d, batch, n, link)
    model = S.GeneralizedLinearModel(A, y, link, S_LIK, LAM)
    c, Gd = _device_grad(X, model)
    c.close()
    bar = R.grad_bar(A, y, X, link, s=S_LIK, lam=LAM)
    ex = R.excess(Gd, R.ref_grad(A, y, X, link, s=S_LIK, lam=LAM), bar)
    exh = R.excess(Gd, model.log_model_grad(X).astype(R.LD), 2 * bar)
    print("glm %s d=%d n=%d batch=%d: vs definition %.3g of the bar, vs host %.3g of 2x the bar"
          % (link, d, n, batch, ex, exh))
    assert np.all(np.isfinite(Gd))
    assert ex <= 1.0
    assert exh <= 1.0


@pytest.mark.parametrize("link", LINKS)
def test_windows(link):
    """Windows that start off a tile boundary and end inside the data: the
    records past the window are real data and must not be summed."""
    d, n, M = 17, 129, 1063
    A, y, X = R.case(d, M, n, link)
    model = S.GeneralizedLinearModel(A, y, link, S_LIK, LAM)
    model.set_batch(3, 61)  # the model's current window is taken over
    c, G = _device_grad(X, model)
    kw = dict(s=S_LIK, lam=LAM, m0=3, count=61)
    worst = R.excess(G, R.ref_grad(A, y, X, link, **kw), R.grad_bar(A, y, X, link, **kw))
    assert worst <= 1.0, worst
    for m0 in (0, 1, 3, 999):
        for cnt in (1, 61, 64):
            c.set_device_batch(m0, cnt)
            G = c.device_logp_grad()
            kw = dict(s=S_LIK, lam=LAM, m0=m0, count=cnt)
            ex = R.excess(G, R.ref_grad(A, y, X, link, **kw), R.grad_bar(A, y, X, link, **kw))
            worst = max(worst, ex)
            assert ex <= 1.0, (m0, cnt, ex)
    print("glm windows %s: worst %.3g of the bar" % (link, worst))
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
        c.set_device_batch(1000, 64)
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
        c.set_device_batch(0, 0)
    c.close()


def test_range():
    """|z| up to 800 (r = y - 1 or y to rounding, e underflows to exactly 0),
    all-zero data, soft labels and no prior: finite and at the bar."""
    d, n, M = 3, 40, 130
    A, y, X = (np.array(a) for a in R.case(d, M, n, "logistic"))
    X[0] = 800.0 * A[0] / (A[0] @ A[0])
    X[1] = -800.0 * A[5] / (A[5] @ A[5])
    X[2] = 800.0 * A[129] / (A[129] @ A[129])
    rng = np.random.default_rng(5)
    soft = rng.uniform(0.0, 1.0, M)
    cases = [("wide", A, y, LAM), ("zero-data", np.zeros_like(A), y, LAM), ("soft", A, soft, LAM),
             ("no-prior", A, y, 0.0), ("zero-data, no prior", np.zeros_like(A), soft, 0.0)]
    for name, Ac, yc, lam in cases:
        model = S.GeneralizedLinearModel(Ac, yc, "logistic", S_LIK, lam)
        c, G = _device_grad(X, model)
        c.close()
        assert np.all(np.isfinite(G)), name
        ex = R.excess(G, R.ref_grad(Ac, yc, X, "logistic", s=S_LIK, lam=lam),
                      R.grad_bar(Ac, yc, X, "logistic", s=S_LIK, lam=lam))
        print("glm range %s: %.3g of the bar, max |z| = %.3g" % (name, ex, np.max(np.abs(X @ Ac.T))))
        assert ex <= 1.0, name


@pytest.mark.parametrize("link", LINKS)
def test_two_calls_and_both_dtypes_give_the_same_bits(link):
    d, n, M = 33, 1000, 1000  # 8 row groups, S > 1
    A, y, X = R.case(d, M, n, link)
    model = S.GeneralizedLinearModel(A, y, link, S_LIK, LAM)
    c, G1 = _device_grad(X, model)
    G2 = c.device_logp_grad()
    c.close()
    assert np.array_equal(G1, G2)
    c32, G3 = _device_grad(X, model, dtype=C.SVGD_F32)
    c32.close()
    assert np.array_equal(G1, G3)


def _window(t, M):
    return (37 * t) % (M - 120), 100 + t


@pytest.mark.parametrize("n,d,M", [(2500, 8, 500), (700, 33, 300)])
def test_device_step_follows_host_gradient_step(n, d, M):
    """Five Adam steps with a window that moves every step: positions within
    1e-12, scale within 1e-13 relative (the bars of test_gpu_device_model.py)."""
    A, y, X0 = R.case(d, M, n, "logistic")
    X0 = X0 * 0.25
    runs = []
    for device in (False, True):
        model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
        c = S.Context(d, n)
        c.set_particles(X0)
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
        if device:
            c.set_device_model(model)
        for t in range(5):
            if device:
                c.set_device_batch(*_window(t, M))
                c.step_device()
            else:
                model.set_batch(*_window(t, M))
                c.step_with_model(model)
        runs.append((c.get_particles(), c.last_scale()[0]))
        c.close()
    err = float(np.max(np.abs(runs[1][0] - runs[0][0])))
    print("glm step n=%d d=%d: positions %.3g, scale rel %.3g"
          % (n, d, err, abs(runs[1][1] / runs[0][1] - 1.0)))
    assert err <= 1e-12
    assert runs[1][1] == pytest.approx(runs[0][1], rel=1e-13)


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
    device steps: the scales are bit-exact and X within 1e-10 of one rank's."""
    n, d, world = 1000, 5, 3
    ranks = _run_ranks(world, n, d)
    model, X0 = W.problem(n, d)
    c = S.Context(d, n)
    one = W.steps(c, model, X0)
    c.close()
    for r in range(world):
        assert ranks[r]["scales"] == one["scales"], r
        assert np.array_equal(ranks[r]["X"], ranks[0]["X"])
    err = float(np.max(np.abs(ranks[0]["X"] - one["X"])))
    print("glm sharded world=%d n=%d: X err %.3g" % (world, n, err))
    assert err <= 1e-10
    assert sorted(ranks[r]["shard"] for r in range(world))[0][0] == 0


def test_ksd_uses_the_device_glm_and_observes_only():
    n, d, M = 700, 8, 300
    A, y, X0 = R.case(d, M, n, "logistic")
    X0 = X0 * 0.25
    model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
    finals = []
    for with_ksd in (True, False):
        c = S.Context(d, n)
        c.set_particles(X0)
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
        c.set_device_model(model)
        c.step_device()
        c.step_device()
        if with_ksd:
            X2 = c.get_particles()
            a = 0.3
            vd, ud = c.ksd(None, a)
            vh, uh = c.ksd(model.log_model_grad(X2), a)
            # the KSD's own bar, 1e-10 max(1, mean|u|), with mean|u| >= |mean u| = |V|
            bar = 1e-10 * max(1.0, abs(vh))
            print("glm ksd: V %.6g dV %.3g dU %.3g bar %.3g" % (vh, abs(vd - vh), abs(ud - uh), bar))
            assert abs(vd - vh) <= bar and abs(ud - uh) <= bar
        c.step_device()
        finals.append((c.get_particles(), c.last_scale()))
        c.close()
    assert np.array_equal(finals[0][0], finals[1][0])
    assert finals[0][1] == finals[1][1]


def test_model_switching(oracle):
    n, d = 200, 4
    A, y, X = R.case(d, 65, n, "gaussian")
    glm = S.GeneralizedLinearModel(A, y, "gaussian", S_LIK, LAM)
    mvn = S.MultivariateNormal(np.zeros(d), np.eye(d) * 2.0)
    c = S.Context(d, n)
    c.set_particles(X)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    with pytest.raises(S.UnsetException, match=r"^SVGDCpp: \[Unset Error\]"):
        c.set_device_batch(0, 1)
    c.set_device_model(mvn)
    np.testing.assert_allclose(c.device_logp_grad(), mvn.log_model_grad(X), rtol=1e-13, atol=1e-14)
    with pytest.raises(S.UnsetException):
        c.set_device_batch(0, 1)  # the Gaussian mirror is no GLM
    c.set_device_model(glm)
    bar = R.grad_bar(A, y, X, "gaussian", s=S_LIK, lam=LAM)
    assert R.excess(c.device_logp_grad(), R.ref_grad(A, y, X, "gaussian", s=S_LIK, lam=LAM), bar) <= 1.0
    c.set_device_model(mvn)  # and back: the GLM is cleared
    np.testing.assert_allclose(c.device_logp_grad(), mvn.log_model_grad(X), rtol=1e-13, atol=1e-14)
    c.set_device_model(glm)
    c.step_device()
    c.set_device_model(None)
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\] Null log-gradient buffer and no device model set\.$"):
        c.step_device()
    with pytest.raises(S.UnsetException, match=r"No device model set"):
        c.device_logp_grad()
    with pytest.raises(S.DimensionMismatchException):
        c.set_device_model(S.GeneralizedLinearModel(np.ones((3, d + 1)), np.ones(3)))
    c.close()
    # the Hessian scale needs the caller's Hessian sum: no device step
    c = S.Context(d, n)
    c.set_particles(X)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    c.set_device_model(glm)
    c.set_scale(C.SVGD_SCALE_HESSIAN, 0.0)
    with pytest.raises(S.UnsetException, match=r"^SVGDCpp: \[Unset Error\]"):
        c.step_device()
    c.close()


class _MovingWindow:
    """Moves the model's window before every step (as a user's loop would)."""

    def __init__(self, model, M):
        self.model, self.M, self.t = model, M, 0

    def __call__(self):
        self.model.set_batch(*_window(self.t, self.M))
        self.t += 1


def test_svgd_class_takes_the_device_step():
    n, d, M, iters = 300, 5, 200, 4
    A, y, X0 = R.case(d, M, n, "logistic")
    X0 = np.ascontiguousarray((X0 * 0.25).T)  # (d, n)

    def build(log, path=None):
        model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
        mover = _MovingWindow(model, M)
        model.Step = mover  # an instance attribute: the type stays exactly the built-in one
        coord = X0.copy()
        kernel = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Median, model)
        args = [d, iters, coord, kernel, model, S.Adam(d, n, 0.05, 0.9, 0.999)]
        if log:
            args += [np.array([-np.inf]), np.array([np.inf]), False, True, path]
        return S.SVGD(*args), coord, model

    sv, coord, _ = build(False)
    sv.Initialize()
    assert sv.UsesDeviceModelStep()
    sv.Run()
    # a manual loop with host gradients
    model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
    c = S.Context(d, n)
    c.set_particles(np.ascontiguousarray(X0.T))
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    for t in range(iters):
        model.set_batch(*_window(t, M))
        c.step_with_model(model)
    Xm = c.get_particles().T
    c.close()
    err = float(np.max(np.abs(coord - Xm)))
    print("glm SVGD class: Run vs manual host-gradient loop %.3g" % err)
    assert err <= 1e-10
    # a Hessian scale and a subclass take the split calls
    class Sub(S.GeneralizedLinearModel):
        pass
    sub = Sub(A, y)
    k = S.GaussianRBFKernel(X0.copy(), S.GaussianRBFKernel.ScaleMethod.Median, sub)
    assert not S.SVGD(d, 1, X0.copy(), k, sub, S.Adam(d, n, 0.05, 0.9, 0.999)).UsesDeviceModelStep()


def test_svgd_class_with_matrix_logging_takes_the_split_path(tmp_path):
    n, d, M, iters = 24, 3, 130, 3
    A, y, X0 = R.case(d, M, n, "logistic")
    X0 = np.ascontiguousarray((X0 * 0.25).T)
    res = []
    for log in (False, True):
        model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
        model.set_batch(5, 100)
        coord = X0.copy()
        kernel = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Median, model)
        args = [d, iters, coord, kernel, model, S.Adam(d, n, 0.05, 0.9, 0.999)]
        if log:
            args += [np.array([-np.inf]), np.array([np.inf]), False, True, str(tmp_path / "log.txt")]
        sv = S.SVGD(*args)
        sv.Initialize()
        assert sv.UsesDeviceModelStep() == (not log)
        sv.Run()
        res.append(coord)
    err = float(np.max(np.abs(res[0] - res[1])))
    print("glm SVGD class: logging (split calls) vs device step %.3g" % err)
    assert err <= 1e-10
    assert (tmp_path / "log.txt").exists()
