"""Device GLM posterior prediction (svgd_glm_predict; k_glm_predict of
svgd_glm_predict.hip) against the np.longdouble definition within the bars of
tests/_glm_predict.py (derived there; the device's table exponential is part
of that derivation).  Shapes vary one axis at a time against the base d = 8,
N = 129, m* = 200, both links at s = 0.7.  Each test prints its worst error as
a fraction of the bar ("glm predict ...")."""
import multiprocessing as mp
import uuid

import numpy as np
import pytest

import _glm as R
import _glm_predict as P
import _gpu_glm_predict_worker as W
import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

pytestmark = pytest.mark.gpu

BASE_D, BASE_N, BASE_M = 8, 129, 200
# d: every KP/4 remainder and the 16-column edges; N (streamed): one row, a
# partial 16-row group, an exact tile, a partial tail tile, several splits;
# m* (stationary): a partial wave, an exact wave, the edges of the 128-record
# work-group, many groups
CASES = [(d, BASE_N, BASE_M) for d in (1, 3, 4, 5, 8, 16, 17, 33, 55, 64)] + \
        [(BASE_D, n, BASE_M) for n in (1, 15, 64, 1000)] + \
        [(BASE_D, BASE_N, m) for m in (1, 15, 16, 127, 128, 129, 1000)]


def _device(X, A, y, link, s=P.S_LIK, dtype=None, repeat=False):
    c = S.Context(X.shape[1], X.shape[0], dtype=dtype)
    c.set_particles(X)
    out = [c.glm_predict(A, y, link, s)]
    if repeat:
        out += [c.glm_predict(A, y, link, s), c.glm_predict(A, None, link, s)]
    c.close()
    return out if repeat else out[0]


@pytest.mark.parametrize("link", P.LINKS)
@pytest.mark.parametrize("d,n,m", CASES)
def test_device_prediction_matches_definition(d, n, m, link):
    A, y, X, ref, bar = P.case(d, n, m, link)
    out, again, noy = _device(X, A, y, link, repeat=True)
    out32 = _device(X, A, y, link, dtype=C.SVGD_F32)
    ex = P.excesses(out, ref, bar)
    print("glm predict %s d=%d n=%d m=%d: mean %.3g var %.3g lpd %.3g of the bar" % ((link, d, n, m) + ex))
    assert len(out) == 3 and len(noy) == 2
    assert all(np.all(np.isfinite(o)) for o in out)
    assert np.all(out[1] >= 0.0)
    assert max(ex) <= 1.0
    for k in range(3):
        assert np.array_equal(out[k], again[k])   # a repeat returns the same bits
        assert np.array_equal(out[k], out32[k])   # fp64 whatever the context's dtype
    assert np.array_equal(out[0], noy[0]) and np.array_equal(out[1], noy[1])  # labels do not touch mean, var


def test_fractional_labels():
    """Labels inside (0, 1) take the second exponential; mixed with 0 / 1
    labels in one wave."""
    A, y, X, _, _ = P.case(8, 129, 200, "logistic")
    rng = np.random.default_rng(5)
    yf = np.where(rng.integers(0, 2, y.shape[0]) == 1, rng.uniform(0.0, 1.0, y.shape[0]), y)
    yf[:32] = y[:32]  # two waves of binary labels only
    out = _device(X, A, yf, "logistic")
    ex = P.excesses(out, P.reference(A, yf, X, "logistic"), P.bars(A, yf, X, "logistic"))
    print("glm predict fractional labels: mean %.3g var %.3g lpd %.3g of the bar" % ex)
    assert max(ex) <= 1.0


def test_edge_cases():
    d, n, m = 8, 129, 200
    for link in P.LINKS:
        A, y, X, ref, bar = P.case(d, n, m, link)
        # identical particles: var >= 0 and within its bar of 0, the mean within its bar of mu(a . theta)
        Xs = np.ascontiguousarray(np.broadcast_to(X[3], X.shape))
        mean, var, lpd = _device(Xs, A, y, link)
        bm, bv, _ = P.bars(A, y, Xs, link)
        z = A.astype(P.LD) @ X[3].astype(P.LD)
        assert np.all(var >= 0.0) and np.all(var <= bv), link
        assert R.excess(mean, R._sigmoid(z) if link == "logistic" else z, bm) <= 1.0
        assert np.all(np.isfinite(lpd))
        # all-zero rows: the logistic mean exactly 1/2 with var exactly 0, the Gaussian mean exactly 0
        mean, var = _device(X, np.zeros_like(A), None, link)
        assert np.all(mean == (0.5 if link == "logistic" else 0.0)) and np.all(var == 0.0), link
    # theta x 100 (|z| >= 800: e underflows): finite, mean in [0, 1]
    A, y, X, _, _ = P.case(d, n, m, "logistic")
    Xw = X * 100.0
    assert np.max(np.abs(Xw @ A.T)) >= 800.0
    out = _device(Xw, A, y, "logistic")
    assert all(np.all(np.isfinite(o)) for o in out)
    assert np.all(out[0] >= 0.0) and np.all(out[0] <= 1.0) and np.all(out[1] >= 0.0)
    ex = P.excesses(out, P.reference(A, y, Xw, "logistic"), P.bars(A, y, Xw, "logistic"))
    print("glm predict wide: mean %.3g var %.3g lpd %.3g of the bar" % ex)
    assert max(ex) <= 1.0
    # the documented -inf: Gaussian link, s = 1, y = 1e3, |z| <= 14
    A, y, X, ref, bar = P.case(d, n, m, "gaussian")
    assert np.max(np.abs(X @ A.T)) <= 14.0
    mean, var, lpd = _device(X, A, np.full(m, 1e3), "gaussian", s=1.0)
    assert np.all(lpd == -np.inf)
    assert max(P.excesses((mean, var), ref[:2], bar[:2])) <= 1.0


def _adam_steps(X0, model, Atest, ytest, observe):
    c = S.Context(X0.shape[1], X0.shape[0])
    c.set_particles(X0)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    c.set_device_model(model)
    c.check(c.lib.svgd_set_timing(c.h, 2))  # the level-2 diagnostic spans are counted
    for t in range(5):
        c.step_device()
        if observe and t < 4:
            c.glm_predict(Atest, ytest, "logistic", P.S_LIK)
    diag = c.diagnostics()
    counts = {k: diag[k] for k in ("steps", "phi_kernel_n", "phi_wait_n", "coll_n", "gather_g_n", "trk_steps",
                                   "trk_miss", "split_steps", "mirror_steps", "spec_steps")}
    res = (c.get_particles(), c.last_scale(), counts)
    c.close()
    return res


def test_pure_observer_and_no_device_model():
    d, n, M = 5, 300, 200
    A, y, X0 = R.case(d, M, n, "logistic")
    X0 = X0 * 0.25
    model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
    At, yt, _ = R.case(d, 129, n, "logistic", 11)
    plain = _adam_steps(X0, model, At, yt, False)
    seen = _adam_steps(X0, model, At, yt, True)
    assert np.array_equal(plain[0], seen[0])
    assert plain[1] == seen[1] and plain[2] == seen[2]
    assert plain[2]["phi_kernel_n"] == 5.0  # one span per step, none from the observer
    # after host-model steps, no device model anywhere
    c = S.Context(d, n)
    c.set_particles(X0)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    c.step_with_model(model)
    Xt = c.get_particles()
    out = c.glm_predict(At, yt, "logistic", P.S_LIK)
    c.step_with_model(model)
    c.close()
    ex = P.excesses(out, P.reference(At, yt, Xt, "logistic"), P.bars(At, yt, Xt, "logistic"))
    print("glm predict after a host-model step: mean %.3g var %.3g lpd %.3g of the bar" % ex)
    assert max(ex) <= 1.0


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


@pytest.mark.parametrize("n", [1000, 2])
def test_sharded_matches_one_rank(n):
    """World 3 on one GPU over the host shared-memory collectives (n = 2:
    rank 2's shard is empty): every rank's vectors bit-equal to each other,
    within the bars of the definition and of the one-rank result."""
    d, world = 5, 3
    ranks = _run_ranks(world, n, d)
    c = S.Context(d, n)
    one = W.predict(c, n, d)
    c.close()
    shards = sorted(ranks[r]["shard"] for r in range(world))
    assert shards[0][0] == 0 and shards[-1][1] == n
    if n == 2:
        assert any(a == b for a, b in shards)  # an empty shard took part
    worst = 0.0
    for link in W.LINKS:
        A, y, X = W.problem(n, d, link)
        ref, bar = P.reference(A, y, X, link), P.bars(A, y, X, link)
        for key, nq in ((link, 3), (link + "_noy", 2)):
            for r in range(1, world):
                assert all(np.array_equal(ranks[0][key][k], ranks[r][key][k]) for k in range(nq)), (key, r)
            ex = max(P.excesses(ranks[0][key], ref[:nq], bar[:nq]))
            ex1 = max(R.excess(ranks[0][key][k], one[key][k].astype(P.LD), bar[k]) for k in range(nq))
            worst = max(worst, ex, ex1)
            assert ex <= 1.0 and ex1 <= 1.0, (key, ex, ex1)
    print("glm predict sharded world=%d n=%d: %.3g of the bar" % (world, n, worst))


def test_errors():
    A = np.array([[0.5, -0.5], [0.25, 1.0], [0.0, -1.0]])
    y = np.array([0.0, 1.0, 0.5])
    c = S.Context(2, 4)
    c.set_particles(np.arange(8.0).reshape(4, 2) / 8)
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\] "):
        c.glm_predict(A, np.array([0.0, 1.5, 0.5]), "logistic")   # a label outside [0, 1]
    assert len(c.glm_predict(A, np.array([0.0, 1.5, 0.5]), "gaussian")) == 3
    with pytest.raises(S.DimensionMismatchException, match=r"^SVGDCpp: \[Dimension Error\] "):
        c.glm_predict(np.zeros((0, 2)))                            # m = 0
    out = np.empty(3)
    rc = c.lib.svgd_glm_predict(c.h, C.SVGD_GLM_LOGISTIC, 1.0, C.dptr(A), None, 3, None, None, C.dptr(out))
    assert rc == C.SVGD_ERR_ARG                                    # lpd without labels
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\] The log predictive density needs labels\.$"):
        c.check(rc)
    for bad in (dict(lik_scale=0.0), dict(lik_scale=np.nan)):
        with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\] "):
            c.glm_predict(A, y, "logistic", **bad)
    assert c.lib.svgd_glm_predict(c.h, 7, 1.0, C.dptr(A), None, 3, None, None, None) == C.SVGD_ERR_ARG
    assert c.lib.svgd_glm_predict(c.h, 0, 1.0, None, None, 3, None, None, None) == C.SVGD_ERR_ARG
    # every output NULL is accepted
    assert c.lib.svgd_glm_predict(c.h, 0, 1.0, C.dptr(A), C.dptr(y), 3, None, None, None) == C.SVGD_OK
    c.close()
    # d = 65: no context of that dimension exists, so svgd_glm_predict's own
    # d <= 64 refusal cannot be reached through one; test rows of another
    # dimension than the context's are refused before the call
    with pytest.raises(S.DimensionMismatchException, match=r"^SVGDCpp: \[Dimension Error\] "):
        S.Context(65, 4)
    c = S.Context(64, 4)
    c.set_particles(np.zeros((4, 64)))
    with pytest.raises(S.DimensionMismatchException, match=r"^SVGDCpp: \[Dimension Error\] "):
        c.glm_predict(np.zeros((3, 65)))
    assert len(c.glm_predict(np.zeros((3, 64)))) == 2
    c.close()
    sim = S.Context(2, 4096, sim_world=4)
    sim.set_particles(np.random.default_rng(3).standard_normal((4096, 2)))
    with pytest.raises(S.DeviceError, match=r"^SVGDCpp: \[Runtime Error\] measurement context"):
        sim.glm_predict(A)
    sim.close()


def test_svgd_class_predict():
    n, d, M, iters = 300, 5, 200, 4
    A, y, X0 = R.case(d, M, n, "logistic")
    At, yt, _ = R.case(d, 129, n, "logistic", 11)
    coord = np.ascontiguousarray((X0 * 0.25).T)  # (d, n)
    model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
    kernel = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Median, model)
    sv = S.SVGD(d, iters, coord, kernel, model, S.Adam(d, n, 0.05, 0.9, 0.999))
    sv.Initialize()
    sv.Run()
    res = sv.Predict(At, yt)
    Xt = np.ascontiguousarray(coord.T)
    host = model.predict(Xt, At, yt)
    bar = P.bars(At, yt, Xt, "logistic", s=1.0)
    ex = tuple(R.excess(o, h.astype(P.LD), b) for o, h, b in zip((res.mean, res.var, res.lpd), host, bar))
    print("glm predict SVGD class vs the host model: mean %.3g var %.3g lpd %.3g of the bar" % ex)
    assert max(ex) <= 1.0
    assert res.accuracy == float(np.mean((res.mean >= 0.5) == (yt >= 0.5)))
    assert res.mean_lpd == float(np.mean(res.lpd))
    assert np.array_equal(res.total_var, res.mean * (1.0 - res.mean)) and res.rmse is None
    nol = sv.Predict(At)
    assert nol.lpd is None and nol.mean_lpd is None and nol.accuracy is None
    assert np.array_equal(nol.mean, res.mean) and np.array_equal(nol.var, res.var)
    # the Gaussian link: total_var and rmse
    Ag, yg, Xg = R.case(d, M, n, "gaussian")
    gm = S.GeneralizedLinearModel(Ag, yg, "gaussian", 0.7, 1.0)
    cg = np.ascontiguousarray((Xg * 0.25).T)
    sg = S.SVGD(d, 1, cg, S.GaussianRBFKernel(cg, S.GaussianRBFKernel.ScaleMethod.Median, gm), gm,
                S.Adam(d, n, 0.05, 0.9, 0.999))
    rg = sg.Predict(Ag, yg)
    assert np.array_equal(rg.total_var, rg.var + 1.0 / 0.7) and rg.accuracy is None
    assert rg.rmse == float(np.sqrt(np.mean((rg.mean - yg) ** 2)))
    # any other model is refused
    mvn = S.MultivariateNormal(np.zeros(d), np.eye(d))
    c2 = coord.copy()
    sv2 = S.SVGD(d, 1, c2, S.GaussianRBFKernel(c2, S.GaussianRBFKernel.ScaleMethod.Median, mvn), mvn,
                 S.Adam(d, n, 0.05, 0.9, 0.999))
    with pytest.raises(TypeError):
        sv2.Predict(At, yt)
