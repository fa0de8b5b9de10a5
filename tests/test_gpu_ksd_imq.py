"""Device kernelized Stein discrepancy under the inverse multiquadric kernel
(svgd_ksd_kernel, Context.ksd(kernel="imq"), SVGD.ComputeKSD(kernel="imq")).

For particles x_i, scores s_i = grad log p(x_i), k = (1 + a |r|^2)^(-1/2),
r = x_i - x_j:

    u_ij   = k s_i.s_j + a k^3 (s_i - s_j).r + a d k^3 - 3 a^2 k^5 |r|^2
    row_i  = (1/N) sum_j u_ij
    KSD2_V = (1/N) sum_i row_i,   KSD2_U = (1/(N(N-1))) sum_{i != j} u_ij

The reference is this direct formula in numpy longdouble (tests/_ksd_imq.py).
Bar: |device - reference| <= 1e-12 max(1, mean|u_ij|) for V, U and every
row_i (a row's bar takes the mean over that row).  Each test prints its
observed error ("ksd imq ..." lines, shown with -s or -rA) before it asserts.
"""
import multiprocessing as mp
import uuid

import numpy as np
import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

import _glm as R
import _gpu_ksd_imq_worker as W
import _ksd_imq as K

pytestmark = pytest.mark.gpu

LD = K.LD


def _check(tag, X, G, a, ref=None, dtype=C.SVGD_F64):
    n, d = X.shape
    c = S.Context(d, n, dtype=dtype)
    c.set_particles(X)
    v, u, rows = c.ksd(G, a, rows=True, kernel="imq")
    c.close()
    ref = K.ksd_imq_ref(X, G, a) if ref is None else ref
    ev, eu, er = K.errors(v, u, rows, ref)
    print("ksd imq %s n=%d d=%d a=%.3g V=%.6g U=%.6g mean|u|=%.3g err/bar V %.3g U %.3g worst row %.3g"
          % (tag, n, d, a, v, u, ref[3], ev, eu, er))
    assert np.isfinite(v) and np.all(np.isfinite(rows))
    assert ev <= 1.0
    if n > 1:
        assert eu <= 1.0
    else:
        assert np.isnan(u)
    assert er <= 1.0
    return v, u, rows


SHAPES = ([(1, 3), (2, 1), (77, 3), (257, 1), (1000, 8)] +
          [(515, d) for d in range(1, 65) if d % 4 in (0, 1)])


@pytest.mark.parametrize("n,d", SHAPES)
def test_ksd_imq_matches_direct_formula(oracle, n, d):
    """Both ends of every KP = 4 ceil(d / 4) instantiation, at a size that is
    ragged against the 128-row work-groups, the 64- and 32-record tiles and
    the column splits; n = 1 and 2 are the degenerate ends."""
    X = oracle.splitmix((n, d), 3.0, 900 + n + d)
    G = K.model(d).log_model_grad(X)
    a = K.scale(d)
    v, u, _ = _check("shape", X, G, a)
    assert v >= 0.0
    if n == 1:
        assert v == pytest.approx(float(G[0] @ G[0]) + a * d, rel=1e-14)


@pytest.mark.parametrize("name", K.EDGE)
def test_ksd_imq_edge_clouds(name):
    """Shifted by +1e3 and +1e6 (the pass works on centred coordinates), three
    outliers at 1e4, two duplicate pairs, anisotropic (1e3, 1, 1e-3), a = 1e6
    and 1e-8, two clusters 40 apart."""
    X, G, a, ref = K.edge_case(name)
    v, u, rows = _check(name, X, G, a, ref)
    assert v >= 0.0
    if name == "a1e6":
        # polynomial tails: unlike the RBF statistic's, the rows are not just the diagonal
        n, d = X.shape
        diag = ((G.astype(LD) ** 2).sum(1) + LD(a) * d) / n
        off = np.abs((rows.astype(LD) - diag).astype(np.float64))
        print("ksd imq a1e6 off-diagonal share of the rows: min %.3g max %.3g (bar of a row about %.3g)"
              % (off.min(), off.max(), K.BAR * max(1.0, float(ref[4].min()))))
        assert np.all(off > 100 * K.BAR * np.maximum(1.0, ref[4]))


@pytest.mark.parametrize("n,d", [(1000, 8), (515, 33)])
def test_rbf_through_the_new_entry_is_svgd_ksd(oracle, n, d):
    X = oracle.splitmix((n, d), 3.0, 37)
    G = K.model(d).log_model_grad(X)
    c = S.Context(d, n)
    c.set_particles(X)
    a = c.ksd(G, K.scale(d), rows=True)
    b = c.ksd(G, K.scale(d), rows=True, kernel="rbf")
    import ctypes

    v, u, rows = ctypes.c_double(), ctypes.c_double(), np.empty(n)
    c.check(c.lib.svgd_ksd_kernel(c.h, C.SVGD_KERNEL_RBF, C.dptr(G), K.scale(d), ctypes.byref(v), ctypes.byref(u),
                                  C.dptr(rows)))
    c.close()
    assert a[0] == b[0] == v.value and a[1] == b[1] == u.value
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[2], rows)


def test_ksd_imq_device_models(oracle):
    """G_shard = None evaluates the device model -- the Gaussian-sum mirror
    and a device GLM: the same result as the host gradient of the same model."""
    n, d = 515, 8
    X = oracle.splitmix((n, d), 3.0, 35)
    A, y, _ = R.case(d, 300, n, "logistic")
    for tag, model, Xm in (("gauss", K.model(d, k=4), X),
                           ("glm", S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0), X / 3.0)):
        c = S.Context(d, n)
        c.set_particles(Xm)
        c.set_device_model(model)
        vd, ud, rd = c.ksd(None, K.scale(d), rows=True, kernel="imq")
        vh, uh, rh = c.ksd(model.log_model_grad(Xm), K.scale(d), rows=True, kernel="imq")
        c.close()
        print("ksd imq device_model %s V=%.6g relV=%.3g relU=%.3g" % (tag, vh, abs(vd - vh) / abs(vh),
                                                                     abs(ud - uh) / abs(uh)))
        assert vd == pytest.approx(vh, rel=1e-12)
        assert ud == pytest.approx(uh, rel=1e-12)
        np.testing.assert_allclose(rd, rh, rtol=0, atol=1e-12 * max(1.0, float(np.max(np.abs(rh)))))


@pytest.mark.parametrize("d", [8, 64])
def test_ksd_imq_f32_context_runs_fp64(oracle, d):
    n = 515
    X = oracle.splitmix((n, d), 3.0, 36 + d)
    G = K.model(d).log_model_grad(X)
    out = []
    for dtype in (C.SVGD_F64, C.SVGD_F32):
        c = S.Context(d, n, dtype=dtype)
        c.set_particles(X)
        out.append(c.ksd(G, K.scale(d), rows=True, kernel="imq"))
        c.close()
    (v0, u0, r0), (v1, u1, r1) = out
    print("ksd imq f32_ctx d=%d relV=%.3g relU=%.3g" % (d, abs(v1 - v0) / abs(v0), abs(u1 - u0) / abs(u0)))
    assert v1 == pytest.approx(v0, rel=1e-13)
    assert u1 == pytest.approx(u0, rel=1e-13)
    np.testing.assert_allclose(r1, r0, rtol=0, atol=1e-13 * float(np.max(np.abs(r0))))


@pytest.mark.parametrize("n,d", [(1000, 8), (515, 33)])
def test_ksd_imq_deterministic_and_blind_to_the_stepping_kernel(oracle, n, d):
    X = oracle.splitmix((n, d), 3.0, 37)
    G = K.model(d).log_model_grad(X)
    res = []
    for stepping in (None, "imq", "rbf"):
        c = S.Context(d, n)
        if stepping:
            c.set_kernel(stepping)
        c.set_particles(X)
        a = c.ksd(G, K.scale(d), rows=True, kernel="imq")
        b = c.ksd(G, K.scale(d), rows=True, kernel=C.SVGD_KERNEL_IMQ)
        assert c.kernel == (stepping or "rbf")  # the statistic does not set it either
        c.close()
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
        res.append(a)
    for r in res[1:]:
        assert r[0] == res[0][0] and r[1] == res[0][1] and np.array_equal(r[2], res[0][2])


def test_ksd_imq_default_scale_is_the_median_heuristic(oracle):
    n, d = 400, 4
    X = oracle.splitmix((n, d), 3.0, 38)
    G = K.model(d).log_model_grad(X)
    c = S.Context(d, n)
    c.set_particles(X)
    got = c.ksd(G, kernel="imq")
    exp = c.ksd(G, c.median_scale()[0], kernel="imq")
    c.close()
    assert got == exp
    ref = K.ksd_imq_ref(X, G, oracle.median_scale(X)[0])
    assert abs(float(LD(got[0]) - ref[0])) <= K.BAR * max(1.0, ref[3])


def _observed_run(oracle, stepping, with_ksd):
    n, d, steps = 12007, 5, 14
    X0 = oracle.splitmix((n, d), 3.0, 41)
    model = K.model(d, k=3)
    c = S.Context(d, n)
    c.set_kernel(stepping)
    c.set_particles(X0)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    c.set_bounds(-np.full(d, 2.5), np.full(d, 2.5))
    c.set_device_model(model)
    c.diagnostics()
    scales, ksds = [], []
    for _ in range(steps):
        c.step_with_model(model)
        scales.append(c.last_scale())
        if with_ksd:
            ksds.append(c.ksd(None, 0.4, kernel="imq"))
    X = c.get_particles()
    dg = c.diagnostics()
    c.close()
    return X, scales, dg, ksds


@pytest.mark.parametrize("stepping", ["rbf", "imq"])
def test_ksd_imq_is_a_pure_observer(oracle, stepping):
    """n = 12007, d = 5, 14 bounded Adam steps -- where the speculative steps
    and the tracked median brackets engage -- under either stepping kernel,
    with an IMQ KSD after every step and with none: the same particles,
    scales, paths and tracked steps."""
    Xa, sa, da, ksds = _observed_run(oracle, stepping, True)
    Xb, sb, db, _ = _observed_run(oracle, stepping, False)
    print("ksd imq observer (%s steps) trk_steps=%d/%d spec_steps=%d/%d KSD2_V first=%.6g last=%.6g"
          % (stepping, da["trk_steps"], db["trk_steps"], da["spec_steps"], db["spec_steps"], ksds[0][0],
             ksds[-1][0]))
    if stepping == "rbf":
        assert db["trk_steps"] >= 3  # the shape does engage the tracked path
    assert np.array_equal(Xa, Xb)
    assert sa == sb
    for key in ("steps", "trk_steps", "trk_miss", "spec_steps", "split_steps", "mirror_steps"):
        assert da[key] == db[key], key
    assert all(np.isfinite(k[0]) and k[0] >= 0.0 for k in ksds)


def test_svgd_compute_ksd_imq(oracle):
    """SVGD.ComputeKSD(kernel="imq") on the d = 2 MVN of tests/test_gpu_ksd.py:
    the reference's value at X0 with the median-heuristic scale, lower after
    60 Adam steps; ComputeKSD() on the same SVGD is still the RBF statistic.
    With an InverseMultiquadricKernel of constant scale, the kernel's own a."""
    n, d = 300, 2
    mu, cov = np.array([-0.6871, 0.8010]), 5 * np.array([[0.2260, 0.1652], [0.1652, 0.6779]])
    X0 = oracle.splitmix((n, d), 3.0, 5)
    coord = np.ascontiguousarray(X0.T).copy()
    model = S.MultivariateNormal(mu, cov)
    G0 = model.log_model_grad(X0)
    kern = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Median, model)
    sv = S.SVGD(d, 60, coord, kern, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    sv.Initialize()
    k0, k0u = sv.ComputeKSD(kernel="imq"), sv.ComputeKSD(unbiased=True, kernel="imq")
    a0 = oracle.median_scale(X0)[0]
    ref = K.ksd_imq_ref(X0, G0, a0)
    assert abs(float(LD(k0) - ref[0])) <= K.BAR * max(1.0, ref[3])
    assert abs(float(LD(k0u) - ref[1])) <= K.BAR * max(1.0, ref[3])
    rbf = K.ksd_rbf_ref(X0, G0, a0)
    assert sv.ComputeKSD() == sv.ComputeKSD(kernel="rbf")
    assert abs(float(LD(sv.ComputeKSD()) - rbf[0])) <= 1e-10 * max(1.0, rbf[3])
    sv.Run()
    k1 = sv.ComputeKSD(kernel="imq")
    print("ksd imq svgd_run KSD2_V %.6g -> %.6g" % (k0, k1))
    assert 0.0 <= k1 < k0
    with pytest.raises(ValueError):
        sv.ComputeKSD(kernel="laplace")
    # an IMQ SVGD with a constant scale: its own a for the IMQ statistic, the median's for the RBF one
    coord = np.ascontiguousarray(X0.T).copy()
    imq = S.InverseMultiquadricKernel(coord, S.InverseMultiquadricKernel.ScaleMethod.Constant, 0.37)
    sq = S.SVGD(d, 1, coord, imq, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    sq.Initialize()
    ref = K.ksd_imq_ref(X0, G0, 0.37)
    assert abs(float(LD(sq.ComputeKSD(kernel="imq")) - ref[0])) <= K.BAR * max(1.0, ref[3])
    assert abs(float(LD(sq.ComputeKSD(unbiased=True, kernel="imq")) - ref[1])) <= K.BAR * max(1.0, ref[3])
    assert abs(float(LD(sq.ComputeKSD()) - rbf[0])) <= 1e-10 * max(1.0, rbf[3])
    # the generic host-kernel path opens a context for the call
    k = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Constant)
    host = S.SVGD(d, 1, coord, k + k, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    assert not host.UsesDevicePath()
    ref = K.ksd_imq_ref(X0, G0, a0)
    assert abs(float(LD(host.ComputeKSD(kernel="imq")) - ref[0])) <= K.BAR * max(1.0, ref[3])


def test_ksd_imq_errors(oracle):
    n, d = 64, 3
    X = oracle.splitmix((n, d), 3.0, 39)
    G = np.zeros((n, d))
    c = S.Context(d, n)
    with pytest.raises(S.UnsetException):
        c.ksd(G, 1.0, kernel="imq")
    c.set_particles(X)
    for a in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
            c.ksd(G, a, kernel="imq")
    with pytest.raises(ValueError, match="no device model set"):
        c.ksd(None, 1.0, kernel="imq")
    for bad in ("laplace", 2, -1):
        with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
            c.ksd(G, 1.0, kernel=bad)
    assert c.lib.svgd_ksd_kernel(c.h, 7, C.dptr(G), 1.0, None, None, None) == C.SVGD_ERR_ARG
    # all outputs NULL is a valid call
    assert c.lib.svgd_ksd_kernel(c.h, C.SVGD_KERNEL_IMQ, C.dptr(G), 1.0, None, None, None) == C.SVGD_OK
    c.close()
    ns = 4096
    sim = S.Context(d, ns, sim_world=4)
    sim.set_particles(oracle.splitmix((ns, d), 3.0, 40))
    with pytest.raises(Exception, match="measurement context"):
        sim.ksd(np.zeros((sim.row1 - sim.row0, d)), 1.0, kernel="imq")
    sim.close()


# ------------------------------------------------ multi-rank on one GPU ------
def _run_ranks(world, n, d, with_ksd):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "svgd_" + uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=W.run, args=(r, world, name, n, d, with_ksd, q)) for r in range(world)]
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


@pytest.mark.parametrize("world,n", [(2, 3001), (3, 6007)])
def test_ksd_imq_sharded_matches_one_rank(oracle, world, n):
    """Ranks on one GPU over the host shared-memory collectives: after 2 steps
    every rank returns the same V and U, equal to one rank's on the same
    particles (1e-12 relative); the ranks' rows, concatenated, are one rank's
    at the bar; and a further step is bit-identical to a run that never
    called the KSD."""
    d = 5
    with_k = _run_ranks(world, n, d, True)
    without = _run_ranks(world, n, d, False)
    X2 = with_k[0]["X2"]
    model = W.model(d)
    G2 = model.log_model_grad(X2)
    one = S.Context(d, n)
    one.set_particles(X2)
    v1, u1, rows1 = one.ksd(G2, W.KSD_A, rows=True, kernel="imq")
    one.close()
    shards = sorted((with_k[r]["shard"], r) for r in range(world))
    rows = np.concatenate([with_k[r]["rows"] for _, r in shards])
    assert rows.shape == (n,)
    for r in range(world):
        res = with_k[r]
        assert np.array_equal(res["X2"], X2)
        assert (res["v"], res["u"]) == (with_k[0]["v"], with_k[0]["u"])
        assert res["v"] == pytest.approx(v1, rel=1e-12)
        assert res["u"] == pytest.approx(u1, rel=1e-12)
        assert np.array_equal(res["X3"], without[r]["X3"]), r
        assert res["scales"] == without[r]["scales"], r
    rabs = K.ksd_imq_ref(X2, G2, W.KSD_A)[4]
    err = float(np.max(np.abs(rows - rows1) / (K.BAR * np.maximum(1.0, rabs))))
    print("ksd imq sharded world=%d n=%d V=%.6g relV=%.3g relU=%.3g worst row err/bar=%.3g"
          % (world, n, v1, abs(with_k[0]["v"] - v1) / abs(v1), abs(with_k[0]["u"] - u1) / abs(u1), err))
    assert err <= 1.0
