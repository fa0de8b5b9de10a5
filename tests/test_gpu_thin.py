"""Device Stein thinning (svgd_stein_thin, Context.stein_thin, SVGD.Thin).

The reference is the definition in numpy longdouble (tests/_thin.py), under
its two criteria:
 1. valid pick -- along the device's own prefix, at every t,
    obj_t[pi_t] <= min_j obj_t[j] + bar_t, bar_t = 1e-12 max(1, max_j (u_jj / 2
    + sum_{s<t} |u(pi_s, j)|)), and |ksd2_t - ref| <= 1e-12 max(1, mean |u| over
    the picked t x t block);
 2. the same picks as the definition and as svgd_stein_thin_host -- asserted
    where the reference alone first shows every runner-up >= 1e3 bars away.
Each test prints its observed figures ("thin ..." lines, shown with -s or
-rA) before it asserts.
"""
import ctypes
import multiprocessing as mp
import uuid

import numpy as np
import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

import _glm as R
import _gpu_thin_worker as W
import _ksd_imq as K
import _thin as T

pytestmark = pytest.mark.gpu

LD = K.LD
KERNELS = ("imq", "rbf")
I64P = ctypes.POINTER(ctypes.c_int64)


def _device(X, G, a, kernel, m, dtype=C.SVGD_F64):
    n, d = X.shape
    c = S.Context(d, n, dtype=dtype)
    c.set_particles(X)
    idx, ksd2 = c.stein_thin(m, G, a, kernel=kernel, trace=True)
    c.close()
    return idx, ksd2


def _host(X, G, a, kernel, m):
    idx, ksd2 = np.empty(m, np.int64), np.empty(m)
    rc = C.lib().svgd_stein_thin_host(S.Context.KERNELS[kernel], X.shape[1], X.shape[0], C.dptr(X), C.dptr(G), a,
                                      m, idx.ctypes.data_as(I64P), C.dptr(ksd2))
    assert rc == C.SVGD_OK
    return idx, ksd2


def _criteria(tag, X, G, a, kernel, m, same_picks=True, dtype=C.SVGD_F64):
    """Criterion 1 always; criterion 2 (after its precondition) when same_picks."""
    idx, ksd2 = _device(X, G, a, kernel, m, dtype)
    eo, ek = T.check_valid(X, G, a, kernel, idx, ksd2)
    line = "thin %s %s n=%d d=%d m=%d a=%.3g ksd2_1=%.6g ksd2_m=%.6g obj excess/bar %.3g ksd2 err/bar %.3g" % (
        tag, kernel, X.shape[0], X.shape[1], m, a, ksd2[0], ksd2[-1], eo, ek)
    if same_picks:
        ref = T.replay(X, G, a, kernel, m, keep_obj=False)
        gap = T.gap_bars(ref)
        line += " min gap/bar %.3g" % gap
    print(line)
    assert np.all(np.isfinite(ksd2))
    assert eo <= 1.0 and ek <= 1.0
    if same_picks:
        assert gap >= T.GAP_BARS  # from the reference alone
        assert np.array_equal(idx, ref["idx"])
        assert np.array_equal(idx, _host(X, G, a, kernel, m)[0])
    return idx, ksd2


SHAPES = ([(1, 3, 4), (2, 1, 5), (77, 3, 100), (257, 1, 40), (1000, 8, 64)] +
          [(515, d, 32) for d in (1, 4, 5, 16, 17, 33, 63, 64)])


@pytest.mark.parametrize("n,d,m", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_thin_matches_definition(oracle, kernel, n, d, m):
    """m > n (forced repeats) at the small sizes; n = 515 is ragged against
    any 64- or 256-wide work-group and its padding, at both ends of the
    coordinate loop's unrolling."""
    X, G, a = T.case(oracle, n, d, 900 + n + d)
    idx, ksd2 = _criteria("shape", X, G, a, kernel, m)
    diag = (G.astype(LD) ** 2).sum(1) + LD(a) * d * (1 if kernel == "imq" else 2)
    # t = 1: pi_1 = argmin u_jj and ksd2_1 = u_{pi_1 pi_1}
    assert idx[0] == int(np.argmin(diag))
    assert abs(float(LD(ksd2[0]) - diag[idx[0]])) <= T.BAR * max(1.0, float(diag[idx[0]]))
    if n == 1:
        assert np.all(idx == 0)
        assert np.all(np.abs((ksd2.astype(LD) - diag[0]).astype(np.float64)) <= T.BAR * max(1.0, float(diag[0])))


@pytest.mark.parametrize("kernel", KERNELS)
def test_thin_past_one_wave_of_partials(oracle, kernel):
    """n = 70001: 274 work-groups of 256, so the cross-work-group reduce reads
    more partials than one pass of its 256 threads.  Criterion 1 (the replay
    stays cheap at m = 8)."""
    X, G, a = T.case(oracle, 70001, 2, 77)
    _criteria("two_boundaries", X, G, a, kernel, 8, same_picks=False)


@pytest.mark.parametrize("kernel", KERNELS)
def test_thin_tie_goes_to_the_lowest_index(oracle, kernel):
    X, G, a = T.case(oracle, 300, 3, 17)
    G = G.copy()
    G[[3, 7]] = 0.0
    idx, ksd2 = _device(X, G, a, kernel, 1)
    assert idx.tolist() == [3]


@pytest.mark.parametrize("name", K.EDGE)
@pytest.mark.parametrize("kernel", KERNELS)
def test_thin_edge_clouds(kernel, name):
    """Shifted by +1e3 and +1e6, three outliers at 1e4, two duplicate pairs
    (which may tie to the last bit: criterion 1 only, as on all of these),
    anisotropic, a = 1e6 and 1e-8, two clusters."""
    X, G, a, _ = K.edge_case(name)
    _criteria(name, np.array(X), np.array(G), a, kernel, 32, same_picks=False)


@pytest.mark.parametrize("kernel", KERNELS)
def test_thin_ksd_of_the_picks_is_the_statistic(oracle, kernel):
    """ksd2_m is Context.ksd's V of a fresh context that holds the picked rows
    (with repeats) and their scores."""
    for n, d, m in ((77, 3, 100), (1000, 8, 64)):
        X, G, a = T.case(oracle, n, d, 900 + n + d)
        idx, ksd2 = _device(X, G, a, kernel, m)
        Xp, Gp = np.ascontiguousarray(X[idx]), np.ascontiguousarray(G[idx])
        c = S.Context(d, m)
        c.set_particles(Xp)
        v, _ = c.ksd(Gp, a, kernel=kernel)
        c.close()
        mabs = (K.ksd_imq_ref if kernel == "imq" else K.ksd_rbf_ref)(Xp, Gp, a)[3]
        print("thin statistic %s n=%d m=%d ksd2_m=%.15g V=%.15g err/bar %.3g"
              % (kernel, n, m, ksd2[-1], v, abs(ksd2[-1] - v) / (T.BAR * max(1.0, mabs))))
        assert abs(ksd2[-1] - v) <= T.BAR * max(1.0, mabs)


def test_thin_device_models(oracle):
    """G_shard = None evaluates the device model -- the Gaussian-sum mirror
    and a device GLM: the picks of the host gradient of the same model."""
    n, d, m = 515, 8, 32
    X = oracle.splitmix((n, d), 3.0, 35)
    A, y, _ = R.case(d, 300, n, "logistic")
    for tag, model, Xm in (("gauss", K.model(d, k=4), X),
                           ("glm", S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0), X / 3.0)):
        Gh = model.log_model_grad(Xm)
        for kernel in KERNELS:
            gap = T.gap_bars(T.replay(Xm, Gh, K.scale(d), kernel, m, keep_obj=False))
            assert gap >= T.GAP_BARS
            c = S.Context(d, n)
            c.set_particles(Xm)
            c.set_device_model(model)
            id_d, k_d = c.stein_thin(m, None, K.scale(d), kernel=kernel, trace=True)
            id_h, k_h = c.stein_thin(m, Gh, K.scale(d), kernel=kernel, trace=True)
            c.close()
            print("thin device_model %s %s ksd2_m=%.6g rel %.3g min gap/bar %.3g"
                  % (tag, kernel, k_h[-1], abs(k_d[-1] - k_h[-1]) / abs(k_h[-1]), gap))
            assert np.array_equal(id_d, id_h)
            np.testing.assert_allclose(k_d, k_h, rtol=1e-12, atol=0)


@pytest.mark.parametrize("n,d,m", [(1000, 8, 64), (515, 33, 32)])
@pytest.mark.parametrize("kernel", KERNELS)
def test_thin_context_variations(oracle, kernel, n, d, m):
    """An SVGD_F32 context (the selection is fp64 whatever the dtype), two
    calls on one state, and either stepping kernel: the same selection."""
    X, G, a = T.case(oracle, n, d, 900 + n + d)
    i0, k0 = _device(X, G, a, kernel, m)
    i1, k1 = _device(X, G, a, kernel, m, dtype=C.SVGD_F32)
    assert np.array_equal(i0, i1)
    np.testing.assert_allclose(k1, k0, rtol=1e-13, atol=0)
    for stepping in ("imq", "rbf"):
        c = S.Context(d, n)
        c.set_kernel(stepping)
        c.set_particles(X)
        ia, ka = c.stein_thin(m, G, a, kernel=kernel, trace=True)
        ib, kb = c.stein_thin(m + 9, G, a, kernel=kernel, trace=True)  # (the pick arrays grow)
        ic, kc = c.stein_thin(m, G, a, kernel=S.Context.KERNELS[kernel], trace=True)
        assert c.kernel == stepping
        c.close()
        assert np.array_equal(ia, i0) and np.array_equal(ka, k0)
        assert np.array_equal(ib[:m], i0) and np.array_equal(kb[:m], k0)
        assert np.array_equal(ic, i0) and np.array_equal(kc, k0)


def test_thin_default_scale_and_plain_return(oracle):
    X, G, a = T.case(oracle, 400, 4, 38)
    c = S.Context(4, 400)
    c.set_particles(X)
    got = c.stein_thin(10, G)
    exp, _ = c.stein_thin(10, G, c.median_scale()[0], kernel="imq", trace=True)
    c.close()
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, exp)


def _observed_run(oracle, stepping, with_thin):
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
    scales, thins = [], []
    for _ in range(steps):
        c.step_with_model(model)
        scales.append(c.last_scale())
        if with_thin:
            thins.append(c.stein_thin(16, None, 0.4, kernel="imq", trace=True))
    X = c.get_particles()
    dg = c.diagnostics()
    c.close()
    return X, scales, dg, thins


@pytest.mark.parametrize("stepping", ["rbf", "imq"])
def test_thin_is_a_pure_observer(oracle, stepping):
    """n = 12007, d = 5, 14 bounded Adam steps -- where the speculative steps
    and the tracked median brackets engage -- with a stein_thin(16) after every
    step and with none: the same particles, scales, paths and tracked steps."""
    Xa, sa, da, thins = _observed_run(oracle, stepping, True)
    Xb, sb, db, _ = _observed_run(oracle, stepping, False)
    print("thin observer (%s steps) trk_steps=%d/%d spec_steps=%d/%d ksd2_16 first=%.6g last=%.6g"
          % (stepping, da["trk_steps"], db["trk_steps"], da["spec_steps"], db["spec_steps"], thins[0][1][-1],
             thins[-1][1][-1]))
    if stepping == "rbf":
        assert db["trk_steps"] >= 3  # the shape does engage the tracked path
    assert np.array_equal(Xa, Xb)
    assert sa == sb
    for key in ("steps", "trk_steps", "trk_miss", "spec_steps", "split_steps", "mirror_steps"):
        assert da[key] == db[key], key
    assert all(np.all(np.isfinite(k)) and np.all(k >= 0.0) and np.all((i >= 0) & (i < 12007)) for i, k in thins)


def test_svgd_thin(oracle):
    """SVGD.Thin on the d = 2 MVN of tests/test_gpu_ksd.py: the points are the
    coordinate matrix's columns at idx, and ksd2 does not rise over the m = 12
    picks (the greedy sequence is not monotone in general: the reference's own
    first rise on this case is at t = 16 (RBF) and t = 18 (IMQ))."""
    n, d, m = 300, 2, 12
    mu, cov = np.array([-0.6871, 0.8010]), 5 * np.array([[0.2260, 0.1652], [0.1652, 0.6779]])
    X0 = oracle.splitmix((n, d), 3.0, 5)
    coord = np.ascontiguousarray(X0.T).copy()
    model = S.MultivariateNormal(mu, cov)
    G0 = model.log_model_grad(X0)
    a0 = oracle.median_scale(X0)[0]
    kern = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Median, model)
    sv = S.SVGD(d, 5, coord, kern, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    sv.Initialize()
    for kernel in KERNELS:
        ref = T.replay(X0, G0, a0, kernel, m, keep_obj=False)
        assert np.all(np.diff(ref["ksd2"].astype(np.float64)) <= 0.0)  # on the reference first
        assert T.gap_bars(ref) >= T.GAP_BARS
        pts, idx, ksd2 = sv.Thin(m, kernel=kernel)
        assert pts.shape == (d, m) and idx.shape == (m,) and ksd2.shape == (m,)
        assert np.array_equal(pts, coord[:, idx])
        assert np.array_equal(idx, ref["idx"])
        eo, ek = T.check_valid(X0, G0, a0, kernel, idx, ksd2)
        print("thin svgd %s ksd2 %.6g -> %.6g obj excess/bar %.3g ksd2 err/bar %.3g" % (kernel, ksd2[0], ksd2[-1], eo, ek))
        assert eo <= 1.0 and ek <= 1.0
        assert np.all(np.diff(ksd2) <= 0.0)
    assert np.array_equal(sv.Thin(m)[1], sv.Thin(m, kernel="imq")[1])
    with pytest.raises(ValueError):
        sv.Thin(m, kernel="laplace")
    with pytest.raises(ValueError):
        sv.Thin(0)
    # an IMQ SVGD with a constant scale: its own a for the IMQ selection
    imq = S.InverseMultiquadricKernel(coord, S.InverseMultiquadricKernel.ScaleMethod.Constant, 0.37)
    sq = S.SVGD(d, 1, coord, imq, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    sq.Initialize()
    ref = T.replay(X0, G0, 0.37, "imq", m, keep_obj=False)
    assert T.gap_bars(ref) >= T.GAP_BARS
    assert np.array_equal(sq.Thin(m)[1], ref["idx"])
    # the generic host-kernel path opens a context for the call
    k = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Constant)
    host = S.SVGD(d, 1, coord, k + k, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    assert not host.UsesDevicePath()
    ref = T.replay(X0, G0, a0, "imq", m, keep_obj=False)
    assert np.array_equal(host.Thin(m)[1], ref["idx"])


def test_thin_errors(oracle):
    n, d = 64, 3
    X = oracle.splitmix((n, d), 3.0, 39)
    G = np.zeros((n, d))
    c = S.Context(d, n)
    with pytest.raises(S.UnsetException):
        c.stein_thin(4, G, 1.0)
    c.set_particles(X)
    for a in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
            c.stein_thin(4, G, a)
    with pytest.raises(ValueError, match="no device model set"):
        c.stein_thin(4, None, 1.0)
    for bad in ("laplace", 2, -1):
        with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
            c.stein_thin(4, G, 1.0, kernel=bad)
    for m in (0, -2):
        with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
            c.stein_thin(m, G, 1.0)
        assert c.lib.svgd_stein_thin(c.h, C.SVGD_KERNEL_IMQ, C.dptr(G), 1.0, m, None, None) == C.SVGD_ERR_ARG
    assert c.lib.svgd_stein_thin(c.h, 7, C.dptr(G), 1.0, 4, None, None) == C.SVGD_ERR_ARG
    # both outputs NULL is a valid call
    assert c.lib.svgd_stein_thin(c.h, C.SVGD_KERNEL_IMQ, C.dptr(G), 1.0, 4, None, None) == C.SVGD_OK
    with pytest.raises(S.DimensionMismatchException):
        c.stein_thin(4, np.zeros((n + 1, d)), 1.0)
    c.close()
    ns = 4096
    sim = S.Context(d, ns, sim_world=4)
    sim.set_particles(oracle.splitmix((ns, d), 3.0, 40))
    with pytest.raises(Exception, match="measurement context"):
        sim.stein_thin(4, np.zeros((sim.row1 - sim.row0, d)), 1.0)
    sim.close()


# ------------------------------------------------ multi-rank on one GPU ------
def _run_ranks(world, n, d, with_thin):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "svgd_" + uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=W.run, args=(r, world, name, n, d, with_thin, q)) for r in range(world)]
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
def test_thin_sharded_matches_one_rank(oracle, world, n):
    """Ranks on one GPU over the host shared-memory collectives: after 2 steps
    every rank returns one rank's indices and ksd2 on the same particles bit
    for bit, and a further step is bit-identical to a run that never thinned.
    (The ranks' processes end before this one opens the GPU: at most
    world + 1 processes hold it at a time.)"""
    d = 5
    with_t = _run_ranks(world, n, d, True)
    without = _run_ranks(world, n, d, False)
    X2 = with_t[0]["X2"]
    G2 = W.model(d).log_model_grad(X2)
    one = S.Context(d, n)
    one.set_particles(X2)
    idx1, ksd1 = one.stein_thin(W.M, G2, W.KSD_A, kernel="imq", trace=True)
    one.close()
    eo, ek = T.check_valid(X2, G2, W.KSD_A, "imq", idx1, ksd1)
    print("thin sharded world=%d n=%d ksd2_m=%.6g obj excess/bar %.3g ksd2 err/bar %.3g"
          % (world, n, ksd1[-1], eo, ek))
    assert eo <= 1.0 and ek <= 1.0
    for r in range(world):
        res = with_t[r]
        assert np.array_equal(res["X2"], X2)
        assert np.array_equal(res["idx"], idx1), r
        assert np.array_equal(res["ksd2"], ksd1), r
        assert np.array_equal(res["X3"], without[r]["X3"]), r
        assert res["scales"] == without[r]["scales"], r
