"""Device MMD (svgd_mmd, Context.mmd, SVGD.ComputeMMD).

The reference is the definition in numpy longdouble (tests/_mmd.py) and the
host form svgd_mmd_host; the bar is 1e-12 absolute (|k| <= 1) on each of the
three means, MMD2_V, MMD2_U and every witness row.  Each test prints its
observed excess over the bar ("mmd ..." lines, shown with -s or -rA) before
it asserts.
"""
import multiprocessing as mp
import uuid

import numpy as np
import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

import _glm as R
import _gpu_mmd_rank_worker as W
import _ksd_imq as K
import _mmd as Q

pytestmark = pytest.mark.gpu

KERNELS = Q.KERNELS


def _device(X, Y, a, kernel, dtype=C.SVGD_F64):
    n, d = X.shape
    c = S.Context(d, n, dtype=dtype)
    c.set_particles(X)
    v, u, wit, m3 = c.mmd(Y, a, kernel=kernel, witness=True, means=True)
    c.close()
    return v, u, m3, wit


def _host(X, Y, a, kernel, witness=True):
    out, wit = np.empty(5), np.empty(X.shape[0]) if witness else None
    rc = C.lib().svgd_mmd_host(S.Context.KERNELS[kernel], X.shape[1], X.shape[0], C.dptr(X), Y.shape[0],
                               C.dptr(np.ascontiguousarray(Y)), a, C.dptr(out[0:]), C.dptr(out[1:]),
                               C.dptr(out[2:]), C.dptr(wit))
    assert rc == C.SVGD_OK
    return out[0], out[1], out[2:5].copy(), wit


def _against(ref, got):
    v, u, m3, wit = got
    return Q.errors(v, u, m3, wit, ref)


def _check(tag, X, Y, a, kernel, dtype=C.SVGD_F64):
    """Device against the longdouble definition and against the host form."""
    got = _device(X, Y, a, kernel, dtype)
    ref = Q.mmd_ref(X, Y, a, kernel)
    hv, hu, hm, hw = _host(X, Y, a, kernel)
    e = _against(ref, got)
    eh = _against((hm.astype(Q.LD), Q.LD(hv), Q.LD(hu), hw.astype(Q.LD)), got)
    print("mmd %s %s n=%d m=%d d=%d a=%.3g V=%.6g U=%.6g err/bar V %.3g U %.3g means %.3g witness %.3g; "
          "against the host form %.3g"
          % (tag, kernel, X.shape[0], Y.shape[0], X.shape[1], a, got[0], got[1], e[0], e[1], e[2], e[3], max(eh)))
    assert max(e) <= 1.0
    assert max(eh) <= 1.0
    return got, ref


SHAPES = ([(1, 1, 2), (2, 3, 1), (1, 65, 3), (65, 1, 3), (77, 1000, 3), (1000, 63, 8), (1000, 64, 8), (1000, 65, 8),
           (257, 129, 1)] + [(515, 333, d) for d in range(1, 65) if d % 4 in (0, 1)])


@pytest.mark.parametrize("n,m,d", SHAPES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_mmd_matches_definition(oracle, kernel, n, m, d):
    """Either set smaller than one tile, M at 63 / 64 / 65, and N = 515,
    M = 333: ragged against 128-row work-groups and 64-record tiles, at both
    ends of every KP.  U is NaN exactly when N < 2 or M < 2; V stays finite."""
    X, Y = Q.clouds(n, m, d, 900 + n + d)
    (v, u, m3, wit), _ = _check("shape", X, Y, Q.scale(n, d), kernel)
    assert np.isnan(u) == (n < 2 or m < 2)
    assert np.isfinite(v) and np.all(np.isfinite(m3)) and np.all(np.isfinite(wit))


@pytest.mark.parametrize("kernel", KERNELS)
def test_mmd_past_one_split_of_partials(oracle, kernel):
    """N = 70001, M = 4097, d = 2: 547 row groups against 1094 and 65 column
    tiles, and the row finish leaves 274 block partials: one more round than
    the final sum's 256 threads take at once.  Scalars and means only.
    The longdouble definition would take minutes here; the reference is
    svgd_mmd_host, whose own error is far below the bar: every k carries a
    few fp64 roundings (about (d + 4) 2^-53 relative, libm's exp and sqrt
    within one unit) and the means are averages of them, and its observed
    error against longdouble is at most 2e-3 bars on every case of
    tests/test_mmd_cpu.py."""
    n, m, d = 70001, 4097, 2
    X, Y = Q.clouds(n, m, d, 77)
    a = Q.scale(n, d)
    c = S.Context(d, n)
    c.set_particles(X)
    v, u, m3 = c.mmd(Y, a, kernel=kernel, means=True)
    c.close()
    hv, hu, hm, _ = _host(X, Y, a, kernel, witness=False)
    ev, eu, em = abs(v - hv) / Q.BAR, abs(u - hu) / Q.BAR, np.abs(m3 - hm).max() / Q.BAR
    print("mmd large %s V=%.9g U=%.9g err/bar V %.3g U %.3g means %.3g" % (kernel, v, u, ev, eu, em))
    assert max(ev, eu, em) <= 1.0


@pytest.mark.parametrize("d", Q.EDGE_DIMS)
@pytest.mark.parametrize("name", Q.EDGE)
@pytest.mark.parametrize("kernel", KERNELS)
def test_mmd_edge_inputs(oracle, kernel, name, d):
    """Both clouds shifted by +1e3 and +1e6, duplicates inside X and inside Y,
    two clusters, Y disjoint from X by 50 standard deviations, a = 1e6 and
    a = 1e-8 (the cancellation case: every k is about 1).  The fp64 emulation
    of the Gram order stays inside the bar on all of them
    (tests/test_mmd_cpu.py)."""
    X, Y, a = Q.edge(name, d)
    (v, u, m3, wit), _ = _check(name, X, Y, a, kernel)
    if name == "disjoint" and kernel == "rbf":
        assert 0.0 <= m3[2] <= Q.BAR
        assert abs(v - (m3[0] + m3[1])) <= Q.BAR
    if name == "a1e6" and kernel == "rbf":
        assert abs(m3[0] - 1.0 / X.shape[0]) <= Q.BAR and abs(m3[1] - 1.0 / Y.shape[0]) <= Q.BAR


@pytest.mark.parametrize("kernel", KERNELS)
def test_mmd_of_the_particles_against_themselves(oracle, kernel):
    """Y = X, the same array: |V| <= bar and every witness row within the bar
    of 0."""
    for n, d in ((515, 5), (300, 17)):
        X, _ = Q.clouds(n, 1, d, 31)
        v, u, m3, wit = _device(X, X, Q.scale(n, d), kernel)
        print("mmd self %s n=%d d=%d |V|/bar %.3g max|wit|/bar %.3g |mxx - myy|/bar %.3g"
              % (kernel, n, d, abs(v) / Q.BAR, np.abs(wit).max() / Q.BAR, abs(m3[0] - m3[1]) / Q.BAR))
        assert abs(v) <= Q.BAR and np.abs(wit).max() <= Q.BAR


@pytest.mark.parametrize("kernel", KERNELS)
def test_mmd_of_a_thinned_subset(oracle, kernel):
    """Y = X[idx] for a stein_thin result whose picks repeat (m > n / 2 on a
    small cloud): inside the bar against the definition."""
    n, d, m = 77, 3, 100
    X = oracle.splitmix((n, d), 3.0, 980)
    G = K.model(d).log_model_grad(X)
    c = S.Context(d, n)
    c.set_particles(X)
    idx = c.stein_thin(m, G, K.scale(d), kernel="imq")
    assert len(set(idx.tolist())) < m  # the picks do repeat
    Y = np.ascontiguousarray(X[idx])
    a = Q.scale(n, d)
    v, u, wit, m3 = c.mmd(Y, a, kernel=kernel, witness=True, means=True)
    c.close()
    e = Q.errors(v, u, m3, wit, Q.mmd_ref(X, Y, a, kernel))
    print("mmd thinned %s V=%.6g err/bar V %.3g U %.3g means %.3g witness %.3g" % ((kernel, v) + e))
    assert max(e) <= 1.0


@pytest.mark.parametrize("n,m,d", [(1000, 65, 8), (515, 333, 33)])
@pytest.mark.parametrize("kernel", KERNELS)
def test_mmd_determinism_and_growth(oracle, kernel, n, m, d):
    """Two calls give the same bits; an SVGD_F32 context gives the bits of an
    SVGD_F64 one; a larger M, then the first one again, on one context (the
    sample's arrays grow); either stepping kernel."""
    X, Y = Q.clouds(n, m, d, 900 + n + d)
    Ybig, _ = Q.clouds(3 * m + 70, 1, d, 12)
    a = Q.scale(n, d)
    v0, u0, m0, w0 = _device(X, Y, a, kernel)
    v1, u1, m1, w1 = _device(X, Y, a, kernel, dtype=C.SVGD_F32)
    assert (v0, u0) == (v1, u1) and np.array_equal(m0, m1) and np.array_equal(w0, w1)
    ref_big = Q.mmd_ref(X, Ybig, a, kernel)
    for stepping in KERNELS:
        c = S.Context(d, n)
        c.set_kernel(stepping)
        c.set_particles(X)
        ra = c.mmd(Y, a, kernel=kernel, witness=True, means=True)
        rb = c.mmd(Ybig, a, kernel=kernel, witness=True, means=True)
        rc = c.mmd(Y, a, kernel=S.Context.KERNELS[kernel], witness=True, means=True)
        assert c.kernel == stepping
        c.close()
        for r in (ra, rc):
            assert (r[0], r[1]) == (v0, u0) and np.array_equal(r[2], w0) and np.array_equal(r[3], m0)
        e = Q.errors(rb[0], rb[1], rb[3], rb[2], ref_big)
        print("mmd growth %s (%s steps) m %d -> %d err/bar V %.3g U %.3g means %.3g witness %.3g"
              % ((kernel, stepping, m, Ybig.shape[0]) + e))
        assert max(e) <= 1.0


def _observed_run(oracle, stepping, with_mmd):
    n, d, steps = 12007, 5, 14
    X0 = oracle.splitmix((n, d), 3.0, 41)
    Y = oracle.splitmix((333, d), 2.0, 43)
    model = K.model(d, k=3)
    c = S.Context(d, n)
    c.set_kernel(stepping)
    c.set_particles(X0)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    c.set_bounds(-np.full(d, 2.5), np.full(d, 2.5))
    c.set_device_model(model)
    c.diagnostics()
    scales, mmds = [], []
    for t in range(steps):
        c.step_with_model(model)
        scales.append(c.last_scale())
        if with_mmd:
            mmds.append(c.mmd(Y, 0.4, kernel=KERNELS[t % 2]))
    X = c.get_particles()
    dg = c.diagnostics()
    c.close()
    return X, scales, dg, mmds


@pytest.mark.parametrize("stepping", ["rbf", "imq"])
def test_mmd_is_a_pure_observer(oracle, stepping):
    """n = 12007, d = 5, 14 bounded Adam steps -- where the speculative steps
    and the tracked median brackets engage -- with an MMD after every step
    and with none: the same particles, scales, paths and tracked steps."""
    Xa, sa, da, mmds = _observed_run(oracle, stepping, True)
    Xb, sb, db, _ = _observed_run(oracle, stepping, False)
    print("mmd observer (%s steps) trk_steps=%d/%d spec_steps=%d/%d V first=%.6g last=%.6g"
          % (stepping, da["trk_steps"], db["trk_steps"], da["spec_steps"], db["spec_steps"], mmds[0][0], mmds[-1][0]))
    if stepping == "rbf":
        assert db["trk_steps"] >= 3  # the shape does engage the tracked path
    assert np.array_equal(Xa, Xb)
    assert sa == sb
    for key in ("steps", "trk_steps", "trk_miss", "spec_steps", "split_steps", "mirror_steps"):
        assert da[key] == db[key], key
    assert all(np.isfinite(v) and np.isfinite(u) and v >= -Q.BAR for v, u in mmds)


def test_mmd_between_the_other_observers(oracle):
    """ksd, stein_thin and glm_predict give the same bits with MMD calls
    between them as without."""
    n, d = 515, 8
    X = oracle.splitmix((n, d), 3.0, 35) / 3.0
    A, y, _ = R.case(d, 300, n, "logistic")
    G = K.model(d).log_model_grad(X)
    Y = oracle.splitmix((200, d), 1.0, 36)
    runs = []
    for with_mmd in (False, True):
        c = S.Context(d, n)
        c.set_particles(X)
        out = []
        for kernel in KERNELS:
            if with_mmd:
                c.mmd(Y, 0.3, kernel=kernel)
            out.append(c.ksd(G, 0.3, rows=True, kernel=kernel))
            if with_mmd:
                c.mmd(Y[:70], 0.3, kernel=kernel, witness=True)
            out.append(c.stein_thin(16, G, 0.3, kernel=kernel, trace=True))
            if with_mmd:
                c.mmd(Y, 0.3, kernel=kernel, means=True)
            out.append(c.glm_predict(A, y))
        c.close()
        runs.append(out)
    for r0, r1 in zip(*runs):
        assert len(r0) == len(r1)
        for x0, x1 in zip(r0, r1):
            assert np.array_equal(np.asarray(x0), np.asarray(x1))


def test_mmd_surface(oracle):
    """Context.mmd's default scale and return shapes; SVGD.ComputeMMD for a
    device-model run, a host-model run and the generic host-kernel path."""
    n, m, d = 300, 120, 2
    X0 = oracle.splitmix((n, d), 3.0, 5)
    Y = oracle.splitmix((m, d), 2.0, 6) + 0.3
    c = S.Context(d, n)
    c.set_particles(X0)
    a0 = c.median_scale()[0]
    got = c.mmd(Y)
    assert isinstance(got, tuple) and len(got) == 2
    assert got == c.mmd(Y, a0, kernel="rbf")
    r = c.mmd(Y, witness=True)
    assert len(r) == 3 and r[2].shape == (n,)
    r = c.mmd(Y, means=True)
    assert len(r) == 3 and r[2].shape == (3,)
    r = c.mmd(Y, kernel="imq", witness=True, means=True)
    assert len(r) == 4 and r[2].shape == (n,) and r[3].shape == (3,)
    c.close()
    # host model, RBF kernel with the median scale: a = ln N / med^2 for both statistics
    coord = np.ascontiguousarray(X0.T).copy()
    mu, cov = np.array([-0.6871, 0.8010]), 5 * np.array([[0.2260, 0.1652], [0.1652, 0.6779]])
    model = S.MultivariateNormal(mu, cov)
    kern = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Median, model)
    sv = S.SVGD(d, 5, coord, kern, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    sv.Initialize()
    Yc = np.ascontiguousarray(Y.T)
    for kernel in KERNELS:
        _, V, U, _ = Q.mmd_ref(X0, Y, a0, kernel)
        v, u = sv.ComputeMMD(Yc, kernel=kernel), sv.ComputeMMD(Yc, unbiased=True, kernel=kernel)
        print("mmd svgd host-model %s V=%.6g U=%.6g err/bar V %.3g U %.3g"
              % (kernel, v, u, abs(float(v - V)) / Q.BAR, abs(float(u - U)) / Q.BAR))
        assert abs(float(v - V)) <= Q.BAR and abs(float(u - U)) <= Q.BAR
    assert sv.ComputeMMD(Yc) == sv.ComputeMMD(Yc, kernel="rbf")
    with pytest.raises(ValueError):
        sv.ComputeMMD(Yc, kernel="laplace")
    with pytest.raises(S.DimensionMismatchException):
        sv.ComputeMMD(np.zeros((d + 1, m)))
    # an IMQ SVGD with a constant scale: its own a for the IMQ statistic
    imq = S.InverseMultiquadricKernel(coord, S.InverseMultiquadricKernel.ScaleMethod.Constant, 0.37)
    sq = S.SVGD(d, 1, coord, imq, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    sq.Initialize()
    assert abs(float(sq.ComputeMMD(Yc, kernel="imq") - Q.mmd_ref(X0, Y, 0.37, "imq")[1])) <= Q.BAR
    # the generic host-kernel path opens a context for the call
    k = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Constant)
    host = S.SVGD(d, 1, coord, k + k, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    assert not host.UsesDevicePath()
    assert abs(float(host.ComputeMMD(Yc) - Q.mmd_ref(X0, Y, a0, "rbf")[1])) <= Q.BAR
    # a device-model run: a GLM whose step runs wholly on the device
    dg = 4
    A, y, Xg = R.case(dg, 200, 256, "logistic")
    Xg = np.array(Xg)
    cg = np.ascontiguousarray(Xg.T).copy()
    glm = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
    kg = S.GaussianRBFKernel(cg, S.GaussianRBFKernel.ScaleMethod.Constant, glm, scale=0.37)
    sg = S.SVGD(dg, 3, cg, kg, glm, S.Adam(dg, 256, 0.05, 0.9, 0.999))
    sg.Initialize()
    assert sg.UsesDeviceModelStep()
    sg.Run()
    Yg = oracle.splitmix((90, dg), 1.0, 8)
    Xr = np.ascontiguousarray(cg.T)
    v = sg.ComputeMMD(np.ascontiguousarray(Yg.T))
    V = Q.mmd_ref(Xr, Yg, 0.37, "rbf")[1]
    print("mmd svgd device-model V=%.6g err/bar %.3g" % (v, abs(float(v - V)) / Q.BAR))
    assert abs(float(v - V)) <= Q.BAR


def test_mmd_errors(oracle):
    n, d = 64, 3
    X = oracle.splitmix((n, d), 3.0, 39)
    Y = oracle.splitmix((10, d), 3.0, 40)
    c = S.Context(d, n)
    with pytest.raises(S.UnsetException):
        c.mmd(Y, 1.0)
    c.set_particles(X)
    for a in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\] The MMD kernel scale"):
            c.mmd(Y, a)
    for bad in ("laplace", 2, -1):
        with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
            c.mmd(Y, 1.0, kernel=bad)
    for bad in (float("nan"), float("inf"), -float("inf")):
        Yb = Y.copy()
        Yb[9, 2] = bad
        with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\] The MMD sample holds a non-finite"):
            c.mmd(Yb, 1.0)
    with pytest.raises(S.DimensionMismatchException):
        c.mmd(np.zeros((10, d + 1)), 1.0)
    with pytest.raises(S.DimensionMismatchException, match=r"^SVGDCpp: \[Dimension Error\]"):
        c.mmd(np.zeros((0, d)), 1.0)
    lib, out = c.lib, np.full(2, -7.0)
    assert lib.svgd_mmd(c.h, 7, C.dptr(Y), 10, 1.0, C.dptr(out), None, None, None) == C.SVGD_ERR_ARG
    assert lib.svgd_last_error(c.h).decode().startswith("SVGDCpp: [Argument Error] Unknown MMD kernel")
    assert lib.svgd_mmd(c.h, C.SVGD_KERNEL_RBF, None, 10, 1.0, C.dptr(out), None, None, None) == C.SVGD_ERR_ARG
    assert lib.svgd_last_error(c.h).decode().startswith("SVGDCpp: [Argument Error] Null MMD sample")
    for m in (0, -2):
        assert lib.svgd_mmd(c.h, C.SVGD_KERNEL_IMQ, C.dptr(Y), m, 1.0, C.dptr(out), None, None, None) == C.SVGD_ERR_DIM
        assert lib.svgd_last_error(c.h).decode().startswith("SVGDCpp: [Dimension Error]")
    assert np.all(out == -7.0)  # nothing written by a refused call
    # every output NULL is a valid call
    assert lib.svgd_mmd(c.h, C.SVGD_KERNEL_IMQ, C.dptr(Y), 10, 1.0, None, None, None, None) == C.SVGD_OK
    c.close()
    ns = 4096
    sim = S.Context(d, ns, sim_world=4)
    sim.set_particles(oracle.splitmix((ns, d), 3.0, 40))
    with pytest.raises(Exception, match="measurement context"):
        sim.mmd(Y, 1.0)
    sim.close()


# ------------------------------------------------ multi-rank on one GPU ------
def _run_ranks(world, n, d, with_mmd):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "svgd_" + uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=W.run, args=(r, world, name, n, d, with_mmd, q)) for r in range(world)]
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


@pytest.mark.parametrize("n", [3001, 6007])
@pytest.mark.parametrize("world", [2, 3])
def test_mmd_sharded_matches_one_rank(oracle, world, n):
    """Ranks on one GPU over the host shared-memory collectives: after 2 steps
    every rank returns the same scalars and means bit for bit, within the bar
    of one rank's on the same particles; the witness shards concatenate to
    one rank's witness within the bar; a sample of world - 1 points leaves
    the last rank no rows of Y; and a further step is bit-identical to a run
    that never called it.  (The ranks' processes end before this one opens
    the GPU: at most world + 1 processes hold it at a time.)"""
    d = 5
    with_m = _run_ranks(world, n, d, True)
    without = _run_ranks(world, n, d, False)
    X2 = with_m[0]["X2"]
    Y = W.sample(d)
    one = S.Context(d, n)
    one.set_particles(X2)
    for kernel in W.KERNELS:
        for key, Yk in ((kernel, Y), (kernel + "_few", Y[:world - 1])):
            v1, u1, w1, m1 = one.mmd(Yk, W.MMD_A, kernel=kernel, witness=True, means=True)
            e1 = Q.errors(v1, u1, m1, w1, Q.mmd_ref(X2, Yk, W.MMD_A, kernel))
            wit = np.concatenate([with_m[r][key][2] for r in range(world)])
            v, u, _, m3 = with_m[0][key]
            es = (abs(v - v1) / Q.BAR, 0.0 if np.isnan(u) and np.isnan(u1) else abs(u - u1) / Q.BAR,
                  np.abs(m3 - m1).max() / Q.BAR, np.abs(wit - w1).max() / Q.BAR)
            print("mmd sharded world=%d n=%d %s m=%d one rank err/bar %.3g; ranks against it V %.3g U %.3g "
                  "means %.3g witness %.3g" % ((world, n, kernel, Yk.shape[0], max(e1)) + es))
            assert max(e1) <= 1.0 and max(es) <= 1.0
            assert np.isnan(u) == (Yk.shape[0] < 2)
            for r in range(world):
                vr, ur, wr, mr = with_m[r][key]
                assert vr == v and (ur == u or (np.isnan(ur) and np.isnan(u))) and np.array_equal(mr, m3), r
                assert wr.shape == (with_m[r]["shard"][1] - with_m[r]["shard"][0],)
    one.close()
    for r in range(world):
        res = with_m[r]
        assert np.array_equal(res["X2"], X2)
        assert np.array_equal(res["X3"], without[r]["X3"]), r
        assert res["scales"] == without[r]["scales"], r
