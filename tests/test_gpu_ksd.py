"""Device kernelized Stein discrepancy (svgd_ksd, Context.ksd, SVGD.ComputeKSD).

For particles x_i, scores s_i = grad log p(x_i), k = exp(-a |r|^2), r = x_i - x_j:

    u_ij   = k_ij [ s_i.s_j + 2a (s_i - s_j).r + 2ad - 4a^2 |r|^2 ]
    row_i  = (1/N) sum_j u_ij
    KSD2_V = (1/N) sum_i row_i,   KSD2_U = (1/(N(N-1))) sum_{i != j} u_ij

The reference is this direct formula in numpy longdouble, in row chunks.  Bar:
|device - reference| <= 1e-10 max(1, mean|u_ij|) for V, U and every row_i (a
row's bar takes the mean over that row) -- the project's fp64 phi bar
(tests/test_gpu_parity.py).  Each test prints its observed error ("ksd ..."
lines, shown with -s or -rA) before it asserts.
"""
import multiprocessing as mp
import uuid

import numpy as np
import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

import _gpu_ksd_worker as W

pytestmark = pytest.mark.gpu

BAR = 1e-10
LD = np.longdouble


def ksd_ref(X, G, a):
    """(V, U, rows, mean|u|, per-row mean|u|, min off-diagonal a |r|^2) in longdouble."""
    n, d = X.shape
    Xl, Gl, al = X.astype(LD), G.astype(LD), LD(a)
    rows, rabs = np.empty(n, LD), np.empty(n, LD)
    diag = (Gl * Gl).sum(1) + 2 * al * d
    chunk = max(1, int(2e6) // (n * d))
    min_arg = np.inf
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        r = Xl[i0:i1, None, :] - Xl[None, :, :]
        r2 = (r * r).sum(-1)
        ss = Gl[i0:i1] @ Gl.T
        dsr = ((Gl[i0:i1, None, :] - Gl[None, :, :]) * r).sum(-1)
        u = np.exp(-al * r2) * (ss + 2 * al * dsr + 2 * al * d - 4 * al * al * r2)
        rows[i0:i1] = u.sum(1) / n
        rabs[i0:i1] = np.abs(u).sum(1) / n
        off = (al * r2).astype(np.float64)
        off[np.arange(i1 - i0), np.arange(i0, i1)] = np.inf
        min_arg = min(min_arg, float(off.min()))
    V = rows.sum() / n
    U = (rows.sum() * n - diag.sum()) / (LD(n) * (n - 1)) if n > 1 else LD(np.nan)
    return V, U, rows, float(rabs.mean()), rabs.astype(np.float64), min_arg


def _model(oracle, d, k=2, seed=7):
    mus = oracle.splitmix((k, d), 3.0, seed + d)
    covs = [np.eye(d) * (1.0 + 0.25 * c) for c in range(k)]
    return S.GaussianSum(list(mus), covs)


def _scale(d):
    """X has scale 3 (variance 3 per coordinate): a typical pair lies at
    |r|^2 = 6 d, where this a gives k = e^-1.5 -- every column matters."""
    return 1.0 / (4.0 * d)


def _check(tag, X, G, a, dtype=C.SVGD_F64):
    n, d = X.shape
    c = S.Context(d, n, dtype=dtype)
    c.set_particles(X)
    v, u, rows = c.ksd(G, a, rows=True)
    c.close()
    V, U, R, mabs, rabs, _ = ksd_ref(X, G, a)
    bar = BAR * max(1.0, mabs)
    ev = abs(float(LD(v) - V))
    eu = abs(float(LD(u) - U)) if n > 1 else 0.0
    rel_rows = np.abs((rows.astype(LD) - R).astype(np.float64)) / (BAR * np.maximum(1.0, rabs))
    print("ksd %s n=%d d=%d a=%.3g V=%.6g U=%.6g errV=%.3g errU=%.3g bar=%.3g worst row err/bar=%.3g"
          % (tag, n, d, a, v, u, ev, eu, bar, float(rel_rows.max())))
    assert np.isfinite(v) and np.all(np.isfinite(rows))
    assert ev <= bar
    if n > 1:
        assert eu <= bar
    else:
        assert np.isnan(u)
    assert float(rel_rows.max()) <= 1.0
    return v, u, rows


SHAPES = ([(1, 3), (2, 1), (77, 3), (257, 1), (256, 2), (1000, 8)] + [(515, d) for d in range(1, 17)] +
          [(515, d) for d in (17, 24, 32, 33, 48, 64)])


@pytest.mark.parametrize("n,d", SHAPES)
def test_ksd_matches_direct_formula(oracle, n, d):
    """Every per-dimension instantiation of the d <= 16 kernel and the tile
    kernel's coordinate classes (32, 48, 64), at sizes that are ragged against
    the row blocks (256 R rows / 64-row tiles), the 64-column chunks and the
    column splits; n = 1 and 2 are the degenerate ends."""
    X = oracle.splitmix((n, d), 3.0, 900 + n + d)
    G = _model(oracle, d).log_model_grad(X)
    a = _scale(d)
    v, u, _ = _check("shape", X, G, a)
    assert v >= 0.0
    if n == 1:
        assert v == pytest.approx(float(G[0] @ G[0]) + 2 * a * d, rel=1e-14)


def test_ksd_shifted_cloud(oracle):
    """A cloud at +1000: the pass works on centred coordinates."""
    n, d = 300, 3
    X0 = oracle.splitmix((n, d), 3.0, 31)
    G = _model(oracle, d).log_model_grad(X0)
    _check("shifted", X0 + 1000.0, G, _scale(d))


def test_ksd_far_outliers(oracle):
    """Three particles 1e4 away from the cloud and from each other: every k
    that involves one underflows, the result is finite and matches."""
    n, d = 300, 3
    X = oracle.splitmix((n, d), 3.0, 32)
    X[0] += 1.0e4
    X[1] -= 1.0e4
    X[2] += np.array([1.0e4, -1.0e4, 0.0])
    G = _model(oracle, d).log_model_grad(X)
    _check("outliers", X, G, _scale(d))


def test_ksd_duplicates(oracle):
    n, d = 300, 3
    X = oracle.splitmix((n, d), 3.0, 33)
    X[5], X[9] = X[4], X[8]
    G = _model(oracle, d).log_model_grad(X)
    _check("duplicates", X, G, _scale(d))


def test_ksd_large_scale_leaves_the_diagonal(oracle):
    """a so large that every off-diagonal k is exactly 0 (a |r|^2 > 745 for
    every pair, checked on the reference's distances): V is the mean of
    u_ii = |s_i|^2 + 2ad over N^2."""
    n, d = 300, 3
    X = oracle.splitmix((n, d), 3.0, 34)
    G = _model(oracle, d).log_model_grad(X)
    a = 1.0e6
    assert ksd_ref(X, G, a)[5] > 800.0
    c = S.Context(d, n)
    c.set_particles(X)
    v, u, rows = c.ksd(G, a, rows=True)
    c.close()
    diag = (G.astype(LD) ** 2).sum(1) + 2 * LD(a) * d
    exp = float(diag.sum() / (LD(n) * n))
    print("ksd large_a V=%.17g expected=%.17g rel=%.3g U=%.3g" % (v, exp, abs(v - exp) / exp, u))
    assert abs(v - exp) <= 1e-13 * exp
    np.testing.assert_allclose(rows, (diag / n).astype(np.float64), rtol=1e-13)
    assert abs(u) <= 1e-13 * exp * n  # (N SR - SD) cancels to rounding of the two sums


def test_ksd_device_model(oracle):
    """G_shard = None evaluates the device model: the same result as the host
    gradient of the same model."""
    n, d = 515, 8
    X = oracle.splitmix((n, d), 3.0, 35)
    model = _model(oracle, d, k=4)
    c = S.Context(d, n)
    c.set_particles(X)
    c.set_device_model(model)
    vd, ud, rd = c.ksd(None, _scale(d), rows=True)
    vh, uh, rh = c.ksd(model.log_model_grad(X), _scale(d), rows=True)
    c.close()
    print("ksd device_model relV=%.3g relU=%.3g" % (abs(vd - vh) / abs(vh), abs(ud - uh) / abs(uh)))
    assert vd == pytest.approx(vh, rel=1e-12)
    assert ud == pytest.approx(uh, rel=1e-12)
    np.testing.assert_allclose(rd, rh, rtol=0, atol=1e-12 * max(1.0, float(np.max(np.abs(rh)))))


@pytest.mark.parametrize("d", [8, 64])
def test_ksd_f32_context_runs_fp64(oracle, d):
    n = 515
    X = oracle.splitmix((n, d), 3.0, 36 + d)
    G = _model(oracle, d).log_model_grad(X)
    out = []
    for dtype in (C.SVGD_F64, C.SVGD_F32):
        c = S.Context(d, n, dtype=dtype)
        c.set_particles(X)
        out.append(c.ksd(G, _scale(d), rows=True))
        c.close()
    (v0, u0, r0), (v1, u1, r1) = out
    print("ksd f32_ctx d=%d relV=%.3g relU=%.3g" % (d, abs(v1 - v0) / abs(v0), abs(u1 - u0) / abs(u0)))
    assert v1 == pytest.approx(v0, rel=1e-13)
    assert u1 == pytest.approx(u0, rel=1e-13)
    np.testing.assert_allclose(r1, r0, rtol=0, atol=1e-13 * float(np.max(np.abs(r0))))


@pytest.mark.parametrize("n,d", [(1000, 8), (515, 33)])
def test_ksd_deterministic(oracle, n, d):
    X = oracle.splitmix((n, d), 3.0, 37)
    G = _model(oracle, d).log_model_grad(X)
    c = S.Context(d, n)
    c.set_particles(X)
    a = c.ksd(G, _scale(d), rows=True)
    b = c.ksd(G, _scale(d), rows=True)
    c.close()
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_ksd_default_scale_is_the_median_heuristic(oracle):
    n, d = 400, 4
    X = oracle.splitmix((n, d), 3.0, 38)
    G = _model(oracle, d).log_model_grad(X)
    c = S.Context(d, n)
    c.set_particles(X)
    got = c.ksd(G)
    exp = c.ksd(G, c.median_scale()[0])
    c.close()
    assert got == exp
    V = ksd_ref(X, G, oracle.median_scale(X)[0])
    assert abs(float(LD(got[0]) - V[0])) <= BAR * max(1.0, V[3])


def _observed_run(oracle, with_ksd):
    n, d, steps = 12007, 5, 14
    X0 = oracle.splitmix((n, d), 3.0, 41)
    model = _model(oracle, d, k=3)
    c = S.Context(d, n)
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
            ksds.append(c.ksd(None, 0.4))
    X = c.get_particles()
    dg = c.diagnostics()
    c.close()
    return X, scales, dg, ksds


def test_ksd_is_a_pure_observer(oracle):
    """n = 12007, d = 5, 14 bounded Adam steps -- where the speculative steps
    and the tracked median brackets engage -- with a KSD after every step and
    with none: the same particles, scales, paths and tracked steps."""
    Xa, sa, da, ksds = _observed_run(oracle, True)
    Xb, sb, db, _ = _observed_run(oracle, False)
    print("ksd observer trk_steps=%d/%d spec_steps=%d/%d KSD2_V first=%.6g last=%.6g"
          % (da["trk_steps"], db["trk_steps"], da["spec_steps"], db["spec_steps"], ksds[0][0], ksds[-1][0]))
    assert db["trk_steps"] >= 3  # the shape does engage the tracked path
    assert np.array_equal(Xa, Xb)
    assert sa == sb
    for key in ("steps", "trk_steps", "trk_miss", "spec_steps", "split_steps", "mirror_steps"):
        assert da[key] == db[key], key
    assert all(np.isfinite(k[0]) and k[0] >= 0.0 for k in ksds)


def test_svgd_compute_ksd_falls_along_a_run(oracle):
    """KSD2_V of a d = 2 MVN target after 60 Adam steps from X0 = 3 uniform is
    below its value at X0, as SVGD.ComputeKSD reports it; the value at X0 is
    the reference's with the median-heuristic scale."""
    n, d = 300, 2
    mu, cov = np.array([-0.6871, 0.8010]), 5 * np.array([[0.2260, 0.1652], [0.1652, 0.6779]])
    X0 = oracle.splitmix((n, d), 3.0, 5)
    coord = np.ascontiguousarray(X0.T).copy()
    model = S.MultivariateNormal(mu, cov)
    kern = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Median, model)
    sv = S.SVGD(d, 60, coord, kern, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    sv.Initialize()
    k0, k0u = sv.ComputeKSD(), sv.ComputeKSD(unbiased=True)
    V = ksd_ref(X0, model.log_model_grad(X0), oracle.median_scale(X0)[0])
    assert abs(float(LD(k0) - V[0])) <= BAR * max(1.0, V[3])
    assert abs(float(LD(k0u) - V[1])) <= BAR * max(1.0, V[3])
    sv.Run()
    k1 = sv.ComputeKSD()
    print("ksd svgd_run KSD2_V %.6g -> %.6g" % (k0, k1))
    assert 0.0 <= k1 < k0


def test_svgd_compute_ksd_constant_scale_and_host_path(oracle):
    """ScaleMethod.Constant passes the kernel's own a; a generic (composed)
    kernel has no context and opens one for the call, with the median scale."""
    n, d = 200, 2
    X0 = oracle.splitmix((n, d), 2.0, 6)
    coord = np.ascontiguousarray(X0.T).copy()
    model = S.MultivariateNormal([0.5, -0.25], [[1.0, 0.2], [0.2, 0.7]])
    G = model.log_model_grad(X0)
    kern = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Constant, scale=0.37)
    sv = S.SVGD(d, 1, coord, kern, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    sv.Initialize()
    V = ksd_ref(X0, G, 0.37)
    assert abs(float(LD(sv.ComputeKSD()) - V[0])) <= BAR * max(1.0, V[3])
    assert abs(float(LD(sv.ComputeKSD(unbiased=True)) - V[1])) <= BAR * max(1.0, V[3])
    rbf = S.GaussianRBFKernel(coord, S.GaussianRBFKernel.ScaleMethod.Constant)
    host = S.SVGD(d, 1, coord, rbf + rbf, model, S.Adam(d, n, 0.1, 0.9, 0.999))
    assert not host.UsesDevicePath()
    Vm = ksd_ref(X0, G, oracle.median_scale(X0)[0])
    assert abs(float(LD(host.ComputeKSD()) - Vm[0])) <= BAR * max(1.0, Vm[3])


def test_ksd_errors(oracle):
    n, d = 64, 3
    X = oracle.splitmix((n, d), 3.0, 39)
    G = np.zeros((n, d))
    c = S.Context(d, n)
    with pytest.raises(S.UnsetException):
        c.ksd(G, 1.0)
    c.set_particles(X)
    for a in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
            c.ksd(G, a)
    with pytest.raises(ValueError, match="no device model set"):
        c.ksd(None, 1.0)
    c.close()
    ns = 4096
    sim = S.Context(d, ns, sim_world=4)
    sim.set_particles(oracle.splitmix((ns, d), 3.0, 40))
    with pytest.raises(Exception, match="measurement context"):
        sim.ksd(np.zeros((sim.row1 - sim.row0, d)), 1.0)
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
def test_ksd_sharded_matches_one_rank(oracle, world, n):
    """Ranks on one GPU over the host shared-memory collectives: after 2 steps
    every rank returns the same V and U, equal to one rank's on the same
    particles (1e-12 relative); the ranks' rows, concatenated, are one rank's
    (at the bar, with max(1, .) = 1); and a further step is bit-identical to
    a run that never called the KSD."""
    d = 5
    with_k = _run_ranks(world, n, d, True)
    without = _run_ranks(world, n, d, False)
    X2 = with_k[0]["X2"]
    model = W.model(d)
    one = S.Context(d, n)
    one.set_particles(X2)
    v1, u1, rows1 = one.ksd(model.log_model_grad(X2), W.KSD_A, rows=True)
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
    err = float(np.max(np.abs(rows - rows1)))
    print("ksd sharded world=%d n=%d V=%.6g relV=%.3g relU=%.3g rows err=%.3g"
          % (world, n, v1, abs(with_k[0]["v"] - v1) / abs(v1), abs(with_k[0]["u"] - u1) / abs(u1), err))
    assert err <= BAR
