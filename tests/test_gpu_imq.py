"""Device inverse multiquadric phi (svgd_imq.hip: svgd_set_kernel(IMQ),
k_imq_prep / k_imq_pass / k_imq_finish) against the np.longdouble definition
of tests/_imq.py.

Bar (tests/_imq.py): max |device - reference| <= 1e-12 max(1, max|phi|);
positions after steps <= 1e-9 (the project's step bar), the median scale
<= 1e-12 relative to the oracle's.  Each test prints its worst error ("imq
...").  The shapes are the smallest at which the tile code can go wrong:
every KP/4 remainder and 16-column block edge in d; one partial tile, the
tile edge, ragged multi-tile and several row groups in N."""
import multiprocessing as mp
import re
import uuid

import numpy as np
import pytest

import _clouds as cl
import _glm as R
import _gpu_imq_rank_worker as W
import _imq as Q
import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

pytestmark = pytest.mark.gpu

DIMS = [1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32, 33, 48, 63, 64]
NS = [1, 15, 64, 129, 1000]
ARG_ERR = r"^SVGDCpp: \[Argument Error\]"


def imq_ctx(X, dtype=None):
    c = S.Context(X.shape[1], X.shape[0], dtype=dtype)
    c.set_particles(X)
    c.set_kernel("imq")
    return c


def dev_phi(X, G, a, dtype=None):
    c = imq_ctx(X, dtype)
    phi = c.phi(G, a)
    c.close()
    return phi


def check(tag, phi, ref):
    err = float(np.max(np.abs(phi - ref)))
    print("imq %s: err %.3g of bar %.3g" % (tag, err, Q.bar(ref)))
    assert np.all(np.isfinite(phi))
    assert err <= Q.bar(ref)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DIMS)
def test_phi_matches_definition_shapes(d, n):
    seed = 900 + 31 * d + n
    X = Q.gaussian(n, d, seed)
    G = cl.gradients(n, d, seed)
    a = Q.median_a(X)
    check("d=%d n=%d a=%.3g" % (d, n, a), dev_phi(X, G, a), Q.imq_phi(X, G, a))


@pytest.mark.parametrize("d,n", [(8, 1000), (33, 129), (64, 300)])
def test_phi_matches_definition_scales(d, n):
    """a = 0 (k = 1: the mean of G), a small, the median's, and 1e6 (only the
    diagonal is left)."""
    seed = 77 + d
    X = Q.gaussian(n, d, seed)
    G = cl.gradients(n, d, seed)
    c = imq_ctx(X)
    for a in (0.0, 1e-3, Q.median_a(X), 1e6):
        check("scales d=%d n=%d a=%.3g" % (d, n, a), c.phi(G, a), Q.imq_phi(X, G, a))
    c.close()


@pytest.mark.parametrize("name", ["shift1e6", "two_d8", "aniso", "gauss_d64"])
def test_phi_matches_definition_clouds(name):
    X, G, a, ref = Q.cloud_case(name)
    check("cloud %s a=%.3g" % (name, a), dev_phi(X, G, a), ref)


def test_phi_duplicates_pure_repulsion_and_pure_drive():
    n, d = 129, 5
    X = np.array(Q.gaussian(n, d, 5))
    X[1::2] = X[0::2][: len(X[1::2])]  # every particle twice: r^2 = 0 through the clamp
    G = cl.gradients(n, d, 5)
    a = 0.8
    check("duplicates", dev_phi(X, G, a), Q.imq_phi(X, G, a))
    X = Q.gaussian(n, d, 6)
    Z = np.zeros_like(G)
    check("G = 0", dev_phi(X, Z, a), Q.imq_phi(X, Z, a))
    check("G large, a tiny", dev_phi(X, 1e8 * G, 1e-12), Q.imq_phi(X, 1e8 * G, 1e-12))


def test_repeat_calls_and_f32_context():
    n, d = 1000, 33  # 8 row groups, ragged tiles, S > 1
    seed = 12
    X = Q.gaussian(n, d, seed)
    G = cl.gradients(n, d, seed)
    a = Q.median_a(X)
    ref = Q.imq_phi(X, G, a)
    c = imq_ctx(X)
    p1 = c.phi(G, a)
    p2 = c.phi(G, a)
    c.close()
    assert np.array_equal(p1, p2)
    check("f64", p1, ref)
    # the IMQ arithmetic is fp64 whatever the dtype (the centring is fp64 too)
    check("f32 context", dev_phi(X, G, a, dtype=C.SVGD_F32), ref)


@pytest.mark.parametrize("d,n", [(8, 1000), (40, 300)])
def test_switching_back_to_rbf_and_names(d, n):
    X = Q.gaussian(n, d, 3)
    G = cl.gradients(n, d, 3)
    a = 0.5 * Q.median_a(X)
    fresh = S.Context(d, n)
    assert fresh.kernel == "rbf"
    rbf_name = fresh.phi_kernel_name()
    assert rbf_name == S.plan_phi_name(d, n) and "imq" not in rbf_name
    fresh.set_particles(X)
    want = fresh.phi(G, a)
    fresh.close()
    c = S.Context(d, n)
    c.set_particles(X)
    c.set_kernel("imq")
    assert c.kernel == "imq"
    assert c.phi_kernel_name() == "k_imq_pass<%d>" % ((d + 3) // 4 * 4)
    c.phi(G, a)
    c.phi(G, a)
    c.set_kernel("rbf")
    assert c.kernel == "rbf" and c.phi_kernel_name() == rbf_name
    got = c.phi(G, a)
    c.close()
    assert np.array_equal(got, want)


def test_refusals():
    c = S.Context(3, 40)
    with pytest.raises(ValueError, match=ARG_ERR):
        c.check(c.lib.svgd_set_kernel(c.h, 2))
    with pytest.raises(ValueError, match=ARG_ERR):
        c.check(c.lib.svgd_set_kernel(c.h, -1))
    with pytest.raises(ValueError, match=ARG_ERR):
        c.set_kernel("matern")
    # IMQ first, then a Hessian or matrix scale
    c.set_kernel("imq")
    with pytest.raises(ValueError, match=ARG_ERR):
        c.set_scale(C.SVGD_SCALE_HESSIAN, 0.0)
    with pytest.raises(ValueError, match=ARG_ERR):
        c.set_scale_matrix(np.eye(3))
    c.set_scale(C.SVGD_SCALE_FIXED, 0.3)  # the scalar methods are accepted
    c.set_scale(C.SVGD_SCALE_MEDIAN, 0.0)
    assert c.kernel == "imq"
    c.close()
    # the scale first, then IMQ
    for setter in (lambda c: c.set_scale(C.SVGD_SCALE_HESSIAN, 0.0), lambda c: c.set_scale_matrix(2.0 * np.eye(3))):
        c = S.Context(3, 40)
        setter(c)
        with pytest.raises(ValueError, match=ARG_ERR):
            c.set_kernel("imq")
        assert c.kernel == "rbf"
        c.close()


def _grad(X):
    return -(X - 0.4) / 1.5


def _device_steps(X0, kind, steps, d):
    n = X0.shape[0]
    c = imq_ctx(X0)
    if kind == "adam":
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    else:
        c.set_optimizer(C.SVGD_OPT_ADAGRAD, 0.05, 0.0, 0.0, 1e-8)
    c.set_bounds(-np.full(d, 1.5), np.full(d, 1.5))
    scales, Xs = [], [X0]
    for _ in range(steps):
        G = np.ascontiguousarray(_grad(Xs[-1]))
        c.check(c.lib.svgd_step(c.h, C.dptr(G)))
        scales.append(c.last_scale()[0])
        Xs.append(c.get_particles())
    c.close()
    assert Xs[-1].shape == (n, d)
    return Xs, scales


@pytest.mark.parametrize("kind", ["adam", "adagrad"])
@pytest.mark.parametrize("n,d", [(1000, 8), (300, 33)])
def test_steps_match_reference_loop(oracle, monkeypatch, n, d, kind):
    """5 steps, bounds on, median scale: the loop built from _imq.py, the
    oracle's median and the oracle's optimizer step; and bit-identical with
    speculation and the tracked bracket switched off."""
    steps = 5
    X0 = oracle.splitmix((n, d), 2.0, 19 + d)
    Xs, scales = _device_steps(X0, kind, steps, d)
    X = Xs[-1]
    opt = oracle.Adam((n, d), 0.05, 0.9, 0.999) if kind == "adam" else oracle.AdaGrad((n, d), 0.05)
    Xr = X0.copy()
    for t in range(steps):
        a_dev = oracle.median_scale(Xs[t])[0]  # the oracle's median of the device's own X_t
        assert abs(scales[t] - a_dev) <= 1e-12 * a_dev, (t, scales[t], a_dev)
        a = oracle.median_scale(Xr)[0]
        phi = Q.imq_phi(Xr, _grad(Xr), a).astype(np.float64)
        oracle.apply_update(Xr, opt.step(phi), -np.full(d, 1.5), np.full(d, 1.5))
    err = float(np.max(np.abs(X - Xr)))
    print("imq steps %s n=%d d=%d: positions err %.3g (bar 1e-9)" % (kind, n, d, err))
    assert err <= 1e-9
    monkeypatch.setenv("SVGD_SPECULATE", "0")
    monkeypatch.setenv("SVGD_TRACK_BRACKET", "0")
    Xs2, scales2 = _device_steps(X0, kind, steps, d)
    assert np.array_equal(X, Xs2[-1]) and scales == scales2


def _model(d):
    import oracle as O
    mus = O.splitmix((3, d), 3.0, 42)
    return S.GaussianSum(list(mus), [np.eye(d) * (1.0 + 0.25 * c) for c in range(3)])


@pytest.mark.parametrize("n,d", [(1000, 8), (300, 33)])
def test_host_model_step_pipelined_equals_split(oracle, n, d):
    X0 = oracle.splitmix((n, d), 3.0, 41)
    out = []
    for pipelined in (True, False):
        c = imq_ctx(X0)
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
        c.set_bounds(-np.full(d, 2.5), np.full(d, 2.5))
        m = _model(d)
        for _ in range(4):
            c.step_with_model(m, pipelined=pipelined)
        out.append(c.get_particles())
        c.close()
    assert np.array_equal(out[0], out[1])
    assert np.max(np.abs(out[0] - X0)) > 1e-3  # the particles moved


def test_device_glm_step_matches_host_gradient_steps():
    d, n, M = 17, 300, 200
    A, y, X0 = R.case(d, M, n, "logistic")
    out = []
    for device in (True, False):
        model = S.GeneralizedLinearModel(A, y, "logistic", 0.7, 1.3)
        c = imq_ctx(X0)
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.01, 0.9, 0.999, 1e-8)
        if device:
            c.set_device_model(model)
        for _ in range(4):
            if device:
                c.step_device()
            else:
                c.step_with_model(model)
        out.append(c.get_particles())
        c.close()
    err = float(np.max(np.abs(out[0] - out[1])))
    print("imq device GLM step vs host gradient: %.3g (bar 1e-12)" % err)
    assert err <= 1e-12
    assert np.max(np.abs(out[0] - X0)) > 1e-3


def _run_ranks(world, n, d, steps):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    name = "svgd_" + uuid.uuid4().hex[:12]
    procs = [ctx.Process(target=W.run, args=(r, world, name, n, d, steps, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = {}
    try:
        for _ in range(world):
            status, rank, X, scales, shard, kname = q.get(timeout=300)
            assert status == "ok", X
            out[rank] = (X, scales, shard, kname)
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return out


def test_three_ranks_match_one_rank():
    n, d, steps = 1000, 8, 4
    multi = _run_ranks(3, n, d, steps)
    X1, s1, _, k1 = _run_ranks(1, n, d, steps)[0]
    assert k1 == "k_imq_pass<8>"
    shards = sorted(v[2] for v in multi.values())
    assert shards[0][0] == 0 and shards[-1][1] == n
    for rank, (X, scales, _, kname) in multi.items():
        assert kname == k1
        assert scales[0] == s1[0], (rank, scales, s1)  # the same X_0: bit-exact
        err = float(np.max(np.abs(X - X1)))
        print("imq 3 ranks, rank %d: X err %.3g (bar 1e-10)" % (rank, err))
        assert err <= 1e-10


class Quadratic(S.Model):
    def __init__(self, d):
        super().__init__(d)

    def log_model_grad(self, X):
        return -X + 0.3


def _svgd(kernel, X, iters, d, log_path=None):
    o = S.SVGDOptions()
    o.Dimension, o.NumIterations, o.CoordinateMatrixPtr = d, iters, X
    o.KernelPtr, o.ModelPtr = kernel, Quadratic(d)
    o.OptimizerPtr = S.Adam(d, X.shape[1], 0.1, 0.9, 0.999)
    if log_path:
        o.LogIntermediateMatrices, o.IntermediateMatricesOutputPath = True, log_path
        o.IntermediateMatricesPrecision = 17
    s = S.SVGD(o)
    s.Initialize()
    s.Run()
    return s


def test_python_class_device_path_matches_generic_host_path(oracle):
    n, d, a, iters = 64, 3, 0.8, 10
    X0 = oracle.splitmix((n, d), 1.0, 11)
    Xd = X0.T.copy()
    k = S.InverseMultiquadricKernel(Xd, S.InverseMultiquadricKernel.ScaleMethod.Constant, a)
    s = _svgd(k, Xd, iters, d)
    assert s.UsesDevicePath() and s.ctx.kernel == "imq"
    Xh = X0.T.copy()
    plain = S.Kernel(d)
    plain.UpdateKernel(S.InverseMultiquadricKernel._value, S.InverseMultiquadricKernel._gradient)
    plain.UpdateParameters([a])
    assert not _svgd(plain, Xh, iters, d).UsesDevicePath()
    err = float(np.max(np.abs(Xd - Xh)))
    print("imq class device vs generic host path: %.3g (bar 1e-10)" % err)
    assert err <= 1e-10


def test_python_class_median_scale_matches_manual_loop(oracle):
    n, d, iters = 64, 3, 5
    X0 = oracle.splitmix((n, d), 1.0, 13)
    Xd = X0.T.copy()
    s = _svgd(S.InverseMultiquadricKernel(Xd), Xd, iters, d)
    assert s.UsesDevicePath()
    opt = S.Adam(d, n, 0.1, 0.9, 0.999)
    Xm = X0.copy()
    for _ in range(iters):
        a = oracle.median_scale(Xm)[0]
        Xm = Xm + opt.Step(Q.imq_phi(Xm, -Xm + 0.3, a).astype(np.float64).T).T
    err = float(np.max(np.abs(Xd.T - Xm)))
    print("imq class median scale vs manual loop: %.3g (bar 1e-9)" % err)
    assert err <= 1e-9


def test_python_class_logged_matrices(oracle, tmp_path):
    n, d, iters = 10, 2, 3
    X0 = oracle.splitmix((n, d), 1.0, 17)
    Xd = X0.T.copy()
    _svgd(S.InverseMultiquadricKernel(Xd), Xd, iters, d, log_path=str(tmp_path / "log.txt"))
    blocks = re.split(r"========== Step \d+ ==========\n", open(tmp_path / "log.txt").read())[1:]
    assert len(blocks) == iters
    Xt = X0
    for b in blocks:
        mats = {}
        for name in ("LogModelGrad", "Kernel", "KernelGrad", "CoordMat"):
            body = b.split(name + "=\n", 1)[1].split("\n\n", 1)[0]
            mats[name] = np.array([[float(v) for v in ln.split()] for ln in body.strip().split("\n")])
        K, Kg = Q.imq_matrices(Xt, oracle.median_scale(Xt)[0])
        np.testing.assert_allclose(mats["Kernel"], K.astype(np.float64), rtol=0, atol=1e-12)
        np.testing.assert_allclose(mats["KernelGrad"], Kg.astype(np.float64), rtol=0, atol=1e-12)
        Xt = mats["CoordMat"].T
