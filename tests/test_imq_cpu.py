"""The inverse multiquadric kernel on the host: svgd_imq_phi_host against the
np.longdouble definition of tests/_imq.py within its bar (1e-12 max(1,
max|phi|)), its refusals and edge cases, the classes' closed forms, a numpy
emulation of the device order at a quarter of the bar on the clouds the bar
was worked out on (so the GPU bar is known to be reachable without a GPU),
and the Python SVGD with this kernel's closed form on the generic host path.
No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _clouds as cl
import _imq as Q
import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [1, 3, 8, 17, 64]
NS = [1, 15, 129, 1000]


def host(X, G, a, row0=0, nrows=None, dim=None):
    X = np.ascontiguousarray(X, dtype=np.float64)
    G = np.ascontiguousarray(G, dtype=np.float64)
    n, d = X.shape
    nrows = n - row0 if nrows is None else nrows
    out = np.full((max(nrows, 0), d), -7.0)
    rc = C.lib().svgd_imq_phi_host(d if dim is None else dim, n, C.dptr(X), C.dptr(G), a, row0, nrows,
                                   C.dptr(out))
    return rc, out


def case(n, d):
    seed = 900 + 31 * d + n
    X = Q.gaussian(n, d, seed)
    return X, cl.gradients(n, d, seed), Q.median_a(X)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("d", DIMS)
def test_host_matches_definition(d, n):
    X, G, a = case(n, d)
    ref = Q.imq_phi(X, G, a)
    rc, phi = host(X, G, a)
    assert rc == C.SVGD_OK
    err = float(np.max(np.abs(phi - ref)))
    print("imq host d=%d n=%d a=%.3g: err %.3g of bar %.3g" % (d, n, a, err, Q.bar(ref)))
    assert err <= Q.bar(ref)
    # row windows: the same bits as the rows of the full call
    for row0, nrows in ((0, 1), (n // 3, n - n // 3), (n - 1, 1), (n, 0)):
        rc, w = host(X, G, a, row0, nrows)
        assert rc == C.SVGD_OK and np.array_equal(w, phi[row0:row0 + nrows])


_CHILD = r"""
import hashlib, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import _clouds as cl, _imq as Q
from svgdcpp_amd import _capi as C
h = hashlib.sha256()
for n, d in ((129, 8), (1000, 17)):
    X = Q.gaussian(n, d, 5 + d)
    G = cl.gradients(n, d, 5 + d)
    out = np.empty((n, d))
    assert C.lib().svgd_imq_phi_host(d, n, C.dptr(X), C.dptr(G), 0.37, 0, n, C.dptr(out)) == 0
    h.update(out.tobytes())
print("digest", h.hexdigest())
"""


def test_bit_equal_across_thread_counts():
    digests = []
    for threads in ("1", "4"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        code = _CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        digests.append([l for l in r.stdout.splitlines() if l.startswith("digest")][0])
    assert digests[0] == digests[1]


def test_refusals():
    X, G, _ = case(15, 3)
    assert host(X, G, 1.0, dim=0)[0] == C.SVGD_ERR_DIM
    assert host(X, G, -1e-300)[0] == C.SVGD_ERR_ARG
    assert host(X, G, float("nan"))[0] == C.SVGD_ERR_ARG
    assert host(X, G, float("inf"))[0] == C.SVGD_ERR_ARG
    assert host(X, G, 1.0, row0=-1, nrows=1)[0] == C.SVGD_ERR_ARG
    assert host(X, G, 1.0, row0=10, nrows=6)[0] == C.SVGD_ERR_ARG
    out = np.empty((15, 3))
    lib = C.lib()
    assert lib.svgd_imq_phi_host(3, 15, None, C.dptr(G), 1.0, 0, 15, C.dptr(out)) == C.SVGD_ERR_ARG
    assert lib.svgd_imq_phi_host(3, 15, C.dptr(X), None, 1.0, 0, 15, C.dptr(out)) == C.SVGD_ERR_ARG
    assert lib.svgd_imq_phi_host(3, 15, C.dptr(X), C.dptr(G), 1.0, 0, 15, None) == C.SVGD_ERR_ARG
    assert lib.svgd_imq_phi_host(3, 0, C.dptr(X), C.dptr(G), 1.0, 0, 0, C.dptr(out)) == C.SVGD_ERR_DIM


def test_zero_scale_is_the_mean_gradient_and_one_particle_is_g():
    X, G, _ = case(129, 8)
    rc, phi = host(X, G, 0.0)
    assert rc == C.SVGD_OK
    assert np.max(np.abs(phi - G.astype(Q.LD).mean(axis=0).astype(np.float64))) <= 1e-14 * np.max(np.abs(G))
    for d in DIMS:
        X, G, _ = case(1, d)
        rc, phi = host(X, G, 2.5)
        assert rc == C.SVGD_OK and np.array_equal(phi, G)


def test_class_closed_forms_against_definition_and_central_differences():
    rng = np.random.default_rng(3)
    for d in (1, 3, 8):
        X = rng.normal(size=(d, 6))
        k = S.InverseMultiquadricKernel(X, S.InverseMultiquadricKernel.ScaleMethod.Constant, 0.7)
        assert k.GetParameters()[0] == 0.7
        k.UpdateParameters([1.3])
        loc, x = rng.normal(size=d), rng.normal(size=d)
        k.UpdateLocation(loc)
        assert abs(k.EvaluateKernel(x) - float(Q.imq_k(x, loc, 1.3))) <= 2e-16
        g = k.EvaluateKernelGrad(x)
        assert np.max(np.abs(g - Q.imq_grad(x, loc, 1.3).astype(np.float64))) <= 4e-16
        for c in range(d):
            e = np.zeros(d)
            e[c] = 1e-6
            fd = (k.EvaluateKernel(x + e) - k.EvaluateKernel(x - e)) / 2e-6
            assert abs(g[c] - fd) < 1e-9  # the difference quotient's own error: O(h^2) + 1e-16 / h
        # the reference's own gradient formula differentiates the same way
        for c in range(d):
            e = np.zeros(d)
            e[c] = 1e-6
            fd = float(Q.imq_k(x + e, loc, 1.3) - Q.imq_k(x - e, loc, 1.3)) / 2e-6
            assert abs(float(Q.imq_grad(x, loc, 1.3)[c]) - fd) < 1e-9
    with pytest.raises(ValueError):
        S.InverseMultiquadricKernel(np.zeros((2, 3)), scale=-1.0)
    with pytest.raises(ValueError):
        k.UpdateParameters([float("nan")])
    with pytest.raises(ValueError):
        S.InverseMultiquadricKernel(np.zeros((2, 3)), 7)


def test_class_composes_like_a_set_kernel():
    X = np.zeros((2, 4))
    imq = S.InverseMultiquadricKernel(X, S.InverseMultiquadricKernel.ScaleMethod.Constant, 0.4)
    rbf = S.GaussianRBFKernel(X, S.GaussianRBFKernel.ScaleMethod.Constant, scale=0.9)
    loc, x = np.array([0.2, -0.4]), np.array([0.5, 0.3])
    k = imq * rbf + imq
    assert type(k) is S.Kernel and len(k.GetParameters()) == 3
    k.UpdateLocation(loc)
    ki = float(Q.imq_k(x, loc, 0.4))
    kr = float(np.exp(-0.9 * (x - loc) @ (x - loc)))
    assert k.EvaluateKernel(x) == pytest.approx(ki * kr + ki, rel=1e-15)
    g = k.EvaluateKernelGrad(x)
    for c in range(2):
        e = np.zeros(2)
        e[c] = 1e-6
        assert abs(g[c] - (k.EvaluateKernel(x + e) - k.EvaluateKernel(x - e)) / 2e-6) < 1e-8


@pytest.mark.parametrize("name", sorted(Q.CLOUDS))
def test_emulated_device_order_keeps_a_quarter_of_the_bar(name):
    """Centred records, the Gram form with s clamped, tile-order fp64 sums and
    the xc_i sum k^3 - sum k^3 xc_j regrouping, in numpy: the device's bar is
    reachable in fp64."""
    X, G, a, ref = Q.cloud_case(name)
    for tile in (64, 32):
        err = float(np.max(np.abs(Q.emulate_device(X, G, a, tile) - ref)))
        print("imq emulation %s tile %d a=%.3g: err %.3g of bar %.3g" % (name, tile, a, err, Q.bar(ref)))
        assert err <= 0.25 * Q.bar(ref)


@pytest.mark.parametrize("d,n", [(8, 1000), (33, 129), (64, 300)])
def test_emulated_device_order_at_the_gpu_tests_scales(d, n):
    """The scales of tests/test_gpu_imq.py: a = 0, 1e-3, the median's and 1e6,
    where only the diagonal is left -- which the device form leaves out of the
    Gram sums by index (its rounding times a would be 1e-8 of G_i)."""
    seed = 77 + d
    X = Q.gaussian(n, d, seed)
    G = cl.gradients(n, d, seed)
    for a in (0.0, 1e-3, Q.median_a(X), 1e6):
        ref = Q.imq_phi(X, G, a)
        err = float(np.max(np.abs(Q.emulate_device(X, G, a, 32 if d > 36 else 64) - ref)))
        print("imq emulation d=%d n=%d a=%.3g: err %.3g of bar %.3g" % (d, n, a, err, Q.bar(ref)))
        assert err <= 0.25 * Q.bar(ref)


class Quadratic(S.Model):
    def __init__(self, d):
        super().__init__(d)

    def log_model_grad(self, X):
        return -X + 0.3


def test_python_svgd_generic_host_path_reproduces_a_manual_loop(oracle):
    """The closed form of InverseMultiquadricKernel given to a plain Kernel
    through UpdateKernel runs SVGD's generic host path; the result equals a
    hand-written loop over the definition."""
    n, d, a, iters = 12, 3, 0.8, 5
    X0 = oracle.splitmix((n, d), 1.0, 11)
    k = S.Kernel(d)
    k.UpdateKernel(S.InverseMultiquadricKernel._value, S.InverseMultiquadricKernel._gradient)
    k.UpdateParameters([a])
    X = X0.T.copy()
    s = S.SVGD(d, iters, X, k, Quadratic(d), S.Adam(d, n, 0.1, 0.9, 0.999))
    assert not s.UsesDevicePath()
    s.Initialize()
    s.Run()
    opt = S.Adam(d, n, 0.1, 0.9, 0.999)
    Xm = X0.copy()
    for _ in range(iters):
        G = -Xm + 0.3
        phi = Q.imq_phi(Xm, G, a).astype(np.float64)
        Xm = Xm + opt.Step(phi.T).T
    np.testing.assert_allclose(X.T, Xm, rtol=0, atol=1e-12)
