"""The kernelized Stein discrepancy on the host: svgd_ksd_host of both kernels
against the np.longdouble definitions of tests/_ksd_imq.py within their bar
(1e-12 max(1, mean|u|) for V, U and every row), the one-particle closed form,
equal bits across thread counts, the refusals, and a numpy emulation of the
device order of the IMQ pass at a quarter of the bar on the clouds the bar was
worked out on (so the GPU bar is known to be reachable without a GPU).
No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _ksd_imq as K
from svgdcpp_amd import _capi as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"rbf": C.SVGD_KERNEL_RBF, "imq": C.SVGD_KERNEL_IMQ}


def host(kernel, X, G, a, dim=None, n=None, want=(True, True, True)):
    X = np.ascontiguousarray(X, dtype=np.float64)
    G = np.ascontiguousarray(G, dtype=np.float64)
    import ctypes

    v, u = ctypes.c_double(-7.0), ctypes.c_double(-7.0)
    rows = np.full(X.shape[0], -7.0)
    rc = C.lib().svgd_ksd_host(kernel, X.shape[1] if dim is None else dim, X.shape[0] if n is None else n,
                               C.dptr(X), C.dptr(G), a, ctypes.byref(v) if want[0] else None,
                               ctypes.byref(u) if want[1] else None, C.dptr(rows) if want[2] else None)
    return rc, v.value, u.value, rows


def case(oracle, n, d):
    X = oracle.splitmix((n, d), 3.0, 700 + n + d)
    return X, K.model(d).log_model_grad(X), K.scale(d)


@pytest.mark.parametrize("n,d", [(77, 3), (300, 17)])
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_host_matches_definition(oracle, kernel, n, d):
    X, G, a = case(oracle, n, d)
    ref = (K.ksd_imq_ref if kernel == "imq" else K.ksd_rbf_ref)(X, G, a)
    rc, v, u, rows = host(KERNELS[kernel], X, G, a)
    assert rc == C.SVGD_OK
    ev, eu, er = K.errors(v, u, rows, ref)
    print("ksd host %s n=%d d=%d a=%.3g V=%.6g U=%.6g: err/bar V %.3g U %.3g worst row %.3g"
          % (kernel, n, d, a, v, u, ev, eu, er))
    assert ev <= 1.0 and eu <= 1.0 and er <= 1.0
    assert v >= 0.0
    # any output may be NULL: the others keep their bits
    rc, v2, _, _ = host(KERNELS[kernel], X, G, a, want=(True, False, False))
    assert rc == C.SVGD_OK and v2 == v
    rc, _, u2, rows2 = host(KERNELS[kernel], X, G, a, want=(False, True, True))
    assert rc == C.SVGD_OK and u2 == u and np.array_equal(rows2, rows)


@pytest.mark.parametrize("d", [1, 3, 64])
def test_one_particle(oracle, d):
    X, G, a = case(oracle, 1, d)
    for kernel, c in (("imq", 1.0), ("rbf", 2.0)):
        rc, v, u, rows = host(KERNELS[kernel], X, G, a)
        assert rc == C.SVGD_OK
        assert v == pytest.approx(float(G[0] @ G[0]) + c * a * d, rel=1e-15)
        assert rows[0] == v
        assert np.isnan(u)


_CHILD = r"""
import ctypes, hashlib, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import oracle
import _ksd_imq as K
from svgdcpp_amd import _capi as C
h = hashlib.sha256()
for kernel in (C.SVGD_KERNEL_RBF, C.SVGD_KERNEL_IMQ):
    for n, d in ((129, 8), (1000, 17)):
        X = oracle.splitmix((n, d), 3.0, 5 + d)
        G = K.model(d).log_model_grad(X)
        v, u, rows = ctypes.c_double(), ctypes.c_double(), np.empty(n)
        assert C.lib().svgd_ksd_host(kernel, d, n, C.dptr(X), C.dptr(G), K.scale(d), ctypes.byref(v),
                                     ctypes.byref(u), C.dptr(rows)) == 0
        h.update(np.array([v.value, u.value]).tobytes())
        h.update(rows.tobytes())
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


def test_refusals(oracle):
    X, G, a = case(oracle, 15, 3)
    for kernel in KERNELS.values():
        assert host(kernel, X, G, a, dim=0)[0] == C.SVGD_ERR_DIM
        assert host(kernel, X, G, a, n=0)[0] == C.SVGD_ERR_DIM
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            rc, v, u, rows = host(kernel, X, G, bad)
            assert rc == C.SVGD_ERR_ARG
            assert v == -7.0 and u == -7.0 and np.all(rows == -7.0)  # nothing written
        lib = C.lib()
        assert lib.svgd_ksd_host(kernel, 3, 15, None, C.dptr(G), a, None, None, None) == C.SVGD_ERR_ARG
        assert lib.svgd_ksd_host(kernel, 3, 15, C.dptr(X), None, a, None, None, None) == C.SVGD_ERR_ARG
    for kernel in (-1, 2, 7):
        assert host(kernel, X, G, a)[0] == C.SVGD_ERR_ARG


@pytest.mark.parametrize("name", K.edge_cases())
def test_emulated_device_order_keeps_a_quarter_of_the_bar(name):
    """Centred records, the three Gram products, r2 clamped, the diagonal by
    index and tile-order fp64 sums, in numpy: the device's bar is reachable in
    fp64."""
    X, G, a, ref = K.edge_case(name)
    for tile in (64, 32):
        v, u, rows = K.emulate_device(X, G, a, tile)
        ev, eu, er = K.errors(v, u, rows, ref)
        print("ksd imq emulation %s tile %d a=%.3g: err/bar V %.3g U %.3g worst row %.3g" % (name, tile, a, ev, eu, er))
        assert max(ev, eu, er) <= 0.25


def test_a_bad_reciprocal_square_root_misses_the_bar():
    """The statistic of a k off by a relative 1e-9 -- a reciprocal square root
    left at its seed is off by more -- misses the row bar on a plain cloud: to
    first order every u_ij moves by k du/dk 1e-9, evaluated here in long
    double next to the reference."""
    X, G, a, ref = K.edge_case("gauss_d8")
    n, d = X.shape
    Xl, Gl, al = X.astype(K.LD), G.astype(K.LD), K.LD(a)
    r = Xl[:, None, :] - Xl[None, :, :]
    r2 = (r * r).sum(-1)
    ss = Gl @ Gl.T
    dsr = ((Gl[:, None, :] - Gl[None, :, :]) * r).sum(-1)
    k = (1 / np.sqrt(1 + al * r2)) * (1 + K.LD(1e-9))
    u = k * ss + al * k ** 3 * dsr + al * d * k ** 3 - 3 * al * al * k ** 5 * r2
    rows = (u.sum(1) / n).astype(np.float64)
    er = K.errors(float(ref[0]), float(ref[1]), rows, ref)[2]
    print("ksd imq k off by 1e-9: worst row err/bar %.3g" % er)
    assert er > 10.0


def test_abi_declares_the_new_functions():
    with open(os.path.join(ROOT, "include", "svgdcpp_amd", "svgd_capi.h")) as f:
        header = f.read()
    for name in ("svgd_ksd_kernel", "svgd_ksd_host"):
        assert name in C.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header)
        assert hasattr(C.lib(), name)
