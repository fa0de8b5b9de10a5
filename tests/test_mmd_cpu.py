"""The MMD on the host: svgd_mmd_host of both kernels against the np.longdouble
definition of tests/_mmd.py within 1e-12 absolute on the three means, V, U and
every witness row; equal bits across thread counts; Y = X; the refusals (the
host function has no context, so a refusal is its code alone: the messages
belong to svgd_mmd and tests/test_gpu_mmd.py); and the numpy emulation of the
device order inside the bar on every edge input the GPU test uses.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _mmd as Q
from svgdcpp_amd import _capi as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"rbf": C.SVGD_KERNEL_RBF, "imq": C.SVGD_KERNEL_IMQ}


def host(kernel, X, Y, a, dim=None, n=None, m=None, want=(True, True, True, True)):
    X = np.ascontiguousarray(X, dtype=np.float64)
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    v, u = np.full(2, -7.0), np.full(2, -7.0)
    m3, wit = np.full(4, -7.0), np.full(X.shape[0] + 1, -7.0)
    rc = C.lib().svgd_mmd_host(kernel, X.shape[1] if dim is None else dim, X.shape[0] if n is None else n,
                               C.dptr(X), Y.shape[0] if m is None else m, C.dptr(Y), a,
                               C.dptr(v) if want[0] else None, C.dptr(u) if want[1] else None,
                               C.dptr(m3) if want[2] else None, C.dptr(wit) if want[3] else None)
    assert v[1] == -7.0 and u[1] == -7.0 and m3[3] == -7.0 and wit[-1] == -7.0  # nothing past the slots
    return rc, v[0], u[0], m3[:3], wit[:-1]


SHAPES = [(1, 1, 1), (2, 1, 3), (77, 1000, 3), (515, 333, 8), (300, 200, 64)]


@pytest.mark.parametrize("n,m,d", SHAPES)
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_host_matches_definition(oracle, kernel, n, m, d):
    X, Y = Q.clouds(n, m, d, 900 + n + d)
    a = Q.scale(n, d)
    ref = Q.mmd_ref(X, Y, a, kernel)
    rc, v, u, m3, wit = host(KERNELS[kernel], X, Y, a)
    assert rc == C.SVGD_OK
    ev, eu, em, ew = Q.errors(v, u, m3, wit, ref)
    print("mmd host %s n=%d m=%d d=%d a=%.3g V=%.6g U=%.6g: err/bar V %.3g U %.3g means %.3g witness %.3g"
          % (kernel, n, m, d, a, v, u, ev, eu, em, ew))
    assert max(ev, eu, em, ew) <= 1.0
    assert np.isnan(u) == (n < 2 or m < 2) and np.isfinite(v)
    # any output may be NULL: the others keep their bits
    for mask in ((True, False, False, False), (False, True, True, False), (False, False, False, True)):
        rc, v2, u2, m32, w2 = host(KERNELS[kernel], X, Y, a, want=mask)
        assert rc == C.SVGD_OK
        assert v2 == (v if mask[0] else -7.0)
        assert (u2 == u or (np.isnan(u2) and np.isnan(u))) if mask[1] else u2 == -7.0
        assert np.array_equal(m32, m3) if mask[2] else np.all(m32 == -7.0)
        assert np.array_equal(w2, wit) if mask[3] else np.all(w2 == -7.0)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_sample_equal_to_the_particles(oracle, kernel):
    """Y = X: V = 0 within the bar, a zero witness, and U in closed form:
    with S = Sxx, U = 2 (S - N) / (N (N - 1)) - 2 S / N^2 = 2 (S - N^2) / (N^2 (N - 1))."""
    n, d = 257, 5
    X, _ = Q.clouds(n, 1, d, 33)
    a = Q.scale(n, d)
    rc, v, u, m3, wit = host(KERNELS[kernel], X, X.copy(), a)
    assert rc == C.SVGD_OK
    S = Q.mmd_ref(X, X, a, kernel)[0][0] * n * n
    closed = float(2 * (S - Q.LD(n) ** 2) / (Q.LD(n) ** 2 * (n - 1)))
    print("mmd host self %s |V|/bar %.3g |U - closed|/bar %.3g max|wit|/bar %.3g"
          % (kernel, abs(v) / Q.BAR, abs(u - closed) / Q.BAR, np.abs(wit).max() / Q.BAR))
    assert abs(v) <= Q.BAR and abs(u - closed) <= Q.BAR and np.abs(wit).max() <= Q.BAR
    assert m3[0] == m3[1]


@pytest.mark.parametrize("d", Q.EDGE_DIMS)
@pytest.mark.parametrize("name", Q.EDGE)
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_emulated_device_order_stays_inside_the_bar(oracle, kernel, name, d):
    """The Gram order of svgd_mmd.hip restated in fp64 numpy stays inside the
    bar on every edge input of tests/test_gpu_mmd.py: the GPU bar is known to
    be reachable in fp64 there."""
    X, Y, a = Q.edge(name, d)
    ref = Q.mmd_ref(X, Y, a, kernel)
    m3, V, U, wit = Q.emulate_device(X, Y, a, kernel)
    ev, eu, em, ew = Q.errors(float(V), float(U), m3, wit, ref)
    print("mmd emulation %s %s d=%d a=%.3g: err/bar V %.3g U %.3g means %.3g witness %.3g"
          % (kernel, name, d, a, ev, eu, em, ew))
    assert max(ev, eu, em, ew) <= 1.0


@pytest.mark.parametrize("d", Q.EDGE_DIMS)
@pytest.mark.parametrize("name", Q.EDGE)
def test_host_on_edge_inputs(oracle, name, d):
    X, Y, a = Q.edge(name, d)
    for kernel in sorted(KERNELS):
        rc, v, u, m3, wit = host(KERNELS[kernel], X, Y, a)
        assert rc == C.SVGD_OK
        ev, eu, em, ew = Q.errors(v, u, m3, wit, Q.mmd_ref(X, Y, a, kernel))
        print("mmd host edge %s %s d=%d: err/bar V %.3g U %.3g means %.3g witness %.3g"
              % (kernel, name, d, ev, eu, em, ew))
        assert max(ev, eu, em, ew) <= 1.0


_CHILD = r"""
import hashlib, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import oracle
import _mmd as Q
from svgdcpp_amd import _capi as C
h = hashlib.sha256()
for kernel in (C.SVGD_KERNEL_RBF, C.SVGD_KERNEL_IMQ):
    for n, m, d in ((129, 77, 8), (3000, 1001, 17)):
        X, Y = Q.clouds(n, m, d, 5 + d)
        out, wit = np.empty(5), np.empty(n)
        assert C.lib().svgd_mmd_host(kernel, d, n, C.dptr(X), m, C.dptr(Y), Q.scale(n, d), C.dptr(out[0:]),
                                     C.dptr(out[1:]), C.dptr(out[2:]), C.dptr(wit)) == 0
        h.update(out.tobytes())
        h.update(wit.tobytes())
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
    X, Y = Q.clouds(15, 9, 3, 3)
    lib = C.lib()
    for kernel in KERNELS.values():
        assert host(kernel, X, Y, 1.0, dim=0)[0] == C.SVGD_ERR_DIM
        assert host(kernel, X, Y, 1.0, n=0)[0] == C.SVGD_ERR_DIM
        for m in (0, -3):
            assert host(kernel, X, Y, 1.0, m=m)[0] == C.SVGD_ERR_DIM
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            rc, v, u, m3, wit = host(kernel, X, Y, bad)
            assert rc == C.SVGD_ERR_ARG
            assert v == -7.0 and u == -7.0 and np.all(m3 == -7.0) and np.all(wit == -7.0)  # nothing written
        for bad in (float("nan"), float("inf"), -float("inf")):
            Yb = Y.copy()
            Yb[8, 2] = bad
            rc, v, u, m3, wit = host(kernel, X, Yb, 1.0)
            assert rc == C.SVGD_ERR_ARG and v == -7.0 and np.all(wit == -7.0)
        assert lib.svgd_mmd_host(kernel, 3, 15, None, 9, C.dptr(Y), 1.0, None, None, None, None) == C.SVGD_ERR_ARG
        assert lib.svgd_mmd_host(kernel, 3, 15, C.dptr(X), 9, None, 1.0, None, None, None, None) == C.SVGD_ERR_ARG
        assert lib.svgd_mmd_host(kernel, 3, 15, C.dptr(X), 9, C.dptr(Y), 1.0, None, None, None, None) == C.SVGD_OK
    for kernel in (-1, 2, 7):
        assert host(kernel, X, Y, 1.0)[0] == C.SVGD_ERR_ARG


def test_abi_declares_the_new_functions():
    with open(os.path.join(ROOT, "include", "svgdcpp_amd", "svgd_capi.h")) as f:
        header = f.read()
    for name in ("svgd_mmd", "svgd_mmd_host"):
        assert name in C.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header)
        assert hasattr(C.lib(), name)
