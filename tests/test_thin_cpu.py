"""Stein thinning on the host: svgd_stein_thin_host of both kernels against the
np.longdouble definition of tests/_thin.py under its two criteria (a valid
pick at every step along the library's own prefix, within
bar_t = 1e-12 max(1, max_j (u_jj / 2 + sum |u(pi_s, j)|)); and the very picks
of the definition where the reference alone shows the runner-up at least 1e3
bars away), equal bits across thread counts, the refusals, and the numpy
emulation of the device order at a quarter of the bar on the clouds the KSD
bar was worked out on.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _ksd_imq as K
import _thin as T
from svgdcpp_amd import _capi as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"rbf": C.SVGD_KERNEL_RBF, "imq": C.SVGD_KERNEL_IMQ}
I64P = ctypes.POINTER(ctypes.c_int64)


def host(kernel, X, G, a, m, dim=None, n=None, want=(True, True)):
    X = np.ascontiguousarray(X, dtype=np.float64)
    G = np.ascontiguousarray(G, dtype=np.float64)
    idx = np.full(max(m, 1) + 1, -7, dtype=np.int64)
    ksd2 = np.full(max(m, 1) + 1, -7.0)
    rc = C.lib().svgd_stein_thin_host(kernel, X.shape[1] if dim is None else dim, X.shape[0] if n is None else n,
                                      C.dptr(X), C.dptr(G), a, m, idx.ctypes.data_as(I64P) if want[0] else None,
                                      C.dptr(ksd2) if want[1] else None)
    assert idx[-1] == -7 and ksd2[-1] == -7.0  # nothing past the m slots
    return rc, idx[:-1], ksd2[:-1]


# (n, d, m): m > n forces repeats; 257 and 1000 cross the host's candidate blocks
SHAPES = [(1, 3, 4), (2, 1, 5), (77, 3, 100), (257, 1, 40), (1000, 8, 64), (2500, 17, 24)]


@pytest.mark.parametrize("n,d,m", SHAPES)
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_host_matches_definition(oracle, kernel, n, d, m):
    X, G, a = T.case(oracle, n, d, 900 + n + d)
    ref = T.replay(X, G, a, kernel, m)
    gap = T.gap_bars(ref)
    rc, idx, ksd2 = host(KERNELS[kernel], X, G, a, m)
    assert rc == C.SVGD_OK
    eo, ek = T.check_valid(X, G, a, kernel, idx, ksd2)
    print("thin host %s n=%d d=%d m=%d a=%.3g ksd2_1=%.6g ksd2_m=%.6g: obj excess/bar %.3g ksd2 err/bar %.3g "
          "min gap/bar %.3g" % (kernel, n, d, m, a, ksd2[0], ksd2[-1], eo, ek, gap))
    assert eo <= 1.0 and ek <= 1.0
    assert gap >= T.GAP_BARS  # from the reference alone: the picks are then the definition's
    assert np.array_equal(idx, ref["idx"])
    if n == 1:
        u00 = float(G[0] @ G[0]) + (1.0 if kernel == "imq" else 2.0) * a * d
        assert np.all(idx == 0) and ksd2 == pytest.approx(np.full(m, u00), rel=1e-15)
    diag = (G * G).sum(1)
    assert idx[0] == int(np.argmin(diag))  # t = 1: argmin u_jj
    # either output may be NULL: the other keeps its bits
    rc, idx2, _ = host(KERNELS[kernel], X, G, a, m, want=(True, False))
    assert rc == C.SVGD_OK and np.array_equal(idx2, idx)
    rc, _, k2 = host(KERNELS[kernel], X, G, a, m, want=(False, True))
    assert rc == C.SVGD_OK and np.array_equal(k2, ksd2)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_tie_goes_to_the_lowest_index(oracle, kernel):
    X, G, a = T.case(oracle, 300, 3, 17)
    G = G.copy()
    G[[3, 7]] = 0.0
    rc, idx, ksd2 = host(KERNELS[kernel], X, G, a, 1)
    assert rc == C.SVGD_OK and idx.tolist() == [3]


@pytest.mark.parametrize("name", K.edge_cases())
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_emulated_device_order_keeps_a_quarter_of_the_bar(kernel, name):
    """The fp64 loop of svgd_thin.hip restated in numpy is a valid selection
    at a quarter of the bar: the GPU bar is known to be reachable in fp64."""
    X, G, a, _ = K.edge_case(name)
    idx, ksd2 = T.emulate_device(X, G, a, kernel, 32)
    eo, ek = T.check_valid(X, G, a, kernel, idx, ksd2)
    print("thin emulation %s %s a=%.3g: obj excess/bar %.3g ksd2 err/bar %.3g" % (kernel, name, a, eo, ek))
    assert eo <= 0.25 and ek <= 0.25


@pytest.mark.parametrize("name", K.EDGE)
def test_host_on_edge_clouds(name):
    X, G, a, _ = K.edge_case(name)
    for kernel in sorted(KERNELS):
        rc, idx, ksd2 = host(KERNELS[kernel], X, G, a, 32)
        assert rc == C.SVGD_OK
        eo, ek = T.check_valid(X, G, a, kernel, idx, ksd2)
        print("thin host edge %s %s: obj excess/bar %.3g ksd2 err/bar %.3g" % (kernel, name, eo, ek))
        assert eo <= 1.0 and ek <= 1.0


_CHILD = r"""
import ctypes, hashlib, sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import oracle
import _thin as T
from svgdcpp_amd import _capi as C
h = hashlib.sha256()
for kernel in (C.SVGD_KERNEL_RBF, C.SVGD_KERNEL_IMQ):
    for n, d, m in ((129, 8, 40), (5000, 17, 30)):
        X, G, a = T.case(oracle, n, d, 5 + d)
        idx, ksd2 = np.empty(m, np.int64), np.empty(m)
        assert C.lib().svgd_stein_thin_host(kernel, d, n, C.dptr(X), C.dptr(G), a, m,
                                            idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), C.dptr(ksd2)) == 0
        h.update(idx.tobytes())
        h.update(ksd2.tobytes())
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
    X, G, a = T.case(oracle, 15, 3, 3)
    lib = C.lib()
    for kernel in KERNELS.values():
        assert host(kernel, X, G, a, 4, dim=0)[0] == C.SVGD_ERR_DIM
        assert host(kernel, X, G, a, 4, n=0)[0] == C.SVGD_ERR_DIM
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            rc, idx, ksd2 = host(kernel, X, G, bad, 4)
            assert rc == C.SVGD_ERR_ARG
            assert np.all(idx == -7) and np.all(ksd2 == -7.0)  # nothing written
        for m in (0, -3):
            rc, idx, ksd2 = host(kernel, X, G, a, m)
            assert rc == C.SVGD_ERR_ARG and np.all(idx == -7) and np.all(ksd2 == -7.0)
        assert lib.svgd_stein_thin_host(kernel, 3, 15, None, C.dptr(G), a, 4, None, None) == C.SVGD_ERR_ARG
        assert lib.svgd_stein_thin_host(kernel, 3, 15, C.dptr(X), None, a, 4, None, None) == C.SVGD_ERR_ARG
        assert lib.svgd_stein_thin_host(kernel, 3, 15, C.dptr(X), C.dptr(G), a, 4, None, None) == C.SVGD_OK
    for kernel in (-1, 2, 7):
        assert host(kernel, X, G, a, 4)[0] == C.SVGD_ERR_ARG
    # a KSD value that is not finite: reported, after the outputs are written
    Gbad = G.copy()
    Gbad[:] = 1e200
    rc, idx, ksd2 = host(C.SVGD_KERNEL_IMQ, X, Gbad, a, 2)
    assert rc == C.SVGD_ERR_RUNTIME and not np.all(np.isfinite(ksd2))


def test_abi_declares_the_new_functions():
    with open(os.path.join(ROOT, "include", "svgdcpp_amd", "svgd_capi.h")) as f:
        header = f.read()
    for name in ("svgd_stein_thin", "svgd_stein_thin_host"):
        assert name in C.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header)
        assert hasattr(C.lib(), name)
