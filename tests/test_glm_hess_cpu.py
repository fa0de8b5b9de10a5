"""Device Hessian sum of the GLM (svgd_glm.hip: k_glm_wpass, k_glm_wgram) --
what can be checked without a GPU.

A numpy emulation of the summation order the kernels use, kept under a
quarter of the bar of tests/test_glm_cpu.py
    hbar = 1e-13 (s (M/B) nrows |A|^T |A| + lambda nrows I)
against the np.longdouble definition (tests/_glm.py); the weight
w = e / (1 + e)^2 from the table exponential against long double out to
|z| = 1400; and the two new symbols of the library."""
import ctypes
import os
import re

import numpy as np
import pytest

import _glm as R
from svgdcpp_amd import _capi as C

DIMS = [1, 3, 8, 17, 55, 64]
ROWS = [1, 63, 1000]
LINKS = ["logistic", "gaussian"]
N = 12
S_LIK, LAM = 0.7, 1.3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _windows(M):
    return [w for w in [(0, M), (3, 61), (M - 1, 1)] if w[0] >= 0 and w[0] + w[1] <= M]


def _emulate_weights(A, X, splits, rng):
    """k_glm_wpass / k_glm_wfinish in plain fp64: particle tiles of 64 rows in
    `splits` contiguous ranges; in a tile, 16-row groups js, and lane hi of a
    record's column holds rows js 16 + hi + 4r: one running sum per (record,
    hi), rows past the shard masked; the 4 hi partials added in hi order, the
    splits in ascending order.  e = exp(-|z|) carries a random +-2.6e-14
    relative error, the table form's bound."""
    n = X.shape[0]
    T = -(-n // 64)
    W = np.zeros(A.shape[0])
    for sp in range(splits):
        lane = np.zeros((4, A.shape[0]))
        for t in range(T * sp // splits, T * (sp + 1) // splits):
            for js in range(4):
                for r in range(4):
                    for hi in range(4):
                        i = t * 64 + js * 16 + hi + 4 * r
                        if i >= n:
                            continue
                        z = A @ X[i]
                        e = np.exp(-np.abs(z)) * (1 + 2.6e-14 * rng.choice([-1.0, 1.0], z.shape))
                        q = 1.0 + e
                        lane[hi] = lane[hi] + e / (q * q)
        W = W + (((lane[0] + lane[1]) + lane[2]) + lane[3])
    return W


def _emulate_gram(A, W, scale, diag):
    """k_glm_wgram / k_glm_hfinish: 64-record blocks, inside a block
    h = fma(W_m a_mr, a_ml, h) with m ascending (here without the fused
    rounding), the blocks added in ascending order, one triangle computed and
    mirrored."""
    M, d = A.shape
    tot = np.zeros((d, d))
    for b0 in range(0, M, 64):
        h = np.zeros((d, d))
        for m in range(b0, min(b0 + 64, M)):
            h = h + (W[m] * A[m])[:, None] * A[m][None, :]
        tot = tot + h
    H = scale * tot + diag * np.eye(d)
    L = np.tril(H)
    return L + np.tril(H, -1).T


def _emulate(A, y, X, link, m0, cnt, splits, rng):
    Aw = A[m0:m0 + cnt]
    n = X.shape[0]
    W = _emulate_weights(Aw, X, splits, rng) if link == "logistic" else np.full(cnt, float(n))
    return _emulate_gram(Aw, W, S_LIK * (A.shape[0] / cnt), LAM * n)


def _hbar(A, n, m0, cnt):
    Aw = np.abs(A[m0:m0 + cnt])
    f = S_LIK * A.shape[0] / cnt
    return R.BAR * (f * n * (Aw.T @ Aw) + LAM * n * np.eye(A.shape[1]))


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("d", DIMS)
def test_device_order_emulation_stays_under_a_quarter_of_the_bar(d, M, link):
    A, y, X = R.case(d, M, N, link)
    rng = np.random.default_rng(d * 1000 + M)
    for m0, cnt in dict.fromkeys(_windows(M)):
        H = _emulate(A, y, X, link, m0, cnt, 1, rng)
        ref = R.ref_neg_hess_sum(A, y, X, link, s=S_LIK, lam=LAM, m0=m0, count=cnt)
        ex = R.excess(H, ref, _hbar(A, N, m0, cnt))
        assert ex <= 0.25, (m0, cnt, ex)
        assert np.array_equal(H, H.T)


@pytest.mark.parametrize("d,M,n,splits", [(8, 4097, 300, 3), (17, 1000, 129, 2), (64, 1000, 1000, 7),
                                          (3, 63, 1000, 16), (8, 1000, 100, 1)])
def test_emulation_with_many_tiles_and_splits(d, M, n, splits):
    """Several particle tiles, a partial last tile and S > 1 splits; also theta
    x 100 (|z| in the hundreds: most weights underflow to 0)."""
    A, y, X = R.case(d, M, n, "logistic")
    rng = np.random.default_rng(d + M + n)
    for f in (1.0, 100.0):
        H = _emulate(A, y, X * f, "logistic", 0, M, splits, rng)
        ref = R.ref_neg_hess_sum(A, y, X * f, "logistic", s=S_LIK, lam=LAM)
        ex = R.excess(H, ref, _hbar(A, n, 0, M))
        assert np.all(np.isfinite(H))
        assert ex <= 0.25, (f, ex)


def _table_exp_neg_abs(z):
    """exp(-|z|) as svgd_glm.hip forms it: u = max(-|z| 4096 log2 e, -1100 4096),
    k = rint(u), 2^(k / 4096) from the table and ldexp, 2^(f / 4096) from the
    levelled polynomial."""
    log2e = float.fromhex("0x1.71547652b82fep+0")
    u = np.maximum(-np.abs(z) * (4096 * log2e), -1100.0 * 4096)
    k = np.rint(u)
    f = u - k
    ki = k.astype(np.int64)
    tab = np.array([float(2 ** (np.longdouble(i) / 4096)) for i in range(4096)])
    poly = (float.fromhex("0x1.ebfbdff82c58fp-27") * f + float.fromhex("0x1.62e42ff4f7b0ap-13")) * f + 1.0
    return np.ldexp(poly * tab[ki & 4095], (ki >> 12).astype(np.int32))


def test_weight_from_the_table_exponential():
    """w = e / (1 + e)^2 against sigma (1 - sigma) in long double for |z| up to
    1400.  Bar: the exponential's relative error 2.6e-14 plus four roundings,
    3e-14 of w (w's condition number in e is |1 - e| / (1 + e) <= 1); beyond
    the double range the weight is exactly 0, and nothing is NaN."""
    z = np.concatenate([np.linspace(-1400.0, 1400.0, 56001), np.linspace(-40.0, 40.0, 80001),
                        [0.0, -0.0, 708.0, 745.2, 745.1, 750.0, 1099.9, 1100.0, 1400.0]])
    # u itself is rounded: |z| 4096 log2e carries 2^-53 relative, i.e. an
    # error of |z| 2^-53 in the exponent -- |z| 1.1e-16 relative in e
    e = _table_exp_neg_abs(z)
    q = 1.0 + e
    w = e / (q * q)
    assert not np.any(np.isnan(w)) and np.all(w >= 0.0) and np.all(w <= 0.25)
    zl = np.abs(z).astype(R.LD)
    el = np.exp(-zl)
    ref = el / ((1 + el) * (1 + el))
    tol = (3e-14 + 2.3e-16 * np.abs(z)) * ref.astype(np.float64) + 5e-324
    assert np.all(np.abs(w - ref.astype(np.float64)) <= tol)
    assert np.all(w[np.abs(z) >= 750.0] == 0.0)  # below the smallest subnormal: exactly 0
    assert np.all(w[z == 0.0] == 0.25)


def test_library_exports_the_new_symbols():
    lib = C.lib()
    for name in ("svgd_device_neg_hess_sum", "svgd_set_device_hessian"):
        fn = getattr(lib, name)  # AttributeError when the library lacks it
        assert fn.restype is ctypes.c_int
    assert C.SIGNATURES["svgd_device_neg_hess_sum"] == (ctypes.c_int, [ctypes.c_void_p,
                                                                      ctypes.POINTER(ctypes.c_double)])
    assert C.SIGNATURES["svgd_set_device_hessian"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert lib.svgd_device_neg_hess_sum.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    assert lib.svgd_set_device_hessian.argtypes == [ctypes.c_void_p, ctypes.c_int]
    # the header declares what _capi.py binds
    hdr = open(os.path.join(ROOT, "include", "svgdcpp_amd", "svgd_capi.h")).read()
    assert re.search(r"int svgd_device_neg_hess_sum\(svgd_ctx \*ctx, double \*H_shard_out\);", hdr)
    assert re.search(r"int svgd_set_device_hessian\(svgd_ctx \*ctx, int on\);", hdr)
    # NULL context: refused before anything is touched
    assert lib.svgd_device_neg_hess_sum(None, None) == C.SVGD_ERR_ARG
    assert lib.svgd_set_device_hessian(None, 1) == C.SVGD_ERR_ARG
