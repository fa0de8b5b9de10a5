"""GLM posterior prediction on the host (svgd_glm_predict_host,
GeneralizedLinearModel.predict) against the np.longdouble definition within
the bars of tests/_glm_predict.py (derived there), its refusals, its optional
arguments and its edge cases.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _glm as R
import _glm_predict as P
import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [1, 3, 8, 17, 55, 64]
SHAPES = [(129, 1000), (1000, 300), (4097, 129)]  # (N particles, M test rows)
LINK_ID = {"logistic": C.SVGD_GLM_LOGISTIC, "gaussian": C.SVGD_GLM_GAUSSIAN}


def host(link, s, A, y, X, want=(True, True, True)):
    """svgd_glm_predict_host -> (rc, mean, var, lpd), an output None where not wanted."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    X = np.ascontiguousarray(X, dtype=np.float64)
    out = [np.full(A.shape[0], -7.0) if w else None for w in want]
    rc = C.lib().svgd_glm_predict_host(LINK_ID[link], s, A.shape[1], C.dptr(A), C.dptr(y), A.shape[0], C.dptr(X),
                                       X.shape[0], C.dptr(out[0]), C.dptr(out[1]), C.dptr(out[2]))
    return (rc, *out)


@pytest.mark.parametrize("link", P.LINKS)
@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("d", DIMS)
def test_host_matches_definition(d, N, M, link):
    A, y, X, ref, bar = P.case(d, N, M, link)
    rc, mean, var, lpd = host(link, P.S_LIK, A, y, X)
    assert rc == C.SVGD_OK
    ex = P.excesses((mean, var, lpd), ref, bar)
    print("glm predict host %s d=%d N=%d M=%d: mean %.3g var %.3g lpd %.3g of the bar" % ((link, d, N, M) + ex))
    assert all(np.all(np.isfinite(o)) for o in (mean, var, lpd))
    assert np.all(var >= 0.0)
    assert max(ex) <= 1.0
    # the model's method: its own link and lik_scale, the same bits
    model = S.GeneralizedLinearModel(A, y, link, P.S_LIK, 1.3)
    out = model.predict(X, A, y)
    assert len(out) == 3 and all(np.array_equal(a, b) for a, b in zip(out, (mean, var, lpd)))
    out = model.predict(X, A)
    assert len(out) == 2 and np.array_equal(out[0], mean) and np.array_equal(out[1], var)


_CHILD = r"""
import hashlib, sys
sys.path[:0] = [%r, %r]
import numpy as np
import _glm as R
from svgdcpp_amd import _capi as C
h = hashlib.sha256()
for link, lid in (("logistic", 0), ("gaussian", 1)):
    for d, N, M in ((8, 129, 1000), (55, 1000, 300)):
        A, y, X = R.case(d, M, N, link)
        out = [np.empty(M) for _ in range(3)]
        assert C.lib().svgd_glm_predict_host(lid, 0.7, d, C.dptr(A), C.dptr(y), M, C.dptr(X), N,
                                             *[C.dptr(o) for o in out]) == 0
        for o in out:
            h.update(o.tobytes())
print("digest", h.hexdigest())
"""


def test_bit_equal_across_thread_counts():
    digests = []
    for threads in ("1", "4"):
        env = dict(os.environ, OMP_NUM_THREADS=threads)
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        digests.append([l for l in r.stdout.splitlines() if l.startswith("digest")][0])
    assert digests[0] == digests[1]


def test_refusals_and_optional_arguments():
    lib = C.lib()
    A = np.array([[0.5, -0.5], [0.25, 1.0], [0.0, -1.0]])
    y = np.array([0.0, 1.0, 0.5])
    X = np.array([[0.1, 0.2], [-0.3, 0.4]])
    o = [np.empty(3) for _ in range(3)]

    def call(link=0, s=1.0, dim=2, A=A, y=y, m=3, X=X, n=2, outs=(0, 1, 2)):
        ptrs = [C.dptr(o[k]) if k in outs else None for k in range(3)]
        return lib.svgd_glm_predict_host(link, s, dim, C.dptr(A) if A is not None else None,
                                         C.dptr(y) if y is not None else None, m,
                                         C.dptr(X) if X is not None else None, n, *ptrs)

    assert call() == C.SVGD_OK
    assert call(A=None) == C.SVGD_ERR_ARG
    assert call(X=None) == C.SVGD_ERR_ARG
    assert call(link=7) == C.SVGD_ERR_ARG
    for s in (0.0, -1.0, np.nan, np.inf):
        assert call(s=s) == C.SVGD_ERR_ARG
    assert call(y=None) == C.SVGD_ERR_ARG                     # lpd without labels
    assert call(y=None, outs=(0, 1)) == C.SVGD_OK
    assert call(m=0) == C.SVGD_ERR_DIM
    assert call(dim=0) == C.SVGD_ERR_DIM
    assert call(n=0) == C.SVGD_ERR_DIM
    for bad in (np.inf, -np.inf, np.nan):
        B, z = A.copy(), y.copy()
        B[2, 1] = bad
        z[2] = bad
        assert call(A=B) == C.SVGD_ERR_ARG
        assert call(y=z) == C.SVGD_ERR_ARG
        assert call(link=1, y=z) == C.SVGD_ERR_ARG
    y2 = np.array([0.0, 1.5, 0.5])
    assert call(y=y2) == C.SVGD_ERR_ARG                       # a logistic label outside [0, 1]
    assert call(link=1, y=y2) == C.SVGD_OK
    # every optional output accepted as NULL, the others unchanged in value
    assert call() == C.SVGD_OK
    full = [a.copy() for a in o]
    for outs in ((), (0,), (1,), (2,), (0, 2), (1, 2)):
        for a in o:
            a.fill(-7.0)
        assert call(outs=outs) == C.SVGD_OK
        for k in range(3):
            assert np.array_equal(o[k], full[k]) if k in outs else np.all(o[k] == -7.0)
    # the Python wrappers raise
    model = S.GeneralizedLinearModel(A, y, "logistic")
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
        model.predict(X, A, y2)
    with pytest.raises(S.DimensionMismatchException, match=r"^SVGDCpp: \[Dimension Error\]"):
        model.predict(X, np.zeros((3, 5)))
    with pytest.raises(S.DimensionMismatchException, match=r"^SVGDCpp: \[Dimension Error\]"):
        model.predict(X, np.zeros((0, 2)))
    # the header declares what _capi.py binds
    hdr = open(os.path.join(ROOT, "include", "svgdcpp_amd", "svgd_capi.h")).read()
    assert "int svgd_glm_predict_host(int link, double lik_scale, int dim, const double *A, const double *y," in hdr
    assert "int svgd_glm_predict(svgd_ctx *ctx, int link, double lik_scale, const double *A, const double *y," in hdr
    assert lib.svgd_glm_predict(None, 0, 1.0, C.dptr(A), None, 3, None, None, None) == C.SVGD_ERR_ARG
    assert lib.svgd_glm_predict.restype is ctypes.c_int


@pytest.mark.parametrize("link", P.LINKS)
def test_identical_particles(link):
    """All particles equal: var >= 0 and within its bar of 0, the mean within
    its bar of mu(a . theta)."""
    A, y, X, _, _ = P.case(8, 129, 1000, link)
    Xs = np.ascontiguousarray(np.broadcast_to(X[3], X.shape))
    rc, mean, var, lpd = host(link, P.S_LIK, A, y, Xs)
    assert rc == C.SVGD_OK
    bm, bv, _ = P.bars(A, y, Xs, link)
    z = A.astype(P.LD) @ X[3].astype(P.LD)
    mu = R._sigmoid(z) if link == "logistic" else z
    assert np.all(var >= 0.0) and np.all(var <= bv)
    assert R.excess(mean, mu, bm) <= 1.0
    assert np.all(np.isfinite(lpd))


def test_wide_logistic_range():
    """theta x 100 (|z| >= 800: e underflows): finite outputs, mean in [0, 1]."""
    A, y, X, _, _ = P.case(8, 129, 1000, "logistic")
    Xw = X * 100.0
    assert np.max(np.abs(Xw @ A.T)) >= 800.0
    rc, mean, var, lpd = host("logistic", P.S_LIK, A, y, Xw)
    assert rc == C.SVGD_OK
    assert all(np.all(np.isfinite(o)) for o in (mean, var, lpd))
    assert np.all(mean >= 0.0) and np.all(mean <= 1.0) and np.all(var >= 0.0)
    ex = P.excesses((mean, var, lpd), P.reference(A, y, Xw, "logistic"), P.bars(A, y, Xw, "logistic"))
    print("glm predict host wide: mean %.3g var %.3g lpd %.3g of the bar" % ex)
    assert max(ex) <= 1.0


def test_documented_minus_infinity():
    """Gaussian link, s = 1, y = 1e3 and |z| <= 14: exp(-(y - z)^2 / 2)
    underflows at every particle, so lpd = -inf (the sum is not max-shifted);
    mean and var are unaffected."""
    A, y, X, ref, bar = P.case(8, 129, 1000, "gaussian")
    assert np.max(np.abs(X @ A.T)) <= 14.0
    rc, mean, var, lpd = host("gaussian", 1.0, A, np.full(A.shape[0], 1e3), X)
    assert rc == C.SVGD_OK
    assert np.all(lpd == -np.inf)
    assert max(P.excesses((mean, var), ref[:2], bar[:2])) <= 1.0
