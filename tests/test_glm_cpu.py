"""Host generalized linear model (svgd_glm_*, GeneralizedLinearModel): no GPU.

Gradient, log p and Hessian sum against the np.longdouble definition
(tests/_glm.py) at its bar; the gradient against central differences of
svgd_glm_logp; a numpy emulation of the device kernel's summation order kept
under a quarter of the bar; the Gaussian link against the MultivariateNormal
of the same posterior; every refusal; the Python API."""
import ctypes

import numpy as np
import pytest

import _glm as R
import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

DIMS = [1, 3, 8, 17, 55, 64]
ROWS = [1, 63, 1000]
LINKS = ["logistic", "gaussian"]
N = 12
S_LIK, LAM = 0.7, 1.3


def _windows(M):
    return [w for w in [(0, M), (3, 61), (M - 1, 1)] if w[0] >= 0 and w[0] + w[1] <= M]


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("d", DIMS)
def test_host_model_matches_definition(d, M, link):
    A, y, X = R.case(d, M, N, link)
    m = S.GeneralizedLinearModel(A, y, link, S_LIK, LAM)
    for m0, cnt in dict.fromkeys(_windows(M)):
        m.set_batch(m0, cnt)
        kw = dict(s=S_LIK, lam=LAM, m0=m0, count=cnt)
        ex = R.excess(m.log_model_grad(X), R.ref_grad(A, y, X, link, **kw), R.grad_bar(A, y, X, link, **kw))
        assert ex <= 1.0, (m0, cnt, ex)
        # log p: 1e-13 of the summed magnitudes of its terms
        Aw, yw, f = np.abs(A[m0:m0 + cnt]), np.abs(y[m0:m0 + cnt]), S_LIK * M / cnt
        Z = np.abs(X) @ Aw.T
        terms = (yw * Z + Z + 1.0) if link == "logistic" else (yw + Z) ** 2
        lbar = R.BAR * (f * terms.sum(axis=1) + LAM / 2 * (X * X).sum(axis=1))
        ex = R.excess(m.log_model(X), R.ref_logp(A, y, X, link, **kw), lbar)
        assert ex <= 1.0, (m0, cnt, ex)
        # Hessian sum: w <= 1 (gaussian) or 1/4 (logistic) per particle and row
        hbar = R.BAR * (f * N * (Aw.T @ Aw) + LAM * N * np.eye(d))
        ex = R.excess(m.neg_hess_sum(X), R.ref_neg_hess_sum(A, y, X, link, **kw), hbar)
        assert ex <= 1.0, (m0, cnt, ex)


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d,M", [(1, 1), (3, 63), (17, 63), (8, 1000)])
def test_gradient_is_the_derivative_of_logp(d, M, link):
    """Central differences of svgd_glm_logp, step h = 1e-5.  Truncation is
    h^2/6 |d^3 log p| <= 2e-11 * s(M/B) sum |a_k|^3 |l'''| (|l'''| <= 0.1,
    zero for the Gaussian link) and rounding 2 * 2^-53 |log p| / h; both are
    far below 1e-6 of the gradient's scale, and a wrong formula is O(1) of it."""
    A, y, X = R.case(d, M, N, link)
    m = S.GeneralizedLinearModel(A, y, link, S_LIK, LAM)
    wins = _windows(M)
    m.set_batch(*wins[-1 if M > 1 else 0])
    G = m.log_model_grad(X)
    h = 1e-5
    fd = np.empty_like(G)
    for k in range(d):
        E = np.zeros_like(X)
        E[:, k] = h
        fd[:, k] = (m.log_model(X + E) - m.log_model(X - E)) / (2 * h)
    m0, cnt = m.batch_
    scale = R.grad_scale(A, y, X, link, s=S_LIK, lam=LAM, m0=m0, count=cnt)
    lp = np.abs(m.log_model(X))[:, None]
    assert np.all(np.abs(G - fd) <= 1e-6 * scale + 4 * 2.0 ** -53 * lp / h)


def _emulate_device(A, y, X, link, s, lam, S_splits, rng):
    """The device kernel's order in plain fp64: records in tiles of 64, each
    tile in blocks of 16, each block's contraction in groups of 4 records
    (one MFMA each, its 4 products added to the accumulator in turn); S
    contiguous tile ranges -> partial sums added s ascending; then
    scale * sum - lambda theta.  The sigmoid's exp is perturbed by a random
    +-2.6e-14 relative, the table form's bound."""
    M, d = A.shape
    T = -(-M // 64)
    Ap = np.zeros((T * 64, d))
    Ap[:M] = A
    yp = np.zeros(T * 64)
    yp[:M] = y
    parts = []
    for sp in range(S_splits):
        acc = np.zeros_like(X)
        for t in range(T * sp // S_splits, T * (sp + 1) // S_splits):
            for b in range(4):
                r0 = t * 64 + b * 16
                Z = X @ Ap[r0:r0 + 16].T
                if link == "logistic":
                    e = np.exp(-np.abs(Z)) * (1 + 2.6e-14 * rng.choice([-1.0, 1.0], Z.shape))
                    Rm = yp[r0:r0 + 16] - np.where(Z >= 0, 1.0, e) / (1 + e)
                else:
                    Rm = yp[r0:r0 + 16] - Z
                for g in range(4):
                    for j in range(4 * g, 4 * g + 4):
                        acc = acc + Rm[:, j:j + 1] * Ap[r0 + j][None, :]
        parts.append(acc)
    tot = np.zeros_like(X)
    for p in parts:
        tot = tot + p
    return s * tot - lam * X


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("d,M,splits", [(1, 63, 1), (3, 1000, 3), (8, 4097, 5), (17, 1000, 16),
                                       (55, 4097, 2), (64, 1000, 4), (64, 4097, 65)])
def test_device_order_emulation_stays_under_a_quarter_of_the_bar(d, M, splits, link):
    A, y, X = R.case(d, M, N, link)
    rng = np.random.default_rng(d * 1000 + M)
    G = _emulate_device(A, y, X, link, S_LIK, LAM, splits, rng)
    ex = R.excess(G, R.ref_grad(A, y, X, link, s=S_LIK, lam=LAM),
                  R.grad_bar(A, y, X, link, s=S_LIK, lam=LAM))
    assert ex <= 0.25, ex


def test_gaussian_link_is_the_normal_posterior():
    """Linear regression: the posterior is N(P^-1 s A^T y, P^-1) with
    P = s A^T A + lambda I, so the GLM's gradient is the MultivariateNormal's.
    Bar 1e-12 of the gradient's scale (observed 3e-16 at cond(P) = 1.7)."""
    d, M = 8, 200
    A, y, X = R.case(d, M, 50, "gaussian")
    s, lam = 0.25, 2.0
    P = s * A.T @ A + lam * np.eye(d)
    mean = np.linalg.solve(P, s * A.T @ y)
    mvn = S.MultivariateNormal(mean, np.linalg.inv(P))
    glm = S.GeneralizedLinearModel(A, y, "gaussian", s, lam)
    scale = R.grad_scale(A, y, X, "gaussian", s=s, lam=lam)
    assert np.all(np.abs(glm.log_model_grad(X) - mvn.log_model_grad(X)) <= 1e-12 * scale)
    np.testing.assert_allclose(glm.neg_hess_sum(X), X.shape[0] * P, rtol=1e-13)


def _create(A, y, link=0, s=1.0, lam=1.0, d=None, M=None, out=True):
    h = ctypes.c_void_p()
    A = None if A is None else np.ascontiguousarray(A, dtype=np.float64)
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    rc = C.lib().svgd_glm_create(ctypes.byref(h) if out else None,
                                 A.shape[1] if d is None else d, A.shape[0] if M is None else M,
                                 C.dptr(A), C.dptr(y), link, s, lam)
    if rc == C.SVGD_OK:
        C.lib().svgd_glm_destroy(h)
    return rc


def test_refusals():
    A, y = np.ones((5, 2)) * 0.5, np.array([0.0, 1.0, 1.0, 0.0, 0.5])
    assert _create(A, y) == C.SVGD_OK  # soft label 0.5 is fine
    assert _create(A, y, out=False) == C.SVGD_ERR_ARG
    assert _create(None, y, d=2, M=5) == C.SVGD_ERR_ARG
    assert _create(A, None, d=2, M=5) == C.SVGD_ERR_ARG
    assert _create(A, y, d=0) == C.SVGD_ERR_DIM
    assert _create(A, y, M=0) == C.SVGD_ERR_DIM
    assert _create(A, y, link=2) == C.SVGD_ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        B = A.copy()
        B[3, 1] = bad
        assert _create(B, y) == C.SVGD_ERR_ARG
        z = y.copy()
        z[2] = bad
        assert _create(A, z) == C.SVGD_ERR_ARG
        assert _create(A, z, link=1) == C.SVGD_ERR_ARG
    for lab in (-1e-9, 1.0 + 1e-9):
        z = y.copy()
        z[0] = lab
        assert _create(A, z) == C.SVGD_ERR_ARG
        assert _create(A, z, link=1) == C.SVGD_OK  # any finite y under the Gaussian link
    for s in (0.0, -1.0, np.nan):
        assert _create(A, y, s=s) == C.SVGD_ERR_ARG
    for lam in (-1e-300, np.nan):
        assert _create(A, y, lam=lam) == C.SVGD_ERR_ARG
    assert _create(A, y, lam=0.0) == C.SVGD_OK
    # batch windows
    h = ctypes.c_void_p()
    assert C.lib().svgd_glm_create(ctypes.byref(h), 2, 5, C.dptr(A), C.dptr(y), 0, 1.0, 1.0) == C.SVGD_OK
    lib = C.lib()
    for m0, cnt in [(0, 0), (0, -1), (0, 6), (5, 1), (4, 2), (-1, 2), (2 ** 62, 2 ** 62)]:
        assert lib.svgd_glm_set_batch(h, m0, cnt) == C.SVGD_ERR_ARG, (m0, cnt)
    for m0, cnt in [(0, 5), (4, 1), (1, 3)]:
        assert lib.svgd_glm_set_batch(h, m0, cnt) == C.SVGD_OK
    assert lib.svgd_glm_set_batch(None, 0, 1) == C.SVGD_ERR_ARG
    X, out = np.zeros((2, 2)), np.zeros((2, 2))
    assert lib.svgd_glm_logp_grad(h, None, 2, C.dptr(out)) == C.SVGD_ERR_ARG
    assert lib.svgd_glm_logp_grad(h, C.dptr(X), 2, None) == C.SVGD_ERR_ARG
    assert lib.svgd_glm_logp_grad(None, C.dptr(X), 2, C.dptr(out)) == C.SVGD_ERR_ARG
    assert lib.svgd_glm_logp(h, C.dptr(X), 2, None) == C.SVGD_ERR_ARG
    assert lib.svgd_glm_neg_hess_sum(h, C.dptr(X), 2, None) == C.SVGD_ERR_ARG
    lib.svgd_glm_destroy(h)


def test_python_api():
    A, y, X = R.case(3, 63, N, "logistic")
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
        S.GeneralizedLinearModel(A, y + 2.0)
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
        S.GeneralizedLinearModel(A, y, lik_scale=0.0)
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
        S.GeneralizedLinearModel(A, y, prior_prec=-1.0)
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
        S.GeneralizedLinearModel(A, y, link="probit")
    with pytest.raises(S.DimensionMismatchException, match=r"^SVGDCpp: \[Dimension Error\]"):
        S.GeneralizedLinearModel(A, y[:-1])
    with pytest.raises(S.DimensionMismatchException, match=r"^SVGDCpp: \[Dimension Error\]"):
        S.GeneralizedLinearModel(np.zeros((0, 3)), np.zeros(0))
    m = S.GeneralizedLinearModel(A, y)
    assert m._handle and m.batch_ == (0, 63) and m.dimension_ == 3
    with pytest.raises(ValueError, match=r"^SVGDCpp: \[Argument Error\]"):
        m.set_batch(60, 4)
    with pytest.raises(S.DimensionMismatchException):
        m.log_model_grad(np.zeros((2, 4)))
    m.set_batch(3, 60)
    G = m.log_model_grad(X)
    out = np.empty_like(X)
    assert m.log_model_grad(X, out=out) is out and np.array_equal(out, G)
    assert np.array_equal(m.EvaluateLogModelGrad(X[2]), G[2])
    assert m.EvaluateLogModel(X[1]) == m.log_model(X)[1]
    assert np.array_equal(m.EvaluateLogModelHessian(X[0]), -m.neg_hess_sum(X[:1]))
    m.Initialize()


def test_gradient_override_is_refused_before_any_c_call():
    from svgdcpp_amd.api import _builtin_glm, _builtin_grad

    class Tempered(S.GeneralizedLinearModel):
        def log_model_grad(self, X, out=None):
            return 0.5 * super().log_model_grad(X)

    class Plain(S.GeneralizedLinearModel):
        pass

    A, y, _ = R.case(3, 63, N, "logistic")
    assert _builtin_glm(S.GeneralizedLinearModel(A, y)) and _builtin_glm(Plain(A, y))
    assert not _builtin_glm(Tempered(A, y)) and not _builtin_grad(Plain(A, y))
    with pytest.raises(TypeError):
        ctx = object.__new__(S.Context)  # no context, no library handle: nothing in C can run
        S.Context.set_device_model(ctx, Tempered(A, y))
