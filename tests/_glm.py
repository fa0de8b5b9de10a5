"""Reference, generator and error bar of the generalized-linear-model tests
(test_glm_cpu.py, test_gpu_glm.py).  The reference is the definition in
np.longdouble; nothing here comes from the oracle.

    z_im = a_m . theta_i
    G_i  = s (M/B) sum_{m in window} r(y_m, z_im) a_m - lambda theta_i
    r    = y - sigma(z) (logistic),  r = y - z (gaussian)

Bar.  Per element (i, k): bar_ik = 1e-13 * scale_ik with
    logistic  scale = s (M/B) sum_m |a_mk| + lambda |theta_ik|
    gaussian  scale = s (M/B) sum_m (|y_m| + |a_m| . |theta_i|) |a_mk| + lambda |theta_ik|
(the sum of the magnitudes of the terms: |r| <= 1 for the logistic link).
Plain fp64 numpy in two summation orders stays within 3.9e-15 of that scale
for d in {1, 3, 8, 17, 55, 64} and M up to 4097 on this generator, and the
device's table exp adds at most 0.25 * 2.6e-14 per term (sigma' <= 1/4):
about 1.1e-14 together, which leaves roughly 9x.
"""
import functools

import numpy as np

LD = np.longdouble
BAR = 1e-13


def generate(d, M, N, link, seed):
    """A uniform in (-1, 1), theta uniform in (-2, 2) * 4 / sqrt(d) (|z| <~ 14),
    y Bernoulli(1/2) (logistic) or uniform (-3, 3) (gaussian)."""
    rng = np.random.default_rng([seed, d, M, N, 0 if link == "logistic" else 1])
    A = rng.uniform(-1.0, 1.0, (M, d))
    X = rng.uniform(-2.0, 2.0, (N, d)) * (4.0 / np.sqrt(d))
    y = (rng.integers(0, 2, M).astype(np.float64) if link == "logistic"
         else rng.uniform(-3.0, 3.0, M))
    return np.ascontiguousarray(A), y, np.ascontiguousarray(X)


def _window(A, y, m0, count):
    M = A.shape[0]
    if count is None:
        m0, count = 0, M
    return A[m0:m0 + count].astype(LD), y[m0:m0 + count].astype(LD), LD(M) / LD(count)


def _sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1 / (1 + e), e / (1 + e))


def ref_grad(A, y, X, link, s=1.0, lam=1.0, m0=0, count=None):
    Aw, yw, f = _window(A, y, m0, count)
    Xl = X.astype(LD)
    Z = Xl @ Aw.T
    R = yw[None, :] - (_sigmoid(Z) if link == "logistic" else Z)
    return LD(s) * f * (R @ Aw) - LD(lam) * Xl


def ref_logp(A, y, X, link, s=1.0, lam=1.0, m0=0, count=None):
    Aw, yw, f = _window(A, y, m0, count)
    Xl = X.astype(LD)
    Z = Xl @ Aw.T
    if link == "logistic":
        L = yw[None, :] * Z - (np.maximum(Z, 0) + np.log1p(np.exp(-np.abs(Z))))
    else:
        L = -(yw[None, :] - Z) ** 2 / 2
    return LD(s) * f * L.sum(axis=1) - LD(lam) / 2 * (Xl * Xl).sum(axis=1)


def ref_neg_hess_sum(A, y, X, link, s=1.0, lam=1.0, m0=0, count=None):
    Aw, yw, f = _window(A, y, m0, count)
    Xl = X.astype(LD)
    if link == "logistic":
        sg = _sigmoid(Xl @ Aw.T)
        W = (sg * (1 - sg)).sum(axis=0)
    else:
        W = np.full(Aw.shape[0], LD(X.shape[0]))
    return LD(s) * f * ((Aw * W[:, None]).T @ Aw) + LD(lam) * X.shape[0] * np.eye(A.shape[1], dtype=LD)


def grad_scale(A, y, X, link, s=1.0, lam=1.0, m0=0, count=None):
    """scale_ik of the bar (fp64 is plenty for a magnitude)."""
    M = A.shape[0]
    if count is None:
        m0, count = 0, M
    Aw, yw = np.abs(A[m0:m0 + count]), np.abs(y[m0:m0 + count])
    f = s * M / count
    if link == "logistic":
        data = np.broadcast_to(f * Aw.sum(axis=0), X.shape)
    else:
        data = f * ((yw[None, :] + np.abs(X) @ Aw.T) @ Aw)
    return data + lam * np.abs(X)


def grad_bar(*args, **kw):
    return BAR * grad_scale(*args, **kw)


def excess(G, ref, bar):
    """max over elements of |G - ref| / bar (<= 1 passes); an all-zero bar
    element (all-zero data column, lambda = 0) must be met exactly."""
    err = np.abs(G.astype(LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    return float(q.max()) if q.size else 0.0


@functools.lru_cache(maxsize=None)
def case(d, M, N, link, seed=7):
    """One generated problem with its full-window reference, computed once and
    shared (the arrays are read-only)."""
    A, y, X = generate(d, M, N, link, seed)
    for a in (A, y, X):
        a.setflags(write=False)
    return A, y, X
