"""Reference and error bars of the GLM posterior-prediction tests
(test_glm_predict_cpu.py, test_gpu_glm_predict.py).  The reference is the
definition in np.longdouble, uncentred and straight from the formulas; nothing
here comes from the library or the oracle.

    z_im   = a_m . theta_i,   mu = sigma (logistic) or the identity (gaussian)
    mean_m = (1/N) sum_i mu(z_im)
    var_m  = (1/N) sum_i (mu(z_im) - mean_m)^2
    lpd_m  = log (1/N) sum_i p(y_m | z_im)
      logistic  p = exp(y z - log(1 + e^z))
      gaussian  p = sqrt(s / 2 pi) exp(-s (y - z)^2 / 2)

Bars.  With T_im = |a_m| . |theta_i| (the magnitude sum of z_im's terms) and
Tbar_m = |a_m| . |theta_bar|:

    quantity   logistic                              gaussian
    mean       1e-13 (1 + mean_i T)                  1e-13 (mean_i T + Tbar)
    var        1e-13 (1 + mean_i T)                  1e-13 mean_i (T + Tbar)^2
    lpd        2e-13 (1 + (1 + |y|) max_i T)         2e-13 (1 + s max_i (|y| + T)^2 / 2)

Derivation.  fp64 rounding of z is a few eps T; |sigma'| <= 1/4 turns it into
an error in mu no larger, on top of mu's own roundings (|mu| <= 1: the "1 +").
For the Gaussian link mu = z, and the centred sum adds roundings of size
eps (T + Tbar).  The variance is a mean of squares of (mu - c): its terms are
bounded by 1 (logistic) and by (T + Tbar)^2 (gaussian).  lpd is the log of a
mean of p = exp(l): an absolute error dl in the exponent is a relative error
in p, hence an absolute one in lpd, and |l| <= (1 + |y|) |z| + log 2 (logistic)
or s (|y| + |z|)^2 / 2 (gaussian) -- the largest exponent any particle's term
can carry, hence max_i.  Plain fp64 numpy implementing the centred sums in two
particle orders, on tests/_glm.py::case for d in {1, 3, 8, 17, 55, 64} and
(N, M) in {(129, 1000), (1000, 300), (4097, 129)}, stays within 0.0016 of the
mean bar, 0.0025 (logistic) / 0.046 (gaussian) of the var bar and 0.024 of the
lpd bar in its 1e-13 form.  The device's table exponential adds at most
2.6e-14 relative per exp: <= 0.25 * 2.6e-14 on sigma, and <= 5.2e-14 absolute
on lpd with its two exps -- which is why lpd gets 2e-13 (about 3.5x left).
On that generator every reference lpd is finite (min -0.92 logistic, -4.2
gaussian at s = 0.7): no case is skipped for non-finite values.
"""
import functools

import numpy as np

import _glm as R

LD = np.longdouble
S_LIK = 0.7
LINKS = ["logistic", "gaussian"]


def reference(A, y, X, link, s=S_LIK):
    """(mean, var, lpd) in long double; lpd is None without y."""
    Z = X.astype(LD) @ A.astype(LD).T                       # (N, m)
    mu = R._sigmoid(Z) if link == "logistic" else Z
    mean = mu.mean(axis=0)
    var = ((mu - mean[None, :]) ** 2).mean(axis=0)
    if y is None:
        return mean, var, None
    yl = y.astype(LD)[None, :]
    with np.errstate(divide="ignore", under="ignore"):
        if link == "logistic":
            p = np.exp(yl * Z - (np.maximum(Z, 0) + np.log1p(np.exp(-np.abs(Z)))))
        else:
            p = np.sqrt(LD(s) / (2 * LD(np.pi))) * np.exp(-LD(s) * (yl - Z) ** 2 / 2)
        lpd = np.log(p.mean(axis=0))
    return mean, var, lpd


def bars(A, y, X, link, s=S_LIK):
    """(mean bar, var bar, lpd bar) per record (fp64 is plenty for a magnitude)."""
    T = np.abs(X) @ np.abs(A).T                             # (N, m)
    Tbar = np.abs(A) @ np.abs(X.mean(axis=0))
    if link == "logistic":
        bm = 1e-13 * (1 + T.mean(axis=0))
        bv = bm.copy()
    else:
        bm = 1e-13 * (T.mean(axis=0) + Tbar)
        bv = 1e-13 * ((T + Tbar[None, :]) ** 2).mean(axis=0)
    if y is None:
        return bm, bv, None
    ya = np.abs(y)
    if link == "logistic":
        bl = 2e-13 * (1 + (1 + ya) * T.max(axis=0))
    else:
        bl = 2e-13 * (1 + s * ((ya[None, :] + T) ** 2).max(axis=0) / 2)
    return bm, bv, bl


def excesses(out, ref, bar):
    """max |out - ref| / bar for each of the quantities present (<= 1 passes)."""
    return tuple(R.excess(o, r, b) for o, r, b in zip(out, ref, bar) if r is not None)


@functools.lru_cache(maxsize=None)
def case(d, N, M, link, seed=7):
    """One generated problem (tests/_glm.py::case: the M data rows are the test
    rows) with its reference and bars, computed once and shared (read-only)."""
    A, y, X = R.case(d, M, N, link, seed)
    ref = reference(A, y, X, link)
    bar = bars(A, y, X, link)
    for a in ref + bar:
        a.setflags(write=False)
    return A, y, X, ref, bar
