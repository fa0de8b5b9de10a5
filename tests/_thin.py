"""References for the Stein thinning tests (svgd_stein_thin,
svgd_stein_thin_host).  TEST HELPER ONLY.

With u_ij, u_ii of tests/_ksd_imq.py (u_ii = |s_i|^2 + a d for the IMQ kernel,
|s_i|^2 + 2 a d for the RBF one, taken by index):

    acc_0[j] = 0
    for t = 1..m:
        obj_t[j] = u_jj / 2 + acc_{t-1}[j]
        pi_t     = the smallest j that attains min_j obj_t[j]
        S_t      = S_{t-1} + 2 acc_{t-1}[pi_t] + u_{pi_t pi_t}
        ksd2_t   = S_t / t^2
        acc_t[j] = acc_{t-1}[j] + u(pi_t, j)

in np.longdouble by direct differences, sharing no arithmetic with the
library.  replay() runs it along a given pick sequence (the definition's own
when none is given) and returns, per pick, the objective vector, the gap
between the best and the second-best distinct objective, ksd2_t,

    bar_t = BAR max(1, max_j (u_jj / 2 + sum_{s<t} |u(pi_s, j)|))

and the mean |u| over the picked t x t block.  BAR = 1e-12 is the project's
IMQ KSD bar (_ksd_imq.BAR), for the same reason: a reciprocal square root left
at its seed must not pass.

Two criteria (check_valid, same_picks_allowed):
 1. valid pick: along the candidate's own prefix, at every t
    obj_t[pi_t] <= min_j obj_t[j] + bar_t and
    |ksd2_t - ksd2_t^ref(prefix)| <= BAR max(1, mean |u| over the t x t block);
 2. same picks as the definition: asserted only where the reference alone
    shows min_t gap_t / bar_t >= GAP_BARS.

emulate_device() restates the device order in fp64 numpy.
"""
import numpy as np

import _ksd_imq as K

LD = np.longdouble
BAR = K.BAR
GAP_BARS = 1e3


def _u_row(Xl, Gl, al, imq, diag, i):
    """u(i, j) for all j in longdouble; u(i, i) = diag[i] by index."""
    d = Xl.shape[1]
    r = Xl[i][None, :] - Xl
    t = (r * r).sum(1)
    ss = Gl @ Gl[i]
    sr = ((Gl[i][None, :] - Gl) * r).sum(1)
    if imq:
        k = 1 / np.sqrt(1 + al * t)
        k3 = k * k * k
        u = k * ss + al * k3 * sr + al * d * k3 - 3 * al * al * k3 * k * k * t
    else:
        u = np.exp(-al * t) * (ss + 2 * al * sr + 2 * al * d - 4 * al * al * t)
    u[i] = diag[i]
    return u


def replay(X, G, a, kernel, m, prefix=None, keep_obj=True):
    """The definition in longdouble along `prefix` (m picks; None: the
    definition's own argmin).  Returns a dict of per-pick lists / arrays:
    idx, obj (the objective vectors, when keep_obj), omin, gap, ksd2, bar,
    mabs (mean |u| over the picked t x t block)."""
    imq = kernel == "imq"
    n, d = X.shape
    Xl, Gl, al = X.astype(LD), G.astype(LD), LD(a)
    diag = (Gl * Gl).sum(1) + (al * d if imq else 2 * al * d)
    acc, aabs = np.zeros(n, LD), np.zeros(n, LD)
    S, Sabs = LD(0), LD(0)
    out = {"idx": np.empty(m, np.int64), "obj": [], "omin": np.empty(m, LD), "gap": np.empty(m),
           "ksd2": np.empty(m, LD), "bar": np.empty(m), "mabs": np.empty(m)}
    for t in range(1, m + 1):
        obj = diag / 2 + acc
        omin = obj.min()
        pi = int(np.argmin(obj)) if prefix is None else int(prefix[t - 1])
        rest = obj[obj != omin]
        out["gap"][t - 1] = float(rest.min() - omin) if rest.size else np.inf
        out["bar"][t - 1] = BAR * max(1.0, float((np.abs(diag) / 2 + aabs).max()))
        S = S + 2 * acc[pi] + diag[pi]
        Sabs = Sabs + 2 * aabs[pi] + abs(diag[pi])
        out["idx"][t - 1] = pi
        out["omin"][t - 1] = omin
        out["ksd2"][t - 1] = S / (LD(t) * t)
        out["mabs"][t - 1] = float(Sabs / (LD(t) * t))
        if keep_obj:
            out["obj"].append(obj)
        u = _u_row(Xl, Gl, al, imq, diag, pi)
        acc = acc + u
        aabs = aabs + np.abs(u)
    return out


def check_valid(X, G, a, kernel, idx, ksd2):
    """Criterion 1 for a candidate (idx, ksd2): (worst (obj_t[pi_t] - min) /
    bar_t, worst |ksd2_t - ref| / its bar), both <= 1 for a valid selection."""
    idx = np.asarray(idx)
    assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < X.shape[0]
    r = replay(X, G, a, kernel, len(idx), prefix=idx)
    eo = max(float(r["obj"][t][idx[t]] - r["omin"][t]) / r["bar"][t] for t in range(len(idx)))
    ek = float(np.max(np.abs((np.asarray(ksd2).astype(LD) - r["ksd2"]).astype(np.float64))
                      / (BAR * np.maximum(1.0, r["mabs"]))))
    return eo, ek


def gap_bars(ref):
    """min over the picks of gap_t / bar_t of a replay() of the definition."""
    return float(np.min(ref["gap"] / ref["bar"]))


def case(oracle, n, d, seed):
    """A uniform cloud of scale 3 with the 2-component Gaussian-sum score of
    _ksd_imq.model and the scale 1 / (4 d)."""
    X = oracle.splitmix((n, d), 3.0, seed)
    return X, K.model(d).log_model_grad(X), K.scale(d)


def emulate_device(X, G, a, kernel, m):
    """The device order (svgd_thin.hip) in fp64 numpy: t, s_pi.s_j and
    (s_pi - s_j).r accumulated over the coordinates in order, k, u with u_jj by
    index, acc += u, obj = u_jj / 2 + acc, the lowest index of the minimum,
    S += 2 acc[pi] + u_pipi.  Returns (idx, ksd2)."""
    imq = kernel == "imq"
    n, d = X.shape
    diag = np.zeros(n)
    for c in range(d):
        diag = diag + G[:, c] * G[:, c]
    diag = diag + (a * d if imq else 2.0 * a * d)
    acc = np.zeros(n)
    idx, ksd2 = np.empty(m, np.int64), np.empty(m)
    S = 0.0
    obj = 0.5 * diag
    for p in range(m):
        pi = int(np.argmin(np.where(np.isnan(obj), np.inf, obj)))
        idx[p] = pi
        S = S + (2.0 * acc[pi] + diag[pi])
        ksd2[p] = S / (float(p + 1) * float(p + 1))
        t, ss, sr = np.zeros(n), np.zeros(n), np.zeros(n)
        for c in range(d):
            r = X[pi, c] - X[:, c]
            t = t + r * r
            ss = ss + G[pi, c] * G[:, c]
            sr = sr + (G[pi, c] - G[:, c]) * r
        if imq:
            k = 1.0 / np.sqrt(np.minimum(1.0 + a * t, 1e300))
            k2 = k * k
            u = k * ss + (k2 * k) * (a * (sr + d) - 3.0 * a * a * (k2 * t))
        else:
            u = np.exp(-a * t) * ((ss + 2.0 * a * sr) + (2.0 * a * d - 4.0 * a * a * t))
        u[pi] = diag[pi]
        acc = acc + u
        obj = 0.5 * diag + acc
    return idx, ksd2
