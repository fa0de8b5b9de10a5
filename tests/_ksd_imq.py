"""References for the kernelized Stein discrepancy tests of both kernels.
TEST HELPER ONLY.

For scores s_i = grad log p(x_i), r = x_i - x_j, t = |r|^2:

    IMQ  k = (1 + a t)^(-1/2):  u_ij = k s_i.s_j + a k^3 (s_i - s_j).r + a d k^3 - 3 a^2 k^5 t
    RBF  k = exp(-a t):         u_ij = k [ s_i.s_j + 2a (s_i - s_j).r + 2ad - 4a^2 t ]
    row_i  = (1/N) sum_j u_ij
    KSD2_V = (1/N) sum_i row_i,   KSD2_U = (1/(N(N-1))) sum_{i != j} u_ij

by direct differences in np.longdouble (the 80-bit x87 format on x86-64),
in row chunks, sharing no arithmetic with the library: no centring, no Gram
form.

The bar of every comparison is BAR max(1, mean|u_ij|) with BAR = 1e-12 for V,
U and every row_i (a row's bar takes that row's mean) -- the IMQ phi bar of
tests/_imq.py, for the same reason: a reciprocal square root left at its seed
must not pass (a k off by a relative 1e-9 misses the row bar by 100x and more
on every cloud below but the a = 1e6 one, which the diagonal dominates).

edge_cases() are the clouds the bar was worked out on; emulate_device()
restates the device order in fp64 numpy (tests/test_ksd_imq_cpu.py keeps it at
a quarter of the bar on all of them).
"""
import functools

import numpy as np

import oracle
import _imq as Q

LD = np.longdouble
BAR = 1e-12


def _ref(X, G, a, imq):
    n, d = X.shape
    Xl, Gl, al = X.astype(LD), G.astype(LD), LD(a)
    rows, rabs = np.empty(n, LD), np.empty(n, LD)
    diag = (Gl * Gl).sum(1) + (al * d if imq else 2 * al * d)
    chunk = max(1, int(2e6) // (n * d))
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        r = Xl[i0:i1, None, :] - Xl[None, :, :]
        r2 = (r * r).sum(-1)
        ss = Gl[i0:i1] @ Gl.T
        dsr = ((Gl[i0:i1, None, :] - Gl[None, :, :]) * r).sum(-1)
        if imq:
            k = 1 / np.sqrt(1 + al * r2)
            k3 = k * k * k
            u = k * ss + al * k3 * dsr + al * d * k3 - 3 * al * al * k3 * k * k * r2
        else:
            u = np.exp(-al * r2) * (ss + 2 * al * dsr + 2 * al * d - 4 * al * al * r2)
        rows[i0:i1] = u.sum(1) / n
        rabs[i0:i1] = np.abs(u).sum(1) / n
    V = rows.sum() / n
    U = (rows.sum() * n - diag.sum()) / (LD(n) * (n - 1)) if n > 1 else LD(np.nan)
    return V, U, rows, float(rabs.mean()), rabs.astype(np.float64)


def ksd_imq_ref(X, G, a):
    """(V, U, rows, mean|u|, per-row mean|u|) of the IMQ statistic in longdouble."""
    return _ref(X, G, a, True)


def ksd_rbf_ref(X, G, a):
    """The same of the RBF statistic (the formula of tests/test_gpu_ksd.py)."""
    return _ref(X, G, a, False)


def errors(v, u, rows, ref):
    """(err V / bar, err U / bar, worst row err / its bar) against a reference
    tuple; err U is 0 where the reference's U is NaN (n = 1)."""
    V, U, R, mabs, rabs = ref
    bar = BAR * max(1.0, mabs)
    ev = abs(float(LD(v) - V)) / bar
    eu = 0.0 if np.isnan(float(U)) else abs(float(LD(u) - U)) / bar
    er = np.abs((np.asarray(rows).astype(LD) - R).astype(np.float64)) / (BAR * np.maximum(1.0, rabs))
    return ev, eu, float(er.max())


# ------------------------------------------------------------------ clouds --
def model(d, k=2, seed=7):
    """The 2-component Gaussian sum of tests/test_gpu_ksd.py (host gradient)."""
    import svgdcpp_amd as S

    mus = oracle.splitmix((k, d), 3.0, seed + d)
    return S.GaussianSum(list(mus), [np.eye(d) * (1.0 + 0.25 * c) for c in range(k)])


def scale(d):
    """X has scale 3: a typical pair lies at |r|^2 = 6 d, where k = 0.63."""
    return 1.0 / (4.0 * d)


def _edge(name):
    n, d = 300, 3
    seed = 50 + sorted(EDGE).index(name)
    X = oracle.splitmix((n, d), 3.0, seed)
    a = scale(d)
    if name == "shift1e3":
        G = model(d).log_model_grad(X)
        return X + 1.0e3, G, a
    if name == "shift1e6":
        G = model(d).log_model_grad(X)
        return X + 1.0e6, G, a
    if name == "outliers":
        X[0] += 1.0e4
        X[1] -= 1.0e4
        X[2] += np.array([1.0e4, -1.0e4, 0.0])
    elif name == "duplicates":
        X[5], X[9] = X[4], X[8]
    elif name == "aniso":
        # (the scale of this cloud's own distances: see the note at edge_case)
        X = X * np.array([1.0e3, 1.0, 1.0e-3])
        a = Q.median_a(X)
    elif name == "a1e6":
        a = 1.0e6
    elif name == "a1e-8":
        a = 1.0e-8
    elif name == "two_d8":
        n, d = 400, 8
        X = Q.two_clusters(n, d, seed)
        a = scale(d)
    return X, model(d).log_model_grad(X), a


EDGE = ("shift1e3", "shift1e6", "outliers", "duplicates", "aniso", "a1e6", "a1e-8", "two_d8")
GAUSS_DIMS = (1, 3, 8, 17, 64)


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(X, G, a, IMQ reference) of a named cloud, computed once; read-only arrays.

    a = 1 / (4 d) on the clouds of scale 3, and the median heuristic's
    ln N / med^2 on the anisotropic one, whose distances are 1000 times
    larger: the Gram form's r2 = n_i + n_j - 2 xc_i.xc_j carries an absolute
    error of about eps max|xc|^2, so k carries a relative a eps max|xc|^2 / 2,
    which stays below the bar while a is on the scale of the cloud's own
    distances (every scale method of the library) and does not for an a
    4e4 times that (a = 1/12 there: 1e-10; the emulation below is then 13
    bars off on a row)."""
    if name.startswith("gauss_d"):
        d = int(name[7:])
        X = Q.gaussian(515, d, 4300 + d)
        G, a = model(d).log_model_grad(X), scale(d)
    else:
        X, G, a = _edge(name)
    ref = ksd_imq_ref(X, G, a)
    for arr in (X, G, ref[2], ref[4]):
        arr.flags.writeable = False
    return X, G, a, ref


def edge_cases():
    return ["gauss_d%d" % d for d in GAUSS_DIMS] + list(EDGE)


# ---------------------------------------------- emulated device arithmetic --
def emulate_device(X, G, a, tile=64):
    """The device order in fp64 numpy: centred records with n_j = |xc_j|^2 and
    p_j = s_j.xc_j, per column tile the three Gram products xx, ss and
    cross = s_i.xc_j + xc_i.s_j, r2 = max(n_i + n_j - 2 xx, 0),
    k = (1 + a r2)^(-1/2), u = k ss + k^3 (a (p_i + d + p_j - cross) - 3 a^2 k^2 r2),
    the column j = i taken as |s_i|^2 + a d by index, row sums added in tile
    order.  Returns (V, U, rows)."""
    n, d = X.shape
    xc = X - X.mean(axis=0)
    nrm = (xc * xc).sum(axis=1)
    p = (G * xc).sum(axis=1)
    diag = (G * G).sum(axis=1) + a * d
    acc = np.zeros(n)
    for j0 in range(0, n, tile):
        xj, gj, nj, pj = xc[j0:j0 + tile], G[j0:j0 + tile], nrm[j0:j0 + tile], p[j0:j0 + tile]
        xx = xc @ xj.T
        ss = G @ gj.T
        cross = G @ xj.T + xc @ gj.T
        r2 = np.maximum(nrm[:, None] + nj[None, :] - 2.0 * xx, 0.0)
        k = 1.0 / np.sqrt(1.0 + a * r2)
        k2 = k * k
        u = k * ss + (k2 * k) * (a * (((p + d)[:, None] + pj[None, :]) - cross) - 3.0 * a * a * (k2 * r2))
        idx = np.arange(len(nj))
        u[j0 + idx, idx] = diag[j0 + idx]  # j = i
        acc += u.sum(axis=1)
    rows = acc / n
    sr, sd = rows.sum(), diag.sum()
    V = sr / n
    U = (n * sr - sd) / (n * (n - 1.0)) if n > 1 else np.nan
    return V, U, rows
