"""Reference for the maximum mean discrepancy tests of both kernels.
TEST HELPER ONLY.

For the particles X (N, d), the sample Y (M, d) and t = |x - y|^2:

    RBF  k = exp(-a t)             IMQ  k = (1 + a t)^(-1/2)
    Sxx = sum_{i,j<N} k(x_i, x_j)  Syy = sum_{i,j<M} k(y_i, y_j)  (the diagonal counts 1 each)
    Sxy = sum_{i<N} sum_{j<M} k(x_i, y_j)
    mean_xx = Sxx / N^2, mean_yy = Syy / M^2, mean_xy = Sxy / (N M)
    V = mean_xx + mean_yy - 2 mean_xy
    U = (Sxx - N) / (N (N - 1)) + (Syy - M) / (M (M - 1)) - 2 mean_xy   (NaN if N < 2 or M < 2)
    wit_i = (1/N) sum_j k(x_i, x_j) - (1/M) sum_j k(x_i, y_j)

by direct differences in np.longdouble (the 80-bit x87 format on x86-64), in
row chunks, sharing no arithmetic with the library: no centring, no Gram
form.  The bar of every comparison is BAR = 1e-12 absolute (|k| <= 1) on the
three means, V, U and every witness row.

emulate_device() restates the device order in fp64 numpy: both sets centred
on the particles' mean, r2 = max(n_i + n_j - 2 x~_i.z~_j, 0) per column tile,
the column j = i of a same-set pass taken as 1 by index, row sums added in
tile order.
"""
import numpy as np

import oracle

LD = np.longdouble
BAR = 1e-12
KERNELS = ("rbf", "imq")

assert np.finfo(LD).eps < 1e-18, "the reference needs an 80-bit (or wider) long double"


def _row_sums(A, B, a, imq, same):
    """sum_j k(a_i, b_j) in longdouble; same: j = i counts exactly 1."""
    na, d = A.shape
    Al, Bl, al = A.astype(LD), B.astype(LD), LD(a)
    out = np.empty(na, LD)
    chunk = max(1, int(2e6) // (B.shape[0] * d))
    for i0 in range(0, na, chunk):
        i1 = min(na, i0 + chunk)
        r = Al[i0:i1, None, :] - Bl[None, :, :]
        t = (r * r).sum(-1)
        k = 1 / np.sqrt(1 + al * t) if imq else np.exp(-al * t)
        if same:
            idx = np.arange(i0, i1)
            k[idx - i0, idx] = 1
        out[i0:i1] = k.sum(1)
    return out


def scalars(sxx, sxy, syy, n, m):
    """(means3, V, U) from the three sums, in the definition's order."""
    T = type(sxx)
    N, M = T(n), T(m)
    mxx, myy, mxy = sxx / (N * N), syy / (M * M), sxy / (N * M)
    V = mxx + myy - 2 * mxy
    U = (sxx - N) / (N * (N - 1)) + (syy - M) / (M * (M - 1)) - 2 * mxy if n > 1 and m > 1 else T(np.nan)
    return np.array([mxx, myy, mxy]), V, U


def mmd_ref(X, Y, a, kernel):
    """(means3, V, U, witness) of the definition in longdouble."""
    imq = kernel == "imq"
    n, m = X.shape[0], Y.shape[0]
    rxx, rxy = _row_sums(X, X, a, imq, True), _row_sums(X, Y, a, imq, False)
    ryy = _row_sums(Y, Y, a, imq, True)
    means, V, U = scalars(rxx.sum(), rxy.sum(), ryy.sum(), n, m)
    return means, V, U, rxx / n - rxy / m


def errors(v, u, means, wit, ref):
    """(err V, err U, worst mean err, worst witness err) / BAR against a
    reference tuple; both U NaN counts 0, one of them NaN counts inf; wit None
    counts 0."""
    M3, V, U, W = ref
    ev = abs(float(LD(v) - V)) / BAR
    if np.isnan(float(U)) or np.isnan(u):
        eu = 0.0 if np.isnan(float(U)) and np.isnan(u) else np.inf
    else:
        eu = abs(float(LD(u) - U)) / BAR
    em = float(np.abs((np.asarray(means).astype(LD) - M3).astype(np.float64)).max()) / BAR
    ew = 0.0 if wit is None else float(np.abs((np.asarray(wit).astype(LD) - W).astype(np.float64)).max()) / BAR
    return ev, eu, em, ew


# ------------------------------------------------------------------ clouds --
def scale(n, d, s=3.0):
    """About ln N / med^2 of a uniform cube of half-width s: a pair's squared
    distance has mean 2 d s^2 / 3, near its median."""
    return float(np.log(max(n, 2)) / (2.0 * d * s * s / 3.0))


def clouds(n, m, d, seed):
    """X: a uniform cube of half-width 3; Y: a narrower one, off centre."""
    X = oracle.splitmix((n, d), 3.0, seed)
    Y = oracle.splitmix((m, d), 2.4, seed + 7919) + 0.5
    return X, Y


def edge(name, d):
    """(X, Y, a) of a named edge input at (300, 200, d)."""
    n, m = 300, 200
    X, Y = clouds(n, m, d, 60 + d + sorted(EDGE).index(name))
    a = scale(n, d)
    if name == "shift1e3":
        X, Y = X + 1.0e3, Y + 1.0e3
    elif name == "shift1e6":
        X, Y = X + 1.0e6, Y + 1.0e6
    elif name == "duplicates":
        X[5], X[9], Y[3], Y[150] = X[4], X[8], Y[2], Y[149]
    elif name == "two_clusters":
        X[: n // 2, 0] += 40.0
        Y[: m // 3, 0] += 40.0
    elif name == "disjoint":
        # 50 standard deviations of the cube (3 / sqrt(3)) along every coordinate
        Y = Y + 50.0 * 3.0 / np.sqrt(3.0)
    elif name == "a1e6":
        a = 1.0e6
    elif name == "a1e-8":
        a = 1.0e-8
    else:
        raise ValueError(name)
    return X, Y, a


EDGE = ("shift1e3", "shift1e6", "duplicates", "two_clusters", "disjoint", "a1e6", "a1e-8")
EDGE_DIMS = (3, 17)


# ---------------------------------------------- emulated device arithmetic --
def emulate_device(X, Y, a, kernel, tile=64):
    """The device order in fp64 numpy.  Returns (means3, V, U, witness)."""
    imq = kernel == "imq"
    n, m = X.shape[0], Y.shape[0]
    mu = X.sum(axis=0) / n
    xc, yc = X - mu, Y - mu
    nx, ny = (xc * xc).sum(axis=1), (yc * yc).sum(axis=1)

    def rows(A, na_, B, nb_, same):
        acc = np.zeros(A.shape[0])
        for j0 in range(0, B.shape[0], tile):
            bj, nj = B[j0:j0 + tile], nb_[j0:j0 + tile]
            r2 = np.maximum(na_[:, None] + nj[None, :] - 2.0 * (A @ bj.T), 0.0)
            k = 1.0 / np.sqrt(1.0 + a * r2) if imq else np.exp(-(a * r2))
            if same:
                idx = np.arange(len(nj))
                k[j0 + idx, idx] = 1.0
            acc += k.sum(axis=1)
        return acc

    rxx, rxy, ryy = rows(xc, nx, xc, nx, True), rows(xc, nx, yc, ny, False), rows(yc, ny, yc, ny, True)
    means, V, U = scalars(np.float64(rxx.sum()), np.float64(rxy.sum()), np.float64(ryy.sum()), n, m)
    return means, V, U, rxx / n - rxy / m
