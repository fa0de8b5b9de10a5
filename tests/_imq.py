"""Reference for the inverse multiquadric (IMQ) kernel tests.  TEST HELPER ONLY.

    k(x, x')  = (1 + a |x - x'|^2)^(-1/2)
    grad_x' k = -a (x' - x) k^3
    phi_i     = (1/N) sum_j [ k_ij G_j + a k_ij^3 (x_i - x_j) ]

by direct differences in np.longdouble (the 80-bit x87 format on x86-64: eps
1.08e-19, asserted by tests/_clouds.py at import), sharing no arithmetic with
the library: no centring, no Gram form, no regrouping.

The bar of every phi comparison is BAR max(1, max|phi|) with BAR = 1e-12: a
reciprocal square root left at a hardware seed or one Newton step short lands
at 1e-10 .. 1e-11 and does not pass.

imq_clouds() are the seven clouds the bar was worked out on; emulate_device()
restates the device order in fp64 numpy (tests/test_imq_cpu.py keeps it at a
quarter of the bar on all of them).
"""
import functools

import numpy as np

import oracle
import _clouds as cl

LD = np.longdouble
BAR = 1e-12


def bar(phi_ref):
    return BAR * max(1.0, float(np.max(np.abs(phi_ref))))


def imq_k(x, y, a):
    """k(x, y) in long double."""
    diff = np.asarray(x, dtype=LD) - np.asarray(y, dtype=LD)
    return 1 / np.sqrt(1 + LD(a) * (diff @ diff))


def imq_grad(x, y, a):
    """grad_x k(x, y) = -a (x - y) k^3 in long double."""
    diff = np.asarray(x, dtype=LD) - np.asarray(y, dtype=LD)
    return -LD(a) * diff * imq_k(x, y, a) ** 3


def imq_phi(X, G, a, block=64):
    """phi (n, d) in long double, blocked by rows."""
    n, d = X.shape
    Xh, Gh, ah = X.astype(LD), G.astype(LD), LD(a)
    out = np.empty((n, d), dtype=LD)
    for i0 in range(0, n, block):
        diff = Xh[i0:i0 + block, None, :] - Xh[None, :, :]  # [i, j] = x_i - x_j
        K = 1 / np.sqrt(1 + ah * (diff * diff).sum(-1))
        out[i0:i0 + block] = (K @ Gh + ah * (diff * (K ** 3)[..., None]).sum(1)) / n
    return out


def imq_matrices(X, a):
    """(K, Kg) as SVGD logs them (SVGD.hpp:345-365): K[j, i] = k(x_j, x_i),
    Kg[j d:(j+1) d, i] = grad_{x_j} k(x_j, x_i); long double."""
    n, d = X.shape
    K = np.empty((n, n), dtype=LD)
    Kg = np.empty((d * n, n), dtype=LD)
    for i in range(n):
        for j in range(n):
            K[j, i] = imq_k(X[j], X[i], a)
            Kg[j * d:(j + 1) * d, i] = imq_grad(X[j], X[i], a)
    return K, Kg


def median_a(X):
    """a = ln N / med^2 from direct long-double differences (tests/_clouds.py)."""
    if X.shape[0] < 2:
        return 1.0
    _, med = cl.hp_stats(X)
    return float(np.log(LD(X.shape[0])) / (LD(med) * LD(med))) if med > 0 else 1.0


# ------------------------------------------------------------------ clouds --
def gaussian(n, d, seed):
    """Standard normal cloud from the splitmix uniforms (Box-Muller): the same
    bits on every machine."""
    u = oracle.splitmix((2, n * d), 0.5, seed) + 0.5  # (0, 1)
    u = np.clip(u, 2.0 ** -40, 1.0 - 2.0 ** -40)
    return (np.sqrt(-2.0 * np.log(u[0])) * np.cos(2.0 * np.pi * u[1])).reshape(n, d)


def two_clusters(n, d, seed, L=40.0):
    X = gaussian(n, d, seed)
    X[: n // 2, 0] += L
    return X


def aniso(n, d, seed):
    return gaussian(n, d, seed) * np.array([1e3, 1.0, 1e-3])[np.arange(d) % 3]


# name -> (n, d, generator): the clouds of the bar
CLOUDS = {
    "gauss_d64": (1000, 64, lambda n, d, s: gaussian(n, d, s)),
    "shift1e3": (1000, 64, lambda n, d, s: gaussian(n, d, s) + 1e3),
    "shift1e6": (1000, 64, lambda n, d, s: gaussian(n, d, s) + 1e6),
    "two_d8": (1000, 8, two_clusters),
    "aniso": (1000, 64, aniso),
    "d1": (1000, 1, lambda n, d, s: gaussian(n, d, s)),
    "d17": (1000, 17, lambda n, d, s: gaussian(n, d, s)),
}


@functools.lru_cache(maxsize=None)
def cloud_case(name, n=None):
    """(X, G, a, phi_ref) of a named cloud at its median a, computed once;
    read-only arrays."""
    n0, d, gen = CLOUDS[name]
    n = n0 if n is None else n
    seed = 4100 + 37 * sorted(CLOUDS).index(name)
    X = gen(n, d, seed)
    G = cl.gradients(n, d, seed)
    a = median_a(X)
    phi = imq_phi(X, G, a)
    for arr in (X, G, phi):
        arr.flags.writeable = False
    return X, G, a, phi


# ---------------------------------------------- emulated device arithmetic --
def emulate_device(X, G, a, tile=64):
    """The device order in fp64 numpy: centred records, n_j = |xc_j|^2, the
    Gram form s = 1 + a max(n_i + n_j - 2 xc_i.xc_j, 0), k = s^(-1/2), sums
    over column tiles added in tile order with the diagonal left out by index,
    phi = (1/N)(G_i + sum k G + a (xc_i sum k^3 - sum k^3 xc_j))."""
    n, d = X.shape
    xc = X - X.mean(axis=0)
    nrm = (xc * xc).sum(axis=1)
    sg = np.zeros((n, d))
    sx = np.zeros((n, d))
    s3 = np.zeros(n)
    for j0 in range(0, n, tile):
        xj, gj, nj = xc[j0:j0 + tile], G[j0:j0 + tile], nrm[j0:j0 + tile]
        r2 = np.maximum(nrm[:, None] + nj[None, :] - 2.0 * (xc @ xj.T), 0.0)
        k = 1.0 / np.sqrt(1.0 + a * r2)
        k[np.arange(j0, j0 + len(nj)), np.arange(len(nj))] = 0.0  # j = i
        k3 = k * k * k
        sg += k @ gj
        sx += k3 @ xj
        s3 += k3.sum(axis=1)
    return (G + sg + a * (xc * s3[:, None] - sx)) / n
