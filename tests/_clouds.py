"""Clustered, shifted and anisotropic particle clouds, and a reference for
them that shares no arithmetic with the oracle's median.  TEST HELPER ONLY.

Almost every other test draws its particles from oracle.splitmix, a centred
uniform cube.  SVGD on a mixture target leaves the particles in separated
clusters, far from the origin, with a different spread per coordinate: the
pair-distance list is then bimodal, with an empty gap that the two averaged
order statistics of an even n can straddle.  cloud() builds such inputs, all
from oracle.splitmix, so every machine gets the same bits.

The reference takes direct differences x_i - x_j in np.longdouble (the
80-bit x87 format on x86-64: eps 1.08e-19; asserted at import).  oracle.median_scale cannot serve off-centre: it
restates the reference's uncentred Gram form (GaussianRBFKernel.hpp:164-188)
and loses about 2^-53 |x|^2 / med^2 (relative error 6.6e-5 on a unit cloud at
offset 1e6, 3.8e-5 on two clusters of spread 1e-6 that are 1 apart).  The
device centres first and is better than the oracle there.  oracle.phi uses
direct differences and agrees with hp_phi to rounding (tests/test_clouds_cpu.py).

Above n^2 d = HP_MAX_WORK the same direct form runs in fp64, so that no test
spends more than a few seconds on the CPU: (d + 2) 2^-53 relative per key,
which is up to 2 (d + 2) 2^-53 of |xc_i|^2 + |xc_j|^2 -- a third of the fp64
key bound at d = 2 (7.7 of 24 units observed at n = 2049), so every fp64 key
test at d <= 16 (n <= 2050) stays on the long-double side; the fp64 form
serves d = 40 at n = 2049 / 2050 (bound 176 units), the F32 bars and the
order statistics of the n = 6000 trajectories.

Kinds (every cluster translation along coordinate 0; the first
round(frac n) rows are the translated cluster, so clusters are contiguous in
row order):

  uniform      splitmix(s = 1), the control
  bal          two clusters, frac 0.5, L = 40, s = 1
  c6040        frac 0.6, L = 40   (a log2e max|xc|^2 > 300 at d = 8)
  c6040_near   frac 0.6, L = 10   (about 46: the symmetric pass proper)
  shift1e3     uniform + 1e3 in every coordinate
  shift1e6     uniform + 1e6 in every coordinate
  aniso        uniform x (1e3, 1, 1e-3, 1e3, 1, 1e-3, ...) per coordinate
  tight        frac 0.6, L = 1, s = 1e-6   (keys and median only: a ~ 1e12)
  tight1e3     tight + 1e3 in every coordinate

The L above are the values the tests settled on; none had to be halved.
tests/test_clouds_cpu.py keeps a numpy emulation of the device arithmetic at
a quarter of every bar on every shape the GPU tests use, with two exceptions
that no change of input can lift (the control has them too) and that its
docstring works out: the fp64 key bar at d = 2 and the F32 key bar.  round()
is Python's (half to even): bal at n = 401 moves 200 rows, at 777 388.
"""
import functools

import numpy as np

import oracle

assert np.finfo(np.longdouble).eps < 1e-18, "the reference needs an 80-bit (or wider) long double"

LD = np.longdouble
HP_MAX_WORK = 2050 * 2050 * 16  # n^2 d above which the direct form runs in fp64

# kind -> (frac, L, s, offset)
_TWO = {
    "bal": (0.5, 40.0, 1.0, 0.0),
    "c6040": (0.6, 40.0, 1.0, 0.0),
    "c6040_near": (0.6, 10.0, 1.0, 0.0),
    "tight": (0.6, 1.0, 1e-6, 0.0),
    "tight1e3": (0.6, 1.0, 1e-6, 1e3),
}
_SHIFT = {"shift1e3": 1e3, "shift1e6": 1e6}
KINDS = ("uniform", "bal", "c6040", "c6040_near", "shift1e3", "shift1e6", "aniso", "tight", "tight1e3")
PHI_KINDS = tuple(k for k in KINDS if not k.startswith("tight"))
F32_PHI_KINDS = ("uniform", "shift1e3", "shift1e6", "aniso", "c6040_near")


# The shapes of tests/test_gpu_clouds.py, shared with tests/test_clouds_cpu.py
# (which keeps every one of them at a quarter of its bar on the CPU).
DIRECT_N = (400, 401)
DIRECT_D64 = (2, 5, 8, 12, 40)
DIRECT_D32 = (7, 20, 64)
BRACKET_N64 = (1000, 2049, 2050)
BRACKET_D64 = (2, 5, 8, 12, 40)
BRACKET_N32 = (1000, 2050)
BRACKET_D32 = (7, 20, 64)
FALLBACK_N = 400
FALLBACK_D64 = (5, 12, 24, 50)  # k_pair_rows R = 4 and 2, k_pair_tiles KP = 32 and 64
FALLBACK_D32 = (3, 7, 10, 14, 20, 64)  # KP = 4, 8, 12, 16, 32, 64
FALLBACK_KINDS = ("bal", "tight", "tight1e3")
BUCKET_SHAPE = (2050, 5)
BUCKET_KINDS = ("bal", "c6040")
TRAJ_N = 6000
TRAJ_D = (2, 8)
TRAJ_KINDS = ("bal", "c6040")
PHI_ROWS = ((777, 3), (777, 12))
PHI_TILES = ((333, 24), (333, 50))
PHI_SYM = ((1700, 8), (4200, 2))
PHI_F32 = ((333, 6), (333, 14), (333, 24), (333, 64))


def key_shapes(kind, f32):
    """Every (n, d) at which the GPU tests take keys or a median of `kind`."""
    if f32:
        s = [(n, d) for n in DIRECT_N for d in DIRECT_D32] + [(n, d) for n in BRACKET_N32 for d in BRACKET_D32]
        if kind in FALLBACK_KINDS:
            s += [(FALLBACK_N, d) for d in FALLBACK_D32]
    else:
        s = [(n, d) for n in DIRECT_N for d in DIRECT_D64] + [(n, d) for n in BRACKET_N64 for d in BRACKET_D64]
        if kind in FALLBACK_KINDS:
            s += [(FALLBACK_N, d) for d in FALLBACK_D64]
        if kind in BUCKET_KINDS:
            s.append(BUCKET_SHAPE)
        if kind in TRAJ_KINDS:
            s += [(TRAJ_N, d) for d in TRAJ_D]
    return sorted(set(s))


def split(kind, n):
    """(rows of the translated cluster, L); (0, 0.0) for a one-cluster kind."""
    if kind not in _TWO:
        return 0, 0.0
    frac, L, _, _ = _TWO[kind]
    return int(round(frac * n)), L


def cloud(kind, n, d, seed):
    if kind in _TWO:
        frac, L, s, off = _TWO[kind]
        X = oracle.splitmix((n, d), s, seed)
        X[:int(round(frac * n)), 0] += L
        return X + off if off else X
    X = oracle.splitmix((n, d), 1.0, seed)
    if kind == "uniform":
        return X
    if kind in _SHIFT:
        return X + _SHIFT[kind]
    if kind == "aniso":
        return X * np.array([1e3, 1.0, 1e-3])[np.arange(d) % 3]
    raise ValueError(kind)


def gradients(n, d, seed):
    """The G of the phi tests: centred uniform in [-8, 8], independent of X.
    At d = 64 the median heuristic leaves K_ij ~ e^-6 off the diagonal, so
    phi_i is close to G_i / N: the scale keeps max|phi| above 0.01 there."""
    return oracle.splitmix((n, d), 8.0, seed + 0x9E37)


# ------------------------------------------------------------- reference ----
def _work_type(n, d):
    return LD if n * n * d <= HP_MAX_WORK else np.float64


def hp_keys(X):
    """Upper-triangle squared distances sum_k (x_ik - x_jk)^2, i < j, in
    np.triu_indices(n, 1) order, from direct differences."""
    n, d = X.shape
    T = _work_type(n, d)
    Xh = X.astype(T)
    out = np.empty(n * (n - 1) // 2, dtype=T)
    pos = 0
    for i in range(n - 1):
        diff = Xh[i + 1:] - Xh[i]
        out[pos:pos + n - 1 - i] = (diff * diff).sum(axis=1)
        pos += n - 1 - i
    return out


def full_list_ranks(n):
    """The upper-list ranks behind the reference's median of all n^2 distances
    (n diagonal zeros, every pair twice): -1 stands for a diagonal zero."""
    tot = n * n
    idx = (tot // 2 - 1, tot // 2) if tot % 2 == 0 else (tot // 2,)
    return tuple(-1 if k < n else (k - n) // 2 for k in idx)


def stats_of_keys(keys, n):
    """((squared order statistics), med) of the full n^2 list from the
    upper-triangle squared distances."""
    ranks = full_list_ranks(n)
    want = sorted({r for r in ranks if r >= 0})
    part = np.partition(keys, want) if want else keys
    sq = tuple(keys.dtype.type(0) if r < 0 else part[r] for r in ranks)
    med = sum(np.sqrt(LD(s)) for s in sq) / len(sq)
    return sq, float(med)


def hp_stats(X):
    return stats_of_keys(hp_keys(X), X.shape[0])


def hp_phi(X, G, a, block=64):
    """phi_hat = (1/N)(G K + [I..I] Kg) (SVGD.hpp:453), K_ij = exp(-a |x_j - x_i|^2),
    Kg_ij = -2 a (x_j - x_i) K_ij, blocked by rows."""
    n, d = X.shape
    T = _work_type(n, d)
    Xh, Gh, ah = X.astype(T), G.astype(T), T(a)
    out = np.empty((n, d), dtype=T)
    for i0 in range(0, n, block):
        diff = Xh[None, :, :] - Xh[i0:i0 + block, None, :]  # [i, j] = x_j - x_i
        K = np.exp(-ah * (diff * diff).sum(-1))
        out[i0:i0 + block] = (K @ Gh - 2 * ah * (diff * K[..., None]).sum(1)) / n
    return out


def centred(X):
    """(xc, |xc|^2) with the mean taken in long double."""
    Xh = X.astype(LD)
    xc = Xh - Xh.mean(axis=0)
    return xc, (xc * xc).sum(axis=1)


class Ref:
    """One cloud with everything the tests compare against, computed once."""

    def __init__(self, kind, n, d, seed):
        self.kind, self.n, self.d = kind, n, d
        self._e32 = None
        self.X = cloud(kind, n, d, seed)
        self.keys = hp_keys(self.X)
        self.sq, self.med = stats_of_keys(self.keys, n)
        self.a = float(np.log(LD(n)) / (LD(self.med) * LD(self.med)))
        xc, nrm = centred(self.X)
        self.xc, self.nrm = xc.astype(np.float64), nrm.astype(np.float64)
        self.nmax = float(nrm.max())
        iu = np.triu_indices(n, 1)
        self.den = self.nrm[iu[0]] + self.nrm[iu[1]]
        for arr in (self.X, self.keys, self.xc, self.nrm, self.den):
            arr.flags.writeable = False  # shared between tests

    def key_error(self, keys):
        """max over pairs of |key - hp_key| / (|xc_i|^2 + |xc_j|^2)."""
        return float(np.max(np.abs(keys.astype(self.keys.dtype) - self.keys) / self.den))

    def e32(self):
        """The same error for fp32 keys from a numpy fp32 Gram on the centred
        coordinates (tests/test_gpu_f32_accuracy.py::test_b3_keys_error_within_fp32)."""
        if self._e32 is None:
            self._e32 = self.key_error(gram_keys(self.xc, self.nrm, np.float32))
        return self._e32

    def y(self, a=None):
        """a log2e max|xc|^2: above 300 the symmetric phi pass hands over."""
        return (self.a if a is None else a) * np.log2(np.e) * self.nmax


@functools.lru_cache(maxsize=2)
def ref(kind, n, d, seed):
    return Ref(kind, n, d, seed)


def seed_of(kind, n, d):
    return 7000 + 131 * KINDS.index(kind) + 17 * d + n


# ---------------------------------------------- emulated device arithmetic --
def gram_keys(xc, nrm, T):
    """Centred Gram-form keys max(|xc_i|^2 + |xc_j|^2 - 2 xc_i.xc_j, 0) in T
    (fp64 or fp32), upper triangle, widened to fp64.  nrm = None: the norms
    are summed in T from the coordinates rounded to T, as a device does."""
    x = xc.astype(T)
    q = (x * x).sum(axis=1) if nrm is None else nrm.astype(T)
    iu = np.triu_indices(x.shape[0], 1)
    g = (x @ x.T)[iu]
    return np.maximum(q[iu[0]] + q[iu[1]] - T(2.0) * g, T(0.0)).astype(np.float64)


def _fma64(a, b, c):
    """fp64 fma(a, b, c): the product and the sum in long double (the 106-bit
    product rounds to 64 bits first: 2^-64 relative, nothing at this scale)."""
    return (np.asarray(a, dtype=LD) * b + c).astype(np.float64)


def chain_keys(xc):
    """The row kernels' fp64 key arithmetic (k_center_d, k_pair_rows,
    k_sample_keys): |xc|^2 and the dot product as fma chains over the
    coordinates, key = max(fma(-2, dot, |xc_i|^2 + |xc_j|^2), 0)."""
    n, d = xc.shape
    i, j = np.triu_indices(n, 1)
    q = np.zeros(n)
    dot = np.zeros(i.size)
    for k in range(d):
        col = np.ascontiguousarray(xc[:, k])
        q = _fma64(col, col, q)
        dot = _fma64(col[i], col[j], dot)
    return np.maximum(_fma64(-2.0, dot, q[i] + q[j]), 0.0)


def fp64_key_bound(d):
    """Forward bound of a centred Gram-form key, relative to |xc_i|^2 +
    |xc_j|^2: (d + 4) 2^-53 for the two norms, the product and the final
    sums, times 4 for the device mean and the summation order."""
    return 4.0 * (d + 4) * 2.0 ** -53


def f32_key_bound(e32):
    return 2.0 * e32 + 2.0 ** -22


def emulated_phi(X, G, a, T):
    """phi from the centred Gram form in T with exp in T, sums in fp64."""
    n = X.shape[0]
    xc = X - X.mean(axis=0)
    x = xc.astype(T)
    q = (x * x).sum(axis=1)
    key = np.maximum(q[:, None] + q[None, :] - T(2.0) * (x @ x.T), T(0.0))
    K = np.exp(-T(a) * key).astype(np.float64)
    x = x.astype(np.float64)
    return (K @ G + 2.0 * a * (x * K.sum(axis=1)[:, None] - K @ x)) / n
