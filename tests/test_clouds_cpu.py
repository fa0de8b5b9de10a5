"""The cloud family of tests/_clouds.py keeps its headroom.  CPU only: these
tests do not load the library.

tests/test_gpu_clouds.py holds the device to bars that come from the number
formats.  Here a numpy emulation of the documented device arithmetic -- the
mean and the centred coordinates in fp64, the Gram form in fp64 or fp32, exp,
sums in fp64 -- runs on every kind at every shape the GPU tests use, and has
to stay at a quarter of each bar, so a red GPU test means the device and not
the input.  Every figure is printed ("clouds_cpu ..." lines, -s or -rA).

Where the quarter cannot hold, and what is asserted instead:

  * fp64 keys at d = 2.  The bar is 4 (d + 4) = 24 units of 2^-53 (|xc_i|^2 +
    |xc_j|^2).  The fma-chain arithmetic of the row kernels has a rigorous
    worst case of 2 d + 7 units (4 for the rounded centred coordinates, d for
    the two norms, d for the dot product, 1 for their sum, 2 for the last
    fma), and the largest of 2 10^6 pairs comes to 6 .. 7.2 of them: 0.25 ..
    0.30 of the bar on every kind, the uniform control included (0.28), so no
    change of input helps.  At d = 2 the emulation is held to its worst case,
    (2 d + 7) / (4 (d + 4)) = 0.46 of the bar; d >= 5 keeps the quarter (worst
    observed 0.23 at d = 5, 0.20 at d = 8, 0.11 at d = 40).  The device
    itself measures 0.20 .. 0.31 of the bar across the kinds.
  * F32 keys.  The bar 2 e32 + 2^-22 is built from e32, the error of the
    numpy fp32 Gram itself, so the emulation sits at e32 / bar < 1/2 by
    construction and reaches 1/4 only if e32 <= 2^-23, less than the rounding
    of one fp32 norm (observed e32: 2.2e-7 .. 9.6e-7, ratio 0.33 .. 0.46).
    What can go wrong with an input is that it inflates e32 and with it the
    bar: e32 is held to the fp32 forward bound (d + 4) 2^-24 (observed at
    most 0.75 of it).
"""
import numpy as np
import pytest

import _clouds as K

U53 = 2.0 ** -53
PHI_TOL = 1e-10
F32_REL = 1e-4


def _say(*a):
    print("clouds_cpu", *a)


# ----------------------------------------------------------- the reference --
def test_hp_stats_rank_mapping_matches_full_sort(oracle):
    """full_list_ranks / stats_of_keys against a sort of the whole n^2 list."""
    for n in range(2, 41):
        for kind in ("uniform", "bal"):
            X = K.cloud(kind, n, 3, 77 + n)
            Xh = X.astype(K.LD)
            full = np.sqrt((((Xh[:, None, :] - Xh[None, :, :]) ** 2).sum(-1)).reshape(-1))
            v = np.sort(full)
            c = v.size
            ref = (v[c // 2 - 1] + v[c // 2]) / 2 if c % 2 == 0 else v[c // 2]
            sq, med = K.hp_stats(X)
            assert len(sq) == (2 if c % 2 == 0 else 1)
            assert med == pytest.approx(float(ref), rel=1e-15), (kind, n)


@pytest.mark.parametrize("n,d", [(400, 3), (400, 8), (1000, 2), (2050, 5), (6000, 2), (6000, 8)])
def test_bal_even_n_straddles_the_gap(oracle, n, d):
    """Exactly n / 2 particles per cluster: the lower half of the n^2 list is
    the n zeros and the within-cluster pairs, so the two averaged statistics
    are the largest within-cluster and the smallest between-cluster distance."""
    m, L = K.split("bal", n)
    assert 2 * m == n
    X = K.cloud("bal", n, d, K.seed_of("bal", n, d))
    (lo, hi), med = K.hp_stats(X)
    _say("straddle n=%d d=%d lo=%.4g hi=%.4g med=%.4g" % (n, d, np.sqrt(float(lo)), np.sqrt(float(hi)), med))
    assert np.sqrt(float(lo)) < L / 2 < np.sqrt(float(hi))
    # a single statistic (odd n) sits at the edge of one population
    Xo = K.cloud("bal", n + 1, d, K.seed_of("bal", n + 1, d))
    (one,), _ = K.hp_stats(Xo)
    assert abs(np.sqrt(float(one)) - L / 2) > L / 4


def test_oracle_median_is_no_reference_off_centre(oracle):
    """Why this reference exists: oracle.median_scale restates the
    reference's uncentred Gram form and loses 2^-53 |x|^2 / med^2.  Fine on
    centred data, off by far more than the 1e-12 the suite asks of the device
    on a cloud at offset 1e6 and on two tight clusters 1 apart."""
    n, d = 400, 3
    rel = {}
    for kind in ("uniform", "c6040", "shift1e3", "shift1e6", "tight"):
        X = K.cloud(kind, n, d, K.seed_of(kind, n, d))
        _, med = K.hp_stats(X)
        rel[kind] = abs(oracle.median_scale(X)[1] - med) / med
        _say("oracle_median kind=%s n=%d d=%d rel err=%.3g" % (kind, n, d, rel[kind]))
    assert rel["uniform"] <= 1e-12 and rel["c6040"] <= 1e-12
    assert rel["shift1e6"] > 1e-9 and rel["tight"] > 1e-9


# -------------------------------------------------------------------- keys --
@pytest.mark.parametrize("kind", K.KINDS)
def test_fp64_keys_keep_their_headroom(oracle, kind):
    worst = 0.0
    for n, d in K.key_shapes(kind, False):
        bar = K.fp64_key_bound(d)
        if n * n * d > K.HP_MAX_WORK and d <= 16:
            # the trajectories' size: the order statistics, as the GPU test
            # checks them, from a BLAS Gram (the reference is fp64 there)
            X = K.cloud(kind, n, d, K.seed_of(kind, n, d))
            sq, _ = K.hp_stats(X)
            xc = X - X.mean(axis=0)
            emu, _ = K.stats_of_keys(K.gram_keys(xc, None, np.float64), n)
            E = bar * 2.0 * float((xc * xc).sum(axis=1).max())
            frac = max(abs(float(a) - float(b)) for a, b in zip(emu, sq)) / E
            limit = 0.25
        else:
            r = K.ref(kind, n, d, K.seed_of(kind, n, d))
            xc = r.X - r.X.mean(axis=0)
            keys = K.chain_keys(xc) if d <= 16 else K.gram_keys(xc, None, np.float64)
            frac = r.key_error(keys) / bar
            limit = 0.25 if d > 2 else (2 * d + 7) / (4.0 * (d + 4))
        _say("fp64_keys kind=%s n=%d d=%d emulation/bar=%.3f limit=%.3f" % (kind, n, d, frac, limit))
        assert frac <= limit, (kind, n, d, frac)
        worst = max(worst, frac)
    _say("fp64_keys kind=%s worst=%.3f" % (kind, worst))


@pytest.mark.parametrize("kind", K.KINDS)
def test_f32_key_bar_is_not_inflated(oracle, kind):
    for n, d in K.key_shapes(kind, True):
        r = K.ref(kind, n, d, K.seed_of(kind, n, d))
        e32 = r.e32()
        _say("f32_keys kind=%s n=%d d=%d e32=%.3g e32/bar=%.3f e32/((d+4) 2^-24)=%.3f" %
             (kind, n, d, e32, e32 / K.f32_key_bound(e32), e32 / ((d + 4) * 2.0 ** -24)))
        assert e32 <= (d + 4) * 2.0 ** -24, (kind, n, d, e32)


# --------------------------------------------------------------------- phi --
def _phi_case(oracle, kind, n, d):
    seed = K.seed_of(kind, n, d)
    X = K.cloud(kind, n, d, seed)
    G = K.gradients(n, d, seed)
    _, med = K.hp_stats(X)
    a = float(np.log(n) / med ** 2)
    ref = K.hp_phi(X, G, a).astype(np.float64)
    return X, G, a, ref


@pytest.mark.parametrize("n,d", K.PHI_ROWS + K.PHI_TILES + K.PHI_SYM)
@pytest.mark.parametrize("kind", K.PHI_KINDS)
def test_fp64_phi_reference_and_headroom(oracle, kind, n, d):
    """hp_phi pins oracle.phi (1e-14 max|phi| up to n = 800; at the
    symmetric-pass sizes, where the GPU test compares with oracle.phi, to a
    hundredth of the 1e-10 bar), max|phi| keeps the absolute bar meaningful,
    and the fp64 emulation keeps a quarter."""
    X, G, a, ref = _phi_case(oracle, kind, n, d)
    top = float(np.max(np.abs(ref)))
    e_or = float(np.max(np.abs(oracle.phi(X, G, a) - ref)))
    e_em = float(np.max(np.abs(K.emulated_phi(X, G, a, np.float64) - ref)))
    xc, nrm = K.centred(X)
    y = a * np.log2(np.e) * float(nrm.max())
    _say("fp64_phi kind=%s n=%d d=%d a=%.4g y=%.4g max|phi|=%.3g oracle=%.3g emulation=%.3g bar/4=%.3g" %
         (kind, n, d, a, y, top, e_or, e_em, PHI_TOL / 4))
    assert top >= 0.01
    if n <= 800:
        assert e_or <= 1e-14 * top
    else:  # the oracle's own sums of n terms: a hundredth of the bar it serves
        assert e_or <= PHI_TOL / 100
    assert e_em <= PHI_TOL / 4
    if kind == "c6040" and d == 8:
        assert y > 300  # the symmetric pass hands the step to the row stream
    if kind == "c6040_near":
        assert y < 300  # the symmetric pass proper


@pytest.mark.parametrize("n,d", K.PHI_F32)
@pytest.mark.parametrize("kind", K.F32_PHI_KINDS)
def test_f32_phi_headroom(oracle, kind, n, d):
    X, G, a, ref = _phi_case(oracle, kind, n, d)
    top = float(np.max(np.abs(ref)))
    e_or = float(np.max(np.abs(oracle.phi(X, G, a) - ref)))
    e_em = float(np.max(np.abs(K.emulated_phi(X, G, a, np.float32) - ref)))
    _say("f32_phi kind=%s n=%d d=%d a=%.4g max|phi|=%.3g emulation/max|phi|=%.3g bar/4=%.3g" %
         (kind, n, d, a, top, e_em / top, F32_REL / 4))
    assert top >= 0.01
    assert e_or <= 1e-14 * top
    assert e_em <= F32_REL / 4 * top


def test_f32_phi_leaves_out_the_far_clusters(oracle):
    """Why the F32 phi tests do not take bal or c6040 (L = 40): the fp32 key
    error 2^-24 |xc|^2 times a is past a quarter of the 1e-4 bar."""
    n, d = 333, 6
    X, G, a, ref = _phi_case(oracle, "c6040", n, d)
    e_em = float(np.max(np.abs(K.emulated_phi(X, G, a, np.float32) - ref))) / float(np.max(np.abs(ref)))
    _say("f32_phi kind=c6040 n=%d d=%d emulation/max|phi|=%.3g (not a GPU case)" % (n, d, e_em))
    assert e_em > F32_REL / 4
