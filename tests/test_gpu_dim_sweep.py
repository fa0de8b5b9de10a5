"""Every per-dimension kernel instantiation against the oracle.

The launchers in svgd_kernels.hip / svgd_collect.hip dispatch over d (or over
the (KP, NCB) tile class pick_tiles derives from d), through the lists of
built.h; each entry is its own
compiled kernel with its own register budget, record stride, LDS layout and
unroll.  This module walks d over every value a user can pick (1..64) with the
smallest shapes that still reach the code in question, so a wrong bound or
stride in one instantiation cannot ship with a green suite:

  1. the dispatch table: which phi kernel each (dtype, d) launches;
  2. fp64 row-stream phi (k_phi_rows<D, R, 8, 8192, 8> + k_phi_reduce), d 1..16;
  3. fp64 full-matrix scale (k_prep_rec_mat + k_phi_rows<D, R, 4, 4096, 1>, the
     4-wave geometry), d 1..16;
  4. fp64 steps (median + phi + the fused optimizer epilogue + host gradient);
  5. fp64 median, direct (k_center_d, k_pair_rows) and bracket
     (k_sample_keys_f32, k_pair_mcol, k_pair_rows) paths, d 1..16, and the
     streamed radix fallback (the histogram passes) in every class;
  6. fp64 tiles (k_phi<double>, k_pair_tiles<double>), d 17..64;
  7. F32 phi (k_phi<float>, k_phi_f32s, k_phi_b3) d 1..64 and F32 median
     (k_pair_tiles<float>, k_pair_tcol) in the KP = 12 / 16 classes;
  8. device gradient (k_gauss_grad<D> and its generic form);
  9. host gradient (CPU; the 4- and 8-particle SIMD blocks), d 1..64.

The reference is always the fp64 CPU oracle or the exact order statistics of
the device's own keys (svgd_debug_pair_keys).  Tolerances are the project's
bars (tests/test_gpu_parity.py, test_gpu_f32.py, test_gpu_device_model.py,
test_capi_cpu.py): fp64 phi max-abs 1e-10, step positions 1e-9, scale rel
1e-12, median bit-exact on own keys, F32 phi 1e-4 max|phi|, F32 median rel
1e-5, device gradient rtol 1e-13 / atol 1e-14 vs the host model and 1e-11 /
1e-12 vs the oracle.  Each test prints its observed error ("dim_sweep ..."
lines, shown with -s or -rA) before it asserts.
"""
import ctypes

import numpy as np
import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

from _dispatch import F32_TABLE, F32_VARIANTS, F64_TABLE, KNOBS, knob_value
from _dispatch import expected_name as _expected_name

gpu = pytest.mark.gpu

PHI_TOL = 1e-10
F32_REL = 1e-4


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    """Every case starts from the library's defaults; a case sets what it needs."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _ctx(X, dtype=C.SVGD_F64):
    n, d = X.shape
    c = S.Context(d, n, dtype=dtype)
    c.set_particles(X)
    return c


def _report(what, n, d, err, bar):
    print("dim_sweep %s n=%d d=%d err=%.3g bar=%.3g" % (what, n, d, err, bar))


# ------------------------------------------------------- 1. dispatch table --
# (the tables: tests/_dispatch.py, also checked without a GPU by tests/test_phi_plan_cpu.py)
@gpu
@pytest.mark.parametrize("d", range(1, 65))
@pytest.mark.parametrize("dtype,table", [(C.SVGD_F64, F64_TABLE), (C.SVGD_F32, F32_TABLE)],
                         ids=["f64", "f32"])
def test_dispatch_table(dtype, table, d):
    """A change that silently reroutes a dimension to another kernel turns this red."""
    c = S.Context(d, 333, dtype=dtype)
    name = c.phi_kernel_name()
    c.close()
    assert name == _expected_name(table, d)
    assert name == S.plan_phi_name(d, 333, dtype)  # the context and the context-free plan agree


# ------------------------------------------------ 2. fp64 row-stream phi ----
def _rows_scale(d):
    """X has scale 2 (variance 4/3 per coordinate): a typical pair lies at
    |x - x'|^2 = 2 d 4/3, where this a gives K = e^-1/2 -- every column
    contributes to every row, and max|phi| stays around 0.05 .. 0.25, so a
    relative error of 1e-8 in any d is above the 1e-10 bar."""
    return 0.5 / (2.0 * d * 4.0 / 3.0)


@gpu
@pytest.mark.parametrize("n,d", [(777, d) for d in range(1, 17)] + [(1280, d) for d in range(9, 17)])
def test_rows_phi_every_d(oracle, n, d):
    """k_phi_rows<D, R, 8, 8192, 8> with several column splits and k_phi_reduce.

    init_ctx takes S = min(2 ceil(resident / row blocks), max(1, n / 256))
    column splits; the first term is at least 2 * 256 / 7, so S = n / 256:
    3 at n = 777 and 5 at n = 1280 (no diagnostic exposes S).  A work-group
    owns 64 R rows: 256 for d <= 8 (R = 4), 128 above (R = 2).  n = 777 is 4
    or 7 row blocks, the last one 9 rows deep (a ragged tail); n = 1280 is ten
    exact blocks of 128.  k_phi_reduce then adds the S partials of d + 1
    elements per row, phi_red_rows(d) = 256 / (d + 1) rows per block."""
    X = oracle.splitmix((n, d), 2.0, 500 + n + d)
    G = oracle.splitmix((n, d), 1.0, 600 + n + d)
    a = _rows_scale(d)
    ref = oracle.phi(X, G, a)
    c = _ctx(X)
    assert c.phi_kernel_name() == _expected_name(F64_TABLE, d)
    out = c.phi(G, a)
    again = c.phi(G, a)
    c.close()
    err = float(np.max(np.abs(out - ref)))
    _report("rows_phi", n, d, err, PHI_TOL)
    assert np.array_equal(out, again)  # deterministic
    assert err <= PHI_TOL


# --------------------------------------------- 3. fp64 full-matrix scale ----
def _spd(d, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d)) * 0.4
    return A @ A.T + np.eye(d) * 0.3


def _indefinite(d, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    lam = rng.uniform(0.2, 1.0, d) * np.where(np.arange(d) % 3 == 1, -0.3, 1.0)
    if d == 1:
        lam = np.array([-0.25])
    if d == 2:
        lam = np.array([0.8, -0.25])
    M = (Q * lam) @ Q.T
    return 0.5 * (M + M.T)  # exactly symmetric


@gpu
@pytest.mark.parametrize("kind", ["spd", "indefinite"])
@pytest.mark.parametrize("d", range(1, 17))
def test_matrix_scale_phi_every_d(oracle, d, kind):
    """k_prep_rec_mat + k_phi_rows<D, R, 4, 4096, 1> (signature rows) at n = 777:
    an SPD M (X scale 2, M / d) and an indefinite one (X scale 1, M / 2 d),
    built as tests/test_gpu_matrix_scale.py builds them."""
    n = 777
    if kind == "spd":
        X = oracle.splitmix((n, d), 2.0, 11 + n + d)
        M = _spd(d, d) / d
    else:
        X = oracle.splitmix((n, d), 1.0, 21 + n + d)
        M = _indefinite(d, d) * (0.5 / d)
        assert np.min(np.linalg.eigvalsh(M)) < 0
    G = oracle.splitmix((n, d), 1.0, 12 + n + d)
    ref = oracle.phi_matrix(X, G, M)
    c = _ctx(X)
    c.set_scale_matrix(M)
    ph = c.phi(G, 0.0)
    Mdev = c.get_scale_matrix()
    c.close()
    err = float(np.max(np.abs(ph - ref)))
    _report("matrix_phi_" + kind, n, d, err, PHI_TOL)
    print("dim_sweep matrix_phi_%s d=%d max|ref|=%.3g" % (kind, d, np.max(np.abs(ref))))
    assert err <= PHI_TOL
    np.testing.assert_allclose(Mdev, M, rtol=1e-15, atol=0)


# ------------------------------------------------------- 4. fp64 steps ------
@gpu
@pytest.mark.parametrize("d", range(1, 17))
def test_step_every_d(oracle, d):
    """Three device steps (n = 777, two-component Gaussian sum, bounds
    [-2.5, 2.5]^d inside the initial [-3, 3]^d so coordinates clamp), each
    against the oracle step from the device's own X_t: the median scale, the
    host gradient, phi and k_phi_reduce's fused optimizer epilogue (Adam /
    AdaGrad / RMSProp by d mod 3) at every d."""
    n = 777
    X = oracle.splitmix((n, d), 3.0, 5 + n + d)
    mus = oracle.splitmix((2, d), 3.0, 6 + n + d)
    covs = np.stack([np.eye(d) * (1.0 + 0.25 * k) for k in range(2)])
    model = S.GaussianSum(list(mus), list(covs))
    c = _ctx(X)
    if d % 3 == 0:
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
        o_opt = oracle.Adam((n, d), 0.05, 0.9, 0.999)
    elif d % 3 == 1:
        c.set_optimizer(C.SVGD_OPT_ADAGRAD, 0.05, 0.0, 0.0, 1e-8)
        o_opt = oracle.AdaGrad((n, d), 0.05)
    else:
        c.set_optimizer(C.SVGD_OPT_RMSPROP, 0.05, 0.9, 0.0, 1e-8)
        o_opt = oracle.RMSProp((n, d), 0.05, 0.9)
    lo, up = -np.full(d, 2.5), np.full(d, 2.5)
    c.set_bounds(lo, up)
    worst, worst_a = 0.0, 0.0
    for _ in range(3):
        Xt = c.get_particles()
        a_ref, _ = oracle.median_scale(Xt)
        G = oracle.logp_grad_gmm(Xt, mus, covs)
        ph_ref = oracle.phi(Xt, G, a_ref)
        c.step_with_model(model)
        a_dev, _, _ = c.last_scale()
        Xref = Xt.copy()
        oracle.apply_update(Xref, o_opt.step(ph_ref), lo, up)
        Xdev = c.get_particles()
        worst = max(worst, float(np.max(np.abs(Xdev - Xref))))
        worst_a = max(worst_a, abs(a_dev - a_ref) / abs(a_ref))
        assert a_dev == pytest.approx(a_ref, rel=1e-12)
        # increments are lr * O(1) -> compare positions with the phi tolerance
        assert np.max(np.abs(Xdev - Xref)) <= 1e-9
    c.close()
    _report("step_pos", n, d, worst, 1e-9)
    _report("step_scale_rel", n, d, worst_a, 1e-12)
    assert np.any(np.abs(Xdev) == 2.5)  # the clamp was exercised


# ------------------------------------------------------ 5. fp64 median ------
def _own_keys(c, n):
    keys = np.empty(n * (n - 1) // 2)
    c.check(c.lib.svgd_debug_pair_keys(c.h, C.dptr(keys), keys.size))
    return keys


def _median_of_keys(keys, n):
    """The median of the full n x n distance list (n zeros + each pair twice)
    from the upper-triangle squared distances."""
    u = np.sort(keys)
    tot = n * n

    def at(k):
        return 0.0 if k < n else np.sqrt(u[(k - n) // 2])
    return (at(tot // 2 - 1) + at(tot // 2)) / 2 if tot % 2 == 0 else at(tot // 2)


def _direct_median_checks(oracle, X, key_rtol=None, key_atol=None):
    n, d = X.shape
    c = _ctx(X)
    a, med = c.median_scale()
    path = c.last_scale()[2]
    keys = _own_keys(c, n)
    c.close()
    if key_rtol is not None:  # device keys agree with the direct-form distances to rounding
        iu = np.triu_indices(n, 1)
        ref_keys = ((X[iu[0]] - X[iu[1]]) ** 2).sum(-1)
        print("dim_sweep direct_keys n=%d d=%d max rel err=%.3g" %
              (n, d, np.max(np.abs(keys - ref_keys) / np.maximum(ref_keys, 1e-300))))
        np.testing.assert_allclose(keys, ref_keys, rtol=key_rtol, atol=key_atol)
    exp = _median_of_keys(keys, n)
    med_ref = oracle.median_scale(X)[1]
    _report("direct_median_rel", n, d, abs(med - med_ref) / med_ref, 1e-12)
    assert path == C.SVGD_MEDIAN_DIRECT
    assert med == exp  # bit-exact selection
    assert med == pytest.approx(med_ref, rel=1e-12)
    assert a == pytest.approx(np.log(n) / (exp * exp), rel=1e-15)


@gpu
@pytest.mark.parametrize("d", range(1, 17))
@pytest.mark.parametrize("n", [127, 400])
def test_median_direct_every_d(oracle, n, d):
    """k_center_d<D> (records without a padding word at d = 3, 7, 11, 15) and
    k_pair_rows<D, 1 | 2>: the keys, the exact selection and the scale."""
    X = oracle.splitmix((n, d), 1.0, 3 * n + d)
    _direct_median_checks(oracle, X, key_rtol=1e-12, key_atol=1e-13)


def _bracket_median(X, monkeypatch, fp64, bf16=True):
    monkeypatch.setenv("SVGD_COLLECT_FP64", "1" if fp64 else "0")
    monkeypatch.setenv("SVGD_MCOL_BF16", "1" if bf16 else "0")
    c = _ctx(X)
    c.set_median_tuning(direct_max_pairs=0, sample_size=1 << 16)  # force the bracket path
    a, med = c.median_scale()
    return c, (a, med, c.last_scale()[2], c.last_median_keys())


# the d tests/test_gpu_collect.py's test_mcol_matches_fp64_collect_and_exact
# leaves out; d <= 8 with both Gram forms (d > 8 always takes the f32 Gram)
MCOL_CASES = [(6, True), (6, False), (7, True), (7, False)] + [(d, False) for d in (9, 10, 11, 13, 14, 15)]


@gpu
@pytest.mark.parametrize("d,bf16", MCOL_CASES, ids=["%d-%s" % (d, "bf16" if b else "f32") for d, b in MCOL_CASES])
@pytest.mark.parametrize("n", [1000, 2049])
def test_mcol_bracket_missing_d(oracle, monkeypatch, n, d, bf16):
    """k_sample_keys_f32<D>, k_pair_mcol<D, BF> and k_pair_rows<D, 0>: the
    matrix-core collect selects the same keys, bit for bit, as the all-fp64
    collect, and the exact order statistics of the device's own keys."""
    X = oracle.splitmix((n, d), 3.0, 7 * n + d)
    c, got = _bracket_median(X, monkeypatch, fp64=False, bf16=bf16)
    exp = _median_of_keys(_own_keys(c, n), n)
    c.close()
    f, ref = _bracket_median(X, monkeypatch, fp64=True)
    f.close()
    assert got[2] in (C.SVGD_MEDIAN_BRACKET, C.SVGD_MEDIAN_REBRACKET), got
    assert ref[2] in (C.SVGD_MEDIAN_BRACKET, C.SVGD_MEDIAN_REBRACKET), ref
    assert got[:2] == ref[:2] and got[3] == ref[3]  # same keys, bit for bit
    assert got[1] == exp
    assert got[1] == pytest.approx(oracle.median_scale(X)[1], rel=1e-12)


FALLBACK_CASES = ([(C.SVGD_F64, d) for d in range(1, 17)] + [(C.SVGD_F64, 20), (C.SVGD_F64, 50)] +
                  [(C.SVGD_F32, d) for d in (2, 6, 10, 14, 20, 50)])


@gpu
@pytest.mark.parametrize("dtype,d", FALLBACK_CASES,
                         ids=["%s-%d" % ("f64" if t == C.SVGD_F64 else "f32", d) for t, d in FALLBACK_CASES])
def test_median_fallback_every_class(oracle, dtype, d):
    """A 1-key candidate capacity overflows every region, so the streamed
    radix select runs the histogram passes k_pair_rows<D, 1> (fp64, every
    d <= 16) and k_pair_tiles<T, KP, 1> (fp64 KP 32 / 64, F32 every KP
    class): still the exact order statistics of the device's own keys."""
    n = 400
    X = oracle.splitmix((n, d), 1.0, 42 + n + d)
    c = _ctx(X, dtype)
    c.set_median_tuning(direct_max_pairs=0, sample_size=1 << 12, candidate_capacity=1)
    a, med = c.median_scale()
    path = c.last_scale()[2]
    exp = _median_of_keys(_own_keys(c, n), n)
    c.close()
    med_ref = oracle.median_scale(X)[1]
    rel = 1e-12 if dtype == C.SVGD_F64 else 1e-5
    _report("fallback_median_rel_" + ("f64" if dtype == C.SVGD_F64 else "f32"), n, d, abs(med - med_ref) / med_ref, rel)
    assert path == C.SVGD_MEDIAN_FALLBACK
    assert med == exp
    assert med == pytest.approx(med_ref, rel=rel)
    assert a == pytest.approx(np.log(n) / (exp * exp), rel=1e-15)


# ------------------------------------------------------- 6. fp64 tiles ------
@gpu
@pytest.mark.parametrize("d", range(17, 65))
def test_tile_phi_every_d(oracle, d):
    """k_phi<double, KP, NCB> takes d at run time inside its KP class: the
    columns d..KP of X and the unused width of V are zero padding.  n = 333 is
    ragged against the 16-, 32-, 64- and 128-row units of the tile kernels."""
    n = 333
    X = oracle.splitmix((n, d), 2.0, 700 + n + d)
    G = oracle.splitmix((n, d), 1.0, 800 + n + d)
    a = 0.05
    ref = oracle.phi(X, G, a)
    c = _ctx(X)
    assert c.phi_kernel_name() == _expected_name(F64_TABLE, d)
    out = c.phi(G, a)
    c.close()
    err = float(np.max(np.abs(out - ref)))
    _report("tile_phi", n, d, err, PHI_TOL)
    assert err <= PHI_TOL


@gpu
@pytest.mark.parametrize("d", [17, 31, 32, 33, 47, 48, 63, 64])
def test_tile_median_direct(oracle, d):
    """k_pair_tiles<double, 32 | 64> either side of each class boundary."""
    n = 300
    X = oracle.splitmix((n, d), 1.0, 3 * n + d)
    _direct_median_checks(oracle, X)


# -------------------------------------------------------------- 7. F32 ------
@gpu
@pytest.mark.parametrize("d,knob,name", F32_VARIANTS,
                         ids=["%d-%s" % (d, {None: "default", "SVGD_PHI_B3": "b3off", "SVGD_PHI_S1V": "ones",
                                             "SVGD_PHI_TILE_GENERIC": "generic"}[k])
                              for d, k, _ in F32_VARIANTS])
def test_f32_phi_every_d(oracle, monkeypatch, d, knob, name):
    """The F32 phi at n = 333 for every d: the default kernels of the
    dispatch table, the fp32-MFMA streamed kernel where the bf16 one is the
    default (SVGD_PHI_B3=0; d = 32 is k_phi_f32s<32, 3>), the bf16 kernel
    with the V column of ones at d = 16 NCB (SVGD_PHI_S1V=0: the only way to
    k_phi_b3<32, 3> and <64, 5>), and the generic fp32 tile kernel where a
    streamed one is the default (SVGD_PHI_TILE_GENERIC=1)."""
    n = 333
    if knob:
        monkeypatch.setenv(knob, knob_value(knob))
    X = oracle.splitmix((n, d), 3.0, 500 + n + d)
    G = oracle.splitmix((n, d), 1.0, 600 + n + d)
    a = float(np.log(n) / (2.0 * d * 3.0))  # typical median-heuristic magnitude
    ref = oracle.phi(X, G, a)
    c = _ctx(X, C.SVGD_F32)
    got_name = c.phi_kernel_name()
    ph = c.phi(G, a)
    c.close()
    assert got_name == (name or _expected_name(F32_TABLE, d))
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(ph - ref)))
    print("dim_sweep f32_phi[%s] n=%d d=%d err/max|phi|=%.3g bar=%.3g" % (got_name, n, d, err / scale, F32_REL))
    assert np.all(np.isfinite(ph))
    assert err <= F32_REL * scale


def _median32(X, monkeypatch, ref):
    monkeypatch.setenv("SVGD_COLLECT_FP64", "1" if ref else "0")
    c = _ctx(X, C.SVGD_F32)
    c.set_median_tuning(direct_max_pairs=0)
    a, med = c.median_scale()
    return c, (a, med, c.last_scale()[2], c.last_median_keys())


@gpu
@pytest.mark.parametrize("d", [9, 10, 12, 13, 15])
@pytest.mark.parametrize("n", [300, 1000])
def test_tcol_missing_d(oracle, monkeypatch, n, d):
    """k_pair_tcol<12 | 16> and k_pair_tiles<float, 12 | 16, .>: the
    matrix-core collect against the tile collect (bit for bit), the exact
    order statistics of the device's own fp32 keys, and the oracle."""
    X = oracle.splitmix((n, d), 3.0, 11 * n + d)
    c, got = _median32(X, monkeypatch, ref=False)
    exp = _median_of_keys(_own_keys(c, n), n)
    c.close()
    f, ref = _median32(X, monkeypatch, ref=True)
    f.close()
    assert got[2] != C.SVGD_MEDIAN_DIRECT, got
    assert got == ref  # same keys and counts: the same path, bit for bit
    assert got[1] == exp
    med_ref = oracle.median_scale(X)[1]
    _report("f32_bracket_median_rel", n, d, abs(got[1] - med_ref) / med_ref, 1e-5)
    assert got[1] == pytest.approx(med_ref, rel=1e-5)


@gpu
def test_f32_median_direct_kp12(oracle):
    """The KP = 12 class with the default tuning (every pair a candidate:
    bracket [0, inf)): fp32 keys, exact selection.  k_pair_tcol deals the
    tiles to its blocks in row bands, so a block's region (sized for an even
    share) may overflow and the streamed radix select takes over: the path is
    printed, not asserted -- both are exact."""
    n, d = 400, 12
    X = oracle.splitmix((n, d), 2.0, 7 * n + d)
    c = _ctx(X, C.SVGD_F32)
    a, med = c.median_scale()
    path = c.last_scale()[2]
    keys = _own_keys(c, n)
    c.close()
    print("dim_sweep f32_direct_median n=%d d=%d path=%d" % (n, d, path))
    assert path in (C.SVGD_MEDIAN_DIRECT, C.SVGD_MEDIAN_FALLBACK)
    # every key is an fp32 value (widened exactly)
    assert np.array_equal(keys.astype(np.float32).astype(np.float64), keys)
    iu = np.triu_indices(n, 1)
    ref_keys = ((X[iu[0]] - X[iu[1]]) ** 2).sum(-1)
    np.testing.assert_allclose(keys, ref_keys, rtol=1e-4, atol=1e-4)
    exp = _median_of_keys(keys, n)
    med_ref = oracle.median_scale(X)[1]
    _report("f32_direct_median_rel", n, d, abs(med - med_ref) / med_ref, 1e-5)
    assert med == exp
    assert med == pytest.approx(med_ref, rel=1e-5)
    assert a == pytest.approx(np.log(n) / (exp * exp), rel=1e-15)


# ---------------------------------------------------- 8. device gradient ----
def _gauss_model(oracle, d, k, seed):
    """Well-conditioned covariances (eigenvalues within [1, 2 + 0.09 * 4 d]):
    the solves stay far inside the gradient tolerances at every d <= 64."""
    mus = oracle.splitmix((k, d), 3.0, seed)
    rng = np.random.default_rng(seed)
    covs = []
    for _ in range(k):
        A = rng.standard_normal((d, d)) * 0.3
        covs.append(A @ A.T + np.eye(d) * (1.0 + rng.random()))
    return mus, np.stack(covs)


@gpu
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("d", [3, 4, 5, 6, 7, 12, 11, 17, 33, 64])
def test_device_gradient_missing_d(oracle, d, k):
    """k_gauss_grad<D> (specialised: 3..7, 12) and its run-time-d form
    (11, 17, 33, 64) against the host model and the oracle."""
    n = 300
    X = oracle.splitmix((n, d), 4.0, 3 + n + d)
    mus, covs = _gauss_model(oracle, d, k, 17 + d + k)
    model = S.GaussianSum(list(mus), list(covs))
    c = _ctx(X)
    c.set_device_model(model)
    Gd = c.device_logp_grad()
    c.close()
    Gh = model.log_model_grad(X)
    Go = oracle.logp_grad_gmm(X, mus, covs)
    print("dim_sweep device_grad n=%d d=%d k=%d max|Gd-Gh|=%.3g max|Gd-Go|=%.3g max|G|=%.3g" %
          (n, d, k, np.max(np.abs(Gd - Gh)), np.max(np.abs(Gd - Go)), np.max(np.abs(Go))))
    np.testing.assert_allclose(Gd, Gh, rtol=1e-13, atol=1e-14)
    # and against the oracle's independent restatement (log-sum-exp)
    np.testing.assert_allclose(Gd, Go, rtol=1e-11, atol=1e-12)


# ------------------------------------------------- 9. host gradient (CPU) ---
@pytest.mark.parametrize("d", range(1, 65))
def test_host_gradient_every_d(oracle, d):
    """svgd_model_logp_grad for k = 1, 3 components and n either side of the
    4- and 8-particle SIMD blocks (1, 7, 8, 9, 67).  Needs no GPU."""
    lib = C.lib()
    for k in (1, 3):
        mus, covs = _gauss_model(oracle, d, k, 31 + d + k)
        h = ctypes.c_void_p()
        assert lib.svgd_model_create(ctypes.byref(h), d, k, C.dptr(np.ascontiguousarray(mus)),
                                     C.dptr(np.ascontiguousarray(covs))) == 0
        try:
            for n in (1, 7, 8, 9, 67):
                X = oracle.splitmix((n, d), 4.0, 3 + n + d)
                G = np.full_like(X, np.nan)
                lib.svgd_model_logp_grad(h, C.dptr(X), n, C.dptr(G))
                np.testing.assert_allclose(G, oracle.logp_grad_gmm(X, mus, covs), rtol=1e-11, atol=1e-12,
                                           err_msg="k=%d n=%d" % (k, n))
        finally:
            lib.svgd_model_destroy(h)
