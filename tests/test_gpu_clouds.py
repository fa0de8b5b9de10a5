"""phi and the median on clustered, shifted and anisotropic clouds.  GPU only.

The rest of the suite draws its particles from a centred uniform cube (plus
single outliers, one translation and coincident points).  After a few dozen
steps on a mixture target the particles sit in separated clusters, far from
the origin, with a different spread per coordinate, and the pair-distance
list is bimodal or has a gap.  tests/_clouds.py builds such inputs and a
long-double reference from direct differences; this module runs on them

  1. the median: keys, selection, ranks and scale on the direct path, the
     bracket path (matrix-core collect against the fp64 collect, bit for bit;
     both sample sizes; both classification Grams), the F32 bracket path, the
     streamed radix fallback and the bucket select against the radix passes;
  2. phi: one case per kernel family at the scale the median heuristic gives
     that cloud -- c6040 at d = 8 has a log2e max|xc|^2 > 300, so the
     symmetric pass hands the step to the row stream (k_phi_sym /
     k_sym_finish / k_sym_apply) and k_phi_rows takes its plain clamped form;
  3. trajectories on a two-mode target: the default step (speculative plan,
     tracked brackets, X mirror) bit-identical to the synchronous one, the
     scale and the positions against the reference at three steps.

Bars (tests/test_clouds_cpu.py keeps a numpy emulation of the device
arithmetic under a fraction of each, on the CPU):
  keys, e = max over pairs |key - hp_key| / (|xc_i|^2 + |xc_j|^2):
      fp64 contexts e <= 4 (d + 4) 2^-53, F32 contexts e <= 2 e32 + 2^-22
      (e32: a numpy fp32 Gram on the same input);
  med bit-equal to the order statistics of the device's own keys, a to
  ln n / med^2 rel 1e-15, each selected squared statistic within
  E = bar 2 max|xc|^2 of the reference's, the ranks those of the plan;
  fp64 phi max-abs 1e-10, F32 phi 1e-4 max|phi|, repeats bit-identical;
  steps: positions 1e-9 against the oracle step from the device's own X_t.
No comparison uses oracle.median_scale: its uncentred Gram form loses
2^-53 |x|^2 / med^2 off-centre (6.6e-5 relative on shift1e6), the device
centres first.  Every case prints its figures ("cloud ..." lines, -s or -rA)
before it asserts.
"""
import ctypes
import functools

import numpy as np
import pytest

import _clouds as K
import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

pytestmark = pytest.mark.gpu

PHI_TOL = 1e-10
F32_REL = 1e-4
F64, F32 = C.SVGD_F64, C.SVGD_F32
PATHS = {C.SVGD_MEDIAN_DIRECT: "DIRECT", C.SVGD_MEDIAN_BRACKET: "BRACKET",
         C.SVGD_MEDIAN_FALLBACK: "FALLBACK", C.SVGD_MEDIAN_REBRACKET: "REBRACKET"}

KNOBS = ("SVGD_PHI_SYM", "SVGD_PHI_B3", "SVGD_PHI_B3_RG", "SVGD_PHI_S1V", "SVGD_PHI_TILE_GENERIC",
         "SVGD_COLLECT_FP64", "SVGD_MCOL_BF16", "SVGD_BUCKET_CAP", "SVGD_MEDIAN_SAMPLE",
         "SVGD_MEDIAN_SIGMA", "SVGD_SPECULATE", "SVGD_TRACK_BRACKET", "SVGD_X_MIRROR",
         "SVGD_TRACK_ERR_MULT", "SVGD_TRACK_MIN_WIDTH")


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    """Every case starts from the library's defaults; a case sets what it needs."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _ctx(X, dtype=F64):
    n, d = X.shape
    c = S.Context(d, n, dtype=dtype)
    c.set_particles(X)
    return c


def _tname(dtype):
    return "f64" if dtype == F64 else "f32"


def _report(what, kind, n, d, err, bar):
    print("cloud %s %s n=%d d=%d err=%.3g bar=%.3g" % (what, kind, n, d, err, bar))


def _ref(kind, n, d):
    return K.ref(kind, n, d, K.seed_of(kind, n, d))


# ================================================================ median ====
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


def _plan_ranks(n):
    lo, hi = ctypes.c_int64(), ctypes.c_int64()
    navg = C.lib().svgd_plan_median_ranks(n, ctypes.byref(lo), ctypes.byref(hi))
    return navg, lo.value, hi.value


def _measure(c):
    """(a, med, path, (sq_lo, sq_hi, rank_lo, rank_hi)) of a median_scale call."""
    a, med = c.median_scale()
    return a, med, c.last_scale()[2], c.last_median_keys()


def _key_bar(r, dtype):
    return K.fp64_key_bound(r.d) if dtype == F64 else K.f32_key_bound(r.e32())


def _check_selected(what, kind, n, d, mk, sq_ref, bar, nmax):
    """The selected squared statistics against the reference's, and the ranks."""
    s_lo, s_hi, r_lo, r_hi = mk
    navg, p_lo, p_hi = _plan_ranks(n)
    E = bar * 2.0 * nmax
    worst = max(abs(float(s_lo) - float(sq_ref[0])), abs(float(s_hi) - float(sq_ref[-1])))
    _report(what + "_stat", kind, n, d, worst, E)
    assert (r_lo, r_hi) == (p_lo, p_hi) == (K.full_list_ranks(n)[0], K.full_list_ranks(n)[-1])
    assert navg == len(sq_ref)
    assert worst <= E


def _median_checks(what, r, c, got, dtype):
    """Everything a median of cloud r on context c must satisfy; returns the
    exact median of the device's own keys."""
    a, med, path, mk = got
    n, d, kind = r.n, r.d, r.kind
    keys = _own_keys(c, n)
    bar = _key_bar(r, dtype)
    e = r.key_error(keys)
    print("cloud %s path %s %s n=%d d=%d: %s" % (what, _tname(dtype), kind, n, d, PATHS.get(path, path)))
    _report(what + "_keys_" + _tname(dtype), kind, n, d, e, bar)
    exp = _median_of_keys(keys, n)
    assert e <= bar
    assert med == exp  # bit-exact selection
    assert med == (np.sqrt(mk[0]) + np.sqrt(mk[1])) / 2
    assert a == pytest.approx(np.log(n) / (exp * exp), rel=1e-15)
    _check_selected(what, kind, n, d, mk, r.sq, bar, r.nmax)
    return exp


DIRECT_CASES = [(F64, d) for d in K.DIRECT_D64] + [(F32, d) for d in K.DIRECT_D32]


@pytest.mark.parametrize("n", K.DIRECT_N)
@pytest.mark.parametrize("dtype,d", DIRECT_CASES, ids=["%s-%d" % (_tname(t), d) for t, d in DIRECT_CASES])
@pytest.mark.parametrize("kind", K.KINDS)
def test_direct_median(kind, dtype, d, n):
    """Every pair a candidate: k_center_d / k_center, k_pair_rows (d <= 16),
    k_pair_tiles<double> (d = 40), the F32 tile kernels.  n = 400 averages
    two statistics (for bal: one from each side of the gap), n = 401 takes one."""
    r = _ref(kind, n, d)
    c = _ctx(r.X, dtype)
    got = _measure(c)
    _median_checks("direct", r, c, got, dtype)
    c.close()
    if dtype == F64:
        assert got[2] == C.SVGD_MEDIAN_DIRECT
    else:  # a row band's region may overflow: the streamed select, as exact
        assert got[2] in (C.SVGD_MEDIAN_DIRECT, C.SVGD_MEDIAN_FALLBACK)


def _bracket(X, monkeypatch, sample, fp64, bf16=True):
    monkeypatch.setenv("SVGD_COLLECT_FP64", "1" if fp64 else "0")
    monkeypatch.setenv("SVGD_MCOL_BF16", "1" if bf16 else "0")
    c = _ctx(X)
    c.set_median_tuning(direct_max_pairs=0, sample_size=sample)  # force the bracket path
    return c, _measure(c)


@pytest.mark.parametrize("n", K.BRACKET_N64)
@pytest.mark.parametrize("d", K.BRACKET_D64)
@pytest.mark.parametrize("kind", K.KINDS)
def test_bracket_median_f64(monkeypatch, kind, d, n):
    """A sampled bracket (2^14 and 2^16 pairs: on bal the sampled quantile
    lands on either side of the gap) and the collect pass: k_pair_mcol with
    the split-bf16 and the f32 classification Gram (d <= 16; above 8 both
    settings take the f32 one), the tile collect at d = 40 -- each bit for bit
    the all-fp64 collect (SVGD_COLLECT_FP64=1) and the exact order statistics
    of the device's own keys."""
    r = _ref(kind, n, d)
    exp = None
    for sample in (1 << 14, 1 << 16):
        f, want = _bracket(r.X, monkeypatch, sample, fp64=True)
        f.close()
        for bf16 in ((True, False) if d <= 16 else (True,)):
            what = "bracket[s=%d,%s]" % (sample, "bf16" if bf16 else "f32")
            c, got = _bracket(r.X, monkeypatch, sample, fp64=False, bf16=bf16)
            if exp is None:
                exp = _median_checks(what, r, c, got, F64)
            else:
                print("cloud %s path f64 %s n=%d d=%d: %s" % (what, kind, n, d, PATHS.get(got[2], got[2])))
            c.close()
            assert got[2] != C.SVGD_MEDIAN_DIRECT and want[2] != C.SVGD_MEDIAN_DIRECT, (what, got, want)
            if kind == "uniform":
                assert got[2] in (C.SVGD_MEDIAN_BRACKET, C.SVGD_MEDIAN_REBRACKET), (what, got)
            assert got[:2] == want[:2] and got[3] == want[3], (what, got, want)  # bit for bit
            assert got[1] == exp, what
            _check_selected(what, kind, n, d, got[3], r.sq, K.fp64_key_bound(d), r.nmax)


def _median32(X, monkeypatch, ref):
    monkeypatch.setenv("SVGD_COLLECT_FP64", "1" if ref else "0")
    c = _ctx(X, F32)
    c.set_median_tuning(direct_max_pairs=0)
    return c, _measure(c)


@pytest.mark.parametrize("n", K.BRACKET_N32)
@pytest.mark.parametrize("d", K.BRACKET_D32)
@pytest.mark.parametrize("kind", K.KINDS)
def test_bracket_median_f32(monkeypatch, kind, d, n):
    """k_pair_tcol / k_pair_tcol3 against k_pair_tiles<float> (the same scale,
    median and selected keys, bit for bit) and the device's own fp32 keys.
    The path is compared on the control only, as everywhere in this module:
    k_pair_tcol deals its tiles in row bands, so on a cloud sorted by cluster
    the blocks that own the within-cluster bands can overflow their regions
    where k_pair_tiles' even deal does not (tight at n = 2050: the streamed
    fallback against the bracket path, the same keys)."""
    r = _ref(kind, n, d)
    c, got = _median32(r.X, monkeypatch, ref=False)
    _median_checks("bracket", r, c, got, F32)
    c.close()
    f, want = _median32(r.X, monkeypatch, ref=True)
    f.close()
    print("cloud bracket path f32 tile collect %s n=%d d=%d: %s" % (kind, n, d, PATHS.get(want[2], want[2])))
    assert got[2] != C.SVGD_MEDIAN_DIRECT and want[2] != C.SVGD_MEDIAN_DIRECT, (got, want)
    assert got[:2] == want[:2] and got[3] == want[3], (got, want)
    if kind == "uniform":
        assert got == want  # the same counts: the same path


FALLBACK_CASES = [(F64, d) for d in K.FALLBACK_D64] + [(F32, d) for d in K.FALLBACK_D32]


@pytest.mark.parametrize("dtype,d", FALLBACK_CASES, ids=["%s-%d" % (_tname(t), d) for t, d in FALLBACK_CASES])
@pytest.mark.parametrize("kind", K.FALLBACK_KINDS)
def test_fallback_median(kind, dtype, d):
    """A 1-key candidate capacity overflows every region: the streamed radix
    select (the histogram passes of k_pair_rows / k_pair_tiles) on a list
    with a gap (bal) and on keys twelve octaves apart (tight)."""
    n = K.FALLBACK_N
    r = _ref(kind, n, d)
    c = _ctx(r.X, dtype)
    c.set_median_tuning(direct_max_pairs=0, sample_size=1 << 12, candidate_capacity=1)
    got = _measure(c)
    _median_checks("fallback", r, c, got, dtype)
    c.close()
    assert got[2] == C.SVGD_MEDIAN_FALLBACK


@pytest.mark.parametrize("kind", K.BUCKET_KINDS)
def test_bucket_select_matches_radix_passes(monkeypatch, kind):
    """SVGD_BUCKET_CAP 16384 (the one-work-group bucket select) and 0 (the
    per-digit passes) on a gapped list: the same (a, med)."""
    n, d = K.BUCKET_SHAPE
    r = _ref(kind, n, d)
    res = []
    for cap in ("16384", "0"):
        monkeypatch.setenv("SVGD_BUCKET_CAP", cap)
        c = _ctx(r.X)
        c.set_median_tuning(direct_max_pairs=0)
        got = _measure(c)
        _median_checks("bucket_cap[%s]" % cap, r, c, got, F64)
        c.close()
        assert got[2] != C.SVGD_MEDIAN_DIRECT
        res.append(got[:2] + (got[3],))
    assert res[0] == res[1]


# =================================================================== phi ====
PHI_NAMES = {
    (F64, 3): "k_phi_rows<3, 4, 8, 8192, 8>", (F64, 12): "k_phi_rows<12, 2, 8, 8192, 8>",
    (F64, 24): "k_phi<double, 32, 2, 8, true, false>", (F64, 50): "k_phi<double, 64, 4, 8, true, false>",
    (F32, 6): "k_phi<float, 8, 1, 4, false, false>", (F32, 14): "k_phi_f32s<16, 1>",
    (F32, 24): "k_phi_b3<32, 2, 8, false, 1>", (F32, 64): "k_phi_b3<64, 4, 8, true, 1>",
}


@functools.lru_cache(maxsize=2)
def _phi_inputs(kind, n, d, use_oracle):
    """(X, G, a, ref, max|xc|^2): a is the median heuristic's scale from the
    long-double statistics, ref hp_phi (oracle.phi for the symmetric-pass
    sizes: tests/test_clouds_cpu.py pins it to hp_phi on these inputs)."""
    seed = K.seed_of(kind, n, d)
    X = K.cloud(kind, n, d, seed)
    G = K.gradients(n, d, seed)
    _, med = K.hp_stats(X)
    a = float(np.log(n) / med ** 2)
    if use_oracle:
        import oracle
        ref = oracle.phi(X, G, a)
    else:
        ref = K.hp_phi(X, G, a).astype(np.float64)
    nmax = float(K.centred(X)[1].max())
    for arr in (X, G, ref):
        arr.flags.writeable = False
    return X, G, a, ref, nmax


def _phi_case(what, kind, n, d, dtype, name, use_oracle=False):
    X, G, a, ref, nmax = _phi_inputs(kind, n, d, use_oracle)
    c = _ctx(X, dtype)
    got_name = c.phi_kernel_name()
    out = c.phi(G, a)
    again = c.phi(G, a)
    c.close()
    top = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(out - ref)))
    y = a * np.log2(np.e) * nmax
    print("cloud %s[%s] %s a=%.4g y=%.4g max|phi|=%.3g" % (what, got_name, kind, a, y, top))
    if dtype == F64:
        _report(what, kind, n, d, err, PHI_TOL)
    else:
        _report(what + "_rel", kind, n, d, err / top, F32_REL)
    assert got_name == name or (name.endswith("*") and got_name.startswith(name[:-1])), got_name
    assert top >= 0.01  # the absolute bar is at least 1e-8 relative
    assert np.all(np.isfinite(out))
    assert np.array_equal(out, again)  # deterministic
    assert err <= (PHI_TOL if dtype == F64 else F32_REL * top)
    return y


@pytest.mark.parametrize("n,d", K.PHI_ROWS + K.PHI_TILES)
@pytest.mark.parametrize("kind", K.PHI_KINDS)
def test_phi_f64(kind, n, d):
    """k_phi_rows<D, 4 | 2> + k_phi_reduce (c6040: the plain clamped exponent
    form) and k_phi<double, 32 | 64>."""
    _phi_case("phi_rows" if d <= 16 else "phi_tiles", kind, n, d, F64, PHI_NAMES[F64, d])


@pytest.mark.parametrize("sym", ["1", "2"])
@pytest.mark.parametrize("n,d", K.PHI_SYM)
@pytest.mark.parametrize("kind", K.PHI_KINDS)
def test_phi_sym(monkeypatch, kind, n, d, sym):
    """The symmetric pass forced (1: k_sym_finish forms phi; 2: the sharded
    form at one rank, k_sym_apply), two work-group blocks of 1536 at d = 8.
    c6040 at d = 8 is past a log2e max|xc|^2 = 300: the record prep hands the
    step to the row stream inside k_phi_sym; c6040_near stays inside."""
    monkeypatch.setenv("SVGD_PHI_SYM", sym)
    y = _phi_case("phi_sym%s" % sym, kind, n, d, F64, "k_phi_sym*", use_oracle=True)
    if kind == "c6040" and d == 8:
        assert y > 300
    if kind == "c6040_near":
        assert y < 300


@pytest.mark.parametrize("n,d", K.PHI_F32)
@pytest.mark.parametrize("kind", K.F32_PHI_KINDS)
def test_phi_f32(kind, n, d):
    """k_phi<float>, k_phi_f32s, k_phi_b3 (KP 32 and 64)."""
    _phi_case("phi_f32", kind, n, d, F32, PHI_NAMES[F32, d])


# ========================================================== trajectories ====
@pytest.mark.parametrize("d", K.TRAJ_D)
@pytest.mark.parametrize("kind", K.TRAJ_KINDS)
def test_two_mode_trajectory(oracle, monkeypatch, kind, d):
    """14 Adam steps on a two-component Gaussian sum whose means are the two
    cluster centres, from the clustered cloud.  A: the defaults (speculative
    plan, tracked brackets, X mirror).  B: all three off.  Every step: the
    same particles and scale, bit for bit.  Steps 0, 6 and 13: the selected
    statistics of X_t against the reference's, and the positions against the
    oracle step from the device's own X_t."""
    n, steps = K.TRAJ_N, 14
    X0 = K.cloud(kind, n, d, K.seed_of(kind, n, d))
    _, L = K.split(kind, n)
    mus = np.zeros((2, d))
    mus[0, 0] = L
    covs = np.stack([np.eye(d), np.eye(d)])
    model = S.GaussianSum(list(mus), list(covs))
    ctxs = []
    for off in (False, True):
        for k in ("SVGD_SPECULATE", "SVGD_TRACK_BRACKET", "SVGD_X_MIRROR"):
            if off:
                monkeypatch.setenv(k, "0")
            else:
                monkeypatch.delenv(k, raising=False)
        c = _ctx(X0)
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.1, 0.9, 0.999, 1e-8)
        c.diagnostics()
        ctxs.append(c)
    A, B = ctxs
    opt = oracle.Adam((n, d), 0.1, 0.9, 0.999)
    bar = K.fp64_key_bound(d)
    paths = []
    for step in range(steps):
        Xt = A.get_particles()
        for c in (A, B):
            c.step_with_model(model)
        Xa, Xb = A.get_particles(), B.get_particles()
        sa, sb = A.last_scale(), B.last_scale()
        paths.append((PATHS.get(sa[2], sa[2]), PATHS.get(sb[2], sb[2])))
        assert np.array_equal(Xa, Xb), step
        assert sa[:2] == sb[:2], step
        a_dev, med_dev = sa[:2]
        G = oracle.logp_grad_gmm(Xt, mus, covs)
        Xr = Xt.copy()
        oracle.apply_update(Xr, opt.step(oracle.phi(Xt, G, a_dev)))
        if step in (0, 6, 13):
            sq, med = K.hp_stats(Xt)
            mk = A.last_median_keys()
            nmax = float(K.centred(Xt)[1].max())
            _check_selected("traj[step %d]" % step, kind, n, d, mk, sq, bar, nmax)
            assert med_dev == (np.sqrt(mk[0]) + np.sqrt(mk[1])) / 2
            assert a_dev == pytest.approx(np.log(n) / (med_dev * med_dev), rel=1e-15)
            err = float(np.max(np.abs(Xa - Xr)))
            _report("traj[step %d]_pos" % step, kind, n, d, err, 1e-9)
            print("cloud traj[step %d] %s d=%d a=%.6g med=%.6g (reference med %.6g)" %
                  (step, kind, d, a_dev, med_dev, med))
            assert err <= 1e-9
    da, db = A.diagnostics(), B.diagnostics()
    for name, dg in (("A", da), ("B", db)):
        print("cloud traj diag %s %s d=%d trk_steps=%d trk_miss=%d spec_steps=%d mirror_steps=%d" %
              (name, kind, d, dg["trk_steps"], dg["trk_miss"], dg["spec_steps"], dg["mirror_steps"]))
    print("cloud traj paths %s d=%d (A, B): %s" % (kind, d, paths))
    A.close()
    B.close()
