"""The update behind every phi path: the optimizer (Adam, AdaGrad, RMSProp),
the min-then-max clamp with per-dimension bounds, at each of the eight update
sites of tests/_update_cases.py.  GPU only.

  * bit-exact: svgd_phi and svgd_step run the same phi kernel with the same
    launch geometry, so the oracle's optimizer and clamp applied to the
    device's own phi must give the device's particles bit for bit
    (the oracle restates the reference without contraction, as opt_apply does)
  * a fixed SPD matrix scale on one case per site that takes one: the same
    bit equality, and phi against oracle.phi_matrix (1e-10 fp64, REL max|ref|
    for F32, tests/test_gpu_f32.py)
  * per-step oracle parity with the median scale where no test had it: fp64
    tiles at d = 24 / 64 and k_sym_apply (scale rel 1e-12, positions 1e-9)
  * a setter between two steps acts from the next step on (svgd_set_bounds
    right behind a step whose chain is still queued), and so does the next
    step's G

The bounds are per dimension (tests/_update_cases.py): a site that clamped
with a shifted dimension's bound fails the bit equality and the box checks.
"""
import functools

import numpy as np
import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

import _update_cases as U
from _dispatch import KNOBS
from test_gpu_f32 import REL
from test_gpu_matrix_scale import _spd

pytestmark = pytest.mark.gpu

OPTS = ["adam", "adagrad", "rmsprop"]


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def set_optimizer(c, oracle, name, shape, lr=0.1):
    """The device optimizer and the oracle's twin of it."""
    if name == "adam":
        c.set_optimizer(C.SVGD_OPT_ADAM, lr, 0.9, 0.999, 1e-8)
        return oracle.Adam(shape, lr, 0.9, 0.999)
    if name == "adagrad":
        c.set_optimizer(C.SVGD_OPT_ADAGRAD, lr, 0.0, 0.0, 1e-8)
        return oracle.AdaGrad(shape, lr)
    c.set_optimizer(C.SVGD_OPT_RMSPROP, lr, 0.9, 0.0, 1e-8)
    return oracle.RMSProp(shape, lr, 0.9)


def make_context(monkeypatch, case, X):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    c = S.Context(case.d, case.n, dtype=U.dtype_of(case))
    c.set_particles(X)
    if case.kernel == "imq":
        c.set_kernel("imq")
    name = c.phi_kernel_name()
    assert name.startswith(case.prefix), (case.id, name)
    return c


@functools.lru_cache(maxsize=None)
def _inputs(case_id):
    """(X0, G, a) of a case, computed once: X at scale 1, G at scale 1 with
    exact zeros in its first row and one row at 1e8 (v and the square root
    see a wide range), a the median scale of X0."""
    import oracle
    case = U.BY_ID[case_id]
    n, d = case.n, case.d
    X = oracle.splitmix((n, d), 1.0, 1000 + 7 * n + d)
    if case.far:
        X[:3] += 40.0
    G = oracle.splitmix((n, d), 1.0, 2000 + 7 * n + d)
    G[0] = 0.0
    # (signs alternating by dimension: that row drives every particle the same
    # way, towards the upper bounds of the even dimensions and the lower
    # bounds of the odd ones)
    G[n // 2] = np.abs(G[n // 2]) * 1e8 * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    a = oracle.median_scale(X)[0]
    for arr in (X, G):
        arr.setflags(write=False)
    return X, G, a


def _step(c, G):
    c.check(c.lib.svgd_step(c.h, C.dptr(G)))


def _run_bit_exact(c, oracle, o_opt, X, G, a, lo, up, steps=3):
    """steps x (the device's own phi, one device step, the oracle's update of
    that phi): particles bit-identical after every step.  Returns X_T, the
    last step's positions before the clamp and the phis."""
    Xo = X.copy()
    phis = []
    for t in range(steps):
        ph = c.phi(G, a)
        _step(c, G)
        delta = o_opt.step(ph)
        Xpre = Xo + delta
        oracle.apply_update(Xo, delta, lo, up)
        Xd = c.get_particles()
        bad = np.flatnonzero((Xd != Xo).ravel())
        assert bad.size == 0, ("step %d: %d elements differ, first at %s, max |diff| %.3g"
                               % (t, bad.size, np.unravel_index(bad[0], Xd.shape),
                                  np.max(np.abs(Xd - Xo))))
        phis.append(ph)
    return Xo, Xpre, phis


@pytest.mark.parametrize("bnd", list(U.BOUNDS))
@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("case", U.CASES, ids=lambda c: c.id)
def test_update_bit_exact(oracle, monkeypatch, case, opt, bnd):
    X, G, a = _inputs(case.id)
    c = make_context(monkeypatch, case, X)
    o_opt = set_optimizer(c, oracle, opt, X.shape)
    c.set_scale(C.SVGD_SCALE_FIXED, a)
    lo, up = U.BOUNDS[bnd](case.d)
    if lo is not None:
        c.set_bounds(lo, up)
    XT, Xpre, phis = _run_bit_exact(c, oracle, o_opt, X, G, a, lo, up)
    c.close()
    assert np.all(np.isfinite(XT))
    assert all(np.all(np.isfinite(p)) for p in phis)
    if lo is not None:
        n_lo, n_up = U.assert_bounds_exercised(XT, lo, up, Xpre)
        # the big row drives the even dimensions up and the odd ones down
        # (d = 3: dimension 0 alone has a box, and the inverted bounds take it)
        assert (n_lo > 0 and n_up > 0) if case.d >= 5 else (n_up > 0 or bnd == "inverted")


MATRIX_CASES = ["rows-r4", "t64-d24", "t32-d6", "f32s-d14", "b3-d24"]


@pytest.mark.parametrize("i,case_id", list(enumerate(MATRIX_CASES)), ids=MATRIX_CASES)
def test_update_bit_exact_matrix_scale(oracle, monkeypatch, i, case_id):
    """A fixed SPD matrix scale (M = _spd(d, d) / d, a = 0 in svgd_phi) on the
    row stream (its 4-wave geometry), both tile kernels + k_opt_update and both
    streamed F32 epilogues; the optimizer rotates over the cases.  G is O(1)
    here (zeros in the first row, no 1e8 row): the phi bars are the project's
    absolute 1e-10 (fp64) and REL max|ref| (F32) for such inputs."""
    case = U.BY_ID[case_id]
    X, G0, _ = _inputs(case_id)
    G = G0.copy()
    G[case.n // 2] = G0[case.n // 2] * 1e-8
    M = _spd(case.d, case.d) / case.d
    c = make_context(monkeypatch, case, X)
    o_opt = set_optimizer(c, oracle, OPTS[i % 3], X.shape)
    c.set_scale_matrix(M)
    lo, up = U.bounds(case.d)
    c.set_bounds(lo, up)
    # the reference phi of X_0 .. X_2 follows the oracle's (= the device's) trajectory
    Xo = X.copy()
    worst = 0.0
    for t in range(3):
        ref = oracle.phi_matrix(Xo, G, M)
        ph = c.phi(G, 0.0)
        tol = 1e-10 if case.dtype == "f64" else REL * float(np.max(np.abs(ref)))
        err = float(np.max(np.abs(ph - ref)))
        worst = max(worst, err / tol)
        print("update_paths matrix %s step %d: phi err %.3g (bar %.3g)" % (case_id, t, err, tol))
        assert err <= tol, (t, err, tol)
        _step(c, G)
        oracle.apply_update(Xo, o_opt.step(ph), lo, up)
        assert np.array_equal(c.get_particles(), Xo), t
    c.close()
    U.assert_bounds_exercised(Xo, lo, up)


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("case_id", ["t64-d24", "t64-d64", "symapp-d8"])
def test_steps_match_oracle_per_step(oracle, monkeypatch, case_id, opt):
    """Five steps of step_with_model (median scale, two-component Gaussian
    sum, per-dimension bounds), each against the oracle step from the
    device's own X_t: fp64 tiles + k_opt_update at d = 24 and 64, k_sym_apply
    at (1700, 8)."""
    case = U.BY_ID[case_id]
    n, d = case.n, case.d
    X, _, _ = _inputs(case_id)
    mus = oracle.splitmix((2, d), 1.0, 77 + d)
    covs = np.stack([np.eye(d) * (1.0 + 0.25 * k) for k in range(2)])
    model = S.GaussianSum(list(mus), list(covs))
    c = make_context(monkeypatch, case, X)
    o_opt = set_optimizer(c, oracle, opt, X.shape)
    lo, up = U.bounds(d)
    c.set_bounds(lo, up)
    worst = worst_a = 0.0
    for t in range(5):
        Xt = c.get_particles()
        a_ref, _ = oracle.median_scale(Xt)
        ph_ref = oracle.phi(Xt, oracle.logp_grad_gmm(Xt, mus, covs), a_ref)
        c.step_with_model(model)
        a_dev = c.last_scale()[0]
        Xref = Xt.copy()
        oracle.apply_update(Xref, o_opt.step(ph_ref), lo, up)
        Xdev = c.get_particles()
        err = float(np.max(np.abs(Xdev - Xref)))
        worst, worst_a = max(worst, err), max(worst_a, abs(a_dev - a_ref) / abs(a_ref))
        assert a_dev == pytest.approx(a_ref, rel=1e-12), t
        assert err <= 1e-9, (t, err)
    c.close()
    print("update_paths per-step %s %s: worst position err %.3g (bar 1e-9), scale rel %.3g (bar 1e-12)"
          % (case_id, opt, worst, worst_a))
    U.assert_bounds_exercised(Xdev, lo, up)


@pytest.mark.parametrize("n,d,prefix", [(8192, 64, "k_phi<double, 64"), (16384, 8, "k_phi_rows<8, 4,")])
def test_set_bounds_acts_from_the_next_step(oracle, n, d, prefix):
    """svgd_step returns with its phi chain queued (fixed scale: nothing in
    the step waits on the host); bounds set right behind it must not reach
    that step's clamp: X_1 is the oracle update of the device's phi clamped
    with the old bounds, X_2 with the new ones, bit for bit.  The shapes give
    a chain that is long against a d-element copy (k_opt_update behind the
    fp64 tiles; the row stream's fused epilogue)."""
    X = oracle.splitmix((n, d), 1.0, 31 + n)
    G = oracle.splitmix((n, d), 1.0, 32 + n)
    a = float(np.log(n) / (2.0 * d / 3.0))  # ln N / E|x - x'|^2 of the uniform cube
    c = S.Context(d, n)
    assert c.phi_kernel_name().startswith(prefix), c.phi_kernel_name()
    c.set_particles(X)
    o_opt = set_optimizer(c, oracle, "adam", X.shape)
    c.set_scale(C.SVGD_SCALE_FIXED, a)
    old = (np.full(d, -10.0), np.full(d, 10.0))
    new = (np.full(d, -0.01), np.full(d, 0.01))
    c.set_bounds(*old)
    Xo = X.copy()
    ph = c.phi(G, a)
    _step(c, G)
    c.set_bounds(*new)
    X1 = c.get_particles()
    oracle.apply_update(Xo, o_opt.step(ph), *old)
    assert np.max(np.abs(Xo)) > 0.5  # (the old bounds clamp nothing, the new ones would)
    early = int(np.sum(np.abs(X1) == 0.01))
    assert np.array_equal(X1, Xo), "%d elements clamped with the bounds set after the step" % early
    ph = c.phi(G, a)
    _step(c, G)
    X2 = c.get_particles()
    oracle.apply_update(Xo, o_opt.step(ph), *new)
    assert np.array_equal(X2, Xo)
    assert np.all(np.abs(X2) <= 0.01) and np.any(X2 == 0.01) and np.any(X2 == -0.01)
    c.close()


def test_next_gradient_does_not_reach_the_queued_step(oracle):
    """The same hazard for G: svgd_step(G1) returns with its phi chain queued,
    and the next step's G2 goes up on the copy stream, which must not land in
    G before that chain has read G1.  X_1 is the oracle update of the device's
    own phi of (X_0, G1), bit for bit (the case above); X_2 is then the oracle
    step of (X_1, G2) at the project's position bar, 1e-9 -- a G2 row read by
    step 1 moves Adam's first increment of that row by up to 2 lr."""
    n, d = 16384, 8
    X = oracle.splitmix((n, d), 1.0, 41 + n)
    G1 = oracle.splitmix((n, d), 1.0, 42 + n)
    G2 = np.ascontiguousarray(-G1[::-1])
    a = float(np.log(n) / (2.0 * d / 3.0))
    c = S.Context(d, n)
    assert c.phi_kernel_name().startswith("k_phi_rows<8, 4,"), c.phi_kernel_name()
    c.set_particles(X)
    o_opt = set_optimizer(c, oracle, "adam", X.shape)
    c.set_scale(C.SVGD_SCALE_FIXED, a)
    ph1 = c.phi(G1, a)
    _step(c, G1)
    _step(c, G2)
    X2 = c.get_particles()
    Xo = X.copy()
    oracle.apply_update(Xo, o_opt.step(ph1))
    oracle.apply_update(Xo, o_opt.step(oracle.phi(Xo, G2, a)))
    err = float(np.max(np.abs(X2 - Xo)))
    print("update_paths queued G: position err %.3g (bar 1e-9)" % err)
    assert err <= 1e-9
    c.close()
