"""The symmetric phi pass (k_phi_sym) after the reordering of a skew step's
LDS reads and the rotated record address: the block-count cases of its unit
plan at d = 8 (B = 1536) and one more-than-a-block case at d = 5 (B = 2048)
and d = 2 (B = 4096), forced with SVGD_PHI_SYM=1 (one-rank finish) and =2
(the sharded form at one rank).  GPU only.

  * phi from identical (X, G, a) against the CPU oracle: max-abs <= 1e-10
  * the two forms: bit-identical to each other
  * two launches of one form: bit-identical
  * three steps (median + phi + Adam) at N = 3073, d = 8 against the oracle
    step: scale rel <= 1e-12, positions <= 1e-9 (test_gpu_sym.py's bars)
  * far outliers at N = 1600, d = 8: the hand-over to the row stream inside
    k_phi_sym, same phi bar
"""
import numpy as np
import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

pytestmark = pytest.mark.gpu

PHI_TOL = 1e-10
A = 0.37

# d = 8: one diagonal tile only; nb = 2 with an almost empty last block;
# nb = 3; nb = 4 (an even count: the half slot is used).  d = 5, d = 2: nb = 2.
SHAPES = [(1536, 8), (1537, 8), (3073, 8), (4700, 8), (2049, 5), (4097, 2)]
FORMS = ["1", "2"]

_inputs = {}  # (n, d) -> (X, G, oracle phi): formed once, never written to
_device = {}  # (n, d, form) -> (first launch, second launch)


def _case(oracle, n, d):
    if (n, d) not in _inputs:
        X = oracle.splitmix((n, d), 2.0, 700 + n + d)
        G = oracle.splitmix((n, d), 1.0, 800 + n + d)
        ref = oracle.phi(X, G, A)
        for v in (X, G, ref):
            v.setflags(write=False)
        _inputs[(n, d)] = (X, G, ref)
    return _inputs[(n, d)]


def _phi_twice(oracle, monkeypatch, n, d, form):
    if (n, d, form) not in _device:
        X, G, _ = _case(oracle, n, d)
        monkeypatch.setenv("SVGD_PHI_SYM", form)
        c = S.Context(d, n)
        c.set_particles(np.array(X))
        assert c.phi_kernel_name().startswith("k_phi_sym")
        p1 = c.phi(np.array(G), A)
        p2 = c.phi(np.array(G), A)
        c.close()
        _device[(n, d, form)] = (p1, p2)
    return _device[(n, d, form)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_forced_sym_phi_matches_oracle_and_repeats(oracle, monkeypatch, n, d, form):
    p1, p2 = _phi_twice(oracle, monkeypatch, n, d, form)
    _, _, ref = _case(oracle, n, d)
    err = float(np.max(np.abs(p1 - ref)))
    print(f"n={n} d={d} form={form}: max-abs err {err:.3g}")
    assert np.array_equal(p1, p2)
    assert err <= PHI_TOL


@pytest.mark.parametrize("n,d", SHAPES)
def test_forced_sym_forms_are_bit_identical(oracle, monkeypatch, n, d):
    one = _phi_twice(oracle, monkeypatch, n, d, "1")[0]
    two = _phi_twice(oracle, monkeypatch, n, d, "2")[0]
    assert np.array_equal(one, two)


@pytest.mark.parametrize("form", FORMS)
def test_three_adam_steps_match_oracle(oracle, monkeypatch, form):
    n, d, k = 3073, 8, 4
    monkeypatch.setenv("SVGD_PHI_SYM", form)
    X = oracle.splitmix((n, d), 3.0, 0x5EED)
    mus = oracle.splitmix((k, d), 3.0, 0x5EEE)
    covs = np.stack([np.eye(d) * (1.0 + 0.25 * q) for q in range(k)])
    model = S.GaussianSum(list(mus), list(covs))
    c = S.Context(d, n)
    c.set_particles(X)
    c.set_optimizer(C.SVGD_OPT_ADAM, 0.1, 0.9, 0.999, 1e-8)
    ref_opt = oracle.Adam((n, d), 0.1, 0.9, 0.999)
    assert c.phi_kernel_name().startswith("k_phi_sym")
    Xt = X.copy()
    for step in range(3):
        c.step_with_model(model)
        a_dev, _, _ = c.last_scale()
        a_ref, _ = oracle.median_scale(Xt)
        assert a_dev == pytest.approx(a_ref, rel=1e-12)
        G = oracle.logp_grad_gmm(Xt, mus, covs)
        Xr = Xt.copy()
        oracle.apply_update(Xr, ref_opt.step(oracle.phi(Xt, G, a_dev)))
        X1 = c.get_particles()
        err = float(np.max(np.abs(X1 - Xr)))
        print(f"form={form} step {step}: max-abs position err {err:.3g}")
        assert err <= 1e-9
        Xt = X1
    c.close()


@pytest.mark.parametrize("form", FORMS)
def test_far_outliers_hand_over_inside_the_kernel(oracle, monkeypatch, form):
    """a log2e max|xc|^2 >> 300 (rows shifted by 40): the record prep's flag
    hands the step to the row stream, which k_phi_sym itself runs; more than
    one block of rows (N = 1600 > B = 1536)."""
    n, d = 1600, 8
    monkeypatch.setenv("SVGD_PHI_SYM", form)
    X = oracle.splitmix((n, d), 1.0, 91)
    X[:3] += 40.0
    G = oracle.splitmix((n, d), 1.0, 92)
    a = 0.5
    ref = oracle.phi(X, G, a)
    c = S.Context(d, n)
    c.set_particles(X)
    assert c.phi_kernel_name().startswith("k_phi_sym")
    ph = c.phi(G, a)
    c.close()
    err = float(np.max(np.abs(ph - ref)))
    print(f"form={form}: max-abs err {err:.3g}")
    assert err <= PHI_TOL
