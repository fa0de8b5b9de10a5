"""The update-site table of tests/_update_cases.py against the plan, without a
GPU: every case's shape and knobs plan the kernel the case names, and the
table reaches each of the eight update sites.  The GPU tests
(tests/test_gpu_update_paths.py, tests/test_gpu_spec_redo.py) assert a
context's phi_kernel_name() against the same prefix.
"""
import numpy as np
import pytest

import svgdcpp_amd as S

import _update_cases as U
from _dispatch import KNOBS


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    """Every case starts from the library's defaults; a case sets what it needs."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("case", [c for c in U.CASES if c.kernel != "imq"], ids=lambda c: c.id)
def test_case_plans_its_kernel(monkeypatch, case):
    for k, v in case.env.items():
        assert k in KNOBS, k  # (only knobs the fixture clears)
        monkeypatch.setenv(k, v)
    name = S.plan_phi_name(case.d, case.n, U.dtype_of(case))
    assert name.startswith(case.prefix), (case.id, name)


def test_case_prefixes_tell_the_paths_apart(monkeypatch):
    """Without its knobs a knob case plans another kernel: the prefixes are
    long enough to notice a knob that no longer acts."""
    for case in U.CASES:
        if case.kernel == "imq" or not case.env:
            continue
        name = S.plan_phi_name(case.d, case.n, U.dtype_of(case))
        assert not name.startswith(case.prefix), (case.id, name)


def test_imq_cases_name_the_padded_dimension():
    for case in U.CASES:
        if case.kernel == "imq":
            assert case.prefix == "k_imq_pass<%d>" % ((case.d + 3) // 4 * 4)
            assert case.site == "k_opt_update" and case.dtype == "f64"


def test_table_names_every_site():
    assert len(U.SITES) == 8
    assert {c.site for c in U.CASES} == set(U.SITES)
    assert len({c.id for c in U.CASES}) == len(U.CASES)
    # k_opt_update behind each of its three phi kernels
    behind = {(c.dtype, c.kernel) for c in U.CASES if c.site == "k_opt_update"}
    assert behind == {("f64", "rbf"), ("f32", "rbf"), ("f64", "imq")}
    # both row-stream geometries, both symmetric dimensions on both forms
    assert {c.d for c in U.CASES if c.site == "k_phi_reduce"} == {5, 12}
    for site in ("k_sym_finish", "k_sym_apply"):
        assert {(c.n, c.d) for c in U.CASES if c.site == site} == {(1700, 8), (1700, 3)}


@pytest.mark.parametrize("d", sorted({c.d for c in U.CASES}))
def test_bounds_are_per_dimension(d):
    lo, up = U.bounds(d)
    s = U.box_scale(d)
    assert lo.shape == up.shape == (d,)
    assert lo[1] == -np.inf and up[1] == np.inf
    assert lo[d - 1] == up[d - 1] == 0.25 * s
    fin = [k for k in range(d - 1) if k != 1]
    assert np.array_equal(lo[fin], [-(0.5 + 0.1 * k) * s for k in fin])
    assert np.array_equal(up[fin], [(0.4 + 0.07 * k) * s for k in fin])
    # no two dimensions share a bound: a shifted element index clamps elsewhere
    assert len(set(lo)) == d and len(set(up)) == d
    # the widest box leaves room for X drawn at scale 1 to lie outside it
    assert -0.8 - 1e-15 <= lo[np.isfinite(lo)].min() and up[np.isfinite(up)].max() <= 0.8
    ilo, iup = U.inverted_bounds(d)
    assert ilo[0] > iup[0]
    assert np.array_equal(ilo[1:], lo[1:]) and np.array_equal(iup[1:], up[1:])
