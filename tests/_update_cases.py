"""The update sites of the phi paths, one table: every place where a phi
kernel (or k_opt_update behind it) applies opt_elem -- the optimizer, the
min-then-max clamp, the speculative backup and the host mirror -- at the
smallest shape that still takes it.  Checked against the plan on the CPU
(tests/test_update_cases_cpu.py) and run on the GPU
(tests/test_gpu_update_paths.py, tests/test_gpu_spec_redo.py).

A case is (id, dtype, n, d, env, kernel, prefix, site):
  dtype   "f64" / "f32"
  env     the knobs the case sets (every other knob of _dispatch.KNOBS unset)
  kernel  "rbf" / "imq" (Context.set_kernel)
  prefix  what phi_kernel_name() / plan_phi_name() must start with (for IMQ
          the name is k_imq_pass<d padded to 4>, chosen after the plan)
  site    the update site, one of SITES
  far     rows 0..2 moved 40 along every axis: the symmetric form leaves its
          exponent range and the row stream's partials are summed by the
          finish / apply (sym_fb_phi, their second record form)
"""
import collections

import numpy as np

from svgdcpp_amd import _capi as C

Case = collections.namedtuple("Case", "id dtype n d env kernel prefix site far")

# the eight opt_elem call sites of svgd_kernels.hip
SITES = ("k_phi_reduce", "k_sym_finish", "k_sym_finish/rows", "k_sym_apply", "k_sym_apply/rows",
         "k_opt_update", "k_phi_f32s", "k_phi_b3")


def _c(id, dtype, n, d, env, prefix, site, kernel="rbf", far=False):
    return Case(id, dtype, n, d, dict(env), kernel, prefix, site, far)


CASES = [
    # k_phi_reduce: R = 4 rows per lane (d <= 8) and R = 2
    _c("rows-r4", "f64", 333, 5, {}, "k_phi_rows<5, 4,", "k_phi_reduce"),
    _c("rows-r2", "f64", 333, 12, {}, "k_phi_rows<12, 2,", "k_phi_reduce"),
    # the symmetric pass, two work-group blocks of 1536 rows (d = 8) / one of
    # 3072 (d = 3): the one-rank finish, and the sharded form at one rank
    _c("symfin-d8", "f64", 1700, 8, {"SVGD_PHI_SYM": "1"}, "k_phi_sym<8>", "k_sym_finish"),
    _c("symfin-d3", "f64", 1700, 3, {"SVGD_PHI_SYM": "1"}, "k_phi_sym<3>", "k_sym_finish"),
    _c("symapp-d8", "f64", 1700, 8, {"SVGD_PHI_SYM": "2"}, "k_phi_sym<8>", "k_sym_apply"),
    _c("symapp-d3", "f64", 1700, 3, {"SVGD_PHI_SYM": "2"}, "k_phi_sym<3>", "k_sym_apply"),
    # ... and their row-stream record form (far outliers)
    _c("symfin-far", "f64", 1700, 8, {"SVGD_PHI_SYM": "1"}, "k_phi_sym<8>", "k_sym_finish/rows", far=True),
    _c("symapp-far", "f64", 1700, 8, {"SVGD_PHI_SYM": "2"}, "k_phi_sym<8>", "k_sym_apply/rows", far=True),
    # fp64 tiles + k_opt_update: KP 32, KP 64, KP 64 with the S1V column
    _c("t64-d24", "f64", 300, 24, {}, "k_phi<double, 32, 2, 8, true, false>", "k_opt_update"),
    _c("t64-d33", "f64", 300, 33, {}, "k_phi<double, 64, 4, 8, true, false>", "k_opt_update"),
    _c("t64-d64", "f64", 300, 64, {}, "k_phi<double, 64, 4, 8, true, true>", "k_opt_update"),
    # generic fp32 tiles + k_opt_update
    _c("t32-d6", "f32", 333, 6, {}, "k_phi<float, 8,", "k_opt_update"),
    _c("t32-d24", "f32", 333, 24, {"SVGD_PHI_TILE_GENERIC": "1"}, "k_phi<float, 32,", "k_opt_update"),
    # the streamed fp32 kernels' fused epilogues
    _c("f32s-d14", "f32", 333, 14, {}, "k_phi_f32s<16, 1>", "k_phi_f32s"),
    _c("f32s-d24", "f32", 333, 24, {"SVGD_PHI_B3": "0"}, "k_phi_f32s<32, 2>", "k_phi_f32s"),
    _c("b3-d24", "f32", 333, 24, {}, "k_phi_b3<32, 2, 8, false, 1>", "k_phi_b3"),
    _c("b3-d64", "f32", 333, 64, {}, "k_phi_b3<64, 4, 8, true, 1>", "k_phi_b3"),
    _c("b3-d64-rg2", "f32", 333, 64, {"SVGD_PHI_B3_RG": "2"}, "k_phi_b3<64, 4, 8, true, 2>", "k_phi_b3"),
    # IMQ + k_opt_update
    _c("imq-d8", "f64", 333, 8, {}, "k_imq_pass<8>", "k_opt_update", kernel="imq"),
    _c("imq-d33", "f64", 300, 33, {}, "k_imq_pass<36>", "k_opt_update", kernel="imq"),
]
BY_ID = {c.id: c for c in CASES}


def dtype_of(case):
    return C.SVGD_F64 if case.dtype == "f64" else C.SVGD_F32


def box_scale(d):
    """The widest box (the last unpinned dimension's) stays inside +-0.8, so
    that X drawn at scale 1 keeps values of the unbounded dimension 1 outside
    every box; 1 while it already does (d <= 5)."""
    return min(1.0, 0.8 / (0.5 + 0.1 * max(0, d - 2)))


def bounds(d):
    """Per-dimension bounds, never uniform: lower[k] = -(0.5 + 0.1 k),
    upper[k] = 0.4 + 0.07 k (times box_scale(d)); dimension 1 unbounded; the
    last dimension pinned (lower == upper == 0.25 box_scale)."""
    s = box_scale(d)
    k = np.arange(d, dtype=np.float64)
    lo, up = -(0.5 + 0.1 * k) * s, (0.4 + 0.07 * k) * s
    lo[d - 1] = up[d - 1] = 0.25 * s
    if d > 1:
        lo[1], up[1] = -np.inf, np.inf
    return lo, up


def inverted_bounds(d):
    """bounds(d) with lower[0] > upper[0]: min with upper first, then max
    with lower (SVGD.hpp:396-399), so lower wins."""
    lo, up = bounds(d)
    lo[0], up[0] = 0.3, -0.2
    return lo, up


BOUNDS = {"none": lambda d: (None, None), "perdim": bounds, "inverted": inverted_bounds}


def assert_bounds_exercised(X, lo, up, Xpre=None, every_dim=True, margin=0.0):
    """The clamp was exercised and used each dimension's own bounds.  X: the
    particles after a step; Xpre (optional): the same step's X_t + increment
    before the clamp (from a reference that is not bit-identical: a crossing
    counts from `margin` on).  every_dim=False (particles driven by a model,
    which may pull a whole dimension inside its box): some dimension instead
    of every one must have particles on a bound.

      * nothing lies outside its own box; a dimension with lower > upper sits
        on lower (min with upper first, then max with lower: lower wins)
      * every bounded dimension has particles on one of its bounds, and every
        finite bound that Xpre crossed is hit exactly
      * dimension 1 (unbounded) holds values outside every other dimension's
        box: a site clamping with a shifted dimension's bound would have
        pulled them in

    Returns the numbers of dimensions with particles on their lower and on
    their upper bound (pinned and inverted dimensions not counted)."""
    n, d = X.shape
    n_lo = n_up = 0
    for k in range(d):
        if lo[k] > up[k]:
            assert np.all(X[:, k] == lo[k]), k
            continue
        assert np.all(X[:, k] >= lo[k]) and np.all(X[:, k] <= up[k]), k
        if not (np.isfinite(lo[k]) or np.isfinite(up[k])):
            continue
        at_lo, at_up = bool(np.any(X[:, k] == lo[k])), bool(np.any(X[:, k] == up[k]))
        assert at_lo or at_up or not every_dim, ("no particle on a bound", k)
        if Xpre is not None:
            assert at_lo or not np.any(Xpre[:, k] < lo[k] - margin), ("lower", k)
            assert at_up or not np.any(Xpre[:, k] > up[k] + margin), ("upper", k)
        if lo[k] < up[k]:
            n_lo, n_up = n_lo + at_lo, n_up + at_up
    if d > 2:
        fin_lo, fin_up = lo[np.isfinite(lo)], up[np.isfinite(up)]
        assert np.any(X[:, 1] < fin_lo.min()) or np.any(X[:, 1] > fin_up.max())
    assert every_dim or n_lo + n_up > 0
    return n_lo, n_up
