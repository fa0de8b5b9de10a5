"""Rank body of tests/test_gpu_shard_paths.py: one process per rank, all ranks
on device 0, collectives through the SVGD_HOSTCOMM host backend with every
step's collective sequence hashed and compared (SVGD_DEBUG_COLL=1), as
tests/_gpu_redo_rank_worker.py.

cfg: n, d, dtype ("f64" / "f32"), env, opt, mode and
  mode "update": a fixed scale a (the oracle's median scale of X_0), or the
      fixed SPD matrix M = _spd(d, d) / d with cfg["matrix"]; three times
      phi(G_rows, a), svgd_step(G_rows), get_particles().  Returns each step's
      phi rows and the all-gathered X.
  mode "steps": the median scale, four steps of step_with_model with
      cfg["model"] "gmm" (the built-in three-component GaussianSum: the
      pipelined svgd_step_host_model) or "elem" (a Python model whose gradient
      -(X - 0.3) is elementwise: G is bit-identical however the rows are
      sliced); cfg["bracket"] sets direct_max_pairs = 0, so the tile-path
      bracket passes run instead of the direct pass.  Returns per step X,
      last_scale() and phi_kernel_name().
"""
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

UPDATE_STEPS = 3
MODEL_STEPS = 4


def inputs(n, d):
    """(X0, G, a): X at scale 1, G at scale 1 with an all-zero first row, a the
    oracle's median scale of X0 (every column contributes to every row)."""
    import oracle as O
    # (seed base 3104: the first from 3000 up at which both two-particle shapes
    # draw a value of the unbounded dimension 1 beyond every box, checked by
    # tests/test_shard_cases_cpu.py::test_inputs_can_exercise_the_bounds)
    X = O.splitmix((n, d), 1.0, 3104 + 7 * n + d)
    G = O.splitmix((n, d), 1.0, 4000 + 7 * n + d)
    G[0] = 0.0
    return X, G, O.median_scale(X)[0]


def matrix(d):
    """The fixed SPD matrix scale of tests/test_gpu_update_paths.py."""
    from test_gpu_matrix_scale import _spd
    return _spd(d, d) / d


def gmm(d):
    """Means and covariances of the three-component Gaussian sum."""
    import oracle as O
    mus = O.splitmix((3, d), 1.0, 6000 + d)
    covs = np.stack([np.eye(d) * (1.0 + 0.25 * k) for k in range(3)])
    return mus, covs


def set_optimizer(c, name):
    from svgdcpp_amd import _capi as C
    if name == "adam":
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.1, 0.9, 0.999, 1e-8)
    elif name == "adagrad":
        c.set_optimizer(C.SVGD_OPT_ADAGRAD, 0.1, 0.0, 0.0, 1e-8)
    else:
        c.set_optimizer(C.SVGD_OPT_RMSPROP, 0.1, 0.9, 0.0, 1e-8)


def elementwise_model(S, d):
    class Elementwise(S.Model):
        def log_model_grad(self, X):
            return -(np.asarray(X, dtype=np.float64) - 0.3)
    return Elementwise(d)


def _update(c, cfg, X0, G, a):
    from svgdcpp_amd import _capi as C
    if cfg.get("matrix"):
        c.set_scale_matrix(matrix(cfg["d"]))
        a = 0.0
    else:
        c.set_scale(C.SVGD_SCALE_FIXED, a)
    G_rows = np.ascontiguousarray(G[c.row0:c.row1])
    phis, Xs, names = [], [], []
    for _ in range(UPDATE_STEPS):
        phis.append(c.phi(G_rows, a))
        c.check(c.lib.svgd_step(c.h, C.dptr(G_rows)))
        Xs.append(c.get_particles())
        names.append(c.phi_kernel_name())
    return {"phi": phis, "X": Xs, "names": names}


def _steps(S, c, cfg):
    d = cfg["d"]
    if cfg.get("bracket"):
        c.set_median_tuning(direct_max_pairs=0)
    if cfg["model"] == "gmm":
        mus, covs = gmm(d)
        model = S.GaussianSum(list(mus), list(covs))
    else:
        model = elementwise_model(S, d)
    Xs, scales, names = [], [], []
    for _ in range(MODEL_STEPS):
        c.step_with_model(model)
        Xs.append(c.get_particles())
        scales.append(c.last_scale())
        names.append(c.phi_kernel_name())
    return {"X": Xs, "scales": scales, "names": names}


def run(rank, world, name, cfg, q):
    try:
        os.environ["SVGD_HOSTCOMM"] = name
        os.environ["SVGD_DEBUG_COLL"] = "1"
        os.environ.update(cfg.get("env") or {})
        import svgdcpp_amd as S
        from svgdcpp_amd import _capi as C
        import _update_cases as U

        n, d = cfg["n"], cfg["d"]
        X0, G, a = inputs(n, d)
        dtype = C.SVGD_F64 if cfg["dtype"] == "f64" else C.SVGD_F32
        c = S.Context(d, n, device=0, world=world, rank=rank, dtype=dtype)
        c.set_particles(X0)
        set_optimizer(c, cfg["opt"])
        c.set_bounds(*U.bounds(d))
        out = _update(c, cfg, X0, G, a) if cfg["mode"] == "update" else _steps(S, c, cfg)
        out["shard"] = (c.row0, c.row1)
        c.close()
        q.put(("ok", rank, out))
    except Exception:
        q.put(("err", rank, traceback.format_exc()))
