"""The forced-redo schedule of tests/test_gpu_spec_redo.py, and its rank body
for the sharded runs: one process per rank, all ranks on device 0, collectives
through the SVGD_HOSTCOMM host backend (as tests/_gpu_rank_worker.py).

The schedule: the bracket path from the first step (direct_max_pairs = 0,
a 2^14 sample), nine steps, a one-key candidate capacity before steps 3 and 6
(every region of the collect pass overflows: a speculative step's device plan
fails, the step is restored and redone, and the redo's own selection takes the
streamed fallback), the default capacity before every other step."""
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS = 9
FAIL = (3, 6)
SYNC_ENV = {"SVGD_SPECULATE": "0", "SVGD_TRACK_BRACKET": "0"}


def tune_bracket(c):
    """Right after creation: small n takes the bracket path and can speculate."""
    c.set_median_tuning(direct_max_pairs=0, sample_size=1 << 14)


def tune_step(c, t):
    c.set_median_tuning(candidate_capacity=1 if t in FAIL else 0)


def set_optimizer(c, name):
    from svgdcpp_amd import _capi as C
    if name == "adam":
        c.set_optimizer(C.SVGD_OPT_ADAM, 0.1, 0.9, 0.999, 1e-8)
    elif name == "adagrad":
        c.set_optimizer(C.SVGD_OPT_ADAGRAD, 0.1, 0.0, 0.0, 1e-8)
    else:
        c.set_optimizer(C.SVGD_OPT_RMSPROP, 0.1, 0.9, 0.0, 1e-8)


def problem(n, d):
    """X_0 at scale 1 and a three-component Gaussian sum."""
    import oracle as O
    X0 = O.splitmix((n, d), 1.0, 5000 + 3 * n + d)
    mus = O.splitmix((3, d), 1.0, 6000 + d)
    covs = np.stack([np.eye(d) * (1.0 + 0.25 * k) for k in range(3)])
    return X0, mus, covs


def run(rank, world, name, cfg, q):
    """cfg: n, d, opt, env.  Returns per step X (all-gathered), last_scale()
    and the rise of spec_steps over the step."""
    try:
        os.environ["SVGD_HOSTCOMM"] = name
        os.environ.update(cfg.get("env") or {})
        import svgdcpp_amd as S
        import _update_cases as U

        n, d = cfg["n"], cfg["d"]
        X0, mus, covs = problem(n, d)
        c = S.Context(d, n, device=0, world=world, rank=rank)
        c.set_particles(X0)
        set_optimizer(c, cfg["opt"])
        c.set_bounds(*U.bounds(d))
        tune_bracket(c)
        model = S.GaussianSum(list(mus), list(covs))
        Xs, scales, spec = [], [], []
        c.diagnostics()
        for t in range(STEPS):
            tune_step(c, t)
            assert c.diagnostics()["spec_steps"] == 0
            c.step_with_model(model)
            Xs.append(c.get_particles())
            scales.append(c.last_scale())
            spec.append(int(c.diagnostics()["spec_steps"]))
        out = {"X": Xs, "scales": scales, "spec": spec, "shard": (c.row0, c.row1),
               "phi_kernel": c.phi_kernel_name()}
        c.close()
        q.put(("ok", rank, out))
    except Exception:
        q.put(("err", rank, traceback.format_exc()))
