"""Rank body of the sharded cases of tests/test_gpu_mmd.py: one process per
rank, all ranks on device 0, collectives through the SVGD_HOSTCOMM host
backend (as tests/_gpu_thin_worker.py).  Two steps, the MMD of the result
against a sample of M points and against its first world - 1 points (the last
rank's shard of Y rows is then empty) (optional), one more step."""
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

MMD_A = 0.4  # about ln N / med^2 of the d = 5 clouds below
M = 1001
KERNELS = ("rbf", "imq")


def model(d):
    import oracle as O
    import svgdcpp_amd as S

    mus = O.splitmix((3, d), 3.0, 42)
    return S.GaussianSum(list(mus), [np.eye(d) * (1.0 + 0.25 * c) for c in range(3)])


def sample(d):
    import oracle as O

    return O.splitmix((M, d), 2.0, 43) + 0.25


def run(rank, world, name, n, d, with_mmd, q):
    try:
        os.environ["SVGD_HOSTCOMM"] = name
        os.environ["SVGD_DEBUG_COLL"] = "1"  # every step's collective sequence compared across ranks
        import oracle as O
        import svgdcpp_amd as S
        from svgdcpp_amd import _capi as C

        X0 = O.splitmix((n, d), 3.0, 41)
        ctx = S.Context(d, n, device=0, world=world, rank=rank)
        ctx.set_particles(X0)
        ctx.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
        ctx.set_bounds(-np.full(d, 2.5), np.full(d, 2.5))
        m = model(d)
        res = {"shard": (ctx.row0, ctx.row1), "scales": []}
        for _ in range(2):
            ctx.step_with_model(m)
            res["scales"].append(ctx.last_scale())
        res["X2"] = ctx.get_particles()
        if with_mmd:
            Y = sample(d)
            for kernel in KERNELS:
                res[kernel] = ctx.mmd(Y, MMD_A, kernel=kernel, witness=True, means=True)
                res[kernel + "_few"] = ctx.mmd(Y[:world - 1], MMD_A, kernel=kernel, witness=True, means=True)
        ctx.step_with_model(m)
        res["scales"].append(ctx.last_scale())
        res["X3"] = ctx.get_particles()
        ctx.close()
        q.put(("ok", rank, res))
    except Exception:
        q.put(("err", rank, traceback.format_exc()))
