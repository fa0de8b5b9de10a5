"""Rank body of tests/test_gpu_imq.py::test_three_ranks_match_one_rank: one
process per rank, all ranks on device 0, collectives through the
SVGD_HOSTCOMM host backend (as tests/_gpu_rank_worker.py), with the inverse
multiquadric kernel set: each rank computes its rows against all N columns of
the all-gathered X and G."""
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(rank, world, name, n, d, steps, q):
    try:
        os.environ["SVGD_HOSTCOMM"] = name
        os.environ["SVGD_DEBUG_COLL"] = "1"  # fails on a rank-dependent collective sequence
        import oracle as O
        import svgdcpp_amd as S
        from svgdcpp_amd import _capi as C

        X0 = O.splitmix((n, d), 3.0, 41)
        mus = O.splitmix((3, d), 3.0, 42)
        covs = [np.eye(d) * (1.0 + 0.25 * c) for c in range(3)]
        ctx = S.Context(d, n, device=0, world=world, rank=rank)
        ctx.set_particles(X0)
        ctx.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
        ctx.set_bounds(-np.full(d, 2.5), np.full(d, 2.5))
        ctx.set_kernel("imq")
        model = S.GaussianSum(list(mus), list(covs))
        scales = []
        for _ in range(steps):
            ctx.step_with_model(model)
            scales.append(ctx.last_scale()[0])
        X = ctx.get_particles()
        name_k = ctx.phi_kernel_name()
        shard = (ctx.row0, ctx.row1)
        ctx.close()
        q.put(("ok", rank, X, scales, shard, name_k))
    except Exception:
        q.put(("err", rank, traceback.format_exc(), None, None, None))
