"""Rank body of the sharded case of tests/test_gpu_glm.py: one process per
rank, all ranks on device 0, collectives through the SVGD_HOSTCOMM host
backend (as tests/_gpu_ksd_worker.py).  Three fully device-resident steps
with the GLM score; every rank holds the whole data set."""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

M, STEPS = 300, 3
WINDOWS = [(0, 300), (7, 130), (236, 64)]


def problem(n, d):
    import _glm as R
    import svgdcpp_amd as S

    A, y, X0 = R.generate(d, M, n, "logistic", 23)
    return S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0), X0 * 0.25


def steps(ctx, model, X0):
    from svgdcpp_amd import _capi as C

    ctx.set_particles(X0)
    ctx.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    ctx.set_device_model(model)
    scales = []
    for t in range(STEPS):
        ctx.set_device_batch(*WINDOWS[t])
        ctx.step_device()
        scales.append(ctx.last_scale())
    return {"shard": (ctx.row0, ctx.row1), "scales": scales, "X": ctx.get_particles()}


def run(rank, world, name, n, d, q):
    try:
        os.environ["SVGD_HOSTCOMM"] = name
        os.environ["SVGD_DEBUG_COLL"] = "1"  # every step's collective sequence compared across ranks
        import svgdcpp_amd as S

        model, X0 = problem(n, d)
        ctx = S.Context(d, n, device=0, world=world, rank=rank)
        res = steps(ctx, model, X0)
        ctx.close()
        q.put(("ok", rank, res))
    except Exception:
        q.put(("err", rank, traceback.format_exc()))
