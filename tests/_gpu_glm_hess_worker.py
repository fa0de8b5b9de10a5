"""Rank body of the sharded case of tests/test_gpu_glm_hess.py: one process
per rank, all ranks on device 0, collectives through the SVGD_HOSTCOMM host
backend (as tests/_gpu_glm_worker.py).  Three fully device-resident steps
under the Hessian scale, the Hessian sum from the device GLM on every rank."""
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

    A, y, X0 = R.generate(d, M, n, "logistic", 29)
    return S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0), A, y, X0 * 0.25


def steps(ctx, model, X0):
    from svgdcpp_amd import _capi as C

    ctx.set_particles(X0)
    ctx.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    ctx.set_scale(C.SVGD_SCALE_HESSIAN, 0.0)
    ctx.set_device_model(model)
    ctx.set_device_hessian(True)
    before, mats = [], []
    for t in range(STEPS):
        before.append(ctx.get_particles())
        ctx.set_device_batch(*WINDOWS[t])
        ctx.step_device()
        mats.append(ctx.get_scale_matrix())
    return {"shard": (ctx.row0, ctx.row1), "before": before, "mats": mats, "X": ctx.get_particles()}


def run(rank, world, name, n, d, q):
    try:
        os.environ["SVGD_HOSTCOMM"] = name
        os.environ["SVGD_DEBUG_COLL"] = "1"  # every step's collective sequence compared across ranks
        import svgdcpp_amd as S

        model, _, _, X0 = problem(n, d)
        ctx = S.Context(d, n, device=0, world=world, rank=rank)
        res = steps(ctx, model, X0)
        ctx.close()
        q.put(("ok", rank, res))
    except Exception:
        q.put(("err", rank, traceback.format_exc()))
