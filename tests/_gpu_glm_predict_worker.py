"""Rank body of the sharded cases of tests/test_gpu_glm_predict.py: one process
per rank, all ranks on device 0, collectives through the SVGD_HOSTCOMM host
backend (as tests/_gpu_glm_hess_worker.py).  Every rank loads the same
particles and calls the collective prediction with the same test data, for
both links, with and without labels."""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

M, S_LIK = 129, 0.7
LINKS = ("logistic", "gaussian")


def problem(n, d, link):
    import _glm as R

    return R.generate(d, M, n, link, 31)  # A, y, X


def predict(ctx, n, d):
    out = {"shard": (ctx.row0, ctx.row1)}
    for link in LINKS:
        A, y, X = problem(n, d, link)
        ctx.set_particles(X)
        out[link] = ctx.glm_predict(A, y, link, S_LIK)
        out[link + "_noy"] = ctx.glm_predict(A, None, link, S_LIK)
    return out


def run(rank, world, name, n, d, q):
    try:
        os.environ["SVGD_HOSTCOMM"] = name
        os.environ["SVGD_DEBUG_COLL"] = "1"  # every step's collective sequence compared across ranks
        import svgdcpp_amd as S

        ctx = S.Context(d, n, device=0, world=world, rank=rank)
        res = predict(ctx, n, d)
        ctx.close()
        q.put(("ok", rank, res))
    except Exception:
        q.put(("err", rank, traceback.format_exc()))
