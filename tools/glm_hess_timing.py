"""Timing of the device Hessian sum of the GLM (svgd_device_neg_hess_sum,
svgd_set_device_hessian) on one GPU -> profiles/glm_hess_timing.json.

Per shape (N particles, d, batch B of a logistic model; the shapes of
tools/glm_timing.py):
  step_device_ms / step_split_ms   svgd_step(ctx, NULL) under the Hessian scale
                    with the device Hessian sum, against the split-call Hessian
                    step with the host sum and the host gradient; alternating
                    in one process on two contexts, each call ended by a
                    synchronise, median of >= 10 after a warm-up
  step_ratio        step_split_ms / step_device_ms (>= 1: the device step is
                    not slower)
  hess_call_ms      svgd_device_neg_hess_sum (with its d x d copy and synchronise)
  host_hess_ms      svgd_glm_neg_hess_sum on the host's OpenMP threads
  hess_kernel_ms    k_glm_wpass + k_glm_wfinish + k_glm_wgram + k_glm_hfinish, and
  score_kernel_ms   k_glm_pass + k_glm_finish, from one `rocprofv3 --kernel-trace
                    --stats` run of its own (a child process: --child)
  kernel_ratio      hess_kernel_ms / score_kernel_ms (expected <= 1.25)

    python tools/glm_hess_timing.py [--repeats 10] [--no-rocprof]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(65536, 8, 4096), (65536, 64, 4096), (16384, 55, 1024)]
HESS_KERNELS = ("k_glm_wpass", "k_glm_wfinish", "k_glm_wgram", "k_glm_hfinish")
SCORE_KERNELS = ("k_glm_pass", "k_glm_finish")


def problem(n, d, B):
    import svgdcpp_amd as S

    rng = np.random.default_rng(n + d + B)
    A = rng.uniform(-1.0, 1.0, (B, d))
    y = rng.integers(0, 2, B).astype(np.float64)
    X = rng.uniform(-2.0, 2.0, (n, d)) * (4.0 / np.sqrt(d))
    return S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0), X


def context(n, d, model, X, device):
    import svgdcpp_amd as S
    from svgdcpp_amd import _capi as C

    c = S.Context(d, n)
    c.set_particles(X)
    c.set_optimizer(C.SVGD_OPT_ADAM, 1e-3, 0.9, 0.999, 1e-8)
    c.set_scale(C.SVGD_SCALE_HESSIAN, 0.0)
    if device:
        c.set_device_model(model)
        c.set_device_hessian(True)
    return c


def median_ms(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def child(n, d, B, repeats):
    """The Hessian-sum call and the score call alone, for the profiler."""
    model, X = problem(n, d, B)
    c = context(n, d, model, X, True)
    for _ in range(repeats + 2):
        c.device_neg_hess_sum()
        c.device_logp_grad()
    c.close()


def kernel_ms(n, d, B, repeats):
    if shutil.which("rocprofv3") is None:
        return None
    out = tempfile.mkdtemp(prefix="glm_hess_prof_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "glm", "--output-format", "csv",
                            "--", sys.executable, os.path.abspath(__file__), "--child", str(n), str(d), str(B),
                            "--repeats", str(repeats)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-500:]}
        res = {}
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key in HESS_KERNELS + SCORE_KERNELS:
                    if key in row["Name"]:
                        res[key + "_ms"] = float(row["AverageNs"]) / 1e6
                        res[key + "_calls"] = int(row["Calls"])
        return res or {"error": "no k_glm kernels in the profiler's statistics"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def measure(n, d, B, repeats, rocprof):
    from svgdcpp_amd import _capi as C

    model, X = problem(n, d, B)
    cd = context(n, d, model, X, True)
    cs = context(n, d, model, X, False)
    res = {"n": n, "d": d, "batch": B, "repeats": repeats,
           "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()}
    H = np.zeros((d, d))
    res["hess_call_ms"] = median_ms(lambda: cd.check(cd.lib.svgd_device_neg_hess_sum(cd.h, C.dptr(H))), repeats)[0]
    res["host_hess_ms"] = median_ms(lambda: model.neg_hess_sum(X), max(3, repeats // 3), warmup=1)[0]
    # the two steps alternating (each on its own context, same state size)
    td, ts = [], []
    for it in range(repeats + 2):
        for which, ctx, acc in (("device", cd, td), ("split", cs, ts)):
            t0 = time.perf_counter()
            if which == "device":
                ctx.step_device()
            else:
                ctx.step_with_model(model, hessian=True)
            ctx.sync()
            if it >= 2:
                acc.append((time.perf_counter() - t0) * 1e3)
    res["step_device_ms"], res["step_split_ms"] = float(np.median(td)), float(np.median(ts))
    res["step_device_ms_max"], res["step_split_ms_min"] = float(max(td)), float(min(ts))
    res["step_ratio"] = res["step_split_ms"] / res["step_device_ms"]
    res["device_step_not_slower"] = res["step_device_ms"] <= res["step_split_ms"]
    cd.close()
    cs.close()
    if rocprof:
        k = kernel_ms(n, d, B, repeats)
        res["rocprof"] = k
        if k and all(key + "_ms" in k for key in HESS_KERNELS + SCORE_KERNELS):
            res["hess_kernel_ms"] = sum(k[key + "_ms"] for key in HESS_KERNELS)
            res["score_kernel_ms"] = sum(k[key + "_ms"] for key in SCORE_KERNELS)
            res["kernel_ratio"] = res["hess_kernel_ms"] / res["score_kernel_ms"]
            res["kernel_ratio_within_margin"] = res["kernel_ratio"] <= 1.25
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", nargs=3, type=int, metavar=("N", "D", "B"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_hess_timing.json"))
    a = ap.parse_args()
    if a.child:
        child(*a.child, a.repeats)
        return
    results = []
    for n, d, B in SHAPES:
        r = measure(n, d, B, max(10, a.repeats), not a.no_rocprof)
        print(json.dumps(r), flush=True)
        results.append(r)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/glm_hess_timing.py", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
