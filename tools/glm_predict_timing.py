"""Timing of the device GLM posterior prediction (svgd_glm_predict) on one GPU
-> profiles/glm_predict_timing.json.

Per shape (N particles, d; the (N, d) pairs of tools/glm_hess_timing.py, each
with m* = 4096 test rows of a logistic model, labels given):
  predict_call_ms   Context.glm_predict in wall ms: the record build and
                    upload, the kernels, the copies back and the synchronise;
                    median of >= 10 after a warm-up
  host_predict_ms   svgd_glm_predict_host on the host's OpenMP threads, on
                    particles that are already on the host
  call_ratio        host_predict_ms / predict_call_ms (>= 1: the device call
                    is not slower)
  predict_kernel_ms k_glm_predict, and
  wpass_kernel_ms   k_glm_wpass of the unchanged Hessian sum on a window of the
                    same 4096 records and the same particles, in the same
                    process, from one `rocprofv3 --kernel-trace --stats` run
                    of its own (a child process: --child)
  kernel_ratio      predict_kernel_ms / wpass_kernel_ms (the same Gram product,
                    three accumulators where wpass has one)

    python tools/glm_predict_timing.py [--repeats 10] [--no-rocprof]
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

SHAPES = [(65536, 8), (65536, 64), (16384, 55)]
M_TEST = 4096
KERNELS = {"k_glm_predict": "k_glm_predict<", "k_glm_wpass": "k_glm_wpass<",
           "k_glm_predict_center": "k_glm_predict_center", "k_glm_predict_finish": "k_glm_predict_finish"}


def problem(n, d):
    rng = np.random.default_rng(n + d + M_TEST)
    A = rng.uniform(-1.0, 1.0, (M_TEST, d))
    y = rng.integers(0, 2, M_TEST).astype(np.float64)
    X = rng.uniform(-2.0, 2.0, (n, d)) * (4.0 / np.sqrt(d))
    return A, y, X


def median_ms(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t))


def child(n, d, repeats):
    """The prediction call and the Hessian-sum call alone, for the profiler."""
    import svgdcpp_amd as S

    A, y, X = problem(n, d)
    c = S.Context(d, n)
    c.set_particles(X)
    c.set_device_model(S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0))
    for _ in range(repeats + 2):
        c.glm_predict(A, y, "logistic", 1.0)
        c.device_neg_hess_sum()
    c.close()


def kernel_ms(n, d, repeats):
    if shutil.which("rocprofv3") is None:
        return None
    out = tempfile.mkdtemp(prefix="glm_predict_prof_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "glm", "--output-format", "csv",
                            "--", sys.executable, os.path.abspath(__file__), "--child", str(n), str(d),
                            "--repeats", str(repeats)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-500:]}
        res = {}
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key, pat in KERNELS.items():
                    if pat in row["Name"]:
                        res[key + "_ms"] = float(row["AverageNs"]) / 1e6
                        res[key + "_calls"] = int(row["Calls"])
        return res or {"error": "no k_glm kernels in the profiler's statistics"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def measure(n, d, repeats, rocprof):
    import svgdcpp_amd as S

    A, y, X = problem(n, d)
    model = S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0)
    c = S.Context(d, n)
    c.set_particles(X)
    res = {"n": n, "d": d, "m_test": M_TEST, "repeats": repeats,
           "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()}
    t = median_ms(lambda: c.glm_predict(A, y, "logistic", 1.0), repeats)
    res["predict_call_ms"], res["predict_call_ms_min"], res["predict_call_ms_max"] = t
    dev = c.glm_predict(A, y, "logistic", 1.0)
    c.close()
    t = median_ms(lambda: model.predict(X, A, y), max(3, repeats // 3), warmup=1)
    res["host_predict_ms"], res["host_predict_ms_min"], res["host_predict_ms_max"] = t
    host = model.predict(X, A, y)
    res["max_abs_diff"] = [float(np.max(np.abs(a - b))) for a, b in zip(dev, host)]
    res["call_ratio"] = res["host_predict_ms"] / res["predict_call_ms"]
    res["device_call_not_slower"] = res["predict_call_ms"] <= res["host_predict_ms"]
    if rocprof:
        k = kernel_ms(n, d, repeats)
        res["rocprof"] = k
        if k and "k_glm_predict_ms" in k and "k_glm_wpass_ms" in k:
            res["predict_kernel_ms"] = k["k_glm_predict_ms"]
            res["wpass_kernel_ms"] = k["k_glm_wpass_ms"]
            res["kernel_ratio"] = res["predict_kernel_ms"] / res["wpass_kernel_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", nargs=2, type=int, metavar=("N", "D"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_predict_timing.json"))
    a = ap.parse_args()
    if a.child:
        child(*a.child, a.repeats)
        return
    results = []
    for n, d in SHAPES:
        r = measure(n, d, max(10, a.repeats), not a.no_rocprof)
        print(json.dumps(r), flush=True)
        results.append(r)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/glm_predict_timing.py", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
