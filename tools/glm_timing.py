"""Timing of the device GLM score (svgd_set_device_glm) on one GPU ->
profiles/glm_timing.json.

Per shape (N particles, d, batch B of a logistic model):
  score_call_ms     svgd_device_logp_grad, median of >= 10 calls after a warm-up
                    (each call ends with a stream synchronise)
  d2h_ms            the same-size device-to-host copy alone (svgd_get_shard)
  score_device_ms   score_call_ms - d2h_ms
  kernel_ms         k_glm_pass + k_glm_finish from a `rocprofv3 --kernel-trace
                    --stats` run of its own (a child process: --child)
  host_grad_ms      svgd_glm_logp_grad on the host's OpenMP threads
  share_of_peak     4 d N B flop / kernel time over the fp64 matrix peak
                    (78.6 TF/s, the figure bench.py uses)
  step_device_ms / step_host_ms   svgd_step(ctx, NULL) against the split-call
                    step with the host gradient, alternating in one process

    python tools/glm_timing.py [--repeats 10] [--no-rocprof]
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
FP64_PEAK_TFLOPS = 78.6


def problem(n, d, B):
    import svgdcpp_amd as S

    rng = np.random.default_rng(n + d + B)
    A = rng.uniform(-1.0, 1.0, (B, d))
    y = rng.integers(0, 2, B).astype(np.float64)
    X = rng.uniform(-2.0, 2.0, (n, d)) * (4.0 / np.sqrt(d))
    return S.GeneralizedLinearModel(A, y, "logistic", 1.0, 1.0), X


def context(n, d, model, X):
    import svgdcpp_amd as S
    from svgdcpp_amd import _capi as C

    c = S.Context(d, n)
    c.set_particles(X)
    c.set_optimizer(C.SVGD_OPT_ADAM, 1e-3, 0.9, 0.999, 1e-8)
    c.set_device_model(model)
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
    """The score call alone, for the profiler."""
    model, X = problem(n, d, B)
    c = context(n, d, model, X)
    for _ in range(repeats + 2):
        c.device_logp_grad()
    c.close()


def kernel_ms(n, d, B, repeats):
    if shutil.which("rocprofv3") is None:
        return None
    out = tempfile.mkdtemp(prefix="glm_prof_")
    try:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "glm", "--output-format", "csv",
                            "--", sys.executable, os.path.abspath(__file__), "--child", str(n), str(d), str(B),
                            "--repeats", str(repeats)], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": (r.stdout + r.stderr)[-500:]}
        res = {}
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key in ("k_glm_pass", "k_glm_finish"):
                    if key in row["Name"]:
                        res[key + "_ms"] = float(row["AverageNs"]) / 1e6
                        res[key + "_calls"] = int(row["Calls"])
        return res or {"error": "no k_glm kernels in the profiler's statistics"}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def measure(n, d, B, repeats, rocprof):
    import ctypes

    from svgdcpp_amd import _capi as C

    model, X = problem(n, d, B)
    c = context(n, d, model, X)
    res = {"n": n, "d": d, "batch": B, "repeats": repeats}
    # both copies land in buffers touched before (a fresh numpy array's first
    # touch would be timed with the copy)
    out = np.zeros((n, d))
    shard = np.zeros((n, d))
    res["score_call_ms"], res["score_call_ms_min"], res["score_call_ms_max"] = median_ms(
        lambda: c.check(c.lib.svgd_device_logp_grad(c.h, C.dptr(out))), repeats)
    res["d2h_ms"] = median_ms(lambda: c.check(c.lib.svgd_get_shard(c.h, C.dptr(shard))), repeats)[0]
    res["score_device_ms"] = res["score_call_ms"] - res["d2h_ms"]
    G = np.empty_like(X)
    res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
    res["host_grad_ms"] = median_ms(lambda: model.log_model_grad(X, out=G), max(3, repeats // 3), warmup=1)[0]
    # the two steps alternating (each on its own context, same state size)
    ch = context(n, d, model, X)
    ch.set_device_model(None)
    td, th = [], []
    for it in range(repeats + 2):
        for which, ctx, acc in (("device", c, td), ("host", ch, th)):
            t0 = time.perf_counter()
            if which == "device":
                ctx.step_device()
            else:
                ctx.step_with_model(model)
            ctx.sync()
            if it >= 2:
                acc.append((time.perf_counter() - t0) * 1e3)
    res["step_device_ms"], res["step_host_ms"] = float(np.median(td)), float(np.median(th))
    c.close()
    ch.close()
    if rocprof:
        k = kernel_ms(n, d, B, repeats)
        res["rocprof"] = k
        if k and "k_glm_pass_ms" in k:
            res["kernel_ms"] = k["k_glm_pass_ms"] + k.get("k_glm_finish_ms", 0.0)
            res["algorithmic_tflops"] = 4.0 * d * n * B / (res["kernel_ms"] * 1e-3) / 1e12
            res["share_of_peak"] = res["algorithmic_tflops"] / FP64_PEAK_TFLOPS
    res["device_step_not_slower"] = res["step_device_ms"] <= res["step_host_ms"]
    res["device_score_beats_host"] = res["score_call_ms"] < res["host_grad_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--child", nargs=3, type=int, metavar=("N", "D", "B"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "glm_timing.json"))
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
        json.dump({"tool": "tools/glm_timing.py", "fp64_peak_tflops": FP64_PEAK_TFLOPS, "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
