"""Timing of the device Stein thinning (svgd_stein_thin) against the host
definition (svgd_stein_thin_host), on one GPU -> profiles/thin_timing.json.

Per shape (N particles, d; IMQ kernel, m picks, scores from a device Gaussian
sum), wall clock around the whole call, synchronised: median (min, max) of
`repeats` after 3 warm-up, for both forms of the pick chain -- one launch per
pick (the default) and k_thin_select between the picks (SVGD_THIN_SELECT=1,
read when the context is created):
  total_ms          the call with m picks
  fixed_ms          the same call with m = 1 (scores, all-gather, prep, one
                    pick, the copy back)
  us_per_pick       (total_ms - fixed_ms) / (m - 1)
  bytes_per_s       N 2d 8 bytes streamed per pick / us_per_pick
  host_ms           one svgd_stein_thin_host call on the same X and the same
                    scores (downloaded), on the host's OpenMP threads: what a
                    user has to do without the device call
The one condition: the device call is not slower than the host one.

    python tools/thin_timing.py [--repeats 10] [--m 1000]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(65536, 8), (65536, 64)]
WARMUP = 3


def model(d):
    import svgdcpp_amd as S

    rng = np.random.default_rng(7 + d)
    mus = rng.normal(size=(2, d))
    return S.GaussianSum(list(mus), [np.eye(d) * (1.0 + 0.25 * c) for c in range(2)])


def timed(c, m, a, repeats):
    t = []
    for it in range(repeats + WARMUP):
        t0 = time.perf_counter()
        out = c.stein_thin(m, None, a, kernel="imq", trace=True)
        if it >= WARMUP:
            t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t)), float(max(t)), out


def measure(n, d, m, repeats):
    import svgdcpp_amd as S
    from svgdcpp_amd import _capi as C

    rng = np.random.default_rng(n + d)
    X = rng.normal(size=(n, d))
    mod = model(d)
    a = 1.0 / (4.0 * d)
    res = {"n": n, "d": d, "m": m, "a": a, "kernel": "imq", "repeats": repeats, "warmup": WARMUP,
           "bytes_per_pick": n * 2 * d * 8}
    picks = {}
    for form, env in (("fused", "0"), ("select", "1")):
        os.environ["SVGD_THIN_SELECT"] = env
        c = S.Context(d, n)
        c.set_particles(X)
        c.set_device_model(mod)
        med, lo, hi, out = timed(c, m, a, repeats)
        fixed = timed(c, 1, a, repeats)[0]
        c.close()
        picks[form] = out
        us = (med - fixed) / (m - 1) * 1e3
        res[form] = {"total_ms": med, "total_ms_min": lo, "total_ms_max": hi, "fixed_ms": fixed,
                     "us_per_pick": us, "bytes_per_s": res["bytes_per_pick"] / (us * 1e-6)}
    os.environ.pop("SVGD_THIN_SELECT")
    res["forms_agree"] = bool(np.array_equal(picks["fused"][0], picks["select"][0])
                              and np.array_equal(picks["fused"][1], picks["select"][1]))
    G = mod.log_model_grad(X)
    idx, ksd2 = np.empty(m, np.int64), np.empty(m)
    t0 = time.perf_counter()
    rc = C.lib().svgd_stein_thin_host(C.SVGD_KERNEL_IMQ, d, n, C.dptr(X), C.dptr(G), a, m,
                                      idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), C.dptr(ksd2))
    res["host_ms"] = (time.perf_counter() - t0) * 1e3
    assert rc == 0
    res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
    res["host_picks_equal_device"] = bool(np.array_equal(idx, picks["fused"][0]))
    res["host_over_device"] = res["host_ms"] / res["fused"]["total_ms"]
    res["device_not_slower_than_host"] = res["fused"]["total_ms"] <= res["host_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thin_timing.json"))
    a = ap.parse_args()
    results = []
    for n, d in SHAPES:
        r = measure(n, d, a.m, max(10, a.repeats))
        print(json.dumps(r), flush=True)
        results.append(r)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/thin_timing.py", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
