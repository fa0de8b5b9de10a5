"""Timing of the device MMD (svgd_mmd) on one GPU -> profiles/mmd_timing.json.

Per shape (N = 65536 particles, d in {8, 64}; a sample of M in {1000, 65536}
points; both kernels), wall clock around the whole call (upload of Y, centre,
the two preps, the three passes, the finish, the copy back), synchronised:
median (min, max) of `repeats` after 3 warm-up.  In the same process, on the
same particles, the IMQ KSD call (svgd_ksd_kernel, scores from a device
Gaussian sum) as the yardstick: it runs three Gram chains over N^2 pairs, the
MMD one over N^2 + N M + M^2 / P, so at M = 1000 the expectation is
"mmd_ms <= ksd_imq_ms".  At d = 8, M = 1000 one svgd_mmd_host call on the
host's OpenMP threads gives the device-to-host ratio.

    python tools/mmd_timing.py [--repeats 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 65536
DIMS = (8, 64)
MS = (1000, 65536)
KERNELS = ("rbf", "imq")
WARMUP = 3


def model(d):
    import svgdcpp_amd as S

    rng = np.random.default_rng(7 + d)
    mus = rng.normal(size=(2, d))
    return S.GaussianSum(list(mus), [np.eye(d) * (1.0 + 0.25 * c) for c in range(2)])


def timed(call, repeats):
    t = []
    for it in range(repeats + WARMUP):
        t0 = time.perf_counter()
        out = call()
        if it >= WARMUP:
            t.append((time.perf_counter() - t0) * 1e3)
    return {"ms": float(np.median(t)), "ms_min": float(min(t)), "ms_max": float(max(t))}, out


def measure(d, repeats):
    import svgdcpp_amd as S
    from svgdcpp_amd import _capi as C

    rng = np.random.default_rng(N + d)
    X = rng.normal(size=(N, d))
    a = float(np.log(N) / (2.0 * d))  # ln N / E|x - x'|^2 of the standard normal cloud
    c = S.Context(d, N)
    c.set_particles(X)
    c.set_device_model(model(d))
    res = {"n": N, "d": d, "a": a, "repeats": repeats, "warmup": WARMUP, "mmd": []}
    res["ksd_imq"], _ = timed(lambda: c.ksd(None, a, kernel="imq"), repeats)
    for m in MS:
        Y = 0.9 * rng.normal(size=(m, d)) + 0.1
        for kernel in KERNELS:
            r, out = timed(lambda: c.mmd(Y, a, kernel=kernel), repeats)
            r.update({"m": m, "kernel": kernel, "mmd2_v": out[0], "mmd2_u": out[1],
                      "over_ksd_imq": r["ms"] / res["ksd_imq"]["ms"]})
            if m == 1000:
                r["not_slower_than_ksd_imq"] = r["ms"] <= res["ksd_imq"]["ms"]
            if m == 1000 and d == 8:
                hv = np.empty(1)
                t0 = time.perf_counter()
                rc = C.lib().svgd_mmd_host(S.Context.KERNELS[kernel], d, N, C.dptr(X), m, C.dptr(Y), a, C.dptr(hv),
                                           None, None, None)
                r["host_ms"] = (time.perf_counter() - t0) * 1e3
                assert rc == 0
                r["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
                r["host_over_device"] = r["host_ms"] / r["ms"]
                r["host_minus_device_v"] = float(hv[0] - out[0])
            res["mmd"].append(r)
    c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mmd_timing.json"))
    a = ap.parse_args()
    results = []
    for d in DIMS:
        r = measure(d, max(10, a.repeats))
        print(json.dumps(r), flush=True)
        results.append(r)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/mmd_timing.py", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
