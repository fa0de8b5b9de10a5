"""Timing of the inverse multiquadric phi pass (svgd_set_kernel(IMQ)) against
the RBF phi kernel of the same shape, on one GPU -> profiles/imq_timing.json.

Per shape (N particles, d; fp64), two contexts in one process, alternating:
  step_ms           svgd_step with a resident host G, each step ended by a
                    synchronise: median of `repeats` after 3 warm-up, timing off
  phi_kernel_ms     PHI_KERNEL_MS / PHI_KERNEL_N at timing level 2 (a diagnostic
                    pass of its own): k_imq_pass alone / the RBF phi kernel alone
  phi_phase_ms      the level-1 phi phase (prep + pass + finish [+ update])
  phi_call_ms       svgd_phi (centring, G upload, prep + pass + finish, copy back)
  host_phi_ms       one svgd_imq_phi_host call over the same N on the host's
                    OpenMP threads (cfg3 only: the condition device < host)

    python tools/imq_timing.py [--repeats 10]
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


def context(n, d, X, kernel):
    import svgdcpp_amd as S
    from svgdcpp_amd import _capi as C

    c = S.Context(d, n)
    c.set_particles(X)
    c.set_optimizer(C.SVGD_OPT_ADAM, 1e-3, 0.9, 0.999, 1e-8)
    c.set_kernel(kernel)
    return c


def alternate(ctxs, fn, repeats):
    """fn(ctx) on every context in turn; per context the wall times after the warm-up."""
    t = {k: [] for k in ctxs}
    for it in range(repeats + WARMUP):
        for k, c in ctxs.items():
            t0 = time.perf_counter()
            fn(c)
            c.sync()
            if it >= WARMUP:
                t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}


def measure(n, d, repeats, host):
    from svgdcpp_amd import _capi as C

    rng = np.random.default_rng(n + d)
    X = rng.normal(size=(n, d))
    G = np.ascontiguousarray(-X)
    ctxs = {"imq": context(n, d, X, "imq"), "rbf": context(n, d, X, "rbf")}
    res = {"n": n, "d": d, "repeats": repeats, "warmup": WARMUP,
           "kernels": {k: c.phi_kernel_name() for k, c in ctxs.items()}}
    step = lambda c: c.check(c.lib.svgd_step(c.h, C.dptr(G)))
    for k, (med, lo, hi) in alternate(ctxs, step, repeats).items():
        res["step_ms_" + k], res["step_ms_min_" + k], res["step_ms_max_" + k] = med, lo, hi
    # the diagnostic pass: level-2 events around the phi kernel alone
    for c in ctxs.values():
        c.check(c.lib.svgd_set_timing(c.h, 2))
        c.diagnostics()
    alternate(ctxs, step, repeats)
    for k, c in ctxs.items():
        phi_ms, med_ms, cnt = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        c.check(c.lib.svgd_get_timing(c.h, ctypes.byref(phi_ms), ctypes.byref(med_ms), ctypes.byref(cnt)))
        dg = c.diagnostics()
        res["phi_kernel_ms_" + k] = dg["phi_kernel_ms"] / max(1.0, dg["phi_kernel_n"])
        res["phi_kernel_n_" + k] = dg["phi_kernel_n"]
        res["phi_phase_ms_" + k] = phi_ms.value / max(1, cnt.value)
        res["median_phase_ms_" + k] = med_ms.value / max(1, cnt.value)
        c.check(c.lib.svgd_set_timing(c.h, 0))
    out = np.zeros((n, d))
    a = ctxs["imq"].last_scale()[0]
    res["a"] = a
    call = lambda c: c.check(c.lib.svgd_phi(c.h, C.dptr(G), a, C.dptr(out)))
    for k, (med, lo, hi) in alternate(ctxs, call, repeats).items():
        res["phi_call_ms_" + k] = med
    res["kernel_ratio_imq_over_rbf"] = res["phi_kernel_ms_imq"] / res["phi_kernel_ms_rbf"]
    res["step_ratio_imq_over_rbf"] = res["step_ms_imq"] / res["step_ms_rbf"]
    if host:
        Xh = ctxs["imq"].get_particles()
        t = []
        for _ in range(2):
            t0 = time.perf_counter()
            rc = C.lib().svgd_imq_phi_host(d, n, C.dptr(Xh), C.dptr(G), a, 0, n, C.dptr(out))
            t.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
        res["host_phi_ms"] = float(min(t))
        res["device_phi_beats_host"] = res["phi_call_ms_imq"] < res["host_phi_ms"]
    for c in ctxs.values():
        c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "imq_timing.json"))
    a = ap.parse_args()
    results = []
    for i, (n, d) in enumerate(SHAPES):
        r = measure(n, d, max(10, a.repeats), host=(i == 0))
        print(json.dumps(r), flush=True)
        results.append(r)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/imq_timing.py", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
