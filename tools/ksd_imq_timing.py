#!/usr/bin/env python3
"""Time the IMQ kernelized Stein discrepancy (Context.ksd(kernel="imq"), device
model, fp64) next to the RBF one and to the IMQ phi kernel, on one GPU
-> profiles/ksd_imq_timing.json.

    python tools/ksd_imq_timing.py [--repeats 10]

Per shape -- cfg3 (N = 65536, d = 8) and N = 65536, d = 64 -- in one process:

  ksd_imq_ms / ksd_rbf_ms   wall clock around the whole call with the device
                 model (gradient, centring, records, pair pass, finish, the
                 copy of the two scalars; the call ends in a stream
                 synchronise), the two statistics alternating: median, min and
                 max of the repeats after 3 warm-up calls of each
  imq_phi_kernel_ms  PHI_KERNEL_MS / PHI_KERNEL_N of diagnostics() at timing
                 level 2 over device-model steps of an IMQ-stepping context, in
                 a pass of its own: k_imq_pass alone (device events)
  host_ksd_imq_ms  one svgd_ksd_host(IMQ) call over the same N on the host's
                 OpenMP threads (cfg3 only: the condition device < host)
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import svgdcpp_amd as S  # noqa: E402
from svgdcpp_amd import _capi as C  # noqa: E402

SHAPES = {"cfg3": (65536, 8), "d64": (65536, 64)}
WARMUP = 3


def measure(name, n, d, repeats, steps, host):
    rng = np.random.default_rng(1234 + d)
    X0 = rng.uniform(-3.0, 3.0, (n, d))
    mus = rng.uniform(-3.0, 3.0, (4, d))
    model = S.GaussianSum(list(mus), [np.eye(d) * (1.0 + 0.25 * c) for c in range(4)])
    ctx = S.Context(d, n)
    ctx.set_particles(X0)
    ctx.set_device_model(model)
    a = ctx.median_scale()[0]
    times = {"imq": [], "rbf": []}
    vals = {}
    for it in range(repeats + WARMUP):
        for kernel in ("imq", "rbf"):
            t0 = time.perf_counter()
            vals[kernel] = ctx.ksd(None, a, kernel=kernel)
            ctx.sync()
            if it >= WARMUP:
                times[kernel].append((time.perf_counter() - t0) * 1e3)
    res = {"name": name, "n": n, "d": d, "a": a, "repeats": repeats, "warmup": WARMUP}
    for kernel in ("imq", "rbf"):
        t = times[kernel]
        res["ksd_%s_ms" % kernel] = statistics.median(t)
        res["ksd_%s_ms_min" % kernel], res["ksd_%s_ms_max" % kernel] = min(t), max(t)
        res["ksd2_v_" + kernel], res["ksd2_u_" + kernel] = vals[kernel]
    res["ratio_imq_over_rbf"] = res["ksd_imq_ms"] / res["ksd_rbf_ms"]
    # the IMQ phi kernel alone: level-2 diagnostic events over device-model
    # steps of a context of its own (a tiny learning rate: the cloud stays put)
    q = S.Context(d, n)
    q.set_particles(X0)
    q.set_optimizer(C.SVGD_OPT_ADAM, 1e-6, 0.9, 0.999, 1e-8)
    q.set_device_model(model)
    q.set_kernel("imq")
    q.check(q.lib.svgd_set_timing(q.h, 2))
    for _ in range(WARMUP):
        q.step_device()
    q.sync()
    q.diagnostics()  # reset the accumulators
    for _ in range(steps):
        q.step_device()
    q.sync()
    dg = q.diagnostics()
    res["imq_phi_kernel"] = q.phi_kernel_name()
    res["imq_phi_kernel_ms"] = dg["phi_kernel_ms"] / dg["phi_kernel_n"] if dg["phi_kernel_n"] else float("nan")
    res["imq_phi_kernel_n"] = dg["phi_kernel_n"]
    res["ratio_ksd_imq_over_imq_phi_kernel"] = res["ksd_imq_ms"] / res["imq_phi_kernel_ms"]
    q.close()
    if host:
        G = model.log_model_grad(X0)
        v, u = ctypes.c_double(), ctypes.c_double()
        t0 = time.perf_counter()
        rc = C.lib().svgd_ksd_host(C.SVGD_KERNEL_IMQ, d, n, C.dptr(X0), C.dptr(G), a, ctypes.byref(v),
                                   ctypes.byref(u), None)
        res["host_ksd_imq_ms"] = (time.perf_counter() - t0) * 1e3
        assert rc == 0
        res["host_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()
        res["host_ksd2_v"] = v.value
        res["device_beats_host"] = res["ksd_imq_ms"] < res["host_ksd_imq_ms"]
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ksd_imq_timing.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--shapes", default="cfg3,d64")
    args = ap.parse_args()
    out = {"tool": "tools/ksd_imq_timing.py", "results": []}
    for name in args.shapes.split(","):
        n, d = SHAPES[name]
        r = measure(name, n, d, args.repeats, args.steps, host=(name == "cfg3"))
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
