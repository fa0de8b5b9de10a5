#!/usr/bin/env python3
"""Time Context.ksd (device model, fp64) next to the phi kernel on the same GPU.

    python tools/ksd_timing.py [--out profiles/ksd_timing.json] [--repeats 10]

Per shape -- cfg2 (N = 16384, d = 2) and cfg3 (N = 65536, d = 8):

  ksd_ms         wall clock around Context.ksd(None, a) (the call ends in a
                 stream synchronise and the copy of the two scalars), after
                 warm-up calls; median and min of the repeats
  phi_kernel_ms  PHI_KERNEL_MS / PHI_KERNEL_N of diagnostics() at timing level
                 2 over device-model steps: the phi pair kernel alone (device
                 events), the figure the KSD pass is compared with (the KSD
                 adds its own translation unit: the phi kernels are the ones
                 the library had before it)
  ratio          ksd_ms (median) / phi_kernel_ms

The KSD figure holds the whole call (gradient, centring, operand prep, pair
pass, finish, synchronise); the pair pass dominates it at these sizes.
"""
import argparse
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

SHAPES = {"cfg2": (16384, 2), "cfg3": (65536, 8)}


def measure(name, n, d, warmup, repeats, steps):
    rng = np.random.default_rng(1234 + d)
    X0 = rng.uniform(-3.0, 3.0, (n, d))
    mus = rng.uniform(-3.0, 3.0, (4, d))
    model = S.GaussianSum(list(mus), [np.eye(d) * (1.0 + 0.25 * c) for c in range(4)])
    ctx = S.Context(d, n)
    ctx.set_particles(X0)
    ctx.set_optimizer(C.SVGD_OPT_ADAM, 0.05, 0.9, 0.999, 1e-8)
    ctx.set_device_model(model)
    # the phi kernel alone: level-2 diagnostic events over device-model steps
    ctx.check(ctx.lib.svgd_set_timing(ctx.h, 2))
    for _ in range(warmup):
        ctx.step_device()
    ctx.sync()
    ctx.diagnostics()  # reset the accumulators
    for _ in range(steps):
        ctx.step_device()
    ctx.sync()
    dg = ctx.diagnostics()
    phi_ms = dg["phi_kernel_ms"] / dg["phi_kernel_n"] if dg["phi_kernel_n"] else float("nan")
    ctx.check(ctx.lib.svgd_set_timing(ctx.h, 0))
    a = ctx.median_scale()[0]
    for _ in range(warmup):
        ctx.ksd(None, a)
    ctx.sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        v, u = ctx.ksd(None, a)
        ctx.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    res = {"name": name, "n": n, "d": d, "a": a, "ksd2_v": v, "ksd2_u": u,
           "ksd_ms_median": statistics.median(times), "ksd_ms_min": min(times), "ksd_ms_max": max(times),
           "repeats": repeats, "phi_kernel": ctx.phi_kernel_name(), "phi_kernel_ms": phi_ms,
           "phi_kernel_n": dg["phi_kernel_n"], "ratio": statistics.median(times) / phi_ms}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ksd_timing.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shapes", default="cfg2,cfg3")
    args = ap.parse_args()
    out = {"tool": "tools/ksd_timing.py", "results": []}
    for name in args.shapes.split(","):
        n, d = SHAPES[name]
        r = measure(name, n, d, args.warmup, args.repeats, args.steps)
        print(json.dumps(r))
        out["results"].append(r)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
