#!/usr/bin/env python3
"""Timing of pjb_knn (the nearest-neighbour search under self-training's SMOTE and ENN) on a warmed context:
20 000 x 28 with k = 5 (SMOTE over a negative set) and 60 000 x 28 with k = 3 (ENN over a whole training matrix).

    python tools/bench_knn.py [--runs 5] [--out profiles/selftrain_knn.json] [--reference_cpu_s S20000,S60000]

Two kinds of run per shape, never mixed (HIP events between the launches lengthen the call):
  * wall time of the call through ffi (pad, copy in, two kernels, copy out, one wait), median of `runs` with min and max, after one warm-up
    call that sizes the context's buffers;
  * `runs` calls on a context with PJB_FLAG_KERNEL_TIMING: device time of kn_partial and kn_merge by HIP events, the median per kernel.
The f64 work of kn_partial is counted from the shape: rows^2 x cols x 3 operations (subtract, multiply, add, each rounded on its own: no
fused multiply-add may be used), and set against a vector f64 peak given with --peak_f64_tflops (MI355X data sheet: 78.6 TFLOP/s, which
counts a fused multiply-add as two operations; without fusion half of it is the most any kernel can reach).
--reference_cpu_s: the seconds `knn_witness time` (tests/golden/knn_witness.cc: the reference's own KNN::execute, one thread) took on the
same matrices, timed by hand on whatever CPU it ran on; written next to the device's figures with the note that it is another machine."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [dict(rows=20000, cols=28, k=5, seed=1), dict(rows=60000, cols=28, k=3, seed=2)]


def shape_matrix(s):
    rng = np.random.RandomState(s["seed"])
    return rng.normal(0, 1, (s["rows"], s["cols"])) * rng.uniform(0.5, 40, s["cols"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selftrain_knn.json"))
    ap.add_argument("--peak_f64_tflops", type=float, default=78.6)
    ap.add_argument("--reference_cpu_s", default=None)
    a = ap.parse_args()
    from portcullis_amd import ffi
    cpu = [float(v) for v in a.reference_cpu_s.split(",")] if a.reference_cpu_s else [None] * len(SHAPES)
    out = []
    for s, cpu_s in zip(SHAPES, cpu):
        m = shape_matrix(s)
        wall = []
        with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS) as ctx:
            first = ctx.knn(m, s["k"])  # warm-up: allocations, code objects
            for _ in range(a.runs):
                t0 = time.perf_counter()
                nn = ctx.knn(m, s["k"])
                wall.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(nn, first) and (nn[:, 0] == np.arange(len(m))).all()  # (no copied rows here: a row is its own nearest)
        dev = {"kn_partial": [], "kn_merge": []}
        with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS | ffi.FLAG_KERNEL_TIMING) as ctx:
            ctx.knn(m, s["k"])
            for _ in range(a.runs):
                ctx.reset_kernel_timing()
                ctx.knn(m, s["k"])
                kt = ctx.kernel_timing()
                for name in dev:
                    dev[name].append(kt[name][1])
        partial_ms = statistics.median(dev["kn_partial"])
        ops = float(s["rows"]) ** 2 * s["cols"] * 3
        tflops = ops / (partial_ms * 1e-3) / 1e12
        rec = dict(
            rows=s["rows"], cols=s["cols"], k=s["k"], matrix_seed=s["seed"],
            wall_ms=dict(median=round(statistics.median(wall), 2), min=round(min(wall), 2), max=round(max(wall), 2), runs=[round(w, 2) for w in wall]),
            device_ms={n: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for n, v in dev.items()},
            f64_operations=ops, kn_partial_tflops=round(tflops, 2),
            share_of_f64_vector_peak=round(tflops / a.peak_f64_tflops, 3), share_of_unfused_f64_vector_peak=round(tflops / (a.peak_f64_tflops / 2), 3),
        )
        if cpu_s is not None:
            rec["reference_cpu"] = dict(seconds=cpu_s, note="the reference's KNN::execute (knn_witness time, one thread) on the same matrix, timed by hand on the "
                                                            "build container's CPU: ANOTHER MACHINE than the device's host, not a like-for-like ratio")
        out.append(rec)
    res = dict(what="pjb_knn", peak_f64_tflops=a.peak_f64_tflops, shapes=out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
