#!/usr/bin/env python3
"""Timing of pjb_forest_grow (`train`'s hot path): 20 000 rows x 29 columns, 250 trees, on a warmed context.

    python tools/bench_train.py [--rows 20000] [--trees 250] [--runs 5] [--out profiles/train_grow.json] [--ranger_cpu_s S]

Two kinds of run, never mixed (HIP events between the launches lengthen the call):
  * wall time of the call, median of `runs` with min and max, after one warm-up call that sizes the context's buffers;
  * one run on a context with PJB_FLAG_KERNEL_TIMING: device time per kernel family, levels (launches of kt_decide) and nodes grown.
--ranger_cpu_s: the time `ranger_witness train` (tests/golden/ranger_witness.cc, ranger 0.3.8, one thread) took on the same matrix, timed by
hand on whatever CPU it ran on; it is written next to the device's figure with the note that it is another machine."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_forest_fixture import matrix  # noqa: E402

MATRIX_SEED = 20250101


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--trees", type=int, default=250)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_grow.json"))
    ap.add_argument("--ranger_cpu_s", type=float, default=None)
    a = ap.parse_args()
    from portcullis_amd import ffi
    m = matrix(np.random.RandomState(MATRIX_SEED), a.rows, True)
    wall = []
    with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS) as ctx:
        forest = ctx.forest_grow(m, a.trees)  # warm-up: allocations, code objects
        for _ in range(a.runs):
            t0 = time.perf_counter()
            ctx.forest_grow(m, a.trees)
            wall.append((time.perf_counter() - t0) * 1e3)
    with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS | ffi.FLAG_KERNEL_TIMING) as ctx:
        ctx.forest_grow(m, a.trees)
        ctx.reset_kernel_timing()
        ctx.forest_grow(m, a.trees)
        kt = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in sorted(ctx.kernel_timing().items()) if k.startswith("kt_")}
    res = dict(
        what="pjb_forest_grow", rows=a.rows, cols=m.shape[1], trees=a.trees, matrix_seed=MATRIX_SEED,
        wall_ms=dict(median=round(statistics.median(wall), 2), min=round(min(wall), 2), max=round(max(wall), 2), runs=[round(w, 2) for w in wall]),
        device_ms_by_kernel=kt, device_ms_total=round(sum(v["ms"] for v in kt.values()), 2),
        levels=kt.get("kt_decide", {}).get("launches", 0), nodes=int(forest.tree_off[-1]), deepest_tree_nodes=int(np.diff(forest.tree_off).max()),
    )
    if a.ranger_cpu_s is not None:
        res["ranger_cpu"] = dict(seconds=a.ranger_cpu_s, note="ranger 0.3.8 (ranger_witness train, one thread) on the same matrix, timed by hand on the "
                                                              "build container's CPU: ANOTHER MACHINE than the device's host, not a like-for-like ratio")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
