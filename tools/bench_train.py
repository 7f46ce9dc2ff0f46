#!/usr/bin/env python3
"""Timing of pjb_forest_grow (`train`'s hot path): 20 000 rows x 29 columns, 250 trees, on a warmed context.

    python tools/bench_train.py [--rows 20000] [--trees 250] [--runs 5] [--out profiles/train_grow.json] [--ranger_cpu_s S]

Two kinds of run, never mixed (HIP events between the launches lengthen the call):
  * wall time of the call, median of `runs` with min and max, after one warm-up call that sizes the context's buffers;
  * one run on a context with PJB_FLAG_KERNEL_TIMING: device time per kernel family, levels (launches of kt_decide) and nodes grown.
--ranger_cpu_s: the time `ranger_witness train` (tests/golden/ranger_witness.cc, ranger 0.3.8, one thread) took on the same matrix, timed by
hand on whatever CPU it ran on; it is written next to the device's figure with the note that it is another machine.

    python tools/bench_train.py --folds 5 [--parent DIR] [--runs 5] [--out profiles/train_cv.json]

k-fold cross-validation (`train --folds`) of the same matrix with the fold vector of tests/cv_model.py, against the same work done the
only way a library without pjb_forest_cv can do it.  Every figure comes from a process of its own (a child of this one, which never
opens the device): the child warms its context with one call of what it measures, then times one call.  `runs` rounds, in each of them,
alternating:
  (a) cv      pjb_forest_cv of this tree;
  (b) split   the tree at --parent (a checkout of the parent commit, built): per fold pjb_forest_grow on the sub-matrix,
              pjb_forest_load, pjb_forest_predict on the held-out rows;
  (c) grow    one pjb_forest_grow of the whole matrix, the parent's and this tree's.
Medians with min - max; then one (a) run under PJB_FLAG_KERNEL_TIMING for the launches and device time per kernel.  Without --parent
only this tree is measured ((b) then runs on this tree's library)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX_SEED = 20250101
SEED = 1236456789


def bench_matrix(rows):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_forest_fixture import matrix
    return matrix(np.random.RandomState(MATRIX_SEED), rows, True)


def bench_folds(rows, k):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cv_model
    return cv_model.assign_folds(rows, k, SEED)


def stats(ms):
    return dict(median=round(statistics.median(ms), 2), min=round(min(ms), 2), max=round(max(ms), 2), runs=[round(w, 2) for w in ms])


def child(a):
    """one process, one tree's package and library: warm-up, then one timed call of each mode asked for; one JSON line"""
    sys.path.insert(0, os.path.abspath(a.tree))
    from portcullis_amd import ffi
    assert os.path.abspath(ffi.__file__).startswith(os.path.abspath(a.tree) + os.sep), ffi.__file__
    m = bench_matrix(a.rows)
    fold = bench_folds(a.rows, a.folds)
    out = {}
    timing = ffi.FLAG_KERNEL_TIMING if a.kernel_timing else 0

    def work(ctx, mode):
        if mode == "cv":
            return ctx.forest_cv(m, fold, a.folds, a.trees)[0]
        if mode == "grow":
            return ctx.forest_grow(m, a.trees)
        pred = np.zeros((len(m), 2))
        for f in range(a.folds):
            ctx.forest_load(ctx.forest_grow(m[fold != f], a.trees))
            pred[fold == f] = ctx.forest_predict(m[fold == f])
        return pred

    for mode in a.child.split(","):
        with ffi.Context(0, flags=ffi.FLAG_NO_CHAINS | timing) as ctx:
            work(ctx, mode)  # warm-up: allocations, code objects
            if a.kernel_timing:
                ctx.reset_kernel_timing()
            t0 = time.perf_counter()
            got = work(ctx, mode)
            out[mode] = dict(ms=(time.perf_counter() - t0) * 1e3)
            if a.kernel_timing:
                out[mode]["kernels"] = {k: dict(launches=v[0], ms=round(v[1], 3)) for k, v in sorted(ctx.kernel_timing().items()) if v[0]}
            if mode != "grow":  # (so that the two routes can be seen to have done the same work)
                out[mode]["pred_sum"] = float(np.asarray(got).sum())
    print("BENCH_CHILD " + json.dumps(out), flush=True)


def run_child(a, tree, modes, kernel_timing=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", modes, "--tree", tree, "--rows", str(a.rows), "--trees", str(a.trees), "--folds", str(a.folds)]
    p = subprocess.run(cmd + (["--kernel_timing"] if kernel_timing else []), capture_output=True, text=True, timeout=600)
    lines = [l for l in p.stdout.split("\n") if l.startswith("BENCH_CHILD ")]
    if p.returncode != 0 or not lines:
        raise SystemExit(f"{' '.join(cmd)}: status {p.returncode}\n{p.stdout[-2000:]}{p.stderr[-4000:]}")
    return json.loads(lines[-1][len("BENCH_CHILD "):])


def main_folds(a):
    parent = os.path.abspath(a.parent) if a.parent else ROOT
    cv, split, grow_new, grow_parent, sums = [], [], [], [], set()
    for _ in range(a.runs):
        new = run_child(a, ROOT, "cv,grow")
        old = run_child(a, parent, "split,grow")
        cv.append(new["cv"]["ms"]), grow_new.append(new["grow"]["ms"])
        split.append(old["split"]["ms"]), grow_parent.append(old["grow"]["ms"])
        sums |= {new["cv"]["pred_sum"], old["split"]["pred_sum"]}
        print(f"round {len(cv)}: cv {cv[-1]:.1f} ms, split {split[-1]:.1f} ms, grow {grow_new[-1]:.1f} ms (parent {grow_parent[-1]:.1f} ms)", file=sys.stderr, flush=True)
    timed = run_child(a, ROOT, "cv", kernel_timing=True)["cv"]
    kernels = timed["kernels"]
    res = dict(
        what="pjb_forest_cv against per-fold pjb_forest_grow + pjb_forest_load + pjb_forest_predict", rows=a.rows, cols=29, trees=a.trees, folds=a.folds,
        matrix_seed=MATRIX_SEED, fold_seed=SEED, rounds=a.runs, parent_tree_measured=bool(a.parent),
        method="every figure from a process of its own: one warm-up call, one timed call; (a) and (c, this commit) in one process, (b) and (c, parent) in the next, alternating",
        a_cv_wall_ms=stats(cv), b_split_wall_ms=stats(split), c_grow_wall_ms=dict(parent=stats(grow_parent), this_commit=stats(grow_new)),
        same_predictions=len(sums) == 1,
        a_device_ms_by_kernel=kernels, a_device_ms_total=round(sum(v["ms"] for v in kernels.values()), 2), a_levels=kernels.get("kt_decide", {}).get("launches", 0),
        a_wall_ms_under_kernel_timing=round(timed["ms"], 2),
    )
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--trees", type=int, default=250)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ranger_cpu_s", type=float, default=None)
    ap.add_argument("--folds", type=int, default=0)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (with --folds)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--kernel_timing", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.folds:
        res = main_folds(a)
        out = a.out or os.path.join(ROOT, "profiles", "train_cv.json")
    else:
        res = main_grow(a)
        out = a.out or os.path.join(ROOT, "profiles", "train_grow.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main_grow(a):
    sys.path.insert(0, ROOT)
    from portcullis_amd import ffi
    m = bench_matrix(a.rows)
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
        wall_ms=stats(wall),
        device_ms_by_kernel=kt, device_ms_total=round(sum(v["ms"] for v in kt.values()), 2),
        levels=kt.get("kt_decide", {}).get("launches", 0), nodes=int(forest.tree_off[-1]), deepest_tree_nodes=int(np.diff(forest.tree_off).max()),
    )
    if a.ranger_cpu_s is not None:
        res["ranger_cpu"] = dict(seconds=a.ranger_cpu_s, note="ranger 0.3.8 (ranger_witness train, one thread) on the same matrix, timed by hand on the "
                                                              "build container's CPU: ANOTHER MACHINE than the device's host, not a like-for-like ratio")
    return res


if __name__ == "__main__":
    main()
