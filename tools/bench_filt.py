#!/usr/bin/env python3
"""Measurement of filt's forest stage: one JSON line to profiles/filt_predict.json (and stdout).

Inputs: 250 000 junctions x 29 variables and 250 trees (DEFAULT_SELFTRAIN_TREES of the reference).  The trees are synthetic.  Their size:
the witness forest that the reference's ranger grew (tests/golden/filt_forest: 8 trees, 300 training rows, minimum node size 10, the settings
of ModelFeatures::trainInstance) has 622 nodes, 0.26 nodes per tree and training row; a self-training run trains on the order of 20 000
junctions, which makes 5 201 nodes a tree (2 600 splits).  A tree is grown by splitting a leaf drawn at random 2 600 times (mean depth of a
leaf about 2 ln(2 600) = 16, the deepest about twice that); split variables are uniform over the 28 features and split values are values of
that variable in the data, so that rows spread over the leaves.

Measured on a warmed context, five runs each, median with min and max: the device time (HIP events around the kernels) of the walk alone
(pjb_forest_predict), of the feature kernel alone (pjb_filt_features) and of both in the fused call (pjb_filt_scores); the wall time of each
call through ffi (PCIe copies included) on a context without event timing; and, for scale, a numpy walk on the host over the first 10 trees
(level by level over all rows), checked bit for bit against the device's walk of the same 10 trees.

    timeout 900 python tools/bench_filt.py
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_ROWS, N_VARS, N_TREES, N_SPLITS, HOST_TREES, RUNS = 250_000, 29, 250, 2600, 10, 5


def grow(rng, np, values):
    """one tree of N_SPLITS splits, numbered as ranger numbers it (children appended in pairs behind their parent)"""
    n = 2 * N_SPLITS + 1
    left, right = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    var, val = np.zeros(n, np.int32), np.zeros(n, np.float64)
    leaves, used = [0], 1
    for _ in range(N_SPLITS):
        k = leaves.pop(int(rng.integers(len(leaves))))
        left[k], right[k] = used, used + 1
        var[k] = int(rng.integers(1, N_VARS))
        val[k] = values[int(rng.integers(len(values))), var[k]]
        leaves += [used, used + 1]
        used += 2
    counts = [[] if left[k] >= 0 else [float(a), float(10 - a)] for k, a in enumerate(rng.integers(0, 11, n))]
    return dict(left=left, right=right, split_var=var, split_value=val, counts=counts)


def numpy_walk(np, forest, trees, X):
    out = np.zeros((len(X), forest.n_classes))
    rows = np.arange(len(X))
    for t in range(trees):
        base = int(forest.tree_off[t])
        node = np.zeros(len(X), np.int64)
        while True:
            l = forest.left[base + node]
            live = l >= 0
            if not live.any():
                break
            go_left = X[rows, forest.split_var[base + node]] <= forest.split_value[base + node]
            node = np.where(live, np.where(go_left, l, forest.right[base + node]), node)
        at = forest.count_off[base + node]
        for c in range(forest.n_classes):
            out[:, c] = out[:, c] + forest.counts[at + c] / np.float64(trees)
    return out


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def main():
    import numpy as np

    import forest_util as fu
    from portcullis_amd import ffi

    rng = np.random.default_rng(250)
    # junction rows on one synthetic target: what the feature kernel reads
    glen = 5_000_000
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), glen).tobytes()
    rows = np.zeros(N_ROWS, dtype=ffi.ROW_DTYPE)
    rows["start"] = np.sort(rng.integers(200, glen - 20_000, N_ROWS))
    rows["end"] = rows["start"] + rng.integers(20, 10_000, N_ROWS)
    rows["left"], rows["right"] = rows["start"] - 50, rows["end"] + 50
    rows["cons_strand"] = rng.integers(0, 3, N_ROWS)
    rows["nb_raw"] = rng.integers(1, 200, N_ROWS)
    rows["nb_rel"] = (rows["nb_raw"] * rng.random(N_ROWS)).astype(np.uint32)
    rows["nb_dist"] = rows["nb_raw"]
    rows["sum_mismatches"] = rng.integers(0, 300, N_ROWS)
    rows["entropy"] = rng.random(N_ROWS) * 6
    rows["maxmmes"] = rng.integers(1, 75, N_ROWS)
    rows["max_min_anc"] = rows["maxmmes"]
    rows["hamming5p"], rows["hamming3p"] = rng.integers(0, 11, N_ROWS), rng.integers(0, 11, N_ROWS)
    rows["jad"] = (rows["nb_raw"][:, None] * np.linspace(1, 0.05, 20)[None, :] * rng.random((N_ROWS, 20))).astype(np.uint32)
    mrl = 100.0
    res = {"workload": f"{N_ROWS} junctions x {N_VARS} variables, {N_TREES} synthetic trees of {2 * N_SPLITS + 1} nodes, 2 classes"}
    with ffi.Context(0, "UNKNOWN", flags=ffi.FLAG_KERNEL_TIMING) as ctx:
        ctx.set_refs([glen])
        ctx.upload_contig(0, genome)
        F = ctx.filt_features(rows, mrl, 0, {})
        X = np.ascontiguousarray(F[:, fu.ACTIVE_FEATURES])
        sample = np.nan_to_num(X[rng.integers(0, N_ROWS, 4096)], nan=0.0, posinf=0.0, neginf=0.0)
        forest = ffi.Forest(N_VARS, 2, [grow(rng, np, sample) for _ in range(N_TREES)], dependent_var=0)
        assert forest.check() is None
        # correctness first: the first HOST_TREES trees, host against device, bit for bit
        small = ffi.Forest(N_VARS, 2, [dict(left=forest.left[a:b], right=forest.right[a:b], split_var=forest.split_var[a:b], split_value=forest.split_value[a:b],
                                            counts=[[] if forest.count_off[k] < 0 else list(forest.counts[forest.count_off[k]:forest.count_off[k] + 2]) for k in range(a, b)])
                                       for a, b in zip(forest.tree_off[:HOST_TREES], forest.tree_off[1:HOST_TREES + 1])], dependent_var=0)
        ctx.forest_load(small)
        dev_small = ctx.forest_predict(X)
        t0 = time.perf_counter()
        host_small = numpy_walk(np, small, HOST_TREES, X)
        res["numpy_walk_host_s"] = {"trees": HOST_TREES, "seconds": round(time.perf_counter() - t0, 3), "cores": 1,
                                    "note": f"level by level over all rows; {N_TREES} trees would take {N_TREES // HOST_TREES} times as long"}
        assert (host_small.view(np.uint64) == dev_small.view(np.uint64)).all(), "device walk differs from the host walk"
        ctx.forest_load(forest)
        pred = ctx.forest_predict(X)                                  # warm: buffers sized
        fused = ctx.filt_scores(rows, mrl, 0, {}, fu.ACTIVE_FEATURES)
        res["fused_equals_separate"] = bool((fused.view(np.uint64) == pred.view(np.uint64)).all())
        walk_ms, feat_ms, fused_ms, fused_parts = [], [], [], []
        for _ in range(RUNS):
            ctx.reset_kernel_timing()
            ctx.forest_predict(X)
            k = ctx.kernel_timing()
            walk_ms.append(k["kr_forest"][1])
            ctx.reset_kernel_timing()
            ctx.filt_features(rows, mrl, 0, {})
            feat_ms.append(ctx.kernel_timing()["kg_features"][1])
            ctx.reset_kernel_timing()
            ctx.filt_scores(rows, mrl, 0, {}, fu.ACTIVE_FEATURES)
            k = ctx.kernel_timing()
            fused_ms.append(k["kr_forest"][1] + k["kg_features"][1])
            fused_parts.append((k["kg_features"][1], k["kr_forest"][1]))
        res["device_ms"] = {"walk_alone": stats(walk_ms), "features_alone": stats(feat_ms), "fused_call_kernels": stats(fused_ms),
                            "fused_call_walk_part": stats([p[1] for p in fused_parts])}
    with ffi.Context(0, "UNKNOWN") as ctx:                            # wall times: no events between the kernels
        ctx.set_refs([glen])
        ctx.upload_contig(0, genome)
        ctx.forest_load(forest)
        ctx.forest_predict(X), ctx.filt_features(rows, mrl, 0, {}), ctx.filt_scores(rows, mrl, 0, {}, fu.ACTIVE_FEATURES)
        wall = {"forest_predict": [], "filt_features": [], "filt_scores": [], "filt_scores_with_features_out": []}
        for _ in range(RUNS):
            for name, call in (("forest_predict", lambda: ctx.forest_predict(X)), ("filt_features", lambda: ctx.filt_features(rows, mrl, 0, {})),
                               ("filt_scores", lambda: ctx.filt_scores(rows, mrl, 0, {}, fu.ACTIVE_FEATURES)),
                               ("filt_scores_with_features_out", lambda: ctx.filt_scores(rows, mrl, 0, {}, fu.ACTIVE_FEATURES, want_features=True))):
                t0 = time.perf_counter()
                call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
        res["wall_ms_through_ffi"] = {k: stats(v) for k, v in wall.items()}
    w = res["device_ms"]["walk_alone"]["median"]
    res["walk_over_features_ratio"] = round(w / res["device_ms"]["features_alone"]["median"], 2)
    res["tree_walks_per_sec"] = round(N_ROWS * N_TREES / (w * 1e-3))
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "filt_predict.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
