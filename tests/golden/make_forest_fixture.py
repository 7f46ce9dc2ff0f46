#!/usr/bin/env python3
"""Witness for filt's forest stage (build container only: it compiles and runs the REFERENCE's own ranger library).

ranger_witness.cc (beside this file, own code) is compiled in a scratch directory against deps/ranger-0.3.8 of the reference
checkout.  With it this script

  * grows a probability forest of 8 trees on a 300 x 29 matrix with the header of the columns the reference leaves active
    ("Genuine" + 28), exactly as ModelFeatures::trainInstance calls Forest::init, and has ranger save it (Forest::saveToFile);
  * reads the saved file back (portcullis_amd.ffi.Forest.from_file, the Python reader of the same layout) and plants, in some rows
    of a 200 x 29 test matrix, values exactly equal to split values of nodes those rows reach: the `<=` edge is in the witness;
  * has ranger load the file and predict the test matrix as JunctionFilter::forestPredict does, and records getPredictions().

Committed under tests/golden/filt_forest/: witness.forest (ranger's bytes), test_matrix.npy and predictions.npy (raw float64 bits).
Nothing compiled and nothing of ranger's text travels.  Never run by a test or by build().

    python tests/golden/make_forest_fixture.py        (needs /root/reference)
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
RANGER = "/root/reference/deps/ranger-0.3.8"
OUT = os.path.join(HERE, "filt_forest")
N_COLS, N_TRAIN, N_TEST, N_TREES = 29, 300, 200, 8


def matrix(rng, n, labelled):
    """Columns shaped like the real ones: counts, ratios, scores, log deviations; the label (column 0) follows a noisy rule."""
    m = np.zeros((n, N_COLS))
    m[:, 1] = rng.poisson(6, n)                         # rna_rel
    m[:, 2] = np.round(rng.uniform(0, 1, n), 3)         # rna_rel2raw
    m[:, 3] = rng.randint(1, 40, n)                     # rna_maxmmes
    m[:, 4] = np.round(rng.exponential(0.4, n), 4)      # rna_missmatch
    m[:, 5] = 0.0                                       # rna_intron (L95 == 0)
    m[:, 6] = rng.randint(0, 11, n)                     # dna_minhamm
    m[:, 7] = 0.0                                       # dna_pws (untrained)
    m[:, 8] = 0.0                                       # dna_ss (untrained)
    m[:, 9:] = np.round(rng.normal(-1.0, 2.5, (n, 20)), 5)
    if labelled:
        s = 0.12 * m[:, 1] + 1.5 * m[:, 2] + 0.05 * m[:, 3] - 1.2 * m[:, 4] + 0.1 * m[:, 6] + 0.05 * m[:, 9] + rng.normal(0, 0.5, n)
        m[:, 0] = (s > np.median(s)).astype(float)
    return m


def walk(forest, t, row):
    """(node, value == split value) for every internal node the row visits in tree t"""
    base = int(forest.tree_off[t])
    k, seen = 0, []
    while forest.left[base + k] >= 0:
        v, s = row[forest.split_var[base + k]], forest.split_value[base + k]
        seen.append((k, v == s))
        k = int(forest.left[base + k] if v <= s else forest.right[base + k])
    return seen


def main():
    from portcullis_amd import ffi
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.RandomState(20240607)
    train, test = matrix(rng, N_TRAIN, True), matrix(rng, N_TEST, False)
    test[:, 0] = 12345.0    # the dependent column is never read
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ranger_witness")
        srcs = [s for s in sorted(glob.glob(os.path.join(RANGER, "src", "*.cpp"))) if os.path.basename(s) not in ("main.cpp", "ArgumentHandler.cpp")]
        subprocess.check_call(["g++", "-O1", "-std=c++11", "-w", f"-I{RANGER}/include", f"-I{RANGER}/include/ranger", "-o", exe,
                               os.path.join(HERE, "ranger_witness.cc")] + srcs + ["-lpthread"])
        train.astype("<f8").tofile(os.path.join(d, "train.f64"))
        subprocess.check_call([exe, "train", os.path.join(d, "train.f64"), str(N_TRAIN), str(N_TREES), os.path.join(d, "witness")])
        forest = ffi.Forest.from_file(os.path.join(d, "witness.forest"))
        assert forest.n_trees == N_TREES and forest.n_vars == N_COLS and forest.n_classes == 2 and forest.check() is None
        # plant: every third row takes, in one tree, the split value of the deepest internal node it reaches
        for r in range(0, N_TEST, 3):
            t = (r // 3) % N_TREES
            seen = walk(forest, t, test[r])
            if seen:
                k = int(forest.tree_off[t]) + seen[-1][0]
                test[r, forest.split_var[k]] = forest.split_value[k]
        on_edge = sum(hit for r in range(N_TEST) for t in range(N_TREES) for _, hit in walk(forest, t, test[r]))
        assert on_edge >= 40, on_edge
        test.astype("<f8").tofile(os.path.join(d, "test.f64"))
        subprocess.check_call([exe, "predict", os.path.join(d, "witness.forest"), os.path.join(d, "test.f64"), str(N_TEST), os.path.join(d, "pred.f64")])
        pred = np.fromfile(os.path.join(d, "pred.f64"), dtype="<f8").reshape(N_TEST, 2)
        raw = open(os.path.join(d, "witness.forest"), "rb").read()
    assert np.isfinite(pred).all() and np.abs(pred.sum(axis=1) - 1).max() < 1e-9 and len(np.unique(pred[:, 0])) > 20
    open(os.path.join(OUT, "witness.forest"), "wb").write(raw)
    np.save(os.path.join(OUT, "test_matrix.npy"), test.astype("<f8"))
    np.save(os.path.join(OUT, "predictions.npy"), pred)
    print(f"witness.forest: {len(raw)} bytes, {N_TREES} trees, {int(forest.tree_off[-1])} nodes, class values {forest.class_values}; "
          f"{on_edge} visits with value == split value; predictions of {N_TEST} rows recorded")


if __name__ == "__main__":
    main()
