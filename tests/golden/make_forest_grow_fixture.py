#!/usr/bin/env python3
"""Witnesses for the growing of a forest (build container only: `main` compiles and runs the REFERENCE's own ranger library).

ranger_witness.cc (beside this file, own code) is compiled in a scratch directory against deps/ranger-0.3.8 of the reference
checkout, as make_forest_fixture.py does, and `ranger_witness train` -- Forest::init as ModelFeatures::trainInstance calls it,
seed 1236456789, default mtry and node size -- grows one forest per case below.  Committed under tests/golden/forest_grow/: ranger's
saved bytes (<case>.forest) and cases.json (seeds and shapes).  The matrices are NOT committed: `case_matrix` makes them again from
the seeds, and the tests import it from here (importing this module touches neither the reference nor the device).

  G1  filt_forest/witness.forest, the existing witness (300 rows, 8 trees): nothing new is committed for it
  G2  ties: 96 rows of small integers, two pairs of identical columns, 16 trees -- equal scores, draw order decides
  G3  one class: 30 rows, all labels 1, 4 trees -- every tree is one terminal node
  G4  10 and 11 rows, 4 trees each: the node size test is `<=`
  G5  1500 rows, 8 trees: lists of 24 trips of 64 positions, nodes larger and smaller than a trip, nodes across trip borders

Never run by a test or by build().

    python tests/golden/make_forest_grow_fixture.py        (needs /root/reference)
"""
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_forest_fixture import N_COLS, matrix  # noqa: E402  (the generator of G1's matrix; numpy only)

RANGER = "/root/reference/deps/ranger-0.3.8"
OUT = os.path.join(HERE, "forest_grow")
SEED = 1236456789
TRIP = 64  # positions a wave of kt_split / kt_partition takes at a time: the only size the kernels know

CASES = [
    dict(name="G1", kind="matrix", rows=300, trees=8, rng=20240607, file="../filt_forest/witness.forest"),
    dict(name="G2", kind="ties", rows=96, trees=16, rng=7101, file="G2.forest"),
    dict(name="G3", kind="one_class", rows=30, trees=4, rng=7102, file="G3.forest"),
    dict(name="G4a", kind="matrix", rows=10, trees=4, rng=7103, file="G4a.forest"),
    dict(name="G4b", kind="matrix", rows=11, trees=4, rng=7104, file="G4b.forest"),
    dict(name="G5", kind="matrix", rows=1500, trees=8, rng=7105, file="G5.forest"),
]


def case_matrix(case):
    """The case's training matrix, float64 [rows, 29], column 0 the label."""
    rng = np.random.RandomState(case["rng"])
    n = case["rows"]
    if case["kind"] == "ties":
        m = rng.randint(0, 4, (n, N_COLS)).astype(np.float64)
        m[:, 10] = m[:, 9]
        m[:, 12] = m[:, 11]
        s = m[:, 1] + m[:, 9] - m[:, 11] + rng.normal(0, 0.8, n)
        m[:, 0] = (s > np.median(s)).astype(np.float64)
        return m
    m = matrix(rng, n, True)
    if case["kind"] == "one_class":
        m[:, 0] = 1.0
    return m


def load_cases():
    """cases.json as committed (what the tests read)"""
    with open(os.path.join(OUT, "cases.json")) as f:
        return json.load(f)["cases"]


def forest_path(case):
    return os.path.normpath(os.path.join(OUT, case["file"]))


class Mt19937_64:
    """std::mt19937_64"""

    def __init__(self, seed):
        m = (1 << 64) - 1
        self.s = [seed & m]
        for i in range(1, 312):
            x = self.s[-1]
            self.s.append((6364136223846793005 * (x ^ (x >> 62)) + i) & m)
        self.at = 312

    def __call__(self):
        s = self.s
        if self.at >= 312:
            for i in range(312):
                y = (s[i] & 0xFFFFFFFF80000000) | (s[(i + 1) % 312] & 0x7FFFFFFF)
                s[i] = s[(i + 156) % 312] ^ (y >> 1) ^ (0xB5026F5AA96619E9 if y & 1 else 0)
            self.at = 0
        y = s[self.at]
        self.at += 1
        y ^= (y >> 29) & 0x5555555555555555
        y ^= (y << 17) & 0x71D67FFFEDA60000
        y ^= (y << 37) & 0xFFF7EEE000000000
        y ^= y >> 43
        return y


def draw_candidates(gen, n_cols, dep, mtry):
    """Tree::createPossibleSplitVarSubset -> drawWithoutReplacementSimple, with libstdc++ 11's uniform_int_distribution
    (multiply-high with a rejection threshold) on a 64-bit generator"""
    rng, out = n_cols - 1, []
    thr = ((1 << 64) - rng) % rng
    while len(out) < mtry:
        prod = gen() * rng
        if (prod & ((1 << 64) - 1)) < rng:
            while (prod & ((1 << 64) - 1)) < thr:
                prod = gen() * rng
        d = prod >> 64
        if d >= dep:
            d += 1
        if d not in out:
            out.append(d)
    return out


def root_candidates(tree, n_cols=N_COLS, dep=0, mtry=5, seed=SEED):
    return draw_candidates(Mt19937_64(((tree + 1) * seed) & 0xFFFFFFFF), n_cols, dep, mtry)


def main():
    sys.path.insert(0, ROOT)
    from portcullis_amd import ffi
    os.makedirs(OUT, exist_ok=True)
    out_cases = []
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ranger_witness")
        srcs = [s for s in sorted(glob.glob(os.path.join(RANGER, "src", "*.cpp"))) if os.path.basename(s) not in ("main.cpp", "ArgumentHandler.cpp")]
        subprocess.check_call(["g++", "-O1", "-std=c++11", "-w", f"-I{RANGER}/include", f"-I{RANGER}/include/ranger", "-o", exe,
                               os.path.join(HERE, "ranger_witness.cc")] + srcs + ["-lpthread"])
        for case in CASES:
            m = case_matrix(case)
            assert m.shape == (case["rows"], N_COLS)
            m.astype("<f8").tofile(os.path.join(d, "train.f64"))
            subprocess.check_call([exe, "train", os.path.join(d, "train.f64"), str(case["rows"]), str(case["trees"]), os.path.join(d, case["name"])])
            raw = open(os.path.join(d, case["name"] + ".forest"), "rb").read()
            if case["name"] == "G1":
                assert raw == open(forest_path(case), "rb").read(), "G1 is the committed witness, grown again from its seed"
            else:
                open(forest_path(case), "wb").write(raw)
            forest = ffi.Forest.from_file(forest_path(case))
            assert forest.n_trees == case["trees"] and forest.n_vars == N_COLS and forest.check() is None
            sizes = np.diff(forest.tree_off)
            rec = dict(case, bytes=len(raw), nodes=int(forest.tree_off[-1]), n_classes=forest.n_classes)
            if case["kind"] == "one_class":
                assert forest.n_classes == 1 and (sizes == 1).all() and (forest.counts == 1.0).all()
            if case["name"] == "G4a":
                assert (sizes == 1).all(), "10 rows are a terminal node"
            if case["name"] == "G4b":
                assert (sizes > 1).any(), "11 rows are split"
            if case["kind"] == "ties":
                both = [t for t in range(case["trees"]) if any(a in c and b in c for c in [root_candidates(t)] for a, b in ((9, 10), (11, 12)))]
                assert both, "no root drew both columns of a copied pair"
                assert any(forest.split_var[forest.tree_off[t]] in (9, 10, 11, 12) for t in both)
                rec["roots_with_a_copied_pair"] = both
            # the first nodes of every tree must be the candidates this file's restatement of the draw allows
            for t in range(case["trees"]):
                if sizes[t] > 1:
                    assert forest.split_var[forest.tree_off[t]] in root_candidates(t), (case["name"], t)
            trips = (case["rows"] + TRIP - 1) // TRIP
            rec["crosses"] = (f"{trips} trip(s) of {TRIP} positions a list" + ("; nodes above and below a trip, nodes across trip borders" if trips > 1 else
                                                                            "; every node inside one trip"))
            print(f"{case['name']}: {len(raw)} bytes, {rec['nodes']} nodes, {forest.n_classes} classes; {rec['crosses']}")
            out_cases.append(rec)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(seed=SEED, n_cols=N_COLS, trip=TRIP, cases=out_cases), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
