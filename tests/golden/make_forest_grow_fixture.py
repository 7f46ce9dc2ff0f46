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

and one per case of MORE below, grown by `ranger_witness train` with its nine arguments -- column count, label column, mtry, node
size and seed as the case names them: levels wider than one and than two waves of nodes (W1, W2), 250 and 17 trees (T250, T17),
the label in another column (D1, D2), 4 to 130 columns (C4, C33, C65, C130), the smallest and the largest mtry of the simple draw
(M1, Mmax), node sizes 1 and 3 (N1, N3), the class 0 alone (Z0), a column with both zeros (ZS), seed 7 (S2).  Of these cases.json
records SHA-256, length and node count of ranger's bytes, and the file is committed only where it is smaller than G5.forest:
tests/grow_model.py restates ranger's growing and supplies the bytes of the others (tests/test_grow_model.py).

Never run by a test or by build().

    python tests/golden/make_forest_grow_fixture.py        (needs /root/reference)
"""
import glob
import hashlib
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
# The cases below call `ranger_witness train` with all nine arguments.  cols, dep (the label's column), mtry, min_node and seed default
# to 29, 0, 0, 0 (ranger's defaults: floor(sqrt(cols - 1)) and 10) and SEED.  Recorded: SHA-256, length and node count of ranger's bytes;
# the file itself only where it is smaller than G5.forest (tests/grow_model.py supplies every byte of the others).
MORE = [
    dict(name="W1", kind="round1", rows=4000, trees=2, rng=4029),
    dict(name="W2", kind="round1", rows=2500, cols=6, mtry=2, min_node=1, trees=2, rng=2506),
    dict(name="T250", kind="round1", rows=64, trees=250, rng=93),
    dict(name="T17", kind="round1", rows=40, trees=17, rng=69),
    dict(name="D1", kind="round1", rows=200, cols=12, dep=7, trees=4, rng=212),
    dict(name="D2", kind="round1", rows=200, cols=12, dep=11, trees=4, rng=213),
    dict(name="C4", kind="ints", rows=150, cols=4, mtry=1, min_node=1, trees=4, rng=154),
    dict(name="C33", kind="round1", rows=120, cols=33, trees=4, rng=153),
    dict(name="C65", kind="round1", rows=120, cols=65, trees=4, rng=185),
    dict(name="C130", kind="round1", rows=120, cols=130, trees=4, rng=250),
    dict(name="M1", kind="round1", rows=300, mtry=1, trees=4, rng=329),
    dict(name="Mmax", kind="round1", rows=300, mtry=13, trees=4, rng=330),
    dict(name="N1", kind="round1", rows=129, min_node=1, trees=4, rng=158),
    dict(name="N3", kind="round1", rows=129, min_node=3, trees=4, rng=159),
    dict(name="Z0", kind="zero_class", rows=30, trees=4, rng=59),
    dict(name="ZS", kind="signed_zeros", rows=80, cols=5, mtry=1, trees=8, rng=85),
    dict(name="S2", kind="round1", rows=300, seed=7, trees=4, rng=331),
]
LARGEST_FILE = 136793  # G5.forest: no larger forest is committed


def case_args(case):
    """(cols, dep, mtry, min_node, seed) of a case: what `Forest.grow`, the model and `ranger_witness train` are given"""
    return case.get("cols", N_COLS), case.get("dep", 0), case.get("mtry", 0), case.get("min_node", 0), case.get("seed", SEED)


def case_matrix(case):
    """The case's training matrix, float64 [rows, cols]: 29 columns and the label in column 0 unless the case says otherwise."""
    rng = np.random.RandomState(case["rng"])
    n = case["rows"]
    cols, dep = case.get("cols", N_COLS), case.get("dep", 0)
    if case["kind"] in ("round1", "zero_class", "ints"):  # unlearnable labels: the trees grow as deep as the node size lets them
        # (`+ 0.0`: rounding leaves -0.0 behind, and a column with both zeros is the business of ZS alone)
        m = rng.randint(0, 4, (n, cols)).astype(np.float64) if case["kind"] == "ints" else rng.normal(size=(n, cols)).round(1) + 0.0
        m[:, dep] = 0.0 if case["kind"] == "zero_class" else rng.randint(0, 2, n)
        return m
    if case["kind"] == "signed_zeros":
        # column 1: both zeros, in no order, and a few positive values; the label is `column 1 > 0` but for a few rows, so the split
        # at zero is the best one of column 1 and its left child (zeros only) has both labels
        m = rng.normal(size=(n, cols)).round(1) + 0.0
        m[:, 1] = np.where(rng.randint(0, 2, n) == 1, 0.0, -0.0)
        pos = rng.choice(n, 12, replace=False)
        m[pos, 1] = rng.randint(1, 4, 12)
        m[:, dep] = m[:, 1] > 0
        flip = rng.choice(n, 6, replace=False)
        m[flip, dep] = 1.0 - m[flip, dep]
        return m
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
        for case in MORE:
            m = case_matrix(case)
            cols, dep, mtry, min_node, seed = case_args(case)
            assert m.shape == (case["rows"], cols)
            m.astype("<f8").tofile(os.path.join(d, "train.f64"))
            subprocess.check_call([exe, "train", os.path.join(d, "train.f64"), str(case["rows"]), str(case["trees"]), os.path.join(d, case["name"])] +
                                  [str(v) for v in (cols, dep, mtry, min_node, seed)])
            raw = open(os.path.join(d, case["name"] + ".forest"), "rb").read()
            keep = len(raw) < LARGEST_FILE
            rec = dict(case, file=case["name"] + ".forest" if keep else None, bytes=len(raw), sha256=hashlib.sha256(raw).hexdigest())
            if keep:
                open(forest_path(rec), "wb").write(raw)
            forest = ffi.Forest.from_file(os.path.join(d, case["name"] + ".forest"))
            assert forest.n_trees == case["trees"] and forest.n_vars == cols and forest.dependent_var == dep and forest.check() is None
            rec.update(nodes=int(forest.tree_off[-1]), n_classes=forest.n_classes)
            sizes = np.diff(forest.tree_off)
            for t in range(case["trees"]):
                if sizes[t] > 1:
                    root = forest.split_var[forest.tree_off[t]]
                    assert root in root_candidates(t, cols, dep, mtry or max(1, int((cols - 1) ** 0.5)), seed), (case["name"], t)
            print(f"{case['name']}: {len(raw)} bytes, {rec['nodes']} nodes, {forest.n_classes} classes" + ("" if keep else "; the hash only"))
            out_cases.append(rec)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(seed=SEED, n_cols=N_COLS, trip=TRIP, cases=out_cases), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
