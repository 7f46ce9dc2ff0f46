"""tests/grow_model.py -- the Python restatement of ranger's growing that the device's grower is held to -- reproduces every forest
ranger 0.3.8 saved (tests/golden/forest_grow: six committed files, and SHA-256 and length of seventeen more cases), and states from
its own facts which case reaches which path of the device's kernels.  No GPU."""
import hashlib
import os
import sys

import numpy as np
import pytest

import grow_model as gm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_forest_grow_fixture as fx  # noqa: E402  (the generator of the matrices; it touches nothing on import)

CASES = {c["name"]: c for c in fx.load_cases()}
OLD = ("G1", "G2", "G3", "G4a", "G4b", "G5")
NEW = ("W1", "W2", "T250", "T17", "D1", "D2", "C4", "C33", "C65", "C130", "M1", "Mmax", "N1", "N3", "Z0", "ZS", "S2")

# condition (grow_model.conditions) -> the case that must meet it: a changed generator cannot quietly empty a case
REACHED_BY = dict(wide64="W1", wide128="W2", start64="G5", end64="G5", span3="W1", left63="W2", uneven="T250", no_split="C4", tied="G2")


@pytest.fixture(scope="module")
def grown():
    """name -> (the model's forest, its facts, rows); made once, never changed"""
    out = {}
    for name, case in CASES.items():
        cols, dep, mtry, min_node, seed = fx.case_args(case)
        m = fx.case_matrix(case)
        assert m.shape == (case["rows"], cols)
        forest, facts = gm.grow(m, case["trees"], seed, mtry, min_node, dep)
        out[name] = (forest, facts, m)
    return out


def test_the_cases_are_the_issues():
    assert tuple(CASES) == OLD + NEW
    assert all("sha256" not in CASES[n] for n in OLD) and all(len(CASES[n]["sha256"]) == 64 for n in NEW)
    largest = os.path.getsize(fx.forest_path(CASES["G5"]))
    for name in NEW:
        assert (CASES[name]["file"] is not None) == (CASES[name]["bytes"] < largest), name
    assert {n for n in NEW if CASES[n]["file"] is None} == {"W2", "T250"}
    c = CASES
    assert (c["W1"]["rows"], c["W1"]["trees"], fx.case_args(c["W1"])) == (4000, 2, (29, 0, 0, 0, fx.SEED))
    assert (c["W2"]["rows"], c["W2"]["trees"], fx.case_args(c["W2"])) == (2500, 2, (6, 0, 2, 1, fx.SEED))
    assert (c["T250"]["rows"], c["T250"]["trees"], c["T17"]["rows"], c["T17"]["trees"]) == (64, 250, 40, 17)
    assert (fx.case_args(c["D1"])[:2], fx.case_args(c["D2"])[:2]) == ((12, 7), (12, 11)) and c["D1"]["rows"] == c["D2"]["rows"] == 200
    assert (c["C4"]["rows"], fx.case_args(c["C4"])[:4]) == (150, (4, 0, 1, 1))
    assert [(c[n]["rows"], fx.case_args(c[n])[0]) for n in ("C33", "C65", "C130")] == [(120, 33), (120, 65), (120, 130)]
    assert (fx.case_args(c["M1"])[2], fx.case_args(c["Mmax"])[2], c["M1"]["rows"], c["Mmax"]["rows"]) == (1, 13, 300, 300)
    assert (fx.case_args(c["N1"])[3], fx.case_args(c["N3"])[3], c["N1"]["rows"], c["N3"]["rows"]) == (1, 3, 129, 129)
    assert (c["Z0"]["rows"], c["ZS"]["rows"], fx.case_args(c["ZS"])[0], fx.case_args(c["S2"])[4], c["S2"]["rows"]) == (30, 80, 5, 7, 300)
    # (tree + 1) * seed wraps around 2^32 from the fourth tree on with the default seed, and never in S2
    assert 4 * fx.SEED > 2**32 > c["S2"]["trees"] * fx.case_args(c["S2"])[4] and all(c[n]["trees"] >= 4 for n in NEW if n not in ("W1", "W2"))


@pytest.mark.parametrize("name", OLD)
def test_model_gives_the_committed_bytes(grown, name):
    assert grown[name][0].to_bytes() == open(fx.forest_path(CASES[name]), "rb").read()


@pytest.mark.parametrize("name", [n for n in NEW if n != "ZS"])
def test_model_gives_rangers_hash(grown, name):
    raw = grown[name][0].to_bytes()
    case = CASES[name]
    assert len(raw) == case["bytes"] and int(grown[name][0].tree_off[-1]) == case["nodes"]
    assert hashlib.sha256(raw).hexdigest() == case["sha256"]
    if case["file"]:
        assert open(fx.forest_path(case), "rb").read() == raw


def test_signed_zeros_differ_from_ranger_in_the_sign_only(grown):
    """ZS: column 1 holds -0.0 and +0.0.  The model (and the device) save the value of the last row of the left child; ranger saves
    the entry of its table of distinct values, which is the zero std::sort happened to leave first."""
    from portcullis_amd import ffi
    forest, _, m = grown["ZS"]
    case = CASES["ZS"]
    assert (np.signbit(m[m[:, 1] == 0, 1]).sum(), (m[:, 1] == 0).sum()) == (38, 68)
    assert not (np.signbit(m[:, 2:]) & (m[:, 2:] == 0)).any()
    ref_raw = open(fx.forest_path(case), "rb").read()
    assert len(ref_raw) == case["bytes"] and hashlib.sha256(ref_raw).hexdigest() == case["sha256"]
    ref = ffi.Forest.from_file(fx.forest_path(case))
    at_zero = np.flatnonzero((forest.left >= 0) & (forest.split_var == 1) & (forest.split_value == 0.0))
    assert len(at_zero) == 10 and set(np.signbit(forest.split_value[at_zero])) == {True, False}, "the split at zero must be the best one somewhere"
    assert not np.signbit(ref.split_value[at_zero]).any()
    assert forest.to_bytes() != ref_raw
    assert gm.clear_zero_signs(forest).to_bytes() == gm.clear_zero_signs(ref).to_bytes() == ref_raw


def test_single_classes(grown):
    for name, value in (("G3", 1.0), ("Z0", 0.0)):
        f = grown[name][0]
        assert f.class_values == [value] and f.n_classes == 1 and list(np.diff(f.tree_off)) == [1] * 4 and list(f.counts) == [1.0] * 4


@pytest.mark.parametrize("what", sorted(REACHED_BY))
def test_coverage_conditions(grown, what):
    name = REACHED_BY[what]
    _, facts, m = grown[name]
    assert gm.conditions(facts, len(m))[what], f"{name} no longer reaches `{what}`"


def test_what_the_cases_are_for(grown):
    widest = {n: max(max(f["levels"]) for f in grown[n][1]) for n in CASES}
    assert max(widest[n] for n in OLD) == 60, "the committed forests stay inside one wave of nodes"
    assert 64 < widest["W1"] <= 128 < widest["W2"]
    # W2: chains of deep levels -- several levels in a row wider than a wave
    assert any(sum(w > 64 for w in f["levels"]) >= 3 for f in grown["W2"][1])
    # T250 with grow_batch 48: the last batch (trees 240..249) has trees of different depth too
    assert len({len(f["levels"]) for f in grown["T250"][1][240:]}) > 1
    # C33, C65, C130: candidates past the first, the second and the fourth word of kt_draw's `seen` bits
    for name, above in (("C33", 31), ("C65", 63), ("C130", 127)):
        f = grown[name][0]
        assert (f.split_var[f.left >= 0] > above).any(), name
    # D1, D2: columns on both sides of the label split somewhere, the label's never
    for name in ("D1", "D2"):
        f, dep = grown[name][0], fx.case_args(CASES[name])[1]
        v = f.split_var[f.left >= 0]
        assert (v < dep).any() and (name == "D2" or (v > dep).any()) and not (v == dep).any() and f.dependent_var == dep
    # N1, N3: children of one row; nodes of 2 and 3 rows split, nodes of 4 to 10 rows split
    for name, size in (("N1", 1), ("N3", 3)):
        f, facts = grown[name][0], grown[name][1]
        split_sizes = {fa["count"][s["node"]] for fa in facts for s in fa["splits"]}
        assert min(split_sizes) == size + 1 and any(c == 1 for fa in facts for c in fa["count"]), name
    # C4: every candidate constant in a node of both labels; M1: one candidate a node
    assert sum(len(f["no_split"]) for f in grown["C4"][1]) > 10


def test_sweep_shapes():
    shapes = gm.sweep_shapes()
    assert 24 <= len(shapes) <= 32 and len({gm.sweep_id(s) for s in shapes}) == len(shapes)
    assert {s["rows"] for s in shapes} == set(gm.SWEEP_ROWS) and {s["cols"] for s in shapes} == set(gm.SWEEP_COLS)
    assert all(s["rows"] < 300 and s["trees"] < 8 for s in shapes)
    assert {s["min_node"] for s in shapes} == {0, 1, 3} and {s["ints"] for s in shapes} == {False, True}
    assert {("first", "middle", "last")[(s["dep"] > 0) + (s["dep"] == s["cols"] - 1)] for s in shapes} == {"first", "middle", "last"}
    classes = set()
    for s in shapes:
        m = gm.sweep_matrix(s)
        forest, _ = gm.grow(m, s["trees"], fx.SEED, 0, s["min_node"], s["dep"])
        assert forest.check() is None and forest.n_trees == s["trees"]
        classes.add(forest.n_classes)
    assert classes == {1, 2}
