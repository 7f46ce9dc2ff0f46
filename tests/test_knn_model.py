"""tests/knn_model.py -- the numpy restatement of KNN::doSlice that the device's search is held to beyond the reference's own lists --
reproduces every list the reference wrote (tests/golden/selftrain/*.nn.npy of the KNN cases), and states the property the tie
matrices were made for.  No GPU."""
import os
import sys

import numpy as np
import pytest

import knn_model as km

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_knn_fixture as fx  # noqa: E402  (the generator of the matrices; it touches nothing on import)

CASES = {c["name"]: c for c in fx.load_cases()["knn"]}
FIRST = ("K700", "R1", "R2", "R3", "R4", "R5", "E63", "E64", "E65", "E129", "I1", "I32", "C2500")
ANCHORS = ("K8", "C31", "T1", "T2")


def test_the_cases_are_the_issues():
    assert tuple(CASES) == FIRST + ANCHORS
    assert (CASES["K8"]["k_used"], CASES["C31"]["cols"], CASES["C31"]["k_used"]) == (8, 31, 5)
    assert [(CASES[n]["kind"], CASES[n]["rows"], CASES[n]["cols"], CASES[n]["k_used"], CASES[n]["chunk"]) for n in ("T1", "T2")] == \
        [("ints", 300, 1, 8, 64), ("ints", 300, 2, 8, 64)]


@pytest.mark.parametrize("name", FIRST + ANCHORS)
def test_model_gives_the_references_lists(name):
    case = CASES[name]
    ref = np.load(fx.path(name + ".nn.npy"))
    assert ref.dtype == np.uint32 and ref.shape == (case["rows"], case["k_used"])
    got = km.knn(fx.case_matrix(case), case["k_used"])
    assert got.dtype == np.uint32 and np.array_equal(got, ref)


@pytest.mark.parametrize("name", ["T1", "T2"])
def test_tie_matrices_tie_across_chunks(name):
    """every row has more than 8 base rows at the distance of its eighth neighbour, in more than one chunk of 64 base rows"""
    case = CASES[name]
    m = fx.case_matrix(case)
    assert km.rows_tied_across_chunks(m, 8, case["chunk"]) == case["rows_tied_across_chunks"] == case["rows"]
    assert case["rows_with_equal_distances"] == case["rows"]
