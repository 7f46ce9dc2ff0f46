"""tests/cv_model.py, the plain-Python definition of `train --folds`, pinned without a device: the fold vector, the Performance strings
against the reference's own Python script (tests/golden/performance_witness.json, made by tests/golden/make_performance_fixture.py), the two
places where the reference's C++ leaves a NaN, and the mean lines against numbers worked out by hand.  The host's C++ Performance
(portcullis/ml/performance.hpp) is held to the same strings through tests/cpp/performance_check.cc."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import cv_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WITNESS = json.load(open(os.path.join(ROOT, "tests", "golden", "performance_witness.json")))
ROWS = WITNESS["rows"]
NAN_F1, NEG_ZERO_MCC = (0, 7, 0, 3), (0, 7, 0, 3)  # nothing called genuine: precision + recall = 0; informedness 0 x markedness -30 = -0.0
HAND = [(8, 8, 2, 2), (6, 9, 1, 4)]


def reference_cpp(tp, tn, fp, fn):
    """(F1, the radicand of MCC) as the reference's C++ computes them, guards and all: a NaN and a value <= -0.0 are what it trips on"""
    pct = lambda a, b: 100.0 * a / b if b else 0.0
    prec, rec = pct(tp, tp + fp), pct(tp, tp + fn)
    below = (1.0 * prec) + rec
    f1 = (1.0 + 1.0) * (prec * rec) / below if below != 0.0 else math.nan
    return f1, (rec + pct(tn, fp + tn) - 100.0) * (prec + pct(tn, tn + fn) - 100.0)


def test_fold_vector():
    for n, k, seed in ((23, 5, 1236456789), (23, 5, 7), (200, 3, 1236456789), (7, 7, 1), (2, 2, 99)):
        v = cm.assign_folds(n, k, seed)
        assert v.dtype == np.int32 and sorted(v) == sorted(i % k for i in range(n))  # a permutation of i % k
        assert np.array_equal(v, cm.assign_folds(n, k, seed))
    # (the same numbers from libstdc++'s std::mt19937_64 and the loop of Train::assignFolds)
    assert list(cm.assign_folds(23, 5, 1236456789)) == [0, 0, 2, 1, 1, 3, 1, 2, 2, 4, 0, 3, 3, 2, 4, 3, 4, 0, 4, 1, 0, 1, 2]
    assert list(cm.assign_folds(23, 5, 7)) == [0, 4, 2, 1, 0, 3, 3, 1, 1, 4, 2, 4, 2, 2, 0, 1, 0, 4, 2, 1, 0, 3, 3]
    assert not np.array_equal(cm.assign_folds(200, 3, 1), cm.assign_folds(200, 3, 2))
    assert list(cm.assign_folds(1, 2, 5)) == [0]


def test_witness_quadruples_are_those_the_script_and_the_cpp_agree_on():
    assert len(ROWS) >= 38 and WITNESS["header"] == cm.LONG_HEADER
    assert len({(r["tp"], r["tn"], r["fp"], r["fn"]) for r in ROWS}) == len(ROWS)
    for r in ROWS:
        q = (r["tp"], r["tn"], r["fp"], r["fn"])
        assert sum(q) > 0, q  # (the script divides by the total)
        f1, x = reference_cpp(*q)
        assert not math.isnan(f1) and (x > 0.0 or (x == 0.0 and math.copysign(1.0, x) > 0)), q
    # and they are not all of one kind: an empty cell of each name, large counts, a table at chance level
    # (tp = 0 is precision + recall = 0: the script's guard, test_the_two_nan_cases_give_zero)
    for cell in ("tn", "fp", "fn"):
        assert any(r[cell] == 0 for r in ROWS), cell
    assert any(r[cell] > 100000 for r in ROWS for cell in ("tp", "tn", "fp", "fn"))
    assert any(r["tp"] * r["tn"] == r["fp"] * r["fn"] and min(r["tp"], r["tn"], r["fp"], r["fn"]) > 0 for r in ROWS)
    assert any(r["long"].split("\t")[12].startswith("-") for r in ROWS)  # a negative informedness


@pytest.mark.parametrize("k", range(len(ROWS)))
def test_long_string_is_the_reference_scripts(k):
    r = ROWS[k]
    assert cm.Performance(r["tp"], r["tn"], r["fp"], r["fn"]).long_string() == r["long"]


def test_the_two_nan_cases_give_zero():
    f1, x = reference_cpp(*NAN_F1)
    assert math.isnan(f1) and x == 0.0 and math.copysign(1.0, x) < 0
    p = cm.Performance(*NAN_F1)
    assert p.f1() == 0.0 and p.mcc() == 0.0 and math.copysign(1.0, p.mcc()) > 0
    assert p.long_string() == "0\t7\t0\t3\t30.00\t0.00\t0.00\t100.00\t0.00\t70.00\t0.00\t70.00\t0.00\t-30.00\t0.00"
    # a radicand below 0 (rounding could leave one where tp * tn == fp * fn; no table we know reaches it): 0, not a NaN
    assert cm.Performance.mcc_of(-1e-14, 2e-14) == 0.0 and cm.Performance.mcc_of(25.0, 4.0) == 10.0
    assert "nan" not in cm.mean_lines([p, cm.Performance(5, 5, 0, 0)])


def test_mean_lines_by_hand():
    """(8, 8, 2, 2): every rate 80 or 50, informedness = markedness = MCC = 60.  (6, 9, 1, 4): prevalence 50, bias 35, recall 60,
    precision 600 / 7, specificity 90, accuracy 75.  Means and population deviations of two values a, b: (a + b) / 2 and |a - b| / 2."""
    perfs = [cm.Performance(*q) for q in HAND]
    assert perfs[0].long_string() == "8\t8\t2\t2\t50.00\t50.00\t80.00\t80.00\t80.00\t80.00\t80.00\t80.00\t60.00\t60.00\t60.00"
    text = cm.mean_lines(perfs)
    lines = text.split("\n")
    assert len(lines) == 11 and lines[-1] == "" and [l[5:18].rstrip() for l in lines[:10]] == list(cm.MEAN_NAMES)
    assert lines[0] == "Mean prevalence   : 50.00% (+/- 0.00%)"
    assert lines[1] == "Mean bias         : 42.50% (+/- 7.50%)"
    assert lines[2] == "Mean recall       : 70.00% (+/- 10.00%)"
    assert lines[3] == "Mean precision    : 82.86% (+/- 2.86%)"
    assert lines[5] == "Mean specificity  : 85.00% (+/- 5.00%)"
    assert lines[6] == "Mean accuracy     : 77.50% (+/- 2.50%)"
    assert lines[7] == "Mean informedness : 55.00% (+/- 5.00%)"
    assert lines[8].startswith("Mean markededness :") and lines[9].startswith("Mean MCC          :")
    f1 = 2.0 * (600.0 / 7 * 60.0) / (600.0 / 7 + 60.0)
    assert lines[4] == "Mean F1           : %.2f%% (+/- %.2f%%)" % ((80.0 + f1) / 2, (80.0 - f1) / 2)


def test_cv_results_text():
    fold, genuine = [0, 1, 0, 1, 0, 1], [1, 1, 0, 0, 1, 0]
    score = [0.9, 0.5, 0.2, 0.7, 0.49, 0.1]
    text = cm.cv_results(fold, 2, genuine, score)
    lines = text.split("\n")
    assert lines[0] == "Fold\t" + cm.LONG_HEADER and lines[1].startswith("1\t1\t1\t0\t1\t") and lines[2].startswith("2\t1\t1\t1\t0\t") and len(lines) == 14
    assert cm.cv_results(fold, 2, genuine, score, threshold=0.49).split("\n")[1].startswith("1\t2\t1\t0\t0\t")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("performance_check") / "performance_check")
    host = os.path.join(ROOT, "portcullis_amd", "host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", f"-I{host}/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "performance_check.cc"),
                           os.path.join(host, "src", "performance.cc")])
    return exe


def test_the_hosts_performance_prints_the_same(checker):
    quads = [(r["tp"], r["tn"], r["fp"], r["fn"]) for r in ROWS] + [NAN_F1] + HAND
    p = subprocess.run([checker] + ["%d,%d,%d,%d" % q for q in quads], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    strings, means = p.stdout.split("--\n")
    assert strings.split("\n")[:-1] == [r["long"] for r in ROWS] + [cm.Performance(*q).long_string() for q in [NAN_F1] + HAND]
    assert means == cm.mean_lines([cm.Performance(*q) for q in quads]) and "nan" not in p.stdout
    # folds of one value: the deviation is 0, whatever the rounding of the two sums leaves
    p = subprocess.run([checker] + ["3,3,1,2"] * 7, capture_output=True, text=True, timeout=60)
    assert p.stdout.split("--\n")[1] == cm.mean_lines([cm.Performance(3, 3, 1, 2)] * 7) and "nan" not in p.stdout
