#!/usr/bin/env python3
"""Witness for the host's Performance strings (build container only: it imports the REFERENCE's own performance.py).

For about forty confusion matrices (tp, tn, fp, fn) the reference's scripts/portcullis/portcullis/performance.py prints its longStr():
the four counts and PREV BIAS SENS SPEC PPV NPV F1 ACC INFO MARK MCC with two decimals -- the columns of the C++ Performance::toLongString
(lib/src/performance.cc:39-57) in the same order, from the same arithmetic.  Recorded in tests/golden/performance_witness.json: the
quadruples and the strings.  Mind the script's constructor order: Performance(tp, fp, fn, tn).

Only quadruples are recorded at which the script and the C++ agree by construction: the script raises where nothing was counted
(prevalence of 0 / 0) and guards F1 and MCC with zeros where the C++ leaves 0 / 0 or the root of -0.0; tests/test_cv_model.py checks, without
the reference, that no recorded quadruple is one of those.  Nothing of the script travels: the fixture holds numbers and strings only.

    python tests/golden/make_performance_fixture.py        (needs /root/reference)
"""
import importlib.util
import json
import math
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/scripts/portcullis/portcullis/performance.py"

# by hand: balanced, perfect, all wrong, one empty cell each, large counts, a chance-level table (tp * tn == fp * fn)
BY_HAND = [(50, 50, 0, 0), (0, 0, 50, 50), (10, 20, 30, 40), (1, 1, 1, 1), (7, 0, 3, 2), (7, 5, 0, 2), (7, 5, 3, 0), (1, 999, 1, 1),
           (999, 1, 1, 1), (123456, 654321, 1234, 4321), (6, 6, 4, 9), (2, 3, 4, 6), (3000000, 1000000, 200000, 90000), (1, 0, 0, 1)]


def agree_by_construction(tp, tn, fp, fn):
    """False where the script raises or answers from a zero guard of its own that the C++ does not have"""
    if tp + tn + fp + fn == 0:
        return False
    pct = lambda a, b: 100.0 * a / b if b else 0.0
    prec, rec = pct(tp, tp + fp), pct(tp, tp + fn)
    if prec + rec == 0.0:
        return False
    x = (rec + pct(tn, fp + tn) - 100.0) * (prec + pct(tn, tn + fn) - 100.0)
    return x > 0.0 or (x == 0.0 and math.copysign(1.0, x) > 0)


def main():
    spec = importlib.util.spec_from_file_location("ref_performance", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = random.Random(20240521)
    quads = list(BY_HAND)
    while len(quads) < 60:
        top = rng.choice((5, 40, 1000, 100000))
        quads.append(tuple(rng.randrange(0, top) for _ in range(4)))
    rows = []
    for tp, tn, fp, fn in quads:
        if not agree_by_construction(tp, tn, fp, fn):
            continue
        rows.append({"tp": tp, "tn": tn, "fp": fp, "fn": fn, "long": mod.Performance(tp, fp, fn, tn).longStr()})
    rows = rows[:40]
    assert len(rows) == 40 and mod.Performance.longHeader().split("\t")[:4] == ["TP", "TN", "FP", "FN"]
    out = {"_made_by": "tests/golden/make_performance_fixture.py", "_reference": "scripts/portcullis/portcullis/performance.py:120-138 (longStr)",
           "header": mod.Performance.longHeader(), "rows": rows}
    with open(os.path.join(HERE, "performance_witness.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rows)} quadruples")


if __name__ == "__main__":
    main()
