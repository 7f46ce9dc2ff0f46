#!/usr/bin/env python3
"""Witness for filt's rule engine (build container only: it imports the REFERENCE's own rule_filter.py and needs pandas).

Every rule file of tests/golden/filt_rules/ is turned into a pandas expression by the reference's json2pandas
(scripts/portcullis/portcullis/rule_filter.py:45-110) and evaluated, as its filter_one does (:341-357), over the oracle's .junctions.tab of
the fixed inputs of tests/filt_cases.py.  Recorded per case and rule file, in tests/golden/filt_rules.json: the junctions that pass
(refname, start, end, consensus strand), in table order.  Together the r*.json files cover every operator, a string column with in / not in,
two keys on one column (name.1, name.2), nested parentheses, an expression whose result depends on & binding tighter than |, a rule that
passes nothing and one that passes everything; default_filter.json is the reference's own file (settings only).

The two x*.json files are rule files the reference's script cannot evaluate, although its rule language allows them: it builds its pandas
expression by textual substitution, which corrupts a plain key beside a suffixed key on the same column (x01) and leaves the value of a
string `eq` unquoted (x02).  For these the fixture records the exception's name; tests/test_host_filt.py checks them against its own
restatement.  Nothing of the script travels: the fixture holds names and coordinates only.

    python tests/golden/make_rule_filter_fixture.py        (needs /root/reference and pandas)
"""
import glob
import importlib.util
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF_DIR = "/root/reference/scripts/portcullis/portcullis"


def load_reference_script():
    sys.path.insert(0, REF_DIR)  # (it imports its neighbour performance.py)
    spec = importlib.util.spec_from_file_location("ref_rule_filter", os.path.join(REF_DIR, "rule_filter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import pandas as pd
    from filt_cases import build_cases, tab_of
    rf = load_reference_script()
    rule_files = sorted(glob.glob(os.path.join(HERE, "filt_rules", "*.json")))
    out = {"_made_by": "tests/golden/make_rule_filter_fixture.py", "_reference": "scripts/portcullis/portcullis/rule_filter.py:45-110 (json2pandas), :341-357",
           "cases": {}}
    precedence_decides = False
    for name, case in build_cases().items():
        df = pd.read_csv(io.StringIO(tab_of(case)), sep="\t", header=0, index_col=0, na_values=rf.na_vals)
        fieldnames = [key for key in dict(df.dtypes)]
        per_rule = {}
        for path in rule_files:
            rule = os.path.basename(path)
            try:
                cmd_in, _ = rf.json2pandas(open(path), fieldnames, "df")
                passed = eval(cmd_in)
            except Exception as e:  # noqa: BLE001 -- the x*.json files: which exception is the recorded fact
                assert rule.startswith("x"), (rule, e)
                per_rule[rule] = {"reference_fails_with": type(e).__name__}
                continue
            assert not rule.startswith("x"), rule
            per_rule[rule] = {"passed": [[str(r), int(s), int(e), str(c)] for r, s, e, c in
                                         zip(passed["refname"], passed["start"], passed["end"], passed["consensus-strand"])]}
            if rule == "r03_precedence.json":
                other = df.loc[((df["rel2raw"] >= 0.8) | (df["entropy"] > 2.0)) & (df["nb_dist_aln"] >= 20)]
                precedence_decides = precedence_decides or len(other) != len(passed)
            print(f"{name}: {rule}: {len(passed)} of {len(df)} junctions pass")
        out["cases"][name] = {"n_rows": len(df), "rules": per_rule}
    assert precedence_decides, "r03 must give another result when read left to right"
    wide = out["cases"]["fuzz_wide_FR"]
    assert len(wide["rules"]["r05_passes_nothing.json"]["passed"]) == 0 and len(wide["rules"]["r06_passes_everything.json"]["passed"]) == wide["n_rows"]
    for rule, got in wide["rules"].items():
        if rule[0] == "r" and rule[:3] not in ("r05", "r06"):
            assert 10 < len(got["passed"]) < wide["n_rows"] - 10, (rule, len(got["passed"]))
    with open(os.path.join(HERE, "filt_rules.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
