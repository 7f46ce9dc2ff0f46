#!/usr/bin/env python3
"""Witness for the initial sets of self-training (build container only: `main` imports the REFERENCE's own rule_filter.py and needs pandas).

The reference's create_training_sets (scripts/portcullis/portcullis/rule_filter.py:134-333) runs under pandas over a generated junction
table, once per rule set of tests/golden/selftrain_data/, and the rows of the two tables it writes and its L95 are recorded in
tests/golden/selftrain_sets.json as keys (refname, start, end, consensus strand), in table order.  Nothing of the script travels.

tests/golden/selftrain_data/ is laid out as the reference's data/ directory: balanced/, precise/ and low_juncs_filter.json are copies of
the reference's files (settings only, like filt_rules/default_filter.json; `main` copies them again), lenient/ and strict/ are rule sets
of this project: lenient leaves twice as many positives as negatives (the SMOTE shape), strict more negatives than positives (the
under-sampling shape).

The table is not committed: `selftrain_table` makes it again from its seed (numpy only), 640 junctions on the coordinates of
tests/golden/spombe_III_30k.fa, and the tests import it from here (importing this module touches nothing).  It is shaped so that the
third positive layer of balanced / precise leaves 100 rows or fewer -- the branch that takes the layer's input back and stops -- and
so that every rule set leaves both sets non-empty; `main` asserts both.

Never run by a test or by build().

    python tests/golden/make_selftrain_sets_fixture.py        (needs /root/reference and pandas)
"""
import argparse
import glob
import io
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "selftrain_data")
REF = "/root/reference"
RULESETS = ("balanced", "precise", "lenient", "strict")
GENOME_NAME, GENOME_LEN = "III", 30000

HEADER = ("index refid refname reflen start end size left right read-strand ss-strand consensus-strand ss1 ss2 canonical_ss score suspicious pfp "
          "nb_raw_aln nb_dist_aln nb_us_aln nb_ms_aln nb_um_aln nb_mm_aln nb_bpp_aln nb_ppp_aln nb_rel_aln rel2raw nb_r1_pos nb_r1_neg nb_r2_pos nb_r2_neg "
          "entropy mean_mismatches mean_readlen max_min_anc maxmmes intron_score hamming5p hamming3p coding pws splice_sig uniq_junc primary_junc "
          "nb_up_juncs nb_down_juncs dist_2_up_junc dist_2_down_junc dist_nearest_junc mm_score coverage up_aln down_aln nb_samples").split() + \
         [f"JAD{k:02d}" for k in range(1, 21)]


def selftrain_table(n=640, seed=9001):
    """(header, rows): the cells of a .junctions.tab as text, sorted by (start, end).  Two kinds of junction, drawn with the seed:
    well supported ones (many reliable alignments, long anchors, few mismatches) and poorly supported ones (some of them very long)."""
    rng = np.random.RandomState(seed)
    taken, rows = set(), []
    while len(rows) < n:
        good = rng.uniform() < 0.68
        if good:
            size = int(40 + rng.lognormal(4.0, 0.6))
        else:
            size = int(rng.uniform(4000, 14000)) if rng.uniform() < 0.3 else int(30 + rng.lognormal(4.5, 0.9))
        size = min(size, 20000)
        start = int(rng.randint(400, GENOME_LEN - 400 - size))
        end = start + size - 1
        if (start, end) in taken:
            continue
        taken.add((start, end))
        anchor_l, anchor_r = int(rng.randint(12, 90)), int(rng.randint(12, 90))
        if good:
            raw = int(rng.randint(4, 200))
            rel = int(round(raw * rng.uniform(0.2, 1.0)))
            mmes = int(rng.randint(6, 46))
            h5, h3 = int(rng.randint(3, 13)), int(rng.randint(3, 13))
            mism = int(rng.binomial(raw, 0.25)) if rng.uniform() < 0.7 else 0
            entropy = rng.uniform(0.8, 5.0)
            css = "CCCCCCCSN"[rng.randint(9)]
            primary = int(rng.uniform() < 0.3)
            suspicious = pfp = 0
        else:
            raw = int(rng.randint(1, 8))
            rel = int(rng.randint(0, 2)) if rng.uniform() < 0.4 else 0
            mmes = int(rng.randint(1, 18))
            h5, h3 = int(rng.randint(0, 8)), int(rng.randint(0, 8))
            mism = int(rng.randint(0, 3 * raw + 1))
            entropy = 0.0 if raw == 1 else rng.uniform(0.0, 1.5)
            css = "CSNN"[rng.randint(4)]
            primary = int(rng.uniform() < 0.5)
            suspicious, pfp = int(rng.uniform() < 0.4), int(rng.uniform() < 0.3)
        rel = min(rel, raw)
        ms = int(rng.randint(0, raw + 1)) if good else int(rng.randint(0, 2)) * (raw - 1)
        um = int(rng.randint(raw // 2, raw + 1))
        dist = max(1, int(round(raw * rng.uniform(0.5, 1.0))))
        strand = "+-"[rng.randint(2)]
        ss1, ss2 = {"C": ("GT", "AG"), "S": ("GC", "AG"), "N": ("AA", "TT")}[css]
        jad = np.sort(rng.randint(0, raw + 1, 20))[::-1]
        jad[0] = raw
        r1p, r1n = raw // 4, raw // 4
        r2p = raw // 4
        cells = [0, 0, GENOME_NAME, GENOME_LEN, start, end, size, start - anchor_l, end + anchor_r, strand, strand, strand, ss1, ss2, css, 0, suspicious, pfp,
                 raw, dist, raw - ms, ms, um, raw - um, raw, raw, rel, "%g" % (rel / raw), r1p, r1n, r2p, raw - r1p - r1n - r2p,
                 "%g" % entropy, "%g" % (mism / raw), 84, mmes, mmes, 0, h5, h3, 0, 0, 0, 1, primary,
                 0, 0, 0, 0, 0, 0, 0, 0, 0, 1] + [int(v) for v in jad]
        rows.append([str(c) for c in cells])
    rows.sort(key=lambda r: (int(r[4]), int(r[5])))
    for k, r in enumerate(rows):
        r[0] = str(k)
    assert len(HEADER) == len(rows[0]) == 75
    return list(HEADER), rows


def table_text(header, rows):
    return "\n".join(["\t".join(header)] + ["\t".join(r) for r in rows]) + "\n"


def key(header, row):
    g = lambda n: row[header.index(n)]
    return [g("refname"), int(g("start")), int(g("end")), g("consensus-strand")]


def layer_files(ruleset):
    """(positive, negative) layer files of a rule set of selftrain_data/, by layer number"""
    number = lambda p: int(p.rsplit("layer", 1)[1].split(".")[0])
    files = glob.glob(os.path.join(DATA, ruleset, "*layer*.json"))
    return (sorted([f for f in files if "pos" in os.path.basename(f)], key=number), sorted([f for f in files if "neg" in os.path.basename(f)], key=number))


def load_sets():
    """selftrain_sets.json as committed (what the tests read)"""
    with open(os.path.join(HERE, "selftrain_sets.json")) as f:
        return json.load(f)


def main():
    import contextlib

    from make_rule_filter_fixture import load_reference_script
    rf = load_reference_script()
    for ruleset in ("balanced", "precise"):
        os.makedirs(os.path.join(DATA, ruleset), exist_ok=True)
        for f in glob.glob(os.path.join(REF, "data", ruleset, "*.json")):
            shutil.copyfile(f, os.path.join(DATA, ruleset, os.path.basename(f)))
    shutil.copyfile(os.path.join(REF, "data", "low_juncs_filter.json"), os.path.join(DATA, "low_juncs_filter.json"))
    header, rows = selftrain_table()
    out = {"_made_by": "tests/golden/make_selftrain_sets_fixture.py", "_reference": "scripts/portcullis/portcullis/rule_filter.py:134-333 (create_training_sets)",
           "n_rows": len(rows), "rulesets": {}}
    with tempfile.TemporaryDirectory() as d:
        tab = os.path.join(d, "in.junctions.tab")
        open(tab, "w").write(table_text(header, rows))
        for ruleset in RULESETS:
            pos_files, neg_files = layer_files(ruleset)
            assert pos_files and neg_files, ruleset
            prefix = os.path.join(d, ruleset)
            args = argparse.Namespace(input=tab, genuine=None, pos_json=pos_files, neg_json=neg_files, prefix=prefix, save_layers=True, save_failed=False,
                                      verbose=False)
            log, err = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(log), contextlib.redirect_stderr(err):
                rf.create_training_sets(args)
            sets = {}
            for which in ("pos", "neg"):
                lines = [l.split("\t") for l in open(f"{prefix}.{which}.junctions.tab").read().split("\n") if l]
                sets[which] = [key(lines[0], r) for r in lines[1:]]
            l95 = open(prefix + ".L95_intron_size.txt").read().split("\n")
            assert l95[0] == "Length of intron at 95th percentile"
            reverted = "Will not filter positive set further" in err.getvalue()
            layers = sorted(os.path.basename(p)[len(ruleset) + 1:] for p in glob.glob(prefix + ".*layer*.tab"))
            out["rulesets"][ruleset] = dict(pos=sets["pos"], neg=sets["neg"], L95=int(l95[1]), positive_layer_reverted=reverted, layer_tables=layers)
            print(f"{ruleset}: {len(sets['pos'])} positive, {len(sets['neg'])} negative, L95 {int(l95[1])}, reverted: {reverted}")
    r = out["rulesets"]
    assert r["balanced"]["positive_layer_reverted"] and r["precise"]["positive_layer_reverted"], "a positive layer of balanced must fall to 100 rows or fewer"
    assert not r["lenient"]["positive_layer_reverted"] and not r["strict"]["positive_layer_reverted"]
    for name, s in r.items():
        assert len(s["pos"]) >= 50 and len(s["neg"]) >= 50, (name, len(s["pos"]), len(s["neg"]))
    assert len(r["lenient"]["pos"]) >= 2 * len(r["lenient"]["neg"]), "lenient is the SMOTE shape"
    assert len(r["strict"]["neg"]) > len(r["strict"]["pos"]), "strict is the under-sampling shape"
    with open(os.path.join(HERE, "selftrain_sets.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    main()
