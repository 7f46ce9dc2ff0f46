"""The whole pipeline with nothing but this repository: prep -> junc -> filt -m witness.forest --threshold t -f rules --save_bad -> bamfilt
on a three-target fuzz set.  What passes is checked against the Python walk of the forest over the DEVICE's feature rows (exact; the oracle's
are within 1e-6, which could flip a branch) followed by the rule file restated here."""
import os
import subprocess

import numpy as np
import pytest

import forest_util as fu
from fuzzgen import make_reads
from test_host_filt import ident, read_tab
from util_bam import PREP_BAM, write_bam, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
STRAND = {"+": 0, "-": 1, "?": 2}


def run(*args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PORTCULLIS_")}
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=env)


def rows_of(ffi, header, rows):
    """the junctions of a .tab as device rows, the way filt makes them: what the table does not hold (the sum of mismatches) from what it does"""
    out = np.zeros(len(rows), dtype=ffi.ROW_DTYPE)
    for k, r in enumerate(rows):
        g = lambda n: r[header.index(n)]
        o = out[k]
        o["refid"], o["start"], o["end"], o["left"], o["right"] = int(g("refid")), int(g("start")), int(g("end")), int(g("left")), int(g("right"))
        o["cons_strand"] = STRAND[g("consensus-strand")]
        o["nb_raw"], o["nb_dist"], o["nb_ms"], o["nb_rel"] = int(g("nb_raw_aln")), int(g("nb_dist_aln")), int(g("nb_ms_aln")), int(g("nb_rel_aln"))
        o["entropy"] = float(g("entropy"))
        o["max_min_anc"], o["maxmmes"], o["hamming5p"], o["hamming3p"] = int(g("max_min_anc")), int(g("maxmmes")), int(g("hamming5p")), int(g("hamming3p"))
        o["sum_mismatches"] = int(round(float(g("mean_mismatches")) * int(g("nb_raw_aln"))))
        o["jad"] = [int(g(f"JAD{i:02d}")) for i in range(1, 21)]
    return out


def test_prep_junc_filt_bamfilt(tmp_path):
    from portcullis_amd import ffi
    refs, contigs, reads = [], [], []
    for tid in range(3):
        genome, rr = make_reads(120 + tid, n_reads=2500, glen=24000 + 1500 * tid)
        for r in rr:
            r["tid"] = tid
        refs.append((f"chr{tid + 1}", len(genome)))
        contigs.append((f"chr{tid + 1}", genome))
        reads += rr
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "genome.fa")
    write_bam(bam, refs, reads, write_index=False)
    write_fasta(fa, contigs, write_index=False)
    prep = str(tmp_path / "prep")
    p = run("prep", "-o", prep, fa, bam)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    junc = str(tmp_path / "junc" / "pc")
    p = run("junc", "-o", junc, prep)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    header, rows = read_tab(junc + ".junctions.tab")
    assert len(rows) > 64

    # ---- what must pass: the forest over the device's own feature rows, then the rules
    forest, _, _ = fu.witness()
    drows = rows_of(ffi, header, rows)
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs([l for _, l in refs])
        for tid, (_, g) in enumerate(contigs):
            ctx.upload_contig(tid, g.encode())
        F = ctx.filt_features(drows, float(rows[0][header.index("mean_readlen")]), 0, {})
    score = 1.0 - fu.walk_predict(forest, F[:, fu.ACTIVE_FEATURES])[:, 0]
    assert len(np.unique(score)) > 5
    t = float(np.sort(score)[len(score) // 3])                      # a score some junction has exactly: `>=` keeps it
    by_forest = score >= t
    assert 0 < (~by_forest).sum() < len(rows) and (score == t).any()

    def rule(r):                                                     # default_filter.json
        g = lambda n: float(r[header.index(n)])
        return g("nb_rel_aln") >= 2 and g("entropy") >= 1.5 and g("maxmmes") >= 10 and g("hamming5p") >= 2 and g("hamming3p") >= 2
    want_pass = [k for k in range(len(rows)) if by_forest[k] and rule(rows[k])]
    want_fail = [k for k in range(len(rows)) if not by_forest[k]] + [k for k in range(len(rows)) if by_forest[k] and not rule(rows[k])]
    assert len(want_pass) > 3 and any(by_forest[k] for k in want_fail)

    out = str(tmp_path / "filt" / "pc")
    p = run("filt", "-m", os.path.join(fu.WITNESS_DIR, "witness.forest"), "--threshold", repr(t), "-f", os.path.join(ROOT, "tests", "golden", "filt_rules", "default_filter.json"),
            "--save_bad", "--save_features", "-o", out, prep, junc + ".junctions.tab")
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    h, got = read_tab(out + ".pass.junctions.tab")
    assert [ident(h, r) for r in got] == [ident(header, rows[k]) for k in want_pass]
    _, bad = read_tab(out + ".fail.junctions.tab")
    assert [ident(h, r) for r in bad] == [ident(header, rows[k]) for k in want_fail]
    # the score column (default stream formatting) and the BED score (fixed, three digits) of the score that went through the table
    for table, ks, suffix in ((got, want_pass, ".pass"), (bad, want_fail, ".fail")):
        bed = open(out + suffix + ".junctions.bed").read().split("\n")[1:-1]
        assert len(bed) == len(ks)
        for r, k, line in zip(table, ks, bed):
            text = "%g" % score[k]
            assert r[h.index("score")] == text, (k, r[h.index("score")], text)
            through_table = float(text) if (by_forest[k]) else score[k]   # (what the forest discards never enters the rule stage)
            assert line.split("\t")[4] == "%.3f" % through_table
    # the feature rows it saved are the device's, at the stream's six digits
    fh, frows = read_tab(out + ".features.testing")
    assert fh == ["refid", "refname", "reflen", "start", "end"] + [ffi.FEATURE_NAMES[k] for k in fu.ACTIVE_FEATURES] and len(frows) == len(rows)
    for fr, k in zip(frows, range(len(rows))):
        assert [c.lstrip("-") if c.endswith(("nan", "inf")) else c for c in fr[5:]] == \
               [("%g" % v).lstrip("-") if not np.isfinite(v) else "%g" % v for v in F[k, fu.ACTIVE_FEATURES]], k

    # ---- bamfilt takes what passed
    filtered = str(tmp_path / "filtered.bam")
    p = run("bamfilt", "-o", filtered, out + ".pass.junctions.tab", os.path.join(prep, PREP_BAM))
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    assert os.path.getsize(filtered) > 100 and os.path.getsize(filtered) < os.path.getsize(bam) + 4096
