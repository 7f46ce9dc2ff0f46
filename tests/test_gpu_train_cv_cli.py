"""`portcullis_amd train --folds` end to end with nothing but this repository: the prep -> junc -> split recipe of
tests/test_gpu_train_cli.py, then train --trees 8 --folds 3.

What is pinned: <prefix>.forest is byte for byte the file a run without --folds writes; <prefix>.cv_scores holds, per junction in sorted
order, the fold tests/cv_model.py deals it and the score 1 - pred[0] of ffi.forest_cv on the matrix built from ffi.filt_features (bit for
bit: %.17g); <prefix>.cv_results is cv_model's text for those scores, byte for byte, and stdout carries the same table; a second run
writes the same bytes.  pjb_forest_cv itself is pinned in test_gpu_forest_cv.py."""
import os
import subprocess

import numpy as np
import pytest

import cv_model as cm
import forest_util as fu
from fuzzgen import make_reads
from test_gpu_filt_cli import rows_of
from test_host_filt import read_tab
from util_bam import write_bam, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
SEED = 1236456789


def run(*args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PORTCULLIS_")}
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=env)


def test_prep_junc_train_folds(tmp_path):
    from portcullis_amd import ffi
    refs, contigs, reads = [], [], []
    for tid in range(6):
        genome, rr = make_reads(140 + tid, n_reads=2500, glen=24000 + 1500 * tid)
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
    text = open(junc + ".junctions.tab").read()
    header, rows = read_tab(text, is_text=True)
    lines = [l for l in text.split("\n") if l]
    label = np.array([int(r[header.index("nb_rel_aln")]) >= 12 and float(r[header.index("entropy")]) >= 2.0 for r in rows])
    assert len(rows) > 150 and 30 < label.sum() < len(rows) - 30
    pos, neg = str(tmp_path / "pos.tab"), str(tmp_path / "neg.tab")
    open(pos, "w").write("\n".join([lines[0]] + [l for l, g in zip(lines[1:], label) if g]) + "\n")
    open(neg, "w").write("\n".join([lines[0]] + [l for l, g in zip(lines[1:], label) if not g][::-1]) + "\n")

    plain, out, again = (str(tmp_path / d / "model") for d in ("plain", "cv", "again"))
    p = run("train", "--trees", "8", "-o", plain, prep, pos, neg)
    assert p.returncode == 0 and "cross validation" not in p.stdout, p.stdout[-1500:] + p.stderr[-1500:]
    assert sorted(os.listdir(os.path.dirname(plain))) == ["model.forest"]
    p = run("train", "--trees", "8", "--folds", "3", "-o", out, prep, pos, neg)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    assert sorted(os.listdir(os.path.dirname(out))) == ["model.cv_results", "model.cv_scores", "model.forest"]
    assert open(out + ".forest", "rb").read() == open(plain + ".forest", "rb").read()

    # ---- the same matrix through the Python binding: the table's own order is the sorted order
    drows = rows_of(ffi, header, rows)
    fold = cm.assign_folds(len(rows), 3, SEED)
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs([l for _, l in refs])
        for tid, (_, g) in enumerate(contigs):
            ctx.upload_contig(tid, g.encode())
        F = ctx.filt_features(drows, float(rows[0][header.index("mean_readlen")]), 0, {})
        M = np.ascontiguousarray(F[:, fu.ACTIVE_FEATURES])
        M[:, 0] = label
        pred, forests = ctx.forest_cv(M, fold, 3, n_trees=8)
    score = 1.0 - pred[:, 0]
    assert len(forests) == 3 and 0 < (score >= 0.5).sum() < len(rows)
    g = lambda r, n: r[header.index(n)]
    want = ["refid\tstart\tend\tstrand\tfold\tgenuine\tscore"]
    want += ["%s\t%s\t%s\t%s\t%d\t%d\t%s" % (g(r, "refid"), g(r, "start"), g(r, "end"), g(r, "consensus-strand"), fold[k] + 1, label[k], "%.17g" % score[k])
             for k, r in enumerate(rows)]
    assert open(out + ".cv_scores").read() == "\n".join(want) + "\n"
    table = cm.cv_results(fold, 3, label, score)
    assert open(out + ".cv_results").read() == table
    assert "Starting 3-fold cross validation\n" + table + "Cross validation completed\n" in p.stdout
    assert table.count("\n") == 1 + 3 + 10 and "nan" not in table

    # another threshold moves the calls, not the scores; a second run writes the same bytes
    q = run("train", "--trees", "8", "-k", "3", "--threshold", "0.9", "-o", again, prep, pos, neg)
    assert q.returncode == 0, q.stdout[-1500:] + q.stderr[-1500:]
    assert open(again + ".cv_scores", "rb").read() == open(out + ".cv_scores", "rb").read()
    assert open(again + ".cv_results").read() == cm.cv_results(fold, 3, label, score, threshold=0.9) != table
    q = run("train", "--trees", "8", "--folds", "3", "-o", again, prep, pos, neg)
    assert q.returncode == 0, q.stdout[-1500:] + q.stderr[-1500:]
    for ext in (".forest", ".cv_results", ".cv_scores"):
        assert open(again + ext, "rb").read() == open(out + ext, "rb").read(), ext
