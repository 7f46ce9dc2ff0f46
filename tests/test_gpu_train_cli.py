"""`portcullis_amd train` end to end with nothing but this repository: prep -> junc, the junction table split into a positive and a negative
table by a fixed rule, train --trees 8 --save_features, then filt --model_file with the model it wrote.

There is no reference pin at this level: the feature rows are SURVEY.md row f4, of which DESIGN.md section 2 lists the Markov scores as pinned
by the reference's own code and the window coordinates and the other columns as a restatement (the device's rows are within 1e-6 of the
oracle's, and a forest grown on them may split elsewhere).  What is pinned: the .forest file is byte for byte
ffi.Forest.grow() of the matrix built from ffi.filt_features of the same junctions in sorted order -- and growing is pinned against ranger
itself in test_gpu_forest_grow.py -- and filt's scores with that model are pjb_forest_predict's."""
import os
import subprocess

import numpy as np
import pytest

import forest_util as fu
from fuzzgen import make_reads
from test_gpu_filt_cli import rows_of
from test_host_filt import ident, read_tab
from util_bam import write_bam, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")


def run(*args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PORTCULLIS_")}
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=env)


def test_prep_junc_train_filt(tmp_path):
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
    assert len(rows) > 150

    # ---- the fixed rule: a junction with a dozen reliable alignments and some entropy is called genuine
    label = np.array([int(r[header.index("nb_rel_aln")]) >= 12 and float(r[header.index("entropy")]) >= 2.0 for r in rows])
    assert 30 < label.sum() < len(rows) - 30
    pos, neg = str(tmp_path / "pos.tab"), str(tmp_path / "neg.tab")
    open(pos, "w").write("\n".join([lines[0]] + [l for l, g in zip(lines[1:], label) if g]) + "\n")
    open(neg, "w").write("\n".join([lines[0]] + [l for l, g in zip(lines[1:], label) if not g][::-1]) + "\n")  # (any order: train sorts)

    out = str(tmp_path / "train" / "model")
    p = run("train", "--trees", "8", "--save_features", "-v", "-o", out, prep, pos, neg)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    assert "OOB" not in p.stdout and "Growing 8 trees" in p.stdout

    # ---- the same matrix through the Python binding: the table's own order is the sorted order
    drows = rows_of(ffi, header, rows)
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_refs([l for _, l in refs])
        for tid, (_, g) in enumerate(contigs):
            ctx.upload_contig(tid, g.encode())
        F = ctx.filt_features(drows, float(rows[0][header.index("mean_readlen")]), 0, {})
        M = np.ascontiguousarray(F[:, fu.ACTIVE_FEATURES])
        M[:, 0] = label
        grown = ffi.Forest.grow(ctx, M, n_trees=8)
        ctx.forest_load(grown)
        pred = ctx.forest_predict(M)
    raw = open(out + ".forest", "rb").read()
    assert grown.n_classes == 2 and int(grown.tree_off[-1]) > 8 * 3
    assert raw == grown.to_bytes()
    assert ffi.Forest.from_file(out + ".forest").check() is None

    # the feature rows it saved: the device's, the label in front, at the stream's six digits
    fh, frows = read_tab(out + ".features.training")
    assert fh == ["refid", "refname", "reflen", "start", "end"] + [ffi.FEATURE_NAMES[k] for k in fu.ACTIVE_FEATURES] and len(frows) == len(rows)
    for k, fr in enumerate(frows):
        assert [fr[1], int(fr[3]), int(fr[4])] == ident(header, rows[k])[:3]
        assert fr[5:] == ["%g" % v for v in M[k]], k

    # ---- filt takes the model: its scores are the walk's
    score = 1.0 - pred[:, 0]
    fout = str(tmp_path / "filt" / "pc")
    p = run("filt", "-m", out + ".forest", "--save_bad", "-o", fout, prep, junc + ".junctions.tab")
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    h, got = read_tab(fout + ".pass.junctions.tab")
    _, bad = read_tab(fout + ".fail.junctions.tab")
    want_pass = [k for k in range(len(rows)) if score[k] >= 0.5]
    want_fail = [k for k in range(len(rows)) if not score[k] >= 0.5]
    assert want_pass and want_fail
    assert [ident(h, r) for r in got] == [ident(header, rows[k]) for k in want_pass]
    assert [ident(h, r) for r in bad] == [ident(header, rows[k]) for k in want_fail]
    for table, ks in ((got, want_pass), (bad, want_fail)):
        assert [r[h.index("score")] for r in table] == ["%g" % score[k] for k in ks]
