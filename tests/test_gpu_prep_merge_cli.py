"""`portcullis_amd prep --merge` and `full --merge` on the device: three coordinate-sorted files -- one with its index beside it, two
without, one of them with nothing on a target, two with unplaced records behind their last target -- become the prepared directory that
the model's order (tests/merge_model.py) written as one file would have made."""
import gzip
import os

import numpy as np
import pytest

import hts_witness
import index_model as im
import merge_model as mm
from fuzzgen import make_reads
from test_gpu_full_cli import DATA, RULES, run, tail
from util_bam import PREP_BAM, PREP_FA, make_prep_dir, read_bam, write_bam, write_fasta

pytestmark = pytest.mark.gpu

PREPARED = sorted([PREP_BAM, PREP_BAM + ".bai", PREP_FA, PREP_FA + ".fai"])


def record_stream_of(path):
    """The alignment records of a BAM file as bytes (the inflated stream behind the header), and its targets."""
    refs, _ = read_bam(path)
    raw = gzip.open(path, "rb").read()
    n_text = int.from_bytes(raw[4:8], "little")
    at = 8 + n_text + 4 + sum(4 + len(n) + 1 + 4 for n, _ in refs)
    return refs, raw[at:], raw[8:8 + n_text].decode()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("prep_merge")
    refs, contigs, reads = [], [], []
    for tid in range(3):  # (the input of test_gpu_full_cli's `few`: under 200 junctions, so that full takes the rule file)
        genome, rr = make_reads(90 + tid, n_reads=400, glen=20000, n_tx=12)
        for k, r in enumerate(rr):
            r["tid"] = tid
            r["name"] = f"t{tid}r{k}" + "x" * (k % 5)
        refs.append((f"chr{tid + 1}", len(genome)))
        contigs.append((f"chr{tid + 1}", genome))
        reads += rr
    unplaced = [dict(tid=-1, pos=-1, cigar=np.zeros(0, np.uint32), seq="ACGTTGCA" * (2 + k % 3), flag=4, mapq=0, xs=None, mtid=-1, mpos=-1, name=f"u{k}")
                for k in range(37)]
    rng = np.random.default_rng(77)
    files = mm.stable_split(reads, 3, rng)
    moved = [r for r in files[2] if r["tid"] == 1]  # nothing on the second target in the third file: the second file takes them
    files[2] = [r for r in files[2] if r["tid"] != 1]
    files[1] = sorted(files[1] + moved, key=mm.merge_key)
    tails = mm.stable_split(unplaced, 2, rng)
    files[0] += tails[0]
    files[2] += tails[1]
    assert sum(len(f) for f in files) == len(reads) + len(unplaced) and all(tails)
    model = mm.merge_reads(files)
    assert [r["tid"] for r in model[-len(unplaced):]] == [-1] * len(unplaced)
    fa = str(d / "genome.fa")
    write_fasta(fa, contigs, write_index=False)
    bams = [str(d / f"in{k}.bam") for k in range(3)]
    for k, b in enumerate(bams):
        write_bam(b, refs, files[k], write_index=(k == 0), block_size=0xFF00 if k != 1 else 5000)
    hand = make_prep_dir(str(d / "hand"), refs, contigs, model)
    built = str(d / "built")
    p = run("prep", "--merge", "-v", "-t", "3", "-o", built, fa, *bams)
    assert p.returncode == 0, tail(p)
    return dict(d=d, refs=refs, fa=fa, bams=bams, files=files, model=model, hand=hand, built=built, stdout=p.stdout, n_unplaced=len(unplaced))


def test_the_directory_and_the_records(case):
    built = case["built"]
    assert sorted(os.listdir(built)) == PREPARED  # what PreparedFiles::valid asks for, and no temp*
    bam = os.path.join(built, PREP_BAM)
    assert os.path.isfile(bam) and not os.path.islink(bam)
    refs, stream, text = record_stream_of(bam)
    assert refs == case["refs"] and "@HD" in text.splitlines()[0] and "SO:coordinate" in text.splitlines()[0]
    assert stream == mm.record_stream(case["model"])
    _, recs = read_bam(bam)
    assert [(r["tid"], r["pos"], r["name"]) for r in recs] == [(r["tid"], r["pos"], r["name"]) for r in case["model"]]
    assert open(bam, "rb").read()[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    for k, f in enumerate(case["files"]):  # -v: records per file, written, unplaced
        placed = sum(1 for r in f if r["tid"] >= 0)
        assert f"{case['bams'][k]}: {placed} placed alignment records, {len(f) - placed} unplaced" in case["stdout"]
    assert f"written: {len(case['model'])} alignment records, {case['n_unplaced']} of them unplaced" in case["stdout"]


def test_the_index_is_the_merged_files(case):
    """The members' sizes are the device deflate's, so write_bam cannot write the same file; tests/index_model.py restates write_bam's
    index for a file as it is cut (held to write_bam's bytes by tests/test_index_model.py), and that is what the .bai must be."""
    bam = os.path.join(case["built"], PREP_BAM)
    assert open(bam + ".bai", "rb").read() == im.index_of(bam)


def test_htslib_reads_the_merged_file(case):
    refs, recs = hts_witness.records(os.path.join(case["built"], PREP_BAM))  # (skips where the witness cannot be built)
    assert refs == case["refs"]
    assert [(r["tid"], r["pos"], r["name"], r["flag"]) for r in recs] == [(r["tid"], r["pos"], r["name"], r["flag"]) for r in case["model"]]


def test_junc_sees_the_same_alignments(case, tmp_path):
    outs = {}
    for name, prep_dir in (("built", case["built"]), ("hand", case["hand"])):
        out = str(tmp_path / name / "pc")
        p = run("junc", "-t", "2", "-o", out, prep_dir)
        assert p.returncode == 0, tail(p)
        outs[name] = (open(out + ".junctions.tab", "rb").read(), open(out + ".junctions.bed", "rb").read())
    assert outs["built"] == outs["hand"]
    assert outs["built"][0].count(b"\n") > 10


def test_second_run_force_and_pieces(case, tmp_path):
    built, want = case["built"], mm.record_stream(case["model"])
    before = {n: os.lstat(os.path.join(built, n)).st_mtime_ns for n in os.listdir(built)}
    p = run("prep", "--merge", "-o", built, case["fa"], *case["bams"])
    assert p.returncode == 0 and "Pre-merged BAM detected" in p.stdout, tail(p)
    assert before == {n: os.lstat(os.path.join(built, n)).st_mtime_ns for n in os.listdir(built)}
    p = run("prep", "--merge", "--force", "-o", built, case["fa"], *case["bams"])
    assert p.returncode == 0 and "Merging 3 BAM files" in p.stdout, tail(p)
    assert sorted(os.listdir(built)) == PREPARED
    assert os.lstat(os.path.join(built, PREP_BAM)).st_mtime_ns != before[PREP_BAM]
    assert record_stream_of(os.path.join(built, PREP_BAM))[1] == want
    # the inputs' indexes built in small pieces: the same records
    small = str(tmp_path / "small")
    p = run("prep", "--merge", "-o", small, case["fa"], *case["bams"], env_extra={"PORTCULLIS_PIECE_BYTES": "4096"})
    assert p.returncode == 0, tail(p)
    assert sorted(os.listdir(small)) == PREPARED and record_stream_of(os.path.join(small, PREP_BAM))[1] == want


def test_full_merges_in_its_prep(case, tmp_path):
    y = str(tmp_path / "full")
    p = run("full", "--merge", "--keep_temp", "--self_train", DATA, "--training_rule", RULES, "-o", y, case["fa"], *case["bams"])
    assert p.returncode == 0, tail(p)
    prep = os.path.join(y, "1-prep")
    assert sorted(os.listdir(prep)) == PREPARED
    assert record_stream_of(os.path.join(prep, PREP_BAM))[1] == mm.record_stream(case["model"])
    assert os.path.exists(os.path.join(y, "2-junc", "portcullis_all.junctions.tab"))
