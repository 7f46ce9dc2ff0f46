"""`portcullis_amd prep --sort` and `full --sort` on the device: a shuffled file and tests/golden/unsorted.bam become the prepared
directory that the model's order -- sorted(records, key=(refID as unsigned, pos)), Python's stable sort -- written as one file would
have made; in one run and in several, alone and in front of a merge."""
import gzip
import os
import re
import struct

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
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def parts_of(path):
    """(targets, header text, the alignment records as a list of byte strings) of a BAM file."""
    refs, _ = read_bam(path)
    raw = gzip.open(path, "rb").read()
    n_text = int.from_bytes(raw[4:8], "little")
    at = 8 + n_text + 4 + sum(4 + len(n) + 1 + 4 for n, _ in refs)
    recs = []
    while at < len(raw):
        (bs,) = struct.unpack_from("<i", raw, at)
        recs.append(raw[at:at + 4 + bs])
        at += 4 + bs
    assert at == len(raw)
    return refs, raw[8:8 + n_text].decode(), recs


def raw_key(rec):
    tid, pos = struct.unpack_from("<ii", rec, 4)
    return (tid & 0xFFFFFFFF, pos)


def sorted_stream(path):
    return b"".join(sorted(parts_of(path)[2], key=raw_key))


def leftovers(d):
    return sorted(n for n in os.listdir(d) if n.startswith(("temp", "sortrun")) or n.endswith(".tmp"))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("prep_sort")
    refs, contigs, reads = [], [], []
    for tid in range(3):  # (the input of test_gpu_full_cli's `few`: under 200 junctions, so that full takes the rule file)
        genome, rr = make_reads(90 + tid, n_reads=400, glen=20000, n_tx=12)
        for k, r in enumerate(rr):
            r["tid"] = tid
            r["name"] = f"t{tid}r{k}" + "x" * (k % 5)
        refs.append((f"chr{tid + 1}", len(genome)))
        contigs.append((f"chr{tid + 1}", genome))
        reads += rr
    reads += [dict(tid=-1, pos=-1, cigar=np.zeros(0, np.uint32), seq="ACGTTGCA" * (2 + k % 3), flag=4, mapq=0, xs=None, mtid=-1, mpos=-1, name=f"u{k}")
              for k in range(37)]
    rng = np.random.default_rng(78)
    shuffled = [reads[k] for k in rng.permutation(len(reads))]
    model = sorted(shuffled, key=mm.merge_key)
    fa = str(d / "genome.fa")
    write_fasta(fa, contigs, write_index=False)
    text = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in refs) + "@PG\tID:aligner\tPN:aligner\tVN:2\n@CO\tkept as it is\n"
    bam, pre = str(d / "shuffled.bam"), str(d / "presorted.bam")
    write_bam(bam, refs, shuffled, write_index=False, block_size=5000, header_text=text)
    write_bam(pre, refs, model, write_index=False)
    hand = make_prep_dir(str(d / "hand"), refs, contigs, model)
    built = str(d / "built")
    p = run("prep", "--sort", "-v", "-o", built, fa, bam)
    assert p.returncode == 0, tail(p)
    return dict(d=d, refs=refs, fa=fa, bam=bam, pre=pre, text=text, shuffled=shuffled, model=model, hand=hand, built=built, stdout=p.stdout)


def test_the_directory_and_the_records(case):
    built = case["built"]
    assert sorted(os.listdir(built)) == PREPARED  # what PreparedFiles::valid asks for, and no sortrun* / temp*
    bam = os.path.join(built, PREP_BAM)
    assert os.path.isfile(bam) and not os.path.islink(bam)
    refs, text, recs = parts_of(bam)
    assert refs == case["refs"]
    assert b"".join(recs) == mm.record_stream(case["model"]) == sorted_stream(case["bam"])
    # @HD says SO:coordinate, the rest of the header is the input's
    want = case["text"].splitlines()
    assert text.splitlines()[0] == "@HD\tVN:1.6\tSO:coordinate\tGO:query" and text.splitlines()[1:] == want[1:]
    assert open(bam, "rb").read()[-28:] == EOF_BLOCK
    assert "sort run 1: 1237 alignment records, 37 of them unplaced" in case["stdout"] and "in 1 run;" in case["stdout"], case["stdout"]


def test_the_index_is_the_sorted_files(case):
    """The members' sizes are the device deflate's, so write_bam cannot write the same file and its .bai names other offsets;
    tests/index_model.py restates write_bam's index for a file as it is cut (held to write_bam's bytes by tests/test_index_model.py),
    and that is what the .bai must be."""
    bam = os.path.join(case["built"], PREP_BAM)
    assert open(bam + ".bai", "rb").read() == im.index_of(bam)


def test_htslib_reads_the_sorted_file_and_its_index(case):
    bam = os.path.join(case["built"], PREP_BAM)
    refs, recs = hts_witness.records(bam)  # (skips where the witness cannot be built)
    assert refs == case["refs"]
    assert [(r["tid"], r["pos"], r["name"], r["flag"]) for r in recs] == [(r["tid"], r["pos"], r["name"], r["flag"]) for r in case["model"]]
    regions = [(0, 0, 20000), (1, 5000, 9000), (2, 19000, 20000)]
    got = hts_witness.query(bam, bam + ".bai", regions)
    for (region, found), (tid, beg, end) in zip(got, regions):
        want = [r["name"] for r in recs if r["tid"] == tid and r["pos"] < end and r["end"] > beg]
        assert [q for _, _, q in found] == want, region


def test_junc_sees_the_same_alignments(case, tmp_path):
    outs = {}
    for name, prep_dir in (("built", case["built"]), ("hand", case["hand"])):
        out = str(tmp_path / name / "pc")
        p = run("junc", "-t", "2", "-o", out, prep_dir)
        assert p.returncode == 0, tail(p)
        outs[name] = open(out + ".junctions.tab", "rb").read()
    assert outs["built"] == outs["hand"]
    assert outs["built"].count(b"\n") > 10


def test_the_golden_unsorted_file(case, tmp_path, golden_dir):
    src, out = os.path.join(golden_dir, "unsorted.bam"), str(tmp_path / "u")
    p = run("prep", "--sort", "-o", out, case["fa"], src)
    assert p.returncode == 0, tail(p)
    assert sorted(os.listdir(out)) == PREPARED
    bam = os.path.join(out, PREP_BAM)
    refs, text, recs = parts_of(bam)
    refs0, text0, recs0 = parts_of(src)
    assert refs == refs0 and b"".join(recs) == b"".join(sorted(recs0, key=raw_key)) and recs != recs0
    lines, lines0 = text.splitlines(), [l for l in text0.splitlines() if l]
    assert lines[0].startswith("@HD") and "SO:coordinate" in lines[0].split("\t")
    assert lines[1:] == (lines0[1:] if lines0 and lines0[0].startswith("@HD") else lines0)
    assert open(bam + ".bai", "rb").read() == im.index_of(bam)
    if hts_witness.available():
        _, seen = hts_witness.records(bam)
        assert [(r["tid"] & 0xFFFFFFFF, r["pos"]) for r in seen] == [raw_key(r) for r in recs]


def test_several_runs(case, tmp_path):
    size = os.path.getsize(case["bam"])
    out = str(tmp_path / "runs")
    p = run("prep", "--sort", "-v", "-t", "2", "-o", out, case["fa"], case["bam"], env_extra={"PORTCULLIS_SORT_RUN_BYTES": str(size // 8)})
    assert p.returncode == 0, tail(p)
    n_runs = int(re.search(r"in (\d+) runs;", p.stdout).group(1))
    assert n_runs >= 3 and f"sort run {n_runs}:" in p.stdout and "Merging %d BAM files" % n_runs in p.stdout, p.stdout
    assert sorted(os.listdir(out)) == PREPARED  # no sortrun*, no temp*
    refs, text, recs = parts_of(os.path.join(out, PREP_BAM))
    one = parts_of(os.path.join(case["built"], PREP_BAM))
    assert (refs, text, b"".join(recs)) == (one[0], one[1], b"".join(one[2]))
    assert open(os.path.join(out, PREP_BAM + ".bai"), "rb").read() == im.index_of(os.path.join(out, PREP_BAM))


def test_a_run_that_fails_half_way_leaves_nothing(case, tmp_path):
    data = open(case["bam"], "rb").read()
    cut = str(tmp_path / "cut.bam")
    open(cut, "wb").write(data[:len(data) * 3 // 4])  # (ends inside a BGZF block)
    out = str(tmp_path / "cut_out")
    # (pieces so small that the index build meets a descent, and the sort closes runs, long before either meets the file's end)
    p = run("prep", "--sort", "-v", "-o", out, case["fa"], cut, env_extra={"PORTCULLIS_SORT_RUN_BYTES": str(len(data) // 8), "PORTCULLIS_PIECE_BYTES": str(len(data) // 8)})
    assert p.returncode == 4 and "Sorting" in p.stdout and "truncated" in p.stderr, tail(p)
    assert not leftovers(out) and not os.path.exists(os.path.join(out, PREP_BAM)) and not os.path.exists(os.path.join(out, PREP_BAM + ".bai"))


def test_sorted_input_is_linked_as_without_the_flag(case, tmp_path):
    outs = []
    for flags in ((), ("--sort",)):
        out = str(tmp_path / ("prep" + "_".join(flags)))
        p = run("prep", *flags, "-o", out, case["fa"], case["pre"])
        assert p.returncode == 0 and "Sorting" not in p.stdout, tail(p)
        assert sorted(os.listdir(out)) == PREPARED and os.path.islink(os.path.join(out, PREP_BAM))
        outs.append({n: (os.path.realpath(os.path.join(out, n)) if os.path.islink(os.path.join(out, n)) else None, open(os.path.join(out, n), "rb").read())
                     for n in PREPARED})
    assert outs[0] == outs[1]


def test_unsorted_input_without_the_flag_is_refused(case, tmp_path):
    out = str(tmp_path / "refused")
    p = run("prep", "-o", out, case["fa"], case["bam"])
    assert p.returncode == 4, tail(p)
    first = next(k for k in range(1, len(case["shuffled"])) if mm.merge_key(case["shuffled"][k]) < mm.merge_key(case["shuffled"][k - 1]))
    assert "not in coordinate order" in p.stderr and "samtools sort" in p.stderr and f"alignment record {first} " in p.stderr and "--sort" in p.stderr
    assert not os.path.exists(os.path.join(out, PREP_BAM + ".bai")) and not leftovers(out)


def test_sort_in_front_of_a_merge(case, tmp_path):
    genome_reads = [r for r in case["model"] if r["tid"] >= 0]
    b_reads = [dict(r, name="b_" + r["name"]) for r in genome_reads[::3]] + [dict(case["model"][-1], name="b_tail")]
    b = str(tmp_path / "b.bam")
    write_bam(b, case["refs"], b_reads, write_index=False)
    out = str(tmp_path / "merged")
    p = run("prep", "--sort", "--merge", "-v", "-o", out, case["fa"], case["bam"], b)
    assert p.returncode == 0, tail(p)
    assert sorted(os.listdir(out)) == PREPARED
    _, _, recs = parts_of(os.path.join(out, PREP_BAM))
    assert b"".join(recs) == mm.record_stream(mm.merge_reads([case["model"], b_reads]))
    # without --sort the unsorted input of a merge is refused as before
    p = run("prep", "--merge", "-o", str(tmp_path / "refused"), case["fa"], case["bam"], b)
    assert p.returncode == 4 and "not in coordinate order" in p.stderr and case["bam"] in p.stderr, tail(p)
    assert not leftovers(str(tmp_path / "refused"))


def test_full_sorts_in_its_prep(case, tmp_path):
    tabs = {}
    for name, flags, bam in (("sorted_here", ("--sort",), case["bam"]), ("presorted", (), case["pre"])):
        y = str(tmp_path / name)
        p = run("full", *flags, "--keep_temp", "--self_train", DATA, "--training_rule", RULES, "-o", y, case["fa"], bam)
        assert p.returncode == 0, tail(p)
        assert sorted(os.listdir(os.path.join(y, "1-prep"))) == PREPARED
        tabs[name] = open(os.path.join(y, "2-junc", "portcullis_all.junctions.tab"), "rb").read()
    assert tabs["sorted_here"] == tabs["presorted"] and tabs["presorted"].count(b"\n") > 10
