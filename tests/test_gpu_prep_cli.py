"""`portcullis_amd prep` builds the BAM index on the device: the directory it makes behaves like a hand-made one."""
import os
import subprocess

import pytest

from fuzzgen import make_reads
from util_bam import PREP_BAM, PREP_FA, make_prep_dir, write_bam, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")


def run(*args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PORTCULLIS_")}
    env.update(env_extra or {})
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=env)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("prep_cli")
    refs, contigs, reads = [], [], []
    for tid in range(3):
        genome, rr = make_reads(90 + tid, n_reads=400, glen=20000 + 1500 * tid)
        for r in rr:
            r["tid"] = tid
        refs.append((f"chr{tid + 1}", len(genome)))
        contigs.append((f"chr{tid + 1}", genome))
        reads += rr
    bam, fa = str(d / "in.bam"), str(d / "genome.fa")
    write_bam(bam, refs, reads, write_index=False)
    write_fasta(fa, contigs, write_index=False)
    hand = make_prep_dir(str(d / "hand"), refs, contigs, reads)  # (write_bam / write_fasta with their indexes)
    built = str(d / "built")
    p = run("prep", "-o", built, fa, bam)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    return dict(d=d, bam=bam, fa=fa, hand=hand, built=built)


def bytes_of(*parts):
    return open(os.path.join(*parts), "rb").read()


def test_a_built_directory_behaves_like_a_hand_made_one(case, tmp_path):
    built, hand = case["built"], case["hand"]
    assert sorted(os.listdir(built)) == sorted([PREP_BAM, PREP_BAM + ".bai", PREP_FA, PREP_FA + ".fai"])  # what PreparedFiles::valid asks for
    assert os.path.islink(os.path.join(built, PREP_BAM)) and os.path.islink(os.path.join(built, PREP_FA))
    assert bytes_of(built, PREP_BAM + ".bai") == bytes_of(hand, PREP_BAM + ".bai")
    assert bytes_of(built, PREP_FA + ".fai") == bytes_of(hand, PREP_FA + ".fai")
    outs = {}
    for name, prep_dir in (("built", built), ("hand", hand)):
        out = str(tmp_path / name / "pc")
        p = run("junc", "-t", "2", "-o", out, prep_dir)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
        outs[name] = (open(out + ".junctions.tab", "rb").read(), open(out + ".junctions.bed", "rb").read())
    assert outs["built"] == outs["hand"]
    assert outs["built"][0].count(b"\n") > 10


def test_the_other_routes(case, tmp_path):
    want = bytes_of(case["hand"], PREP_BAM + ".bai")
    # --copy: regular files with the same bytes
    out = str(tmp_path / "copied")
    p = run("prep", "-o", out, "--copy", case["fa"], case["bam"])
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    for name, src in ((PREP_BAM, case["bam"]), (PREP_FA, case["fa"])):
        assert not os.path.islink(os.path.join(out, name)) and bytes_of(out, name) == bytes_of(src)
    assert bytes_of(out, PREP_BAM + ".bai") == want
    # a second run changes nothing
    before = {n: os.lstat(os.path.join(out, n)).st_mtime_ns for n in os.listdir(out)}
    p = run("prep", "-o", out, "--copy", case["fa"], case["bam"])
    assert p.returncode == 0 and "Pre-indexed BAM detected" in p.stdout
    assert before == {n: os.lstat(os.path.join(out, n)).st_mtime_ns for n in os.listdir(out)}
    # --force rebuilds
    p = run("prep", "-o", out, "--force", case["fa"], case["bam"])
    assert p.returncode == 0 and "Indexing" in p.stdout, p.stdout[-1500:] + p.stderr[-1500:]
    assert os.path.islink(os.path.join(out, PREP_BAM)) and bytes_of(out, PREP_BAM + ".bai") == want
    assert all(os.lstat(os.path.join(out, n)).st_mtime_ns > before[n] for n in before)
    # tiny pieces: blocks and records straddle nearly every one
    out = str(tmp_path / "pieces")
    p = run("prep", "-o", out, case["fa"], case["bam"], env_extra={"PORTCULLIS_PIECE_BYTES": "4096"})
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-1500:]
    assert bytes_of(out, PREP_BAM + ".bai") == want


def test_an_unsorted_file_is_refused(case, tmp_path, golden_dir):
    p = run("prep", "-o", str(tmp_path / "u"), case["fa"], os.path.join(golden_dir, "unsorted.bam"))
    assert p.returncode == 4, p.stdout[-800:] + p.stderr[-800:]
    assert "not in coordinate order" in p.stderr and "samtools sort" in p.stderr and "alignment record 1 " in p.stderr
