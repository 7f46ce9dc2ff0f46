"""`portcullis_amd prep --merge` and `full --merge` where they need no device: the flag in both help texts, the refusals that the
inputs' headers decide (status 4, before a device is opened), one BAM with the flag being plain prep, and what is left behind when
there is no device to merge on."""
import os
import subprocess

import pytest

from fuzzgen import make_reads
from util_bam import PREP_BAM, PREP_FA, write_bam, write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
DATA = os.path.join(ROOT, "tests", "golden", "selftrain_data")


def run(mode, *args, no_device=True):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    if no_device:  # (on a GPU box: hide the devices from the HIP runtime)
        env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"
    return subprocess.run([EXE, mode, *args], capture_output=True, text=True, timeout=60, env=env)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Two targets of fuzzgen reads split over two files, and their genome: (dir, refs, fa, [reads of a, reads of b])."""
    d = tmp_path_factory.mktemp("merge_in")
    refs, contigs, reads = [], [], []
    for tid in range(2):
        genome, rr = make_reads(50 + tid, n_reads=150, glen=9000 + 1000 * tid)
        for k, r in enumerate(rr):
            r["tid"] = tid
            r["name"] = f"t{tid}r{k}"
        refs.append((f"chr{tid + 1}", len(genome)))
        contigs.append((f"chr{tid + 1}", genome))
        reads += rr
    fa = str(d / "genome.fa")
    write_fasta(fa, contigs)
    return d, refs, fa, [reads[0::2], reads[1::2]]


def header(refs, extra=""):
    return "@HD\tVN:1.4\tSO:coordinate\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in refs) + extra


def refused(p, *words):
    assert p.returncode == 4, (p.returncode, p.stdout, p.stderr)
    for w in words:
        assert w in p.stdout + p.stderr, (w, p.stdout, p.stderr)


def leftovers(out):
    return sorted(n for n in (os.listdir(out) if os.path.isdir(out) else []) if n.startswith("temp") or n.endswith(".tmp"))


def test_merge_is_in_both_help_texts():
    for mode in ("prep", "full"):
        p = run(mode, "--help")
        assert p.returncode == (0 if mode == "prep" else 1) and "--merge" in p.stdout, mode  # (full --help leaves with 1, as the reference's does)
    assert "Usage: portcullis_amd prep [options] <genome-file> <bam-file>" in run("prep", "--help").stdout  # (the usage line stays)


def test_mismatched_dictionaries_are_refused(inputs, tmp_path):
    _, refs, fa, (ra, rb) = inputs
    a, b, out = str(tmp_path / "a.bam"), str(tmp_path / "b.bam"), str(tmp_path / "prep")
    write_bam(a, refs, ra)
    other = [refs[0], (refs[1][0], refs[1][1] + 7)]
    write_bam(b, other, rb)
    refused(run("prep", "--merge", "-o", out, fa, a, b), "reference dictionary", b, "target 1", refs[1][0])
    assert not os.path.exists(os.path.join(out, PREP_BAM)) and not leftovers(out)
    write_bam(b, [refs[0], ("chrOther", refs[1][1])], rb)
    refused(run("prep", "--merge", "-o", out, fa, a, b), "target 1 is chrOther")
    write_bam(b, refs + [("chr9", 500)], rb)
    refused(run("prep", "--merge", "-o", out, fa, a, b), "3 targets", "chr9")


def test_read_group_collision_is_refused(inputs, tmp_path):
    _, refs, fa, (ra, rb) = inputs
    a, b, out = str(tmp_path / "a.bam"), str(tmp_path / "b.bam"), str(tmp_path / "prep")
    write_bam(a, refs, ra, header_text=header(refs, "@RG\tID:lane1\tSM:liver\n"))
    write_bam(b, refs, rb, header_text=header(refs, "@RG\tID:lane1\tSM:brain\n"))
    refused(run("prep", "--merge", "-o", out, fa, a, b), "@RG", "ID lane1")
    assert not os.path.exists(os.path.join(out, PREP_BAM)) and not leftovers(out)


def test_one_bam_with_the_flag_is_plain_prep(inputs, tmp_path):
    _, refs, fa, (ra, _) = inputs
    bam = str(tmp_path / "one.bam")
    write_bam(bam, refs, ra)  # (its index beside it: no device on this route)
    outs = []
    for flags in ((), ("--merge",)):
        out = str(tmp_path / ("prep" + "_".join(flags)))
        p = run("prep", *flags, "-o", out, fa, bam)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append({n: os.path.realpath(os.path.join(out, n)) for n in sorted(os.listdir(out)) if os.path.islink(os.path.join(out, n))})
        assert sorted(os.listdir(out)) == sorted([PREP_BAM, PREP_BAM + ".bai", PREP_FA, PREP_FA + ".fai"])
    assert outs[0] == outs[1] and len(outs[0]) == 4


def test_without_a_device_nothing_is_left_behind(inputs, tmp_path):
    _, refs, fa, (ra, rb) = inputs
    a, b, out = str(tmp_path / "a.bam"), str(tmp_path / "b.bam"), str(tmp_path / "prep")
    write_bam(a, refs, ra)
    write_bam(b, refs, rb, write_index=False)
    p = run("prep", "--merge", "-o", out, fa, a, b)
    refused(p, "No MI355X", "no CPU fallback")
    assert not leftovers(out) and not os.path.exists(os.path.join(out, PREP_BAM))
    # several files without the flag: today's refusal, from prep and from full
    refused(run("prep", "-o", out, fa, a, b), "More than one BAM file", "samtools merge")


def test_full_passes_the_flag_to_its_prep(inputs, tmp_path):
    _, refs, fa, (ra, rb) = inputs
    a, b, out = str(tmp_path / "a.bam"), str(tmp_path / "b.bam"), str(tmp_path / "full")
    write_bam(a, refs, ra)
    write_bam(b, refs, rb)
    refused(run("full", "--self_train", DATA, "-o", out, fa, a, b), "More than one BAM file", "samtools merge")
    # with the flag its prep goes on to the merge, which is what needs the device
    p = run("full", "--merge", "--self_train", DATA, "-o", out, fa, a, b)
    refused(p, "No MI355X", "merged on the GPU", "no CPU fallback")
    assert os.listdir(out) == ["1-prep"] and not leftovers(os.path.join(out, "1-prep"))
