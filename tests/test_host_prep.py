"""`portcullis_amd prep` where it needs no device: linking a directory whose inputs carry their indexes, building the .fai,
and every refusal -- each leaves with status 4 and a message that says what to do instead."""
import os
import subprocess

import pytest

from fuzzgen import make_reads
from util_bam import PREP_BAM, PREP_FA, write_bam, write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")


def prep(*args, env_extra=None, no_device=False):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    if no_device:  # (on a GPU box: hide the devices from the HIP runtime)
        env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"
    env.update(env_extra or {})
    return subprocess.run([EXE, "prep", *args], capture_output=True, text=True, timeout=60, env=env)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """Three targets of fuzzgen reads: (dir, refs, contigs, reads)."""
    d = tmp_path_factory.mktemp("prep_in")
    refs, contigs, reads = [], [], []
    for tid in range(3):
        genome, rr = make_reads(40 + tid, n_reads=200, glen=12000 + 1000 * tid)
        for r in rr:
            r["tid"] = tid
        refs.append((f"chr{tid + 1}", len(genome)))
        contigs.append((f"chr{tid + 1}", genome))
        reads += rr
    return d, refs, contigs, reads


def test_with_both_indexes_beside_the_inputs_prep_only_links(inputs, tmp_path):
    _, refs, contigs, reads = inputs
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "genome.fa")
    write_bam(bam, refs, reads)
    write_fasta(fa, contigs)
    out = str(tmp_path / "deep" / "prep")
    # (no device may be opened on this route: with the devices hidden it must still succeed)
    p = prep("-o", out, fa, bam, no_device=True)
    assert p.returncode == 0, p.stdout + p.stderr
    for name, src in ((PREP_BAM, bam), (PREP_BAM + ".bai", bam + ".bai"), (PREP_FA, fa), (PREP_FA + ".fai", fa + ".fai")):
        q = os.path.join(out, name)
        assert os.path.islink(q) and os.path.realpath(q) == os.path.realpath(src), name
    assert "Portcullis prep completed." in p.stdout
    # a second run finds everything and changes nothing
    before = {n: os.lstat(os.path.join(out, n)).st_mtime_ns for n in os.listdir(out)}
    p = prep("-o", out, fa, bam, no_device=True)
    assert p.returncode == 0 and "Pre-indexed BAM detected" in p.stdout and "Prepped genome file detected" in p.stdout
    assert before == {n: os.lstat(os.path.join(out, n)).st_mtime_ns for n in os.listdir(out)}


def test_a_missing_fai_is_built(inputs, tmp_path):
    _, refs, contigs, reads = inputs
    bam, fa, fa2 = str(tmp_path / "in.bam"), str(tmp_path / "genome.fa"), str(tmp_path / "indexed.fa")
    write_bam(bam, refs, reads)
    write_fasta(fa, contigs, write_index=False)
    write_fasta(fa2, contigs)
    out = str(tmp_path / "prep")
    p = prep("-o", out, "--copy", fa, bam, no_device=True)
    assert p.returncode == 0, p.stdout + p.stderr
    fai = os.path.join(out, PREP_FA + ".fai")
    assert not os.path.islink(fai) and open(fai, "rb").read() == open(fa2 + ".fai", "rb").read()
    assert not os.path.exists(fa + ".fai")  # built in the directory, not beside the input
    for name, src in ((PREP_BAM, bam), (PREP_BAM + ".bai", bam + ".bai"), (PREP_FA, fa)):  # --copy: regular files, same bytes
        q = os.path.join(out, name)
        assert not os.path.islink(q) and open(q, "rb").read() == open(src, "rb").read(), name


def refused(p, *texts):
    assert p.returncode == 4, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    for t in texts:
        assert t in p.stderr, (t, p.stderr[-800:])


def test_refusals(inputs, tmp_path):
    _, refs, contigs, reads = inputs
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "genome.fa")
    write_bam(bam, refs, reads, write_index=False)
    write_fasta(fa, contigs)
    out = str(tmp_path / "prep")
    refused(prep("-o", out, fa, bam, bam), "More than one BAM file", "samtools merge")
    refused(prep("-o", out, "--use_csi", fa, bam), "CSI", "samtools index -c")
    # no index beside the BAM and no device to build one
    refused(prep("-o", out, fa, bam, no_device=True), "No MI355X (HIP device) is visible", "no CPU fallback")
    assert not os.path.exists(os.path.join(out, PREP_BAM + ".bai"))
    # a target BAI cannot cover, named by the header: refused before any device is looked for
    big = str(tmp_path / "big.bam")
    write_bam(big, [("huge", 1 << 29)] + refs, [dict(r, tid=r["tid"] + 1) for r in reads], write_index=False)
    refused(prep("-o", str(tmp_path / "prep_big"), fa, big, no_device=True), "BAI cannot index this target: huge", "samtools index -c")
    refused(prep("-o", out, str(tmp_path / "nothing.fa"), bam), "Could not find genome file at")
    refused(prep("-o", out, fa, str(tmp_path / "nothing.bam")), "Could not find BAM file at")
    refused(prep("-o", out, "--frobnicate", fa, bam), "Unknown option: --frobnicate")


def test_help_and_usage():
    p = prep("--help")
    assert p.returncode == 0 and "Usage: portcullis_amd prep [options] <genome-file> <bam-file>" in p.stdout
    for opt in ("--output", "--force", "--copy", "--use_csi", "--threads", "--verbose", "--help"):
        assert opt in p.stdout, opt
    p = prep("only_one_argument")
    assert p.returncode == 1 and "Usage: portcullis_amd prep" in p.stdout
    p = subprocess.run([EXE, "frobnicate"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "portcullis_amd prep [options] <genome-file> <bam-file>" in p.stderr
