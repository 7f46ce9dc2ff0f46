"""`portcullis_amd prep --sort` and `full --sort` where they need no device: the flag is parsed and in both help texts, the refusals
that need no device keep their status 4 and leave nothing behind, and a sorted file with its index beside it is plain prep."""
import os
import subprocess

import pytest

from fuzzgen import make_reads
from util_bam import PREP_BAM, PREP_FA, write_bam, write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
DATA = os.path.join(ROOT, "tests", "golden", "selftrain_data")


def run(mode, *args):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"  # (on a GPU box: hide the devices from the HIP runtime)
    return subprocess.run([EXE, mode, *args], capture_output=True, text=True, timeout=60, env=env)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("sort_in")
    genome, reads = make_reads(61, n_reads=120, glen=9000)
    for k, r in enumerate(reads):
        r["tid"] = 0
        r["name"] = f"r{k}"
    refs = [("chr1", len(genome))]
    fa = str(d / "genome.fa")
    write_fasta(fa, [("chr1", genome)])
    return d, refs, fa, reads


def refused(p, *words):
    assert p.returncode == 4, (p.returncode, p.stdout, p.stderr)
    for w in words:
        assert w in p.stdout + p.stderr, (w, p.stdout, p.stderr)


def leftovers(out):
    return sorted(n for n in (os.listdir(out) if os.path.isdir(out) else []) if n.startswith(("temp", "sortrun")) or n.endswith(".tmp"))


def test_sort_is_in_both_help_texts():
    for mode in ("prep", "full"):
        p = run(mode, "--help")
        assert p.returncode == (0 if mode == "prep" else 1), mode  # (full --help leaves with 1, as the reference's does)
        assert "--sort" in p.stdout and "--merge" in p.stdout and "sorted on the GPU" in p.stdout, mode
    assert "Usage: portcullis_amd prep [options] <genome-file> <bam-file>" in run("prep", "--help").stdout  # (the usage line stays)


def test_the_flag_is_an_option_and_nothing_else_is(inputs, tmp_path):
    _, refs, fa, reads = inputs
    bam = str(tmp_path / "one.bam")
    write_bam(bam, refs, reads)
    p = run("prep", "--sorted", "-o", str(tmp_path / "x"), fa, bam)
    assert p.returncode != 0 and "Unknown option: --sorted" in p.stdout + p.stderr
    p = run("prep", "--sort", "-o", str(tmp_path / "y"), fa, bam)  # (not taken for a file name: two positionals are left)
    assert p.returncode == 0, p.stdout + p.stderr


def test_sorted_input_with_its_index_is_plain_prep(inputs, tmp_path):
    _, refs, fa, reads = inputs
    bam = str(tmp_path / "one.bam")
    write_bam(bam, refs, reads)  # (its index beside it: no device on this route, with or without the flag)
    outs = []
    for flags in ((), ("--sort",), ("--sort", "--merge")):
        out = str(tmp_path / ("prep" + "_".join(flags)))
        p = run("prep", *flags, "-o", out, fa, bam)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append({n: os.path.realpath(os.path.join(out, n)) for n in sorted(os.listdir(out)) if os.path.islink(os.path.join(out, n))})
        assert sorted(os.listdir(out)) == sorted([PREP_BAM, PREP_BAM + ".bai", PREP_FA, PREP_FA + ".fai"])
    assert outs[0] == outs[1] == outs[2] and len(outs[0]) == 4


def test_refusals_that_need_no_device(inputs, tmp_path):
    _, refs, fa, reads = inputs
    bam, out = str(tmp_path / "one.bam"), str(tmp_path / "prep")
    write_bam(bam, refs, reads)
    refused(run("prep", "--sort", "--use_csi", "-o", out, fa, bam), "CSI", "not built into portcullis_amd prep")
    refused(run("prep", "--sort", "-o", out, fa, str(tmp_path / "missing.bam")), "Could not find BAM file at")
    refused(run("full", "--sort", "--use_csi", "--self_train", DATA, "-o", str(tmp_path / "full"), fa, bam), "CSI")
    assert not leftovers(out) and not os.path.exists(os.path.join(out, PREP_BAM))
    # several files still need --merge, with or without --sort
    refused(run("prep", "--sort", "-o", out, fa, bam, bam), "More than one BAM file", "samtools merge")


def test_without_a_device_the_refusal_is_loud(inputs, tmp_path):
    """An input without an index beside it needs the device before anyone knows whether it is sorted."""
    _, refs, fa, reads = inputs
    bam, out = str(tmp_path / "shuffled.bam"), str(tmp_path / "prep")
    write_bam(bam, refs, reads[::-1], write_index=False)
    for mode, tail_args in (("prep", ()), ("full", ("--self_train", DATA))):
        p = run(mode, "--sort", *tail_args, "-o", out + mode, fa, bam)
        refused(p, "No MI355X", "no CPU fallback")
        assert not leftovers(out + mode) and not leftovers(os.path.join(out + mode, "1-prep"))
