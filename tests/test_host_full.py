"""`portcullis_amd full` where it needs no device: its help, and every refusal -- each leaves with status 4 and the message of the stage
that owns it, before anything beyond prep's own directory is made."""
import os
import subprocess

import pytest

from fuzzgen import make_reads
from util_bam import PREP_BAM, PREP_FA, write_bam, write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
DATA = os.path.join(ROOT, "tests", "golden", "selftrain_data")

OPTIONS = ("--threads", "--verbose", "--help", "--output", "--bam_filter", "--exon_gff", "--intron_gff", "--source", "--force", "--copy", "--keep_temp",
           "--use_csi", "--orientation", "--strandedness", "--separate", "--extra", "--reference", "--max_length", "--canonical", "--min_cov", "--save_bad",
           "--training_rule", "--self_train", "--devices")


def full(*args, no_device=False):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    if no_device:  # (on a GPU box: hide the devices from the HIP runtime)
        env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = "-1"
    return subprocess.run([EXE, "full", *args], capture_output=True, text=True, timeout=60, env=env)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """A genome with its index, a coordinate-sorted BAM without one: (genome, bam)."""
    d = tmp_path_factory.mktemp("full_in")
    refs, contigs, reads = [], [], []
    for tid in range(2):
        genome, rr = make_reads(60 + tid, n_reads=150, glen=9000 + 1000 * tid)
        for r in rr:
            r["tid"] = tid
        refs.append((f"chr{tid + 1}", len(genome)))
        contigs.append((f"chr{tid + 1}", genome))
        reads += rr
    bam, fa = str(d / "in.bam"), str(d / "genome.fa")
    write_bam(bam, refs, reads, write_index=False)
    write_fasta(fa, contigs)
    return fa, bam


def test_help_and_usage():
    for args in (("--help",), ()):
        p = full(*args)
        assert p.returncode == 1, (args, p.returncode, p.stderr[-300:])
        assert "Portcullis Full Pipeline Mode Help" in p.stdout and "Usage: portcullis_amd full [options]" in p.stdout
        assert "<genome-file> <bam-file>" in p.stdout
        for opt in OPTIONS:
            assert opt in p.stdout, opt
        for short in ("-t [", "-v [", "-o [", "-b [", "-r ["):
            assert short in p.stdout, short
        for hidden in ("--save_features", "--save_layers"):  # hidden, as in the reference
            assert hidden not in p.stdout, hidden
    p = subprocess.run([EXE, "frobnicate"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "portcullis_amd full [options]" in p.stderr
    for line in ("portcullis_amd junc [options] <prep_data_dir>", "portcullis_amd prep [options] <genome-file> <bam-file>"):  # the others stay
        assert line in p.stderr


def refused(p, *texts):
    assert p.returncode == 4, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    for t in texts:
        assert t in p.stderr, (t, p.stderr[-800:])


def test_refused_before_any_file_is_touched(inputs, tmp_path):
    fa, bam = inputs
    out = str(tmp_path / "out")
    refused(full("-o", out, fa, bam), "--self_train")
    refused(full("-o", out, "--self_train", str(tmp_path / "no_such_data"), fa, bam), "Could not find the self-training data directory at")
    refused(full("-o", out, "--self_train", DATA, "--training_rule", "no_such_rules", fa, bam), "Could not find suitable directory containing training rules")
    empty = tmp_path / "data" / "hollow"
    empty.mkdir(parents=True)
    refused(full("-o", out, "--self_train", str(tmp_path / "data"), "--training_rule", "hollow", fa, bam), "Not enough positive and negative layers found in hollow")
    refused(full("-o", out, "--self_train", DATA, str(tmp_path / "nothing.fa"), bam), "Could not find genome file at")
    refused(full("-o", out, "--self_train", DATA, "--frobnicate", fa, bam), "Unknown option: --frobnicate")
    assert not os.path.exists(out)


def test_what_prep_refuses_is_refused_with_its_message(inputs, tmp_path):
    fa, bam = inputs
    for k, (args, texts) in enumerate(((("--self_train", DATA, fa, str(tmp_path / "nothing.bam")), ("Could not find BAM file at",)),
                                       (("--self_train", DATA, fa, bam, bam), ("More than one BAM file", "samtools merge")),
                                       (("--self_train", DATA, "--use_csi", fa, bam), ("CSI", "samtools index -c")))):
        out = str(tmp_path / f"out{k}")
        refused(full("-o", out, *args), *texts)
        assert os.listdir(out) == ["1-prep"] and os.listdir(os.path.join(out, "1-prep")) == [], args


def test_without_a_device_the_index_cannot_be_built_and_junc_is_not_started(inputs, tmp_path):
    fa, bam = inputs
    out = str(tmp_path / "out")
    p = full("-o", out, "--self_train", DATA, fa, bam, no_device=True)
    refused(p, "No MI355X (HIP device) is visible", "no CPU fallback")
    assert "Running full portcullis pipeline" in p.stdout and "Preparing input data (BAMs + genome)\n------------------------------------" in p.stdout
    assert os.listdir(out) == ["1-prep"]  # no 2-junc
    # what prep itself leaves at this point: the links, no index
    assert sorted(os.listdir(os.path.join(out, "1-prep"))) == sorted([PREP_BAM, PREP_FA, PREP_FA + ".fai"])
