"""`--build_csi` where it needs no device: the depth rule of pjb_csi_depth, the help texts, the refusal without a device, and
linking a `.csi` that lies beside the input."""
import os
import subprocess

import csi_model as cm
from portcullis_amd import ffi
from test_host_prep import EXE, inputs, prep, refused  # noqa: F401  (inputs: a fixture)
from util_bam import PREP_BAM, PREP_FA, write_bam, write_fasta


def test_the_depth_is_the_one_htslib_chooses():
    for lens, want in (([16_128], 0), ([16_129], 1), ([2**29 - 256], 5), ([2**29 - 255], 6), ([2**31 - 1], 6), ([1_300_000, 5_000, 70_000, 40], 3),
                       ([248_956_422, 16_569], 5), ([1_000_000], 2), ([], 0), ([0], 0)):
        assert ffi.csi_depth(lens) == want == cm.depth_for(lens), lens
    for n in range(0, 19):  # every edge of the rule: 2^(14 + 3 n) - 256 is the last length of depth n
        s = 1 << (14 + 3 * n)
        if s - 255 < 2**31:
            assert (ffi.csi_depth([s - 256]), ffi.csi_depth([s - 255])) == (n, n + 1)


def test_the_help_texts_name_the_flag():
    p = prep("--help")
    assert p.returncode == 0 and "--build_csi" in p.stdout and "-C" in p.stdout and "--use_csi" in p.stdout
    p = subprocess.run([EXE, "full", "--help"], capture_output=True, text=True, timeout=60)
    assert "--build_csi" in p.stdout and "CSI output" not in p.stdout
    p = subprocess.run([EXE, "bamfilt", "--help"], capture_output=True, text=True, timeout=60)
    assert "--use_csi" in p.stdout and ".csi is written" in p.stdout


def test_without_a_device_no_csi_is_built(inputs, tmp_path):
    _, refs, contigs, reads = inputs
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "genome.fa")
    write_bam(bam, refs, reads)  # (a .bai beside it does not help: --build_csi wants a .csi)
    write_fasta(fa, contigs)
    out = str(tmp_path / "prep")
    for flags in (("--build_csi",), ("-C",), ("--use_csi", "--build_csi")):
        refused(prep("-o", out, *flags, fa, bam, no_device=True), "No MI355X (HIP device) is visible", "no CPU fallback")
        assert not os.path.exists(os.path.join(out, PREP_BAM + ".csi")) and not os.path.exists(os.path.join(out, PREP_BAM + ".bai"))
    # the long target's refusal names the way out, and --build_csi gets past the header to the device it lacks
    big = str(tmp_path / "big.bam")
    write_bam(big, [("huge", 1 << 29)] + refs, [dict(r, tid=r["tid"] + 1) for r in reads], write_index=False)
    refused(prep("-o", str(tmp_path / "prep_big"), fa, big, no_device=True), "BAI cannot index this target: huge", "samtools index -c", "--build_csi")
    refused(prep("-o", str(tmp_path / "prep_big"), "--build_csi", fa, big, no_device=True), "No MI355X (HIP device) is visible")
    refused(prep("-o", out, "--use_csi", fa, bam, no_device=True), "CSI", "samtools index -c", "--build_csi")


def test_a_csi_beside_the_input_is_linked(inputs, tmp_path):
    _, refs, contigs, reads = inputs
    bam, fa = str(tmp_path / "in.bam"), str(tmp_path / "genome.fa")
    write_bam(bam, refs, reads, write_index=False)
    open(bam + ".csi", "wb").write(cm.container(cm.payload_of(bam)))
    write_fasta(fa, contigs)
    out = str(tmp_path / "prep")
    p = prep("-o", out, "--build_csi", fa, bam, no_device=True)
    assert p.returncode == 0, p.stdout + p.stderr
    for name, src in ((PREP_BAM, bam), (PREP_BAM + ".csi", bam + ".csi"), (PREP_FA, fa), (PREP_FA + ".fai", fa + ".fai")):
        q = os.path.join(out, name)
        assert os.path.islink(q) and os.path.realpath(q) == os.path.realpath(src), name
    assert not os.path.lexists(os.path.join(out, PREP_BAM + ".bai"))
    # --copy: the same bytes as regular files; a second run changes nothing
    out2 = str(tmp_path / "prep2")
    p = prep("-o", out2, "--copy", "-C", fa, bam, no_device=True)
    assert p.returncode == 0, p.stdout + p.stderr
    q = os.path.join(out2, PREP_BAM + ".csi")
    assert not os.path.islink(q) and open(q, "rb").read() == open(bam + ".csi", "rb").read()
    p = prep("-o", out2, "--copy", "-C", fa, bam, no_device=True)
    assert p.returncode == 0 and "Pre-indexed BAM detected" in p.stdout
