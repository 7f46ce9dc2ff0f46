"""`--build_csi` through the programs: prep builds `<sorted>.csi` on the device (alone, behind --sort and --merge, inside full), junc
and bamfilt read it, bamfilt writes one of its own, and a file with a target past 2^30 is served.  Every index is compared, as inflated
payload, with tests/csi_model.py; the BGZF container the device's DEFLATE makes is checked on its own."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import csi_model as cm
import index_model as im
from fuzzgen import make_reads
from util_bam import PREP_BAM, PREP_FA, write_bam, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
DATA = os.path.join(ROOT, "tests", "golden", "selftrain_data")


def run(*args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PORTCULLIS_")}
    env.update(env_extra or {})
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=env)


def ok(p):
    assert p.returncode == 0, f"status {p.returncode}\n" + p.stdout[-1500:] + p.stderr[-1500:]
    return p


def bytes_of(*parts):
    return open(os.path.join(*parts), "rb").read()


def assert_csi_of(bam, csi=None):
    """The .csi beside `bam` (or at `csi`) is a sound container whose payload is the model's for that file."""
    payload = cm.check_container(bytes_of(csi or bam + ".csi"))
    assert payload == cm.payload_of(bam)
    return payload


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The input of test_gpu_prep_cli.py, prepared with a BAI and with a CSI."""
    d = tmp_path_factory.mktemp("prep_csi_cli")
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
    bai, csi = str(d / "bai"), str(d / "csi")
    ok(run("prep", "-o", bai, fa, bam))
    ok(run("prep", "--build_csi", "-v", "-o", csi, fa, bam))
    return dict(d=d, refs=refs, contigs=contigs, reads=reads, bam=bam, fa=fa, bai=bai, csi=csi)


def test_prep_leaves_a_csi_and_no_bai(case, tmp_path):
    built = case["csi"]
    assert sorted(os.listdir(built)) == sorted([PREP_BAM, PREP_BAM + ".csi", PREP_FA, PREP_FA + ".fai"])
    payload = assert_csi_of(os.path.join(built, PREP_BAM))
    assert cm.parse(payload)[1] == 1  # (targets of ~20 kb)
    # -C, --use_csi --build_csi and tiny pieces give the same file
    for k, (flags, env) in enumerate(((("-C",), None), (("--use_csi", "--build_csi"), None), (("--build_csi",), {"PORTCULLIS_PIECE_BYTES": "4096"}))):
        out = str(tmp_path / f"again{k}")
        ok(run("prep", *flags, "-o", out, case["fa"], case["bam"], env_extra=env))
        assert cm.check_container(bytes_of(out, PREP_BAM + ".csi")) == payload and not os.path.lexists(os.path.join(out, PREP_BAM + ".bai"))
    # junc reads it, and finds what it finds through the BAI
    outs = {}
    for name, opts, prep_dir in (("csi", ("-c",), built), ("bai", (), case["bai"])):
        out = str(tmp_path / name / "pc")
        ok(run("junc", "-t", "2", *opts, "-o", out, prep_dir))
        outs[name] = (bytes_of(out + ".junctions.tab"), bytes_of(out + ".junctions.bed"))
    assert outs["csi"] == outs["bai"] and outs["csi"][0].count(b"\n") > 10


def test_a_header_with_a_long_target(case, tmp_path):
    """test_host_prep's big.bam: a target of 2^29 bases in the header, the reads on the others."""
    big = str(tmp_path / "big.bam")
    write_bam(big, [("huge", 1 << 29)] + case["refs"], [dict(r, tid=r["tid"] + 1) for r in case["reads"]], write_index=False)
    p = run("prep", "-o", str(tmp_path / "refused"), case["fa"], big)
    assert p.returncode == 4 and "BAI cannot index this target: huge" in p.stderr and "--build_csi" in p.stderr
    out = str(tmp_path / "prep_big")
    ok(run("prep", "--build_csi", "-o", out, case["fa"], big))
    assert cm.parse(assert_csi_of(os.path.join(out, PREP_BAM)))[1] == 6
    ok(run("junc", "-c", "-t", "2", "-o", str(tmp_path / "j" / "pc"), out))
    assert bytes_of(str(tmp_path / "j" / "pc") + ".junctions.tab").count(b"\n") > 10


def test_behind_sort_and_merge(case, tmp_path):
    rng = np.random.default_rng(17)
    reads = case["reads"]
    shuffled = str(tmp_path / "shuffled.bam")
    write_bam(shuffled, case["refs"], [reads[k] for k in rng.permutation(len(reads))], write_index=False)
    halves = [str(tmp_path / f"half{k}.bam") for k in (0, 1)]
    for k, h in enumerate(halves):
        write_bam(h, case["refs"], reads[k::2], write_index=False)
    for name, flags, bams in (("sort", ("--sort",), [shuffled]), ("merge", ("--merge",), halves), ("both", ("--sort", "--merge"), [shuffled, halves[0]])):
        a, b = str(tmp_path / (name + "_bai")), str(tmp_path / (name + "_csi"))
        ok(run("prep", *flags, "-o", a, case["fa"], *bams))
        ok(run("prep", *flags, "--build_csi", "-o", b, case["fa"], *bams))
        assert sorted(os.listdir(b)) == sorted([PREP_BAM, PREP_BAM + ".csi", PREP_FA, PREP_FA + ".fai"]), name  # (no temporary index is left)
        assert bytes_of(a, PREP_BAM) == bytes_of(b, PREP_BAM), name
        assert_csi_of(os.path.join(b, PREP_BAM))


def test_full_and_bamfilt(tmp_path):
    """`full --build_csi` gives the junction and filter files of `full`; its bamfilt and a bamfilt --use_csi of its own write the
    .csi of the filtered file beside the .bai they write anyway, and htslib answers with either alike."""
    from test_gpu_full_cli import make_input, tree
    from test_oracle_htslib_witness import regions_for

    fa, bam = make_input(tmp_path, 90, 3, 400, 12, 20000)
    x, y = str(tmp_path / "bai"), str(tmp_path / "csi")
    common = ("-b", "--keep_temp", "--self_train", DATA, "--training_rule", "balanced")
    ok(run("full", *common, "-o", x, fa, bam))
    ok(run("full", *common, "--build_csi", "-o", y, fa, bam))
    for under in ("2-junc", "3-filt"):
        want, got = tree(x, under), tree(y, under)
        assert sorted(got) == sorted(want) and len(want) >= 2
        for k in want:
            assert got[k] == want[k], k
    assert os.path.exists(os.path.join(y, "1-prep", PREP_BAM + ".csi")) and not os.path.lexists(os.path.join(y, "1-prep", PREP_BAM + ".bai"))
    filtered = os.path.join(y, "portcullis.filtered.bam")
    assert bytes_of(filtered) == bytes_of(x, "portcullis.filtered.bam") and bytes_of(filtered + ".bai") == bytes_of(x, "portcullis.filtered.bam.bai")
    assert not os.path.exists(os.path.join(x, "portcullis.filtered.bam.csi"))
    assert_csi_of(filtered)
    # bamfilt --use_csi by itself, on the directory full left
    own = str(tmp_path / "own.bam")
    ok(run("bamfilt", "--use_csi", "-o", own, os.path.join(y, "3-filt", "portcullis_filtered.pass.junctions.tab"), os.path.join(y, "1-prep", PREP_BAM)))
    assert bytes_of(own) == bytes_of(filtered) and bytes_of(own + ".bai") == bytes_of(filtered + ".bai")
    assert_csi_of(own)
    refs = [(name, n) for name, n in zip(("chr1", "chr2", "chr3"), cm.ref_lens_of(gzip.open(own, "rb").read()))]
    regions = regions_for(refs, 40)
    with_bai = cm.witness_query(own, own + ".bai", regions)
    assert cm.witness_query(own, own + ".csi", regions) == with_bai
    assert sum(len(h) for _, h in with_bai) > 100


def test_a_target_past_2_to_the_30(case, tmp_path):
    """The long input of csi_model through prep: the file the device wrote serves htslib and BamReader::regionSpan."""
    from test_host_region import parse

    long_bam = str(tmp_path / "long.bam")
    cm.write_bam_long(long_bam, cm.LONG_REFS, cm.long_reads(), block_size=cm.LONG_BLOCK)
    out = str(tmp_path / "prep_long")
    ok(run("prep", "--build_csi", "--copy", "-o", out, case["fa"], long_bam, env_extra={"PORTCULLIS_PIECE_BYTES": "20000"}))
    bam = os.path.join(out, PREP_BAM)
    assert cm.parse(assert_csi_of(bam))[1] == 6
    recs = im.build(bam)[3]
    regions = cm.long_regions()[::6] + cm.long_regions()[-6:]
    for (reg, hits), want in zip(cm.witness_query(bam, bam + ".csi", regions), cm.brute_force(recs, regions)):
        assert [(p, e) for p, e, _ in hits] == want, reg
    # regionSpan with that index: each target's span starts at its first record and covers its last
    host, csrc = os.path.join(ROOT, "portcullis_amd", "host"), os.path.join(ROOT, "portcullis_amd", "csrc")
    exe = str(tmp_path / "region_span")
    subprocess.check_call(["g++", "-O1", "-std=c++17", f"-I{host}/include", f"-I{ROOT}/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "region_span.cc"),
                           f"-L{host}", "-lportcullis_host", f"-L{csrc}", "-lportcullis_amd", f"-Wl,-rpath,{host}", f"-Wl,-rpath,{csrc}"])
    raw, blocks, ustart, first, last, n_ref = parse(bam)
    p = subprocess.run([exe, bam, "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().split("\n")
    assert len(lines) == n_ref == 2
    for line in lines:
        f = line.split()
        tid, off, n, first_u, same = int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[5])
        b0 = int(np.searchsorted(ustart, first[tid], side="right") - 1)
        assert off == blocks[b0][0] and first_u == first[tid] - int(ustart[b0]) and same == 1
        b_last = int(np.searchsorted(ustart, last[tid] - 1, side="right") - 1)
        assert off + n >= blocks[b_last][0] + blocks[b_last][1]
