"""`portcullis_amd junc --device_mem` (and `full --device_mem`): a run whose group chains do not fit the budget falls back to a chain
per target and writes the same files; a budget that one target alone does not fit ends the run with the device-error status and a
message that names the ways out.

Six equal targets whose index order is not their name order (chr1, chr10, chr11, chr12, chr2, chr3), planned as two groups of
three; one worker, file-piece ingest.  The budgets are worked out from what the unlimited runs report on their [memory] line:
R1 / O1, the records and the rest at the peak of the grouped run; R2, the records of the run with a chain per target."""
import os
import re
import subprocess

import pytest

from fuzzgen import make_reads
from util_bam import make_prep_dir, write_bam, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "portcullis_amd", "host", "portcullis_amd")
DATA = os.path.join(ROOT, "tests", "golden", "selftrain_data")
NAMES = ("chr1", "chr10", "chr11", "chr12", "chr2", "chr3")
GLEN = 12000
GROUP_BASES = 50000  # three members of 12 000 bases + their gaps (3 x 16 128), not four
MEMORY = re.compile(r"^\[memory\] peak held (\d+) \(records (\d+), other (\d+)\); limit (\d+|none); groups flushed early: (\d+); largest target: (\S+) (\d+)$", re.M)
ENV = {"PORTCULLIS_PIECE_BYTES": "4096", "PORTCULLIS_GROUP_BASES": str(GROUP_BASES), "PORTCULLIS_CTX_PER_GPU": "1", "PJB_PRINT_CHAIN_PLAN": "1"}


def run(*args, plan="groups", env_extra=None):
    assert os.path.exists(EXE), f"{EXE} missing: run __graft_entry__.build()"
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PORTCULLIS_", "PJB_"))}
    env.update(ENV, PORTCULLIS_CHAIN_PLAN=plan)
    env.update(env_extra or {})
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300, env=env)


def junc(prep, out, *opts, plan="groups"):
    return run("junc", "-o", out, "--ingest", "device", "-t", "1", "-v", "--devices", "1", *opts, prep, plan=plan)


def tail(p):
    return f"status {p.returncode}\n" + p.stdout[-1500:] + p.stderr[-2500:]


def memory_line(p):
    m = MEMORY.findall(p.stderr)
    assert len(m) == 1, tail(p)
    peak, records, other, limit, flushed, name, big = m[0]
    assert int(peak) == int(records) + int(other)
    return dict(peak=int(peak), records=int(records), other=int(other), limit=None if limit == "none" else int(limit), flushed=int(flushed),
                largest=(name, int(big)))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The input (as a prepared directory, and as the genome and BAM `full` starts from), the unlimited runs and the oracle's files."""
    from oracle import oracle
    from test_gpu_host_cli import oracle_outputs, _plan_from_stderr
    d = tmp_path_factory.mktemp("device_mem")
    refs, contigs, reads = [], [], []
    for tid, name in enumerate(NAMES):
        g, rr = make_reads(900 + tid, n_reads=250, glen=GLEN)
        for r in rr:
            r["tid"] = tid
            if r.get("mtid", -1) >= 0:
                r["mtid"] = tid
        reads += rr
        refs.append((name, len(g)))
        contigs.append((name, g))
    assert len({ln for _, ln in refs}) == 1
    prep = make_prep_dir(str(d / "prep"), refs, contigs, reads, block_size=4096)
    bam, fa = str(d / "in.bam"), str(d / "genome.fa")
    write_bam(bam, refs, reads, block_size=4096, write_index=False)
    write_fasta(fa, contigs, write_index=False)
    # run 1: groups, no budget
    p1 = junc(prep, str(d / "run1" / "pc"))
    assert p1.returncode == 0, tail(p1)
    groups, chains = _plan_from_stderr(p1.stderr)
    assert groups == [[0, 1, 2], [3, 4, 5]] and sorted(chains) == ["group 0,1,2", "group 3,4,5"], (groups, chains)
    m1 = memory_line(p1)
    assert m1["limit"] is None and m1["flushed"] == 0 and m1["largest"][0] in NAMES and m1["largest"][1] > 0, m1
    # run 2: a chain per target, no budget
    p2 = junc(prep, str(d / "run2" / "pc"), plan="targets")
    assert p2.returncode == 0, tail(p2)
    m2 = memory_line(p2)
    exp = oracle_outputs(oracle, prep, "UNKNOWN")
    files = {ext: open(str(d / "run1" / "pc") + ext, "rb").read() for ext in (".junctions.tab", ".junctions.bed")}
    assert files[".junctions.tab"] == exp["tab"] and files[".junctions.bed"] == exp["bed"]
    print(f"run 1: {m1}\nrun 2: {m2}")
    return dict(d=d, prep=prep, fa=fa, bam=bam, files=files, R1=m1["records"], O1=m1["other"], R2=m2["records"])


def budget(case):
    # a condition on the input, not on the code: the groups must hold at least twice the records a chain per target does
    assert case["R1"] >= 2 * case["R2"], case
    return case["O1"] + case["R2"] + (case["R1"] - case["R2"]) // 2


def test_groups_that_do_not_fit_go_target_by_target(case):
    limit = budget(case)
    out = str(case["d"] / "run3" / "pc")
    p = junc(case["prep"], out, "--device_mem", str(limit))
    assert p.returncode == 0, tail(p)
    m = memory_line(p)
    print(f"run 3: {m}")
    assert m["limit"] == limit and m["flushed"] >= 1 and m["peak"] <= limit, m
    assert f" - Device memory: {limit} bytes per GPU\n" in p.stdout
    assert "device memory ran short" in p.stderr and "[chain] target " in p.stderr, tail(p)  # (PJB_PRINT_CHAIN_PLAN: each demotion)
    for ext, blob in case["files"].items():
        assert open(out + ext, "rb").read() == blob, ext


def test_the_environment_sets_the_budget_too(case):
    limit = budget(case)
    out = str(case["d"] / "run3e" / "pc")
    p = run("junc", "-o", out, "--ingest", "device", "-t", "1", "-v", "--devices", "1", case["prep"], env_extra={"PORTCULLIS_DEVICE_MEM": str(limit)})
    assert p.returncode == 0, tail(p)
    assert memory_line(p)["limit"] == limit
    assert open(out + ".junctions.tab", "rb").read() == case["files"][".junctions.tab"]


def test_a_budget_no_target_fits_ends_the_run(case):
    limit = case["O1"] // 2
    out = str(case["d"] / "run4" / "pc")
    p = junc(case["prep"], out, "--device_mem", str(limit))
    assert p.returncode == 4, tail(p)
    err = [ln for ln in p.stderr.splitlines() if ln.startswith("Error: ")]
    assert len(err) == 1, tail(p)
    for text in ("out of device memory: wanted ", f"limit {limit}", "--device_mem", "--devices N"):
        assert text in err[0], err[0]
    assert re.search(r"target chr\d+ does not fit", err[0]), err[0]
    assert not os.path.exists(out + ".junctions.tab")


def test_full_forwards_the_budget(case):
    limit = budget(case)
    out = str(case["d"] / "full")
    p = run("full", "-o", out, "-t", "1", "-v", "--devices", "1", "--device_mem", str(limit), "--self_train", DATA, case["fa"], case["bam"])
    # (197 junctions, fewer than the 200 self-training wants: filt takes the lenient rule file, as in tests/test_gpu_full_cli.py, and the run ends well)
    assert p.returncode == 0 and "Portcullis completed." in p.stdout, tail(p)
    m = memory_line(p)
    assert m["limit"] == limit and m["flushed"] >= 1 and m["peak"] <= limit, m
    assert open(os.path.join(out, "2-junc", "portcullis_all.junctions.tab"), "rb").read() == case["files"][".junctions.tab"]
