"""`portcullis_amd junc --extra` with the chain plan of pjb_plan_groups (PORTCULLIS_CHAIN_PLAN=groups): the chains the program queues
are the planner's groups, and the files equal the oracle's and those of the target-by-target plan byte for byte."""
import numpy as np
import pytest

from fuzzgen import make_reads
from test_gpu_host_cli import _plan_from_stderr, check
from util_bam import make_prep_dir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("ingest,threads", [("device", 6), ("host", 2)])
def test_program_extra_plans_its_chains_like_plan_groups(tmp_path, orc, monkeypatch, ingest, threads):
    """25 small targets with the proportions of GRCh38, three of them without alignments, read names shared between targets: with
    PORTCULLIS_CHAIN_PLAN=groups `junc --extra` finishes them in the groups pjb_plan_groups makes -- named on stderr under
    PJB_PRINT_CHAIN_PLAN --, .tab / .bed (mm_score, coverage, up_aln, down_aln among the columns) are the oracle's, and the
    target-by-target plan writes the same bytes."""
    from portcullis_amd import ffi, synth
    scale = 10000
    lens = [max(3000, ln // scale) for ln in synth.GRCH38]
    lens[24] = 3000
    empty = {7, 19, 24}
    refs, contigs, reads = [], [], []
    rng = np.random.default_rng(77)
    pool = []
    for tid, ln in enumerate(lens):
        if tid in empty:
            g = ("ACGT" * (ln // 4 + 1))[:ln]
        else:
            g, rr = make_reads(700 + tid, n_reads=250, paired=True, glen=ln, n_tx=4)
            for k, r in enumerate(rr):
                r["tid"] = tid
                if r.get("mtid", -1) >= 0:
                    r["mtid"] = tid
                if pool and rng.random() < 0.25:  # (multi-mapped fragments, also across targets)
                    r["name"] = pool[int(rng.integers(0, len(pool)))]
                else:
                    r["name"] = f"frag{tid}_{k}"
                    pool.append(r["name"])
                if "N" not in r["cigar"] and rng.random() < 0.02:
                    r["flag"] |= 0x4
            reads += rr
        refs.append((f"chr{tid + 1}", len(g)))
        contigs.append((f"chr{tid + 1}", g))
    prep = make_prep_dir(str(tmp_path / "prep"), refs, contigs, reads, block_size=20000)
    group_bases = (1 << 30) // scale
    monkeypatch.setenv("PORTCULLIS_CHAIN_PLAN", "groups")
    monkeypatch.setenv("PORTCULLIS_GROUP_BASES", str(group_bases))
    monkeypatch.setenv("PORTCULLIS_CTX_PER_GPU", "1")
    monkeypatch.setenv("PJB_PRINT_CHAIN_PLAN", "1")
    opts = ("--extra", "--ingest", ingest, "--devices", "1")
    p, exp = check(prep, tmp_path, orc, "FR", threads=threads, extra_opts=opts)
    rows = exp["rows"]
    assert (rows["up_aln"] > 0).any() and (rows["coverage"] != 0).any() and (rows["mm_score"] < 1).any()
    want = ffi.plan_groups([ln for _, ln in refs], [t for t in range(25) if t not in empty], group_bases)
    assert len(want) >= 3 and max(len(g) for g in want) >= 4
    groups, chains = _plan_from_stderr(p.stderr)
    assert groups == want, (groups, want)
    assert sorted(chains) == sorted(("group " + ",".join(map(str, g))) if len(g) > 1 else f"target {g[0]}" for g in want), chains
    grouped = {ext: open(str(tmp_path / "out" / "pc") + ext, "rb").read() for ext in (".junctions.tab", ".junctions.bed")}
    monkeypatch.setenv("PORTCULLIS_CHAIN_PLAN", "targets")
    out2 = tmp_path / "singles"
    p2, _ = check(prep, out2, orc, "FR", threads=threads, extra_opts=opts)
    _, chains2 = _plan_from_stderr(p2.stderr)
    assert len(chains2) == 22 and all(c.startswith("target ") for c in chains2)
    for ext, blob in grouped.items():
        assert open(str(out2 / "out" / "pc") + ext, "rb").read() == blob
