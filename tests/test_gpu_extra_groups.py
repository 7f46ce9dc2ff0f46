"""`junc --extra` with target groups: a PJB_FLAG_EXTRA context takes pjb_finish_group_begin / _end, and rows, per-target results and
the rows of pjb_extra_finish are those of finishing the targets one by one -- byte for byte, the doubles as bit patterns: the
arithmetic is the same -- and those of the oracle."""
import numpy as np
import pytest

from extra_util import add_names, assert_extra_equal, batch_with_names, oracle_extra
from fuzzgen import make_reads
from parity import assert_rows_equal

pytestmark = pytest.mark.gpu

ERR_ARG = -16
GROUP_APART = 32  # pjb_timing.repeat_reasons: the group collected last was taken apart, its members finished one by one


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi as f
    assert f.device_count() >= 1
    return f


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o
    return o


def _contigs(seed, n_contigs, n_reads=1200, paired=False, **kw):
    rng = np.random.default_rng(seed)
    pool, out = [], []
    for t in range(n_contigs):
        genome, reads = make_reads(seed * 10 + t, n_reads=n_reads, paired=paired, **kw)
        add_names(reads, rng, f"c{t}", pool)  # (names shared across contigs: the multiplicities are file-wide)
        out.append((genome, reads))
    return out


def run_plan(ffi, orc, contigs, plan, orientation="UNKNOWN", queue=1, split=None):
    """The contigs through a fresh PJB_FLAG_EXTRA context, finished in the chains of `plan` (lists of tids; one tid: pjb_finish_contig_begin,
    several: pjb_finish_group_begin), at most `queue` chains queued at once.  -> rows, extra rows, {tid: region result}, [timing per chain]"""
    with ffi.Context(0, orientation, flags=ffi.FLAG_EXTRA) as ctx:
        ctx.set_refs([len(g) for g, _ in contigs])
        ctx.clear_rows()
        for tid, (genome, reads) in enumerate(contigs):
            ctx.upload_contig(tid, genome.encode())
            if not reads:
                continue
            b = batch_with_names(orc, reads)
            if split and b.n > 4:
                cuts = sorted(set([0, b.n] + [int(b.n * f) for f in split]))
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    ctx.submit_batch(tid, b.slice(lo, hi))
            else:
                ctx.submit_batch(tid, b)
        regs, timings, queued = {}, [], []

        def end(chain):
            if len(chain) > 1:
                regs.update(ctx.finish_group_end(chain))
            else:
                regs[chain[0]] = ctx.finish_contig_end(chain[0])
            timings.append(ctx.timing())

        for chain in plan:
            if len(queued) >= queue:
                end(queued.pop(0))
            if len(chain) > 1:
                ctx.finish_group_begin(chain)
            else:
                ctx.finish_contig_begin(chain[0])
            queued.append(chain)
        for chain in queued:
            end(chain)
        rows = ctx.collect()
        extra = ctx.extra_finish()
    return rows, extra, regs, timings


def singles(ffi, orc, contigs, orientation="UNKNOWN"):
    return run_plan(ffi, orc, contigs, [[t] for t in range(len(contigs))], orientation)


def assert_same_bits(got, want, what):
    """(rows, extra rows, region results) of two runs: every byte, mm_score and coverage as bit patterns."""
    rows, extra, regs = got[:3]
    srows, sextra, sregs = want[:3]
    assert rows.tobytes() == srows.tobytes(), what
    assert len(extra) == len(sextra), what
    for f in ("mm_score", "coverage"):
        a, b = extra[f].view(np.uint64), sextra[f].view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (what, f, bad.size, int(rows["refid"][bad[0]]), int(rows["start"][bad[0]]), extra[f][bad[0]], sextra[f][bad[0]])
    for f in ("up_aln", "down_aln"):
        bad = np.nonzero(extra[f] != sextra[f])[0]
        assert bad.size == 0, (what, f, bad.size, int(rows["refid"][bad[0]]), int(rows["start"][bad[0]]), extra[f][bad[0]], sextra[f][bad[0]])
    assert extra.tobytes() == sextra.tobytes(), what
    assert regs == sregs, what


_BASELINES = {}


def check_plans(ffi, orc, contigs, plans, orientation="UNKNOWN", split=None, key=None):
    """Every plan against the oracle and, bit for bit, against the target-by-target run on a context of its own (`key`: both are kept
    for the next test on the same contigs)."""
    if key is None or key not in _BASELINES:
        orows, _ = oracle_extra(orc, contigs, orientation)
        want = singles(ffi, orc, contigs, orientation)
        assert_rows_equal(want[0], orows)
        assert_extra_equal(want[0], want[1], orows)
        if key is not None:
            _BASELINES[key] = (orows, want)
    else:
        orows, want = _BASELINES[key]
    out = []
    for plan, queue in plans:
        got = run_plan(ffi, orc, contigs, plan, orientation, queue=queue, split=split)
        assert_rows_equal(got[0], orows)
        assert_extra_equal(got[0], got[1], orows)
        assert_same_bits(got, want, (plan, queue))
        out.append(got)
    return orows, want, out


# ---- a. fuzzed contigs ---------------------------------------------------------------------------------------------------------

SEEDS = list(range(101, 114))


def _fuzz_case(seed):
    n = 6 + seed % 3
    paired = bool(seed % 2)
    return _contigs(seed, n, paired=paired), ("FR" if paired else "UNKNOWN"), n


@pytest.mark.parametrize("seed", SEEDS)
def test_extra_one_group_equals_singles_and_oracle(ffi, orc, seed):
    """Six to eight targets, names shared between them, finished as ONE chain."""
    contigs, orientation, n = _fuzz_case(seed)
    _, want, (got,) = check_plans(ffi, orc, contigs, [([list(range(n))], 1)], orientation, key=seed)
    extra = got[1]
    assert (extra["up_aln"] > 0).any() and (extra["down_aln"] > 0).any() and (extra["mm_score"] < 1).any() and (extra["coverage"] != 0).any()
    assert all(not (t["repeat_reasons"] & GROUP_APART) for t in got[3])  # (a group chain, not its members one by one)


@pytest.mark.parametrize("seed", SEEDS)
def test_extra_two_groups_and_a_single(ffi, orc, seed):
    """Two groups and a single target in between, collected chain after chain and with all three chains queued at once; ragged
    batches (a member's records in several batches)."""
    contigs, orientation, n = _fuzz_case(seed)
    plan = [list(range(0, 3)), [3], list(range(4, n))]
    check_plans(ffi, orc, contigs, [(plan, 1), (plan, 3)], orientation, split=(0.1, 0.55, 0.56) if seed % 2 else None, key=seed)


# ---- b. the hand-over rule -----------------------------------------------------------------------------------------------------

def test_extra_groups_hand_over_between_members_and_chains(ffi, orc):
    """JunctionSystem::calcCoverage hands every target's depth to the junctions of the NEXT target that has unspliced records.  Members
    without alignments, with spliced records only (not in the pileup) and without junctions; the first and the last target of the file
    as group members; a coverage source in the chain before the junctions'."""
    a = _contigs(31, 4, n_reads=1500)
    rng = np.random.default_rng(9)
    g2, r2 = make_reads(311, n_reads=600)
    r2 = [r for r in r2 if "N" in r["cigar"]]
    g4, r4 = make_reads(312, n_reads=400)
    r4 = [r for r in r4 if "N" not in r["cigar"]]
    add_names(r2, rng, "x2")
    add_names(r4, rng, "x4")
    #          0     1: no alignments       2: spliced only  3   4: no junctions  5     6
    contigs = [a[0], ("ACGT" * 500, None), (g2, r2), a[1], (g4, r4), a[2], a[3]]
    plans = [([[0, 1, 2], [3, 4], [5, 6]], 3),     # 3 takes 0's depth, 5 takes 4's: sources in the chain before
             ([[0, 1, 2, 3], [4, 5, 6]], 2),
             ([[0, 1, 2, 3, 4, 5, 6]], 1),
             ([[0, 1, 2], [3], [4, 5, 6]], 3),     # a single chain between two groups: source and junctions in different kinds of chain
             ([[0], [1, 2, 3, 4, 5], [6]], 2)]
    orows, want, outs = check_plans(ffi, orc, contigs, plans)
    for rows, extra, _, _ in outs:
        assert (extra["coverage"][rows["refid"] == 0] == 0).all()   # first target: never visited
        assert (extra["coverage"][rows["refid"] == 2] == 0).all()   # spliced-only target: not in the pileup, never visited
        assert (extra["coverage"][rows["refid"] == 3] != 0).any()   # target 0's depth
        assert (extra["coverage"][rows["refid"] == 5] != 0).any()   # target 4's depth (a target without junctions is a source all the same)
        assert not (rows["refid"] == 4).any() and not (rows["refid"] == 1).any()


# ---- c. member boundaries ------------------------------------------------------------------------------------------------------

def _edge_contig(glen, tag, rng):
    """Junctions whose windows leave the target at both ends, unspliced records from position 0 and up to the last base, records
    without a reference span, deletions."""
    g = "".join(rng.choice(list("ACGT"), size=glen))
    n = glen
    reads = [dict(pos=0, cigar="10M20N30M", seq="A" * 40, xs="+"),      # left anchor from 0: start - 20 < 0
             dict(pos=0, cigar="30M", seq="C" * 30),                     # starts at position 0 of the member
             dict(pos=0, cigar="9M", seq=None, l_qseq=9),
             dict(pos=5, cigar="12S", seq="A" * 12),                     # no reference span
             dict(pos=9, cigar="30M", seq="A" * 30),
             dict(pos=10, cigar="4I", seq="A" * 4),                      # no span, at the intron's start
             dict(pos=12, cigar="8M2D12M1D9M", seq=None, l_qseq=29),     # deletions inside the donor / acceptor windows
             dict(pos=30, cigar="8S", seq="A" * 8),
             dict(pos=31, cigar="10M", seq=None, l_qseq=10),
             dict(pos=n - 60, cigar="30M20N10M", seq="A" * 40, xs="-"),  # right anchor up to the last base: end + 20 > len
             dict(pos=n - 52, cigar="7M3D10M1D20M", seq=None, l_qseq=37),
             dict(pos=n - 40, cigar="40M", seq="G" * 40),                # ends on the last base of the member
             dict(pos=n - 30, cigar="30M", seq="G" * 30),
             dict(pos=n - 12, cigar="6S", seq="A" * 6),
             dict(pos=n - 9, cigar="9M", seq=None, l_qseq=9),
             dict(pos=n - 1, cigar="1M", seq="A")]
    reads.sort(key=lambda r: r["pos"])
    for k, r in enumerate(reads):
        r["name"] = f"{tag}.{k}"
        r.setdefault("flag", 0)
    return g, reads


def test_extra_groups_member_boundaries(ffi, orc):
    """What happens at the seam between two members of a group's virtual sequence: records ending on the last base of member m and
    starting at position 0 of member m + 1, junction windows that reach below 0 / past the member's length (clipped in the member's own
    coordinates), records without a span at equal positions in several members, deletions in several members.  A neighbour's records
    must add nothing."""
    rng = np.random.default_rng(17)
    fuzz = _contigs(41, 2, n_reads=900)
    contigs = [_edge_contig(600, "e0", rng), _edge_contig(600, "e1", rng), fuzz[0], _edge_contig(900, "e3", rng), _edge_contig(640, "e4", rng), fuzz[1]]
    plans = [([[0, 1, 2, 3, 4, 5]], 1), ([[0, 1], [2, 3, 4, 5]], 2), ([[0, 1, 2], [3, 4], [5]], 3), ([[0], [1, 2, 3, 4], [5]], 1)]
    orows, want, outs = check_plans(ffi, orc, contigs, plans)
    rows, extra = want[0], want[1]
    for tid in (0, 1, 3, 4):
        sel = rows["refid"] == tid
        assert sel.sum() == 2 and (extra["up_aln"][sel] > 0).all() and (extra["down_aln"][sel] > 0).any()
    assert (extra["coverage"][rows["refid"] == 1] != 0).any() and (extra["coverage"][rows["refid"] == 4] != 0).any()  # (depth of 0 and of 3)


# ---- d. the dense fallback -----------------------------------------------------------------------------------------------------

def test_extra_group_with_a_pileup_is_taken_apart(ffi, orc):
    """A member where htslib's 8000-record cap bites (as in test_extra_pileup_cap) needs the depth vector: the group is taken apart --
    pjb_timing.repeat_reasons says so -- before anything of it is committed, its members go one by one, and the chains queued behind
    it are queued again."""
    genome, reads = make_reads(11, glen=6000, n_reads=1500, L=(60, 120))
    rng = np.random.default_rng(3)
    spliced = [r for r in reads if "N" in r["cigar"]]
    anchor = spliced[len(spliced) // 2]["pos"]
    deep = []
    for k in range(12000):
        p = max(0, anchor - 40 + int(rng.integers(0, 6)))
        deep.append(dict(pos=p, cigar=f"{int(rng.integers(40, 90))}M", seq=None, l_qseq=0, flag=0))
    allr = sorted(reads + deep, key=lambda r: r["pos"])
    add_names(allr, rng, "d", unmapped_frac=0.0)
    depth, kept = orc.depth(len(genome), batch_with_names(orc, allr))
    n_unspliced = sum(1 for r in allr if "N" not in r["cigar"] and not (r.get("flag", 0) & 4))
    assert kept < n_unspliced and depth.max() >= 7999          # the cap really dropped records in the oracle
    fuzz = _contigs(51, 4, n_reads=900)
    contigs = [fuzz[0], (genome, allr), fuzz[1], fuzz[2], fuzz[3]]
    orows, want, outs = check_plans(ffi, orc, contigs, [([[0, 1, 2], [3, 4]], 2), ([[0], [1, 2, 3, 4]], 1)])
    for (_, _, _, timings), holds_pile in zip(outs, ([True, False], [False, True])):
        assert [bool(t["repeat_reasons"] & GROUP_APART) for t in timings] == holds_pile, timings   # the chain with target 1, and only that one


# ---- e. refusals ---------------------------------------------------------------------------------------------------------------

def test_extra_dense_option_refuses_groups(ffi, orc):
    """pjb_set_option("extra_dense", 1) builds a depth vector per target: pjb_finish_group_begin answers PJB_ERR_ARG ("not as a group"),
    nothing is queued, and the targets finish one by one."""
    contigs = _contigs(61, 3, n_reads=900)
    orows, _ = oracle_extra(orc, contigs)
    with ffi.Context(0, "UNKNOWN", flags=ffi.FLAG_EXTRA) as ctx:
        ctx.set_refs([len(g) for g, _ in contigs])
        ctx.clear_rows()
        ctx.set_option("extra_dense", 1)
        for tid, (genome, reads) in enumerate(contigs):
            ctx.upload_contig(tid, genome.encode())
            ctx.submit_batch(tid, batch_with_names(orc, reads))
        with pytest.raises(ffi.PjbError) as e:
            ctx.finish_group_begin([0, 1, 2])
        assert e.value.code == ERR_ARG, e.value
        assert ctx.finish_ready()          # (nothing queued)
        for tid in range(3):
            ctx.finish_contig(tid)
        rows, extra = ctx.collect(), ctx.extra_finish()
    assert_rows_equal(rows, orows)
    assert_extra_equal(rows, extra, orows)


def test_extra_context_keeps_the_other_refusals(ffi, orc):
    """More than PJB_GROUP_MAX members and a genome with a character outside the 16-letter alphabet are "not as a group" on a
    PJB_FLAG_EXTRA context as on any other."""
    contigs = _contigs(62, 2, n_reads=600)
    g = contigs[0][0][:200] + "J" + contigs[0][0][201:]
    with ffi.Context(0, "UNKNOWN", flags=ffi.FLAG_EXTRA) as ctx:
        ctx.set_refs([len(g), len(contigs[1][0])] + [1000] * ffi.GROUP_MAX)
        ctx.clear_rows()
        ctx.upload_contig(0, g.encode())
        ctx.upload_contig(1, contigs[1][0].encode())
        for tid in range(2):
            ctx.submit_batch(tid, batch_with_names(orc, contigs[tid][1]))
        with pytest.raises(ffi.PjbError) as e:
            ctx.finish_group_begin([0, 1])
        assert e.value.code == ERR_ARG, e.value
        with pytest.raises(ffi.PjbError) as e:
            ctx.finish_group_begin(list(range(1, ffi.GROUP_MAX + 2)))
        assert e.value.code == ERR_ARG, e.value
        ctx.finish_contig(0)
        ctx.finish_contig(1)
        assert len(ctx.collect()) == len(ctx.extra_finish()) > 0
