"""The chain-wide block-span bound B (ContigStats::max_span) and the window-check list.

A closed read of two and more introns goes on k4b_generic's second list only where some junction's anchor window can reach over
one of its introns from the neighbouring one.  B = the chain's longest alignment without its N operations bounds istart - lStart
and rEnd - iend of every pair, so for a block of `blk` reference positions between introns of nl_prev and nl_next positions

    left:  prev_istart >= anc_l[j]  needs  blk + nl_prev     <= B
    right: next_iend + 1 <= anc_r[j] needs  blk + nl_next + 1 <= B

Every case compares rows and region with the oracle, with the test on (the default) and off (pjb_set_option("window_skip", 0)),
and looks at pjb_timing.checked_reads: the reads on the second list."""
import numpy as np
import pytest

from fixtures_micro import read_from_genome
from parity import assert_rows_equal, region_equal
from portcullis_amd.records import ReadBatch
from test_gpu_edge_cases import G, rd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi
    return ffi


def checked(ffi, orc, reads, genome=G, orientation="UNKNOWN"):
    """Rows and region equal the oracle's with the test on and off -> (checked_reads with it, checked_reads without)."""
    reads = sorted(reads, key=lambda r: r["pos"])
    b = ReadBatch.from_reads(reads)
    orows, oreg = orc.find_juncs(0, len(genome), genome, b, orientation)
    out = []
    for skip in (1, 0):
        with ffi.Context(0, orientation) as ctx:
            ctx.set_option("window_skip", skip)
            ctx.set_refs([len(genome)])
            drows, dreg = ffi.run_contig(ctx, 0, genome.encode(), [b])
            region_equal(dreg, oreg)
            assert_rows_equal(drows, orows)
            out.append(ctx.timing()["checked_reads"])
    return tuple(out)


# read X's second intron lies under the right anchor of Y, which shares X's first junction (X's third block carries a
# substitution there: the walks see it, the closed form of X's first pair does not); Z is the mirror image on X's second junction
X_RIGHT = [rd(1000, "50M60N50M60N50M", sub=105), rd(1030, "20M60N130M")]
X_LEFT = [rd(1000, "50M60N50M60N50M", sub=40), rd(1030, "130M60N20M")]
# a generic read whose deletion makes it the chain's longest (span 550), and a two-intron read that only it makes reachable (nl + b2 = 350)
LONG_D = rd(2000, "40M400D40M900N70M")
SAFE_TWO = rd(4000, "50M300N50M300N50M")


def test_nothing_to_check(ffi, orc):
    reads = [rd(100 + i, "50M2000N50M3000N50M") for i in range(10)] + [rd(120, "30M2000N70M"), rd(2200, "50M3000N50M"), rd(5300, "50M100N50M")]
    assert checked(ffi, orc, reads) == (0, 10)


@pytest.mark.parametrize("reads", [X_RIGHT, X_LEFT], ids=["right", "left"])
def test_the_check_must_run(ffi, orc, reads):
    # B = 150; X: blk + nl = 110 -- listed, fails the check (the other read's anchor reaches over its other intron), takes the walks
    assert checked(ffi, orc, reads) == (1, 1)
    # without the other read nothing reaches: X is listed all the same (the bound cannot tell) and passes the check
    assert checked(ffi, orc, reads[:1]) == (1, 1)


@pytest.mark.parametrize("side,d,listed", [("left", -1, 1), ("left", 0, 1), ("left", 1, 0), ("right", -1, 1), ("right", 0, 0), ("right", 1, 0)])
def test_the_boundary(ffi, orc, side, d, listed):
    """B = 200, fixed by a one-intron read of that span; the read under test (span 100, blk = 40) has blk + nl (left) or blk + nl2 (right)
    at B - 1, B, B + 1 and the other intron far too long to matter.  Left: listed up to B.  Right: listed below B (the + 1 of the test)."""
    B = 200
    n_near, n_far = B + d - 40, 2000
    cig = f"30M{n_near}N40M{n_far}N30M" if side == "left" else f"30M{n_far}N40M{n_near}N30M"
    assert checked(ffi, orc, [rd(1000, cig), rd(3500, "100M500N100M")]) == (listed, 1)


def test_bound_from_a_generic_read(ffi, orc):
    assert checked(ffi, orc, [SAFE_TWO]) == (0, 1)
    # (window_skip = 0 lists the closed generic read as well)
    assert checked(ffi, orc, [LONG_D, SAFE_TWO]) == (1, 2)


@pytest.mark.parametrize("where", ["head", "tail"])
def test_partial_tile(ffi, orc, where):
    """1 500 reads: a whole tile (k1_count's rows path) and a partial one (its rounds); the reads that matter in the one, then in the other."""
    special = X_RIGHT + X_LEFT[1:] + [LONG_D, SAFE_TWO]
    n_fill = 1500 - len(special)
    fill = [rd(900 if where == "tail" else 4500, "50M") for _ in range(n_fill)]
    # X (blk + nl = 110) and SAFE_TWO (350) are reachable with B = 550
    assert checked(ffi, orc, special + fill) == (2, 3)


def test_tile_of_many_operations(ffi, orc):
    """A whole tile with more than 3 072 operations leaves k1_count's rows path for its rounds."""
    special = X_RIGHT + [LONG_D, SAFE_TWO]
    fill = [rd(4500, "10M1I10M1D10M2I10M") for _ in range(1100 - len(special))]  # (behind them: the reads that matter are in the whole tile)
    assert checked(ffi, orc, special + fill) == (2, 3)


def test_group_bound_is_the_chains(ffi, orc):
    """Two targets as one chain: B comes from member 0's long read, and member 1's two-intron read is listed; finished one by one it is not."""
    members = [[LONG_D, rd(3000, "50M100N50M")], X_RIGHT + [SAFE_TWO]]
    want = []
    for tid, reads in enumerate(members):
        b = ReadBatch.from_reads(sorted(reads, key=lambda r: r["pos"]))
        orows, oreg = orc.find_juncs(tid, len(G), G, b, "UNKNOWN")
        want.append((b, orows, oreg))
    for skip, singles, grouped in ((1, [0, 1], 2), (0, [1, 2], 3)):
        with ffi.Context(0, "UNKNOWN") as ctx:
            ctx.set_option("window_skip", skip)
            ctx.set_refs([len(G), len(G)])
            for tid in (0, 1):
                ctx.upload_contig(tid, G.encode())
            ctx.clear_rows()
            for tid, (b, orows, oreg) in enumerate(want):
                ctx.submit_batch(tid, b)
                region_equal(ctx.finish_contig(tid), oreg)
                assert ctx.timing()["checked_reads"] == singles[tid]
            assert_rows_equal(ctx.collect(), np.concatenate([w[1] for w in want]))
            ctx.clear_rows()
            for tid, (b, _, _) in enumerate(want):
                ctx.submit_batch(tid, b)
            ctx.finish_group_begin([0, 1])
            regs = ctx.finish_group_end([0, 1])
            for tid, (_, _, oreg) in enumerate(want):
                region_equal(regs[tid], oreg)
            assert ctx.timing()["checked_reads"] == grouped
            assert_rows_equal(ctx.collect(), np.concatenate([w[1] for w in want]))


def test_record_escape_values_reach_k4b_generic(ffi, orc):
    """l_qseq >= 0xffff does not fit the spliced list's record (all-ones there: the kernels fetch it): a read of the closed two-intron shape
    that fails the window check, one with a deletion (closed by k1_generic) and one with a hard clip (the walks' list)."""
    rng = np.random.default_rng(5)
    g = "".join(rng.choice(list("ACGT"), size=150000))
    reads = [read_from_genome(g, 1000, "33000M60N50M60N33000M", sub=33000 + 50 + 5), read_from_genome(g, 33980, "20M60N130M"),
             read_from_genome(g, 70000, "33000M5D100M60N50M60N33000M"), read_from_genome(g, 103085, "20M60N130M"),
             read_from_genome(g, 72000, "5H33000M60N40000M")]
    assert all(len(r["seq"]) >= 0xffff for r in reads[::2])
    assert checked(ffi, orc, reads, genome=g) == (2, 2)
