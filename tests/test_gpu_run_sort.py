"""The run route of the dense-id sort (kd_assign's id runs per tile, the sorted run list, rs_place) against the radix route.

A stable sort is unique, so both routes must hand k4_pairs the same arrays: every case runs with pjb_set_option("run_sort", 1) and 0,
compares rows and region with the oracle and the two routes' collect() bytes with each other.  The shapes are the smallest at which
the kernels can go wrong: tile edges (4 096 pairs a tile), one junction over three tiles, ids that are not monotone within a tile,
a tile whose ids do not fit the window (forced with "run_window", and with 2 100 junctions in one tile), groups, chains without
pairs, and a PJB_FLAG_EXTRA context."""
import numpy as np
import pytest

from extra_util import add_names, assert_extra_equal, batch_with_names, oracle_extra
from fixtures_micro import read_from_genome
from fuzzgen import make_reads
from parity import assert_rows_equal, region_equal
from portcullis_amd.records import ReadBatch
from test_gpu_edge_cases import G, rd

pytestmark = pytest.mark.gpu

RUNS = 64  # pjb_timing.repeat_reasons: the tiles' ids did not lie in a window (or the run list was full); repeated on the radix route


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi
    return ffi


def routes(ffi, orc, reads, genome=G, window=0):
    """Rows and region equal the oracle's on both routes, and the routes' rows are the same bytes -> (timing with run_sort 1, with 0)."""
    reads = sorted(reads, key=lambda r: r["pos"])  # (stable: reads of one position keep their order)
    b = ReadBatch.from_reads(reads)
    orows, oreg = orc.find_juncs(0, len(genome), genome, b, "UNKNOWN")
    out, raw = [], []
    for run_sort in (1, 0):
        with ffi.Context(0, "UNKNOWN") as ctx:
            ctx.set_option("run_sort", run_sort)
            ctx.set_option("run_window", window)
            ctx.set_refs([len(genome)])
            drows, dreg = ffi.run_contig(ctx, 0, genome.encode(), [b])
            region_equal(dreg, oreg)
            assert_rows_equal(drows, orows)
            raw.append(drows.tobytes())
            out.append(ctx.timing())
    assert raw[0] == raw[1]
    return tuple(out)


def alternating(P):
    """P one-intron reads of two overlapping junctions (introns [1050, 1149] and [1060, 1159]) alternating in BAM order over 20 read
    positions; each junction's reads of one position come as a, b, a, b: same junction, same position, another end -- an order that is
    not stable changes the junctions' distinct-alignment and entropy counts."""
    reads = []
    for k in range(P):
        pos = 1000 + (k * 20) // P
        first = (1050 if k % 2 == 0 else 1060) - pos
        last = (50, 40)[(k // 2) % 2] - (0 if k % 2 == 0 else 10)
        reads.append(rd(pos, f"{first}M100N{last}M"))
    return reads


@pytest.mark.parametrize("P", [1, 4095, 4096, 4097, 8192, 8193])
def test_tile_edges(ffi, orc, P):
    t1, t0 = routes(ffi, orc, alternating(P))
    assert t1["repeats"] == 0 and t1["sort_passes"] == 1, t1
    assert t0["repeats"] == 0 and t0["sort_passes"] == 2, t0


def test_one_deep_junction_over_three_tiles(ffi, orc):
    """8 300 pairs of one junction with 20 pairs of four neighbouring junctions (two with smaller ids, two with larger) sprinkled through
    them: the counts of the tiles before, and a run list that holds one id for many tiles."""
    n = 8300
    reads = []
    for k in range(n):
        pos = 990 + (k * 30) // n
        reads.append(rd(pos, f"{1050 - pos}M100N{50 - k % 3}M"))
    for q in range(20):
        pos = 990 + ((q * 415 + 7) * 30) // n
        start = (1040, 1045, 1055, 1065)[q % 4]
        reads.append(rd(pos, f"{start - pos}M{100 + q % 4}N45M"))
    t1, t0 = routes(ffi, orc, reads)
    assert t1["repeats"] == 0 and t1["sort_passes"] == 1, t1


def test_second_introns_far_away(ffi, orc):
    """Two-intron reads whose second intron lies 30 kb on, among one-intron reads near their first intron, and junctions in between
    further along: the ids of a tile are not monotone."""
    rng = np.random.default_rng(17)
    g = "".join(rng.choice(list("ACGT"), size=40000))
    reads = []
    for k in range(300):
        pos = 1000 + k // 10
        if k % 3 == 0:
            reads.append(read_from_genome(g, pos, f"{1050 - pos}M2000N50M30000N50M"))
        elif k % 3 == 1:
            reads.append(read_from_genome(g, pos, f"{1050 - pos}M2000N{40 + k % 7}M"))
        else:
            reads.append(read_from_genome(g, pos, f"{1045 - pos}M2005N50M"))
    reads += [read_from_genome(g, 2000 + 3 * k, "50M300N50M") for k in range(40)]           # (ids between the near and the far ones)
    reads += [read_from_genome(g, 33040 + k, f"{60 - k}M100N50M") for k in range(10)]        # (and the far intron's neighbours)
    t1, t0 = routes(ffi, orc, reads, genome=g)
    assert t1["repeats"] == 0 and t1["sort_passes"] == 1, t1


SIX = [rd(1000 + 10 * k, f"50M{100 + k}N50M") for k in range(6)]


def test_forced_window_overflow(ffi, orc):
    """A tile of six ids and a window of four: the chain is closed, repeated on the radix route, and the context's next chain plans the
    radix route itself."""
    t1, t0 = routes(ffi, orc, SIX, window=4)
    assert t1["repeats"] >= 1 and t1["repeat_reasons"] & RUNS, t1
    assert t0["repeats"] == 0, t0
    b = ReadBatch.from_reads(SIX)
    with ffi.Context(0, "UNKNOWN") as ctx:
        ctx.set_option("run_window", 4)
        ctx.set_refs([len(G), len(G)])
        for tid in (0, 1):
            orows, oreg = orc.find_juncs(tid, len(G), G, b, "UNKNOWN")
            drows, dreg = ffi.run_contig(ctx, tid, G.encode(), [b])
            region_equal(dreg, oreg)
            assert_rows_equal(drows, orows)
            t = ctx.timing()
            if tid == 0:
                assert t["repeats"] >= 1 and t["repeat_reasons"] & RUNS and t["sort_passes"] >= 2, t
            else:
                assert t["repeats"] == 0 and t["repeat_reasons"] == 0 and t["sort_passes"] >= 2, t


def test_window_of_six_holds_six(ffi, orc):
    t1, _ = routes(ffi, orc, SIX, window=6)
    assert t1["repeats"] == 0 and t1["sort_passes"] == 1, t1


def test_natural_window_overflow(ffi, orc):
    """2 100 reads of 2 100 junctions in one tile: their ids span more than the 2 048 of the window."""
    reads = [rd(100 + k, "30M100N30M") for k in range(2100)]
    t1, t0 = routes(ffi, orc, reads)
    assert t1["repeats"] >= 1 and t1["repeat_reasons"] & RUNS, t1
    assert t0["repeats"] == 0, t0


def test_window_full(ffi, orc):
    """2 048 junctions in one tile fill the window exactly (16 000 unspliced reads behind them: the run list's room follows the
    pair limit, and the pair limit the reads)."""
    reads = [rd(100 + k, "30M100N30M") for k in range(2048)] + [rd(5000, "30M")] * 16000
    t1, _ = routes(ffi, orc, reads)
    assert t1["repeats"] == 0 and t1["sort_passes"] == 1, t1


def test_run_list_full(ffi, orc):
    """The same junctions without the unspliced reads: the room is pair_limit / 8 + 64 a tile = 800 entries, the tile wants 2 048."""
    reads = [rd(100 + k, "30M100N30M") for k in range(2048)]
    t1, t0 = routes(ffi, orc, reads)
    assert t1["repeats"] >= 1 and t1["repeat_reasons"] & RUNS, t1
    assert t0["repeats"] == 0, t0


def test_groups(ffi, orc):
    """Three members as one chain (its first member's pairs reach into the second tile) and a lone target queued behind it:
    groups == singles == oracle, on both routes."""
    members = [alternating(4200), [r for r in SIX], alternating(300) + [rd(2000, "50M700N50M")], alternating(100)]
    want = []
    for tid, reads in enumerate(members):
        b = ReadBatch.from_reads(sorted(reads, key=lambda r: r["pos"]))
        orows, oreg = orc.find_juncs(tid, len(G), G, b, "UNKNOWN")
        want.append((b, orows, oreg))
    all_rows = np.concatenate([w[1] for w in want])
    raw = []
    for run_sort in (1, 0):
        with ffi.Context(0, "UNKNOWN") as ctx:
            ctx.set_option("run_sort", run_sort)
            ctx.set_refs([len(G)] * 4)
            for tid in range(4):
                ctx.upload_contig(tid, G.encode())
            ctx.clear_rows()
            for tid, (b, _, oreg) in enumerate(want):
                ctx.submit_batch(tid, b)
                region_equal(ctx.finish_contig(tid), oreg)
                assert ctx.timing()["repeats"] == 0
            singles = ctx.collect()
            assert_rows_equal(singles, all_rows)
            ctx.clear_rows()
            for tid, (b, _, _) in enumerate(want):
                ctx.submit_batch(tid, b)
            ctx.finish_group_begin([0, 1, 2])
            ctx.finish_contig_begin(3)  # (two chains queued at once)
            regs = ctx.finish_group_end([0, 1, 2])
            t = ctx.timing()
            assert t["repeats"] == 0 and t["sort_passes"] == (1 if run_sort else 2), t
            for tid in range(3):
                region_equal(regs[tid], want[tid][2])
            region_equal(ctx.finish_contig_end(3), want[3][2])
            grouped = ctx.collect()
            assert_rows_equal(grouped, all_rows)
            assert grouped.tobytes() == singles.tobytes()
            raw.append(grouped.tobytes())
    assert raw[0] == raw[1]


@pytest.mark.parametrize("reads", [[rd(1000, "100M"), rd(1010, "90M")], [rd(1000, "100M"), rd(1010, "50M100N50M")]], ids=["no_pair", "one_pair"])
def test_degenerate_chains(ffi, orc, reads):
    t1, t0 = routes(ffi, orc, reads)
    assert t1["repeats"] == 0 and t0["repeats"] == 0


def test_extra(ffi, orc):
    """A PJB_FLAG_EXTRA context: rows and extra columns equal the oracle's and each other on both routes."""
    rng = np.random.default_rng(23)
    genome, reads = make_reads(231, n_reads=3000)
    add_names(reads, rng, "r")
    contigs = [(genome, reads)]
    orows, _ = oracle_extra(orc, contigs)
    raw = []
    for run_sort in (1, 0):
        with ffi.Context(0, "UNKNOWN", flags=ffi.FLAG_EXTRA) as ctx:
            ctx.set_option("run_sort", run_sort)
            ctx.set_refs([len(genome)])
            ctx.clear_rows()
            ctx.upload_contig(0, genome.encode())
            ctx.submit_batch(0, batch_with_names(orc, reads))
            ctx.finish_contig(0)
            t = ctx.timing()
            assert t["repeats"] == 0 and t["sort_passes"] == (1 if run_sort else 2), t
            rows = ctx.collect()
            extra = ctx.extra_finish()
        assert_rows_equal(rows, orows)
        assert_extra_equal(rows, extra, orows)
        raw.append((rows.tobytes(), extra.tobytes()))
    assert raw[0] == raw[1]


def test_timing_on_ordinary_input(ffi, orc):
    genome, reads = make_reads(5, n_reads=3000, paired=True)
    t1, t0 = routes(ffi, orc, reads, genome=genome)
    assert t1["repeats"] == 0 and t1["sort_passes"] == 1, t1
    assert t0["repeats"] == 0 and t0["sort_passes"] == 2, t0
