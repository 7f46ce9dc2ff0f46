"""k4_pairs folds a RANGE of 64-pair slices a wavefront (pjb_set_option("pair_range", n): n slices a range; the fragment rule is
frag_slot in pjb_device.hip.h).  Every fragment field is an integer sum, maximum or minimum, so how the pairs are grouped cannot show
in a row: every case runs with pair_range 1 (a fragment a slice), 2 and the default, on dense ids (the masks are written) and on the
full keys (null masks), rows and region must equal the oracle's and the collect() bytes of all six settings must be identical.

With pair_range 2 a range holds 128 pairs, so a few hundred reads reach every edge: a range's last slice partly filled, a junction
that begins exactly with a range (the skipped slot) or with a slice inside one, slices in which every lane begins a junction, the
previous pair carried from the slice before against the one a range's first slice fetches (equal read positions and ends on both
sides of an edge: nb_dist and entropy would show a wrong one), a last range of one pair, no pair at all."""
import numpy as np
import pytest

from extra_util import add_names, assert_extra_equal, batch_with_names, oracle_extra
from fuzzgen import make_reads
from parity import assert_rows_equal, region_equal
from portcullis_amd.records import ReadBatch
from test_gpu_edge_cases import G, rd
from test_gpu_run_sort import alternating

pytestmark = pytest.mark.gpu

ERR_ARG = -16  # PJB_ERR_ARG
SETTINGS = [(pr, dense) for pr in (1, 2, None) for dense in (1, 0)]  # (None: the default range)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi
    return ffi


def configure(ctx, pair_range, dense):
    if pair_range is not None:
        ctx.set_option("pair_range", pair_range)
    ctx.set_option("dense_ids", dense)


def all_settings(ffi, orc, reads, genome=G, settings=SETTINGS):
    """Rows and region equal the oracle's under every setting, and the settings' rows are the same bytes -> the oracle's rows."""
    reads = sorted(reads, key=lambda r: r["pos"])  # (stable: reads of one position keep their order)
    b = ReadBatch.from_reads(reads)
    orows, oreg = orc.find_juncs(0, len(genome), genome, b, "UNKNOWN")
    raw = []
    for pair_range, dense in settings:
        with ffi.Context(0, "UNKNOWN") as ctx:
            configure(ctx, pair_range, dense)
            ctx.set_refs([len(genome)])
            drows, dreg = ffi.run_contig(ctx, 0, genome.encode(), [b])
            assert ctx.timing()["repeats"] == 0
        region_equal(dreg, oreg)
        assert_rows_equal(drows, orows)
        raw.append(drows.tobytes())
    assert all(r == raw[0] for r in raw)
    return orows


def junction(n, start=1050, nlen=100, ends=(50, 49, 48), first_pos=990, spread=30):
    """n one-intron reads of the junction [start, start + nlen - 1] over `spread` read positions, their ends cycling through `ends`."""
    reads = []
    for k in range(n):
        pos = first_pos + (k * spread) // n
        reads.append(rd(pos, f"{start - pos}M{nlen}N{ends[k % len(ends)]}M"))
    return reads


@pytest.mark.parametrize("P", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257])
def test_range_edges(ffi, orc, P):
    """Two alternating junctions: the array's end on every side of a slice's and a range's edge (257: a last range of one pair)."""
    all_settings(ffi, orc, alternating(P))


@pytest.mark.parametrize("P", [513, 1025])
def test_last_range_of_one_pair_at_the_default(ffi, orc, P):
    """(the default range holds 512 pairs -- and 1 025 pairs are a last range of one pair for ranges of 256 and 1 024 as well)"""
    all_settings(ffi, orc, alternating(P), settings=[(None, 1), (1, 1)])


def test_one_junction_over_four_ranges(ffi, orc):
    orows = all_settings(ffi, orc, junction(400))
    assert len(orows) == 1 and orows["nb_raw"][0] == 400


@pytest.mark.parametrize("at", [128, 64])
def test_junction_begins_at_an_edge(ffi, orc, at):
    """The second junction's first pair is pair `at` of the sorted array: 128 begins a range of two slices (the slot before its
    fragment's stays unused), 64 a slice inside one."""
    orows = all_settings(ffi, orc, junction(at) + junction(100, start=1060))
    assert list(orows["nb_raw"]) == [at, 100]


def test_every_lane_a_head(ffi, orc):
    """130 junctions of one pair each -- two slices in which every lane begins a junction, and two more in the third --, then one
    junction of 300 pairs."""
    reads = [rd(100 + k, "30M100N30M") for k in range(130)] + junction(300)
    orows = all_settings(ffi, orc, reads)
    assert len(orows) == 131 and orows["nb_raw"].max() == 300


def test_previous_pair_across_edges(ffi, orc):
    """One junction whose pairs -- in BAM order, which is their sorted order -- alternate between two ends, except for stretches of
    identical alignments (same position, same end) that straddle a slice's edge (pairs 60-68), a range's edge at pair_range 2
    (124-132, 250-258) and the default's (508-516), and one that ends exactly at an edge (183-191): a distinct alignment is counted
    where position or end differ from the pair before, and the pair before lane 0 comes from registers or from memory."""
    same = set()
    for a, b in ((60, 69), (124, 133), (183, 192), (250, 259), (508, 517)):  # (an odd number of pairs: the next one's end differs)
        same.update(range(a + 1, b))  # (these repeat the pair before them)
    reads, last = [], 50
    n = 530
    for k in range(n):
        pos = 1000 + k // 20
        if k not in same:
            last = 50 - (k % 2) - 2 * ((k // 20) % 2)  # (never the end of the pair before: 50, 49 | 48, 47 by position)
        reads.append(rd(pos, f"{1050 - pos}M100N{last}M"))
    orows = all_settings(ffi, orc, reads)
    assert len(orows) == 1 and orows["nb_raw"][0] == n and orows["nb_dist"][0] == n - len(same)


def test_chain_without_pairs(ffi, orc):
    orows = all_settings(ffi, orc, [rd(1000, "100M"), rd(1010, "90M")])
    assert len(orows) == 0


def test_group_of_two_targets(ffi, orc):
    """Two members as one chain (the first member's third junction begins inside a slice): the group's rows are the members' own."""
    members = [alternating(70) + junction(200, start=1200, first_pos=1140), alternating(300)]
    want = []
    for tid, reads in enumerate(members):
        b = ReadBatch.from_reads(sorted(reads, key=lambda r: r["pos"]))
        orows, oreg = orc.find_juncs(tid, len(G), G, b, "UNKNOWN")
        want.append((b, orows, oreg))
    all_rows = np.concatenate([w[1] for w in want])
    raw = []
    for pair_range, dense in SETTINGS:
        with ffi.Context(0, "UNKNOWN") as ctx:
            configure(ctx, pair_range, dense)
            ctx.set_refs([len(G)] * 2)
            for tid in range(2):
                ctx.upload_contig(tid, G.encode())
            ctx.clear_rows()
            for tid, (b, _, _) in enumerate(want):
                ctx.submit_batch(tid, b)
            ctx.finish_group_begin([0, 1])
            regs = ctx.finish_group_end([0, 1])
            assert ctx.timing()["repeats"] == 0
            for tid in range(2):
                region_equal(regs[tid], want[tid][2])
            rows = ctx.collect()
        assert_rows_equal(rows, all_rows)
        raw.append(rows.tobytes())
    assert all(r == raw[0] for r in raw)


def test_extra(ffi, orc):
    """A PJB_FLAG_EXTRA context: rows and extra columns equal the oracle's and each other under every setting."""
    rng = np.random.default_rng(29)
    genome, reads = make_reads(233, n_reads=3000)
    add_names(reads, rng, "r")
    orows, _ = oracle_extra(orc, [(genome, reads)])
    batch = batch_with_names(orc, reads)
    raw = []
    for pair_range, dense in SETTINGS:
        with ffi.Context(0, "UNKNOWN", flags=ffi.FLAG_EXTRA) as ctx:
            configure(ctx, pair_range, dense)
            ctx.set_refs([len(genome)])
            ctx.clear_rows()
            ctx.upload_contig(0, genome.encode())
            ctx.submit_batch(0, batch)
            ctx.finish_contig(0)
            assert ctx.timing()["repeats"] == 0
            rows = ctx.collect()
            extra = ctx.extra_finish()
        assert_rows_equal(rows, orows)
        assert_extra_equal(rows, extra, orows)
        raw.append((rows.tobytes(), extra.tobytes()))
    assert all(r == raw[0] for r in raw)


def test_deep_junction_at_the_default(ffi, orc):
    """30 000 pairs of one junction: dozens of ranges, and k5_frag_reduce's atomics from several wavefronts on one junction.  (20 000
    unspliced reads behind them: the pair limit follows the reads, and the chain is not to be repeated for it.)"""
    reads = junction(30000, ends=(50, 49, 48, 47, 46)) + [rd(5000, "30M")] * 20000
    orows = all_settings(ffi, orc, reads, settings=[(None, 1), (None, 0)])
    assert len(orows) == 1 and orows["nb_raw"][0] == 30000


@pytest.mark.parametrize("value", [0, 3, 6, 64, -1])
def test_bad_value(ffi, value):
    with ffi.Context(0, "UNKNOWN") as ctx:
        with pytest.raises(ffi.PjbError) as e:
            ctx.set_option("pair_range", value)
        assert e.value.code == ERR_ARG
        for ok in (1, 2, 4, 8, 16, 32):
            ctx.set_option("pair_range", ok)
