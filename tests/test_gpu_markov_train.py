"""pjb_markov_train (ctx.markov_train): the eight Markov models of `filt --self_train` / `train --markov` trained on the device, against the
models the oracle's orc_filt_features trains on the same junctions -- which the committed witnesses pin to the reference's own
markov_model.cc (tests/test_oracle_markov_witness.py).  The counts are integers and the one division is the host's, so every table is
compared bit for bit (the f64 values viewed as u64) and every size exactly: no tolerance anywhere in this file."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TABLES = ("exon", "intron", "donor_t", "donor_f", "acceptor_t", "acceptor_f", "donor_pw", "acceptor_pw")
ORACLE_SIZES = ("exon_size", "intron_size", "donor_pw_size", "acceptor_pw_size")
SEG = 4096  # MARKOV_SEG of pjb_markov.hip.h: the segment a wavefront takes
POS, NEG = 0, 1  # PJB_STRAND_*
G0_LEN, G1_LEN = 150_000, 5_000


@pytest.fixture(scope="module")
def ffi():
    from portcullis_amd import ffi as f
    assert f.device_count() >= 1
    return f


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle as o
    return o


def random_genome(rng, n):
    return bytearray(b"ACGT"[k] for k in rng.integers(0, 4, n))


@pytest.fixture(scope="module")
def genomes():
    rng = np.random.default_rng(20260101)
    g0 = random_genome(rng, G0_LEN)
    g0[1000:1040] = b"N" * 40
    g0[70000:70003] = b"RYK"
    g0[90000:90300] = bytes(g0[90000:90300]).lower()
    return [bytes(g0), bytes(random_genome(rng, G1_LEN))]


def make_rows(ffi, juncs):
    """juncs: (refid, start, end, strand).  The other fields are what a feature row needs to be finite."""
    rows = np.zeros(len(juncs), dtype=ffi.ROW_DTYPE)
    for k, (refid, start, end, strand) in enumerate(juncs):
        rows[k]["refid"], rows[k]["start"], rows[k]["end"], rows[k]["cons_strand"] = refid, start, end, strand
    rows["left"], rows["right"] = rows["start"] - 30, rows["end"] + 30
    rows["nb_raw"], rows["nb_dist"], rows["nb_rel"], rows["max_min_anc"], rows["maxmmes"] = 7, 5, 4, 20, 18
    rows["entropy"], rows["hamming5p"], rows["hamming3p"] = 1.5, 6, 7
    rows["jad"] = 3
    return rows


def oracle_rows(orc, rows):
    out = np.zeros(len(rows), dtype=orc.ROW_DTYPE)  # (the oracle's row is wider than the device's: field by field)
    for name in set(orc.ROW_DTYPE.names) & set(rows.dtype.names):
        out[name] = rows[name]
    return out


def oracle_models(orc, genomes, rows, cp, pas, fail):
    """the oracle's models over the listed rows (the rows no list names are left out: the oracle also scores every row it is given)"""
    used = sorted(set(map(int, cp)) | set(map(int, pas)) | set(map(int, fail)))
    remap = {k: i for i, k in enumerate(used)}
    sub = rows[used] if used else rows[:0]
    F, models, _ = orc.filt_features([len(g) for g in genomes], dict(enumerate(genomes)), oracle_rows(orc, sub), [],
                                     [remap[int(k)] for k in cp], [remap[int(k)] for k in pas], [remap[int(k)] for k in fail])
    return models, F


def assert_same_models(got, want):
    for name in TABLES:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.shape == w.shape, name
        diff = np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))
        assert diff.size == 0, (name, int(diff[0]), float(g[diff[0]]), float(w[diff[0]]), diff.size)
        # the size of every table: the rows that were trained (the oracle reports four of them itself)
        assert got[name + "_size"] == int((w.reshape(-1, 5).sum(axis=1) > 0).sum()), name
    for k in ORACLE_SIZES:
        assert got[k] == want[k], (k, got[k], want[k])


@pytest.fixture(scope="module")
def ctx(ffi, genomes):
    with ffi.Context(0, "UNKNOWN") as c:
        c.set_refs([len(g) for g in genomes])
        for t, g in enumerate(genomes):
            c.upload_contig(t, g)
        yield c


@pytest.fixture(scope="module")
def world(ffi, orc, genomes):
    rng = np.random.default_rng(7)
    juncs = []
    for k, n in enumerate((65_539, 65_542, 65_543, 7, 6, 1, 4_096, 4_097, 300, 301)):
        start = 2_000 + 997 * k
        juncs.append((0, start, start + n - 1, k & 1))
    juncs.append((0, 100, 400, POS))                                  # the exon window before it is clamped at 0
    juncs.append((0, G0_LEN - 51 - 500, G0_LEN - 51, NEG))            # ... and the one behind this at the contig's end
    for k in range(200):
        tid = int(rng.integers(0, 2))
        n = int(rng.integers(20, 3_001))
        start = int(rng.integers(0, (G0_LEN, G1_LEN)[tid] - n))
        juncs.append((tid, start, start + n - 1, int(rng.integers(0, 2))))
    rows = make_rows(ffi, juncs)
    idx = np.arange(len(rows))
    even, odd = idx[::2], idx[1::2]
    models, _ = oracle_models(orc, genomes, rows, even, even, odd)
    return dict(rows=rows, even=even, odd=odd, models=models)


def test_whole_world(ctx, world):
    got = ctx.markov_train(world["rows"], world["even"], world["even"], world["odd"])
    assert_same_models(got, world["models"])
    assert got["exon_size"] > 100 and got["intron_size"] > 1000 and got["donor_pw_size"] == 23 and got["acceptor_pw_size"] == 23
    assert got["transitions"] > 65_543


def test_the_world_shows_the_16_bit_gate(orc, genomes, world):
    """the world can tell a gated intron from a counted one: without the 65 539-base intron the intron table is the same, without the
    65 543-base one it is not (rows 0 and 2, both in `cp`)"""
    rows, even = world["rows"], world["even"]
    without = lambda r: oracle_models(orc, genomes, rows, even[even != r], [], [])[0]["intron"].view(np.uint64)
    whole = oracle_models(orc, genomes, rows, even, [], [])[0]["intron"].view(np.uint64)
    assert np.array_equal(without(0), whole) and not np.array_equal(without(2), whole)


GATE = [0, 1, 5, 6, 7, 8, 65_535, 65_536, 65_541, 65_542, 65_543, 131_078, 131_079]
EDGES = sorted({n for s in (64, 256, 1_024, 4_096, 16_384, SEG) for n in (s - 1, s, s + 1, 2 * s + 5)})


@pytest.mark.parametrize("strand", [POS, NEG])
@pytest.mark.parametrize("n", GATE + [n for n in EDGES if n not in GATE])
def test_lone_junction(ffi, orc, ctx, genomes, n, strand):
    """one positive junction with an intron of n bases (n = 0: end = start - 1): the 16-bit length gate, and the segments' edges"""
    rows = make_rows(ffi, [(0, 1_500, 1_500 + n - 1, strand)])
    got = ctx.markov_train(rows, [0], [0], [])
    want, _ = oracle_models(orc, genomes, rows, [0], [0], [])
    assert_same_models(got, want)
    trains = (n if n > 0 else 1) % 65_536 > 6        # (an intron of 0 bases is fetched as one base: faidx_fetch_seq's clamp)
    assert (got["intron_size"] > 0) == trains
    assert got["donor_f_size"] == 0 and got["acceptor_f_size"] == 0 and got["exon_size"] > 0


def test_contended_counters(ffi, orc):
    """a 100 000-base poly-A stretch as one intron: every lane of every wavefront adds to the same counter"""
    rng = np.random.default_rng(3)
    g = bytes(random_genome(rng, 1_000)) + b"A" * 100_000 + bytes(random_genome(rng, 1_000))
    rows = make_rows(ffi, [(0, 1_000, 100_999, POS)])
    with ffi.Context(0, "UNKNOWN") as c:
        c.set_refs([len(g)])
        c.upload_contig(0, g)
        got = c.markov_train(rows, [0], [], [])
    assert got["intron_size"] == 1 and got["intron"][0] == 1.0 and np.count_nonzero(got["intron"]) == 1   # intron[AAAAA][A]
    assert got["transitions"] == 100_000 - 5 + 2 * (201 - 5)
    want, _ = oracle_models(orc, [g], rows, [0], [], [])
    assert_same_models(got, want)


def test_empty_lists(orc, ctx, genomes, world):
    rows, even, odd = world["rows"], world["even"], world["odd"]
    zero = lambda m, names: all(m[n + "_size"] == 0 and not m[n].any() for n in names)
    m = ctx.markov_train(rows, [], even, odd)
    assert zero(m, ("exon", "intron")) and m["donor_t_size"] > 0 and m["donor_f_size"] > 0
    assert_same_models(m, oracle_models(orc, genomes, rows, [], even, odd)[0])
    m = ctx.markov_train(rows, even, even, [])
    assert zero(m, ("donor_f", "acceptor_f")) and m["donor_t_size"] > 0 and m["exon_size"] > 0
    assert_same_models(m, oracle_models(orc, genomes, rows, even, even, [])[0])
    m = ctx.markov_train(rows, [], [], [])
    assert zero(m, TABLES) and m["transitions"] == 0
    m = ctx.markov_train(rows[:0], [], [], [])
    assert zero(m, TABLES)


def test_an_index_listed_twice_counts_twice(orc, ctx, genomes, world):
    rows = world["rows"]
    cp, pas, fail = [0, 2, 2, 12, 40, 40, 40], [6, 6, 14, 15], [9, 21, 9]
    got = ctx.markov_train(rows, cp, pas, fail)
    want, _ = oracle_models(orc, genomes, rows, cp, pas, fail)
    assert_same_models(got, want)
    once, _ = oracle_models(orc, genomes, rows, sorted(set(cp)), sorted(set(pas)), sorted(set(fail)))
    assert not np.array_equal(once["intron"], want["intron"]) and not np.array_equal(once["donor_f"], want["donor_f"])


def test_refusals(ffi, genomes, world):
    rows = world["rows"]
    on_second = np.flatnonzero(rows["refid"] == 1)
    assert on_second.size
    with ffi.Context(0, "UNKNOWN") as c:
        c.set_refs([len(g) for g in genomes])
        c.upload_contig(0, genomes[0])                      # the second target's genome is not uploaded
        with pytest.raises(ffi.PjbError, match="genome was not uploaded"):
            c.markov_train(rows, [int(on_second[0])], [], [])
        with pytest.raises(ffi.PjbError, match="genome was not uploaded"):
            c.markov_train(rows, [], [int(on_second[0])], [])
        for lists in (([len(rows)], [], []), ([], [0, len(rows)], []), ([], [], [-1])):
            with pytest.raises(ffi.PjbError, match="list"):
                c.markov_train(rows, *lists)
        ok = c.markov_train(rows, np.flatnonzero(rows["refid"] == 0)[:4], [], [])   # the context still works
        assert ok["intron_size"] > 0


def test_feature_rows_from_device_models(ctx, world):
    """ctx.filt_features with the device's models is ctx.filt_features with the oracle's"""
    rows = world["rows"]
    mine = ctx.markov_train(rows, world["even"], world["even"], world["odd"])
    a = ctx.filt_features(rows, 100.0, 800, mine)
    b = ctx.filt_features(rows, 100.0, 800, world["models"])
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert (a[:, 11] != 0).any() and (a[:, 12] != 0).any() and (a[:, 13] != 0).any() and (a[:, 9] > 0).any()
