"""The BAM index built on the device (pjb_index_begin / _piece / _end through ffi.Context.index_bam) against the Python
restatement of tests/index_model.py and the bytes write_bam writes while it builds the file."""
import os

import numpy as np
import pytest

import index_model as im
from portcullis_amd import ffi
from util_bam import write_bam

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK_SIZES = [0xFF00, 4096, 777]


@pytest.fixture(scope="module")
def ctx():
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as c:
        yield c


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """{block size: path} of the mixed input, each with the .bai write_bam wrote beside it."""
    d = tmp_path_factory.mktemp("mixed")
    reads = im.mixed_reads()
    out = {}
    for bs in BLOCK_SIZES:
        out[bs] = str(d / f"m{bs}.bam")
        write_bam(out[bs], im.MIXED_REFS, reads, block_size=bs)
    return out


def device_bai(ctx, path_or_bytes, n_ref, piece_blocks=None):
    res = ctx.index_bam(path_or_bytes, piece_blocks)
    return im.serialise_result(n_ref, res), res


def level_of(b):
    return next(l for l, first in ((5, 4681), (4, 585), (3, 73), (2, 9), (1, 1), (0, 0)) if b >= first)


# ---- 1. bytes equal the model
@pytest.mark.parametrize("block_size", BLOCK_SIZES)
def test_bytes_equal_write_bam(ctx, mixed, block_size):
    p = mixed[block_size]
    want = open(p + ".bai", "rb").read()
    got, res = device_bai(ctx, p, len(im.MIXED_REFS))
    assert res["n_records"] == len(im.mixed_reads())
    assert got == want
    per_target, _ = im.parse_bai(got)
    bins = per_target[0][0]
    assert len({level_of(b) for b in bins}) >= 4
    assert sum(len(c) > 1 for c in bins.values()) > 10


@pytest.mark.parametrize("seg", [1, 2, 5])
def test_false_record_start_is_repaired(mixed, monkeypatch, seg):
    """The indexer's record walk repairs a guessed start that is not a boundary (the PJB_TEST_FALSE_START hook moves the start
    of one 64 KB segment by a byte), as the ingest's does: in one piece the input is 14 segments, and the index is the same."""
    p = mixed[0xFF00]
    monkeypatch.setenv("PJB_TEST_FALSE_START", str(seg))
    with ffi.Context(flags=ffi.FLAG_KERNEL_TIMING | ffi.FLAG_NO_CHAINS) as c:
        got, res = device_bai(c, p, len(im.MIXED_REFS), None)
        assert "bam_repair_start" in c.kernel_timing()  # (the hook was not inert)
    assert got == open(p + ".bai", "rb").read()
    assert res["n_records"] == len(im.mixed_reads())


# ---- 2. the cut does not matter
def test_the_cut_does_not_matter(ctx, mixed):
    p = mixed[777]
    data = open(p, "rb").read()
    starts = ffi.bgzf_block_starts(data)
    assert len(starts) - 1 > 1000
    eof_start = starts[-2]
    want = open(p + ".bai", "rb").read()
    straddled = 0
    for piece_blocks in (None, 64, 3, 7):
        got, res = device_bai(ctx, data, len(im.MIXED_REFS), piece_blocks)
        assert got == want, piece_blocks
        nvs = res["next_voffsets"]
        assert nvs[-1] == eof_start << 16, piece_blocks
        straddled += sum(1 for nv in nvs[:-1] if nv & 0xFFFF)
    # (records are ~150 bytes and blocks 777: most cuts fall inside a record, which then starts the next piece's first block)
    assert straddled > 100


# ---- 3. runs across thread, wavefront and block boundaries
def test_runs_of_every_length(ctx, tmp_path):
    reads = im.run_reads()
    p = str(tmp_path / "r.bam")
    write_bam(p, [("one", 1_000_000)], reads)
    want = open(p + ".bai", "rb").read()
    assert im.index_of(p) == want
    for piece_blocks in (None, 5):
        got, res = device_bai(ctx, p, 1, piece_blocks)
        assert res["n_records"] == len(reads)
        assert got == want, piece_blocks


# ---- 4. empty and degenerate inputs
def test_degenerate_inputs(ctx, tmp_path):
    from test_index_model import record_ending_on_a_block_end

    refs = [("a", 1000)]
    for name, reads in (("none", []), ("unplaced", [dict(tid=-1, pos=-1, cigar="", seq="ACGT")] * 3)):
        p = str(tmp_path / (name + ".bam"))
        write_bam(p, refs, reads)
        got, res = device_bai(ctx, p, 1)
        assert got == open(p + ".bai", "rb").read() == im.index_of(p), name
        assert res["n_records"] == len(reads) and len(res["chunks"]) == 0
    p, _ = record_ending_on_a_block_end(tmp_path)
    for piece_blocks in (None, 1):
        got, res = device_bai(ctx, p, 1, piece_blocks)
        assert got == open(p + ".bai", "rb").read() == im.index_of(p)
        assert res["chunks"][0]["vend"] == ffi.bgzf_block_starts(open(p, "rb").read())[-2] << 16  # the EOF block's start


# ---- 5. errors
def small_sorted(n=400):
    reads = [dict(tid=0, pos=10 + 7 * k, cigar="20M", seq="ACGTACGTACGTACGTACGT") for k in range(n)]
    reads += [dict(tid=1, pos=5 + 3 * k, cigar="20M", seq="ACGTACGTACGTACGTACGT") for k in range(n)]
    return [("a", 50_000), ("b", 50_000)], reads


def expect_error(ctx, code, text, data, piece_blocks=None):
    with pytest.raises(ffi.PjbError) as e:
        ctx.index_bam(data, piece_blocks)
    assert e.value.code == code, str(e.value)
    assert text in str(e.value), str(e.value)


@pytest.mark.parametrize("piece_blocks", [None, 2])
def test_unsorted_is_refused_with_the_ordinal(ctx, tmp_path, piece_blocks):
    refs, reads = small_sorted()
    # one record moved before its predecessor
    moved = list(reads)
    moved[301], moved[300] = moved[300], moved[301]
    p = str(tmp_path / "u1.bam")
    write_bam(p, refs, moved, block_size=4096, write_index=False)
    expect_error(ctx, -14, "alignment record 301 lies before its predecessor", open(p, "rb").read(), piece_blocks)
    # a target change backwards
    back = reads[:450] + [dict(reads[0])] + reads[450:]
    write_bam(p, refs, back, block_size=4096, write_index=False)
    expect_error(ctx, -14, "alignment record 450 lies before its predecessor", open(p, "rb").read(), piece_blocks)


def test_the_unsorted_fixture_is_refused(ctx):
    p = os.path.join(GOLDEN, "unsorted.bam")
    recs = [(tid, pos) for tid, pos, _, _ in im.build(p)[3]]
    first = next(k for k in range(1, len(recs)) if (recs[k][0] & 0xFFFFFFFF, recs[k][1]) < (recs[k - 1][0] & 0xFFFFFFFF, recs[k - 1][1]))
    expect_error(ctx, -14, f"alignment record {first} lies before its predecessor", open(p, "rb").read())


def test_data_that_ends_inside_a_record(ctx, tmp_path):
    refs, reads = small_sorted()
    p = str(tmp_path / "t.bam")
    write_bam(p, refs, reads, block_size=777, write_index=False)
    data = open(p, "rb").read()
    starts = ffi.bgzf_block_starts(data)
    ref_lens, header_bytes = ffi.bam_header(data, starts)
    ctx.set_refs(ref_lens)
    ctx.index_begin()
    nv = ctx.index_piece(data[:starts[10]], 0, header_bytes, False)  # not the last: the cut record is the next piece's
    assert nv & 0xFFFF and nv >> 16 == starts[9]
    ctx.index_begin()
    with pytest.raises(ffi.PjbError) as e:
        ctx.index_piece(data[:starts[10]], 0, header_bytes, True)
    assert e.value.code == -22 and "ends inside an alignment record" in str(e.value)


def test_a_target_beyond_the_table(ctx, tmp_path):
    refs, reads = small_sorted()
    p = str(tmp_path / "b.bam")
    write_bam(p, refs, reads, write_index=False)
    data = open(p, "rb").read()
    _, header_bytes = ffi.bam_header(data)
    ctx.set_refs([50_000])  # the file's second target is not in the table
    ctx.index_begin()
    with pytest.raises(ffi.PjbError) as e:
        ctx.index_piece(data, 0, header_bytes, True)
    assert e.value.code == -22, str(e.value)


def test_calls_out_of_order(tmp_path):
    refs, reads = small_sorted(10)
    p = str(tmp_path / "o.bam")
    write_bam(p, refs, reads, write_index=False)
    data = open(p, "rb").read()
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as c:
        c.set_refs([50_000, 50_000])
        for call in (lambda: c.index_piece(data, 0, 0, True), c.index_end):
            with pytest.raises(ffi.PjbError) as e:
                call()
            assert e.value.code == -19, str(e.value)
        c.index_begin()
        with pytest.raises(ffi.PjbError) as e:
            c.index_end()  # no last piece yet
        assert e.value.code == -19


def test_a_record_longer_than_a_piece(ctx, tmp_path):
    refs = [("a", 50_000)]
    reads = [dict(tid=0, pos=5, cigar="3000M", seq="ACGT" * 750)]
    p = str(tmp_path / "l.bam")
    write_bam(p, refs, reads, block_size=777, write_index=False)
    expect_error(ctx, -16, "longer than the piece", open(p, "rb").read(), 2)
    got, _ = device_bai(ctx, p, 1, 64)
    assert got == im.index_of(p)


# ---- 6. the reference's fixtures, against the indexes samtools wrote
@pytest.mark.parametrize("name", ["sorted.bam", "clipped3.bam"])
def test_against_the_samtools_indexes(ctx, name):
    from test_index_model import assert_same_where_it_counts

    p = os.path.join(GOLDEN, name)
    n_ref = len(ffi.bam_header(open(p, "rb").read())[0])
    got, _ = device_bai(ctx, p, n_ref)
    assert got == im.index_of(p)
    ours, _ = im.parse_bai(got)
    theirs, _ = im.parse_bai(open(p + ".bai", "rb").read())
    assert_same_where_it_counts(ours, theirs, im.build(p)[3])


# ---- 7. query completeness on the produced bytes
def test_a_lookup_finds_every_overlapping_record(ctx, mixed):
    p = mixed[4096]
    got, _ = device_bai(ctx, p, len(im.MIXED_REFS), 50)
    per_target, _ = im.parse_bai(got)
    records = im.build(p)[3]
    rng = np.random.default_rng(5)
    for t, (_, length) in enumerate(im.MIXED_REFS):
        bins, lin, _ = per_target[t]
        mine = [(pos, end, vs) for tid, pos, end, vs in records if tid == t]
        for _ in range(200):
            beg = int(rng.integers(0, length))
            end = min(length, beg + int(rng.choice([1, 50, 2_000, 40_000, 400_000])))
            w = beg >> 14
            min_off = lin[w] if w < len(lin) else (lin[-1] if lin else 0)
            ranges = [(vs, ve) for b in im.reg2bins(beg, end) for vs, ve in bins.get(b, []) if ve > min_off]
            for pos, rend, vs in mine:
                if pos < end and rend > beg:
                    assert any(a <= vs < e for a, e in ranges), (t, beg, end, pos, rend)
