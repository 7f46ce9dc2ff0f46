"""The CSI built on the device (pjb_index_begin_csi / _piece / _end_csi through ffi.Context.index_bam(csi_depth=...)) against
tests/csi_model.py, which tests/test_csi_model.py holds to htslib.  Inflated payloads are compared byte for byte."""
import struct

import pytest

import csi_model as cm
import index_model as im
from portcullis_amd import ffi
from util_bam import write_bam

pytestmark = pytest.mark.gpu

BLOCK_SIZES = [0xFF00, 4096, 777]
N_MIXED = len(im.MIXED_REFS)


@pytest.fixture(scope="module")
def ctx():
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as c:
        yield c


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    d = tmp_path_factory.mktemp("csi_mixed")
    reads = im.mixed_reads()
    out = {}
    for bs in BLOCK_SIZES:
        out[bs] = str(d / f"m{bs}.bam")
        write_bam(out[bs], im.MIXED_REFS, reads, block_size=bs, write_index=False)
    return out


@pytest.fixture(scope="module")
def mixed_want(mixed):
    """{(block size, depth): the model's payload}; depth None is the model's own choice."""
    return {(bs, d): cm.payload_of(mixed[bs], d) for bs in BLOCK_SIZES for d in (None, 0, 5, 6)}


@pytest.fixture(scope="module")
def long_bam(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("csi_long") / "long.bam")
    cm.write_bam_long(p, cm.LONG_REFS, cm.long_reads(), block_size=cm.LONG_BLOCK)
    return p


def device_csi(ctx, path_or_bytes, n_ref, depth, piece_blocks=None):
    res = ctx.index_bam(path_or_bytes, piece_blocks, csi_depth=depth)
    assert res["min_shift"] == 14
    return cm.serialise_result(n_ref, res), res


# ---- 1. the mixed input: block sizes, depths, cuts
@pytest.mark.parametrize("depth", [-1, 0, 5, 6])
@pytest.mark.parametrize("block_size", BLOCK_SIZES)
def test_payload_equals_the_model(ctx, mixed, mixed_want, block_size, depth):
    got, res = device_csi(ctx, mixed[block_size], N_MIXED, depth)
    assert res["n_records"] == len(im.mixed_reads())
    assert res["depth"] == (3 if depth < 0 else depth)
    assert got == mixed_want[block_size, None if depth < 0 else depth]
    _, _, per_target, rest = cm.parse(got)
    assert rest == b""
    if depth != 0:
        assert len({cm.level_of(b) for b in per_target[0][0]}) >= 3


@pytest.mark.parametrize("depth", [-1, 0, 5, 6])
def test_the_cut_does_not_matter(ctx, mixed, mixed_want, depth):
    data = open(mixed[777], "rb").read()
    want = mixed_want[777, None if depth < 0 else depth]
    for piece_blocks in (None, 64, 3, 7):
        got, res = device_csi(ctx, data, N_MIXED, depth, piece_blocks)
        assert got == want, piece_blocks
        assert res["n_records"] == len(im.mixed_reads())


@pytest.mark.parametrize("block_size", BLOCK_SIZES)
def test_depth_5_has_the_chunks_of_the_bai(ctx, mixed, block_size):
    bai = ctx.index_bam(mixed[block_size])["chunks"].copy()
    csi = ctx.index_bam(mixed[block_size], csi_depth=5)["chunks"]
    assert len(bai) > 100 and bai.tobytes() == csi.tobytes()


# ---- 2. runs across thread, wavefront and block boundaries
def test_runs_of_every_length(ctx, tmp_path):
    reads = im.run_reads()
    p = str(tmp_path / "r.bam")
    write_bam(p, [("one", 1_000_000)], reads, write_index=False)
    want = cm.payload_of(p)
    assert cm.parse(want)[1] == 2
    for piece_blocks in (None, 5):
        got, res = device_csi(ctx, p, 1, -1, piece_blocks)
        assert res["n_records"] == len(reads) and res["depth"] == 2
        assert got == want, piece_blocks


# ---- 3. a target past 2^30
def test_the_long_target(ctx, long_bam, tmp_path):
    want = cm.payload_of(long_bam)
    n_ref, depth, bins, loff, recs = cm.build(long_bam)
    assert depth == 6
    for piece_blocks in (None, 3):
        got, res = device_csi(ctx, long_bam, 2, -1, piece_blocks)
        assert res["depth"] == 6 and res["n_records"] == len(recs)
        assert got == want, piece_blocks
    # loffset by value, from the records: bin 0 starts at window 0, which no record touches before the target's first one;
    # the first level-6 bin behind 2^29 has the offset of the first record that overlaps its 16 kb
    _, _, per_target, _ = cm.parse(got)
    mine = [(pos, end, vs) for tid, pos, end, vs in recs if tid == 0]
    assert per_target[0][0][0][0] == mine[0][2]
    b = min(b for b in per_target[0][0] if b >= cm.level_first(6) + (2**29 >> 14))
    w = b - cm.level_first(6)
    assert per_target[0][0][b][0] == next(vs for pos, end, vs in mine if pos >> 14 <= w <= (end - 1) >> 14)
    assert {cm.level_of(x) for x in per_target[0][0]} >= {0, 3, 4, 5, 6}
    # htslib loads it and answers as the records say
    f = str(tmp_path / "long.csi")
    open(f, "wb").write(cm.container(got))
    regions = cm.long_regions()
    assert len(regions) == 612
    total = 0
    for (reg, hits), w in zip(cm.witness_query(long_bam, f, regions), cm.brute_force(recs, regions)):
        assert [(p, e) for p, e, _ in hits] == w, reg
        total += len(w)
    assert total > 50_000


# ---- 4. what untouched leading windows take
def gap_reads():
    reads = []
    base = 43 * 16384  # the first record of "a" lies in window 43; the 128 kb bin above it starts at window 40
    for k in range(300):
        reads.append(dict(tid=0, pos=base + 5 + 40 * k, cigar="30M", seq="A" * 30))
    for k in range(40):  # across the 43 | 44 boundary, and across 47 | 48 into the 1 Mb bin that starts at window 0
        reads.append(dict(tid=0, pos=base + 16_000 + 3 * k, cigar="20M600N20M", seq="A" * 40))
    for k in range(40):
        reads.append(dict(tid=0, pos=48 * 16384 - 300 + 3 * k, cigar="20M600N20M", seq="A" * 40))
    for k in range(200):
        reads.append(dict(tid=0, pos=90 * 16384 + 100 * k, cigar="30M", seq="A" * 30))
    reads.sort(key=lambda r: r["pos"])
    for k in range(215):  # "c": from window 2 on, with reads across 2 | 3
        reads.append(dict(tid=2, pos=2 * 16384 + 10 + 81 * k, cigar="25M100N25M", seq="A" * 50))
    return [("a", 2_000_000), ("gap", 100_000), ("c", 500_000)], reads


@pytest.mark.parametrize("depth", [-1, 5])
def test_leading_windows_take_the_first_record(ctx, tmp_path, depth):
    refs, reads = gap_reads()
    p = str(tmp_path / "g.bam")
    write_bam(p, refs, reads, block_size=1500, write_index=False)
    n_ref, d, bins, loff, recs = cm.build(p, None if depth < 0 else depth)
    first = {t: next(vs for tid, _, _, vs in recs if tid == t) for t in (0, 2)}
    # the model's own answer has the case in it: bins whose first window lies before every record
    assert sum(v == first[0] for v in loff[0].values()) >= 3 and sum(v == first[2] for v in loff[2].values()) >= 2
    assert bins[1] == {}
    for piece_blocks in (None, 4):
        got, _ = device_csi(ctx, p, 3, depth, piece_blocks)
        assert got == cm.serialise(n_ref, d, bins, loff), piece_blocks


# ---- 5. errors
def expect_error(call, code, text=""):
    with pytest.raises(ffi.PjbError) as e:
        call()
    assert e.value.code == code, str(e.value)
    assert text in str(e.value), str(e.value)


def test_depths_that_cannot_be(ctx):
    ctx.set_refs([2**29])
    expect_error(lambda: ctx.index_begin(5), -16)
    ctx.index_begin(6)
    ctx.index_begin(-1)
    ctx.set_refs([1000])
    expect_error(lambda: ctx.index_begin(7), -16)


def test_the_ends_do_not_cross(ctx, mixed):
    data = open(mixed[0xFF00], "rb").read()
    ref_lens, header_bytes = ffi.bam_header(data)
    ctx.set_refs(ref_lens)
    ctx.index_begin(5)
    ctx.index_piece(data, 0, header_bytes, True)
    expect_error(ctx.index_end, -19)
    ctx.index_begin()
    ctx.index_piece(data, 0, header_bytes, True)
    expect_error(ctx.index_end_csi, -19)


@pytest.mark.parametrize("piece_blocks", [None, 2])
def test_unsorted_is_refused_as_in_bai_mode(ctx, tmp_path, piece_blocks):
    from test_gpu_bam_index import small_sorted

    refs, reads = small_sorted()
    moved = list(reads)
    moved[301], moved[300] = moved[300], moved[301]
    p = str(tmp_path / "u.bam")
    write_bam(p, refs, moved, block_size=4096, write_index=False)
    data = open(p, "rb").read()
    texts = []
    for depth in (None, -1, 6):
        with pytest.raises(ffi.PjbError) as e:
            ctx.index_bam(data, piece_blocks, csi_depth=depth)
        assert e.value.code == -14
        texts.append(str(e.value))
    assert "alignment record 301 lies before its predecessor" in texts[0]
    assert texts[1] == texts[0] and texts[2] == texts[0]


def test_a_bai_of_the_long_input_is_still_refused(ctx, long_bam):
    expect_error(lambda: ctx.index_bam(long_bam), -16, "BAI cannot index this target")


# ---- 6. empty and degenerate inputs
def test_degenerate_inputs(ctx, tmp_path):
    from test_index_model import record_ending_on_a_block_end

    refs = [("a", 1000)]
    for name, reads in (("none", []), ("unplaced", [dict(tid=-1, pos=-1, cigar="", seq="ACGT")] * 3)):
        p = str(tmp_path / (name + ".bam"))
        write_bam(p, refs, reads, write_index=False)
        got, res = device_csi(ctx, p, 1, -1)
        assert got == cm.payload_of(p) == b"CSI\x01" + struct.pack("<iiiii", 14, 0, 0, 1, 0), name
        assert res["n_records"] == len(reads) and len(res["chunks"]) == 0 and res["depth"] == 0
    p, _ = record_ending_on_a_block_end(tmp_path)
    for piece_blocks in (None, 1):
        for depth in (-1, 6):
            got, res = device_csi(ctx, p, 1, depth, piece_blocks)
            assert got == cm.payload_of(p, None if depth < 0 else depth)
            assert res["chunks"][0]["vend"] == ffi.bgzf_block_starts(open(p, "rb").read())[-2] << 16  # the EOF block's start
