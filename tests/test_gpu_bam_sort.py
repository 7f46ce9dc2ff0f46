"""An unsorted file's records put in coordinate order on the device (pjb_bam_sort_begin / _piece / _end through
ffi.Context.bam_sort) against the model: sorted(reads, key=merge_model.merge_key), Python's stable sort by (refID as unsigned,
pos).  The members are inflated with zlib, concatenated and compared byte for byte with the stream the model's order gives."""
import os
import re

import numpy as np
import pytest

import merge_model as mm
from fuzzgen import make_reads
from portcullis_amd import ffi
from util_bam import bam_header, write_bam, write_bgzf

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_BGZF = -16, -19, -22


@pytest.fixture(scope="module")
def ctx():
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as c:
        yield c


@pytest.fixture(scope="module")
def scratch(tmp_path_factory):
    return str(tmp_path_factory.mktemp("sort"))


def simple_read(tid, pos, name, l=20, aux=b""):
    return dict(tid=tid, pos=pos, cigar=f"{l}M", seq="ACGT" * (l // 4) + "A" * (l % 4), flag=0, mapq=60, xs=None, mtid=-1, mpos=-1, name=name, aux=aux)


def bam_bytes(scratch, refs, reads, src_block=0xFF00):
    path = os.path.join(scratch, "in.bam")
    write_bam(path, refs, reads, block_size=src_block, write_index=False)
    return open(path, "rb").read()


def check(res, reads, block_bytes=0xFF00):
    """A result against the model; returns the model's list."""
    want_reads = sorted(reads, key=mm.merge_key)
    want = mm.record_stream(want_reads)
    assert res["n_records"] == len(reads)
    assert res["n_unplaced"] == sum(1 for r in reads if r["tid"] == -1)
    assert res["raw_bytes"] == len(want)
    parts = mm.inflate_members(res["members"], res["member_size"])
    assert len(parts) == (len(want) + block_bytes - 1) // block_bytes
    assert all(len(p) == block_bytes for p in parts[:-1])  # every member but the last is cut at block_bytes
    assert not parts or 0 < len(parts[-1]) <= block_bytes
    got = b"".join(parts)
    if got != want:
        k = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else min(len(got), len(want))
        raise AssertionError(f"sorted stream differs from the model at byte {k} of {len(want)} (got {len(got)})")
    in_order = [mm.merge_key(r) for r in reads] == [mm.merge_key(r) for r in want_reads]
    assert res["was_sorted"] == int(in_order)
    return want_reads


def sort(ctx, scratch, refs, reads, piece_blocks=None, block_bytes=0xFF00, src_block=0xFF00):
    res = ctx.bam_sort(bam_bytes(scratch, refs, reads, src_block), piece_blocks, block_bytes)
    return res, check(res, reads, block_bytes)


# ---- 1. several targets, records that straddle blocks, pieces of every size
@pytest.fixture(scope="module")
def shuffled_case():
    genome, reads = make_reads(41, n_reads=2000, paired=True)
    refs = [("chr0", len(genome) + 7), ("chr1", len(genome)), ("chr2", len(genome) + 300)]
    rng = np.random.default_rng(17)
    for k, r in enumerate(reads):
        r["tid"] = int(rng.integers(0, 3))
        r["mtid"] = r["tid"] if r.get("mtid", -1) >= 0 else -1
        r["name"] = f"q{k}" + "x" * (k % 7)
    reads += [dict(simple_read(-1, -1, f"un{k}", l=20 + k % 9), flag=4) for k in range(50)]
    reads = [reads[k] for k in rng.permutation(len(reads))]
    return refs, reads


@pytest.mark.parametrize("piece_blocks", [1, 3, None])
def test_several_targets_whatever_the_pieces(ctx, scratch, shuffled_case, piece_blocks):
    refs, reads = shuffled_case
    assert 2000 <= len(reads) <= 2100
    res, want = sort(ctx, scratch, refs, reads, piece_blocks, block_bytes=4096, src_block=512)
    assert res["n_records"] == len(reads) and res["n_unplaced"] == 50 and res["was_sorted"] == 0
    assert all(r["tid"] == -1 for r in want[-50:])
    assert res["pieces"] == 1 if piece_blocks is None else res["pieces"] > 50


# ---- 2. ties keep the input order, among placed and among unplaced records
def test_stability(ctx, scratch):
    refs = [("chr1", 5000)]
    rng = np.random.default_rng(2)
    reads = []
    for k in range(600):
        if k % 5 == 4:
            reads.append(dict(simple_read(-1, -1, f"u{k}", l=20 + k % 11), flag=4))
        else:
            reads.append(simple_read(0, int(rng.choice([7, 8, 900, 4999])), f"s{k}" + "y" * (k % 3), l=20 + k % 13))
    res, want = sort(ctx, scratch, refs, reads, piece_blocks=4, block_bytes=1024, src_block=2048)
    assert len({r["name"] for r in reads}) == 600 and res["was_sorted"] == 0
    at = {r["name"]: k for k, r in enumerate(reads)}
    for a, b in zip(want, want[1:]):
        if mm.merge_key(a) == mm.merge_key(b):
            assert at[a["name"]] < at[b["name"]]


# ---- 3. input that is in order already
def test_sorted_input_is_the_identity(ctx, scratch):
    refs = [("chr1", 20000), ("chr2", 700)]
    reads = [simple_read(0, k * 66, f"id{k}" + "x" * (k % 5), l=20 + k % 31) for k in range(300)]
    reads += [simple_read(1, 7 * k, f"other{k}") for k in range(20)] + [dict(simple_read(-1, -1, f"u{k}"), flag=4) for k in range(5)]
    res, want = sort(ctx, scratch, refs, reads, piece_blocks=2, src_block=4096)
    assert res["was_sorted"] == 1 and [id(r) for r in want] == [id(r) for r in reads]
    res, _ = sort(ctx, scratch, refs, reads[:1])
    assert res["was_sorted"] == 1 and res["n_records"] == 1
    res, _ = sort(ctx, scratch, refs, [])
    assert res["was_sorted"] == 1 and res["n_records"] == 0 and res["raw_bytes"] == 0 and len(res["member_size"]) == 0 and res["members"] == b""


# ---- 4. the key's width: 32-bit keys, 64-bit keys, and the edge between them
def occupied_bits(refs):
    longest = max(l for _, l in refs)
    return (longest - 1).bit_length() + len(refs).bit_length()


def edge_reads(refs, rng, n_extra=40):
    """Records at pos 0, 1, 2^28 (where the target has it) and len - 1 of the first and the last target, more in between, some
    unplaced: shuffled."""
    reads = []
    for t in (0, len(refs) - 1):
        ln = refs[t][1]
        for p in (0, 1, 1 << 28, ln - 1):
            if p < ln:
                reads.append(simple_read(t, p, f"e{t}_{p}"))
    for k in range(n_extra):
        t = int(rng.integers(0, len(refs)))
        reads.append(simple_read(t, int(rng.integers(0, refs[t][1])), f"x{k}", l=20 + k % 17))
    reads += [dict(simple_read(-1, -1, f"u{k}"), flag=4) for k in range(6)]
    return [reads[k] for k in rng.permutation(len(reads))]


@pytest.mark.parametrize("lens, bits", [([300, 5000], 15), ([(1 << 29) - 1] * 20, 34), ([(1 << 29) - 1] * 7, 32), ([(1 << 29) - 1] * 8, 33)])
def test_key_width(ctx, scratch, lens, bits):
    refs = [(f"t{k}", l) for k, l in enumerate(lens)]
    assert occupied_bits(refs) == bits
    reads = edge_reads(refs, np.random.default_rng(bits))
    res, want = sort(ctx, scratch, refs, reads, piece_blocks=3, src_block=1024)
    assert res["was_sorted"] == 0
    if bits > 15:  # the last target's last base sorts just before the unplaced records
        assert want[-7]["tid"] == len(refs) - 1 and want[-7]["pos"] == lens[-1] - 1


# ---- 5. the gather: every combination of source and destination alignment
def test_gather_phases(ctx, scratch):
    refs = [("chr1", 100000)]
    rng = np.random.default_rng(8)
    reads = [simple_read(0, int(rng.integers(0, 100000)), "g" + "n" * int(rng.integers(0, 8)) + str(k), l=20 + int(rng.integers(0, 9))) for k in range(400)]
    src_at, at = {}, len(bam_header(refs))  # (one piece: a record's source address is the buffer's -- aligned -- plus its place in the file's stream)
    for r in reads:
        src_at[r["name"]] = at
        at += len(mm.record_bytes(r))
    phases, at = set(), 0
    for r in sorted(reads, key=mm.merge_key):
        phases.add((src_at[r["name"]] % 4, at % 4))
        at += len(mm.record_bytes(r))
    assert len(phases) == 16, sorted(phases)
    sort(ctx, scratch, refs, reads)


# ---- 6. errors: each a return code, and a fresh run works after each
def good_case(ctx, scratch):
    refs = [("chr1", 5000), ("chr2", 900)]
    sort(ctx, scratch, refs, [simple_read(1, 5, "b"), simple_read(0, 77, "a"), simple_read(0, 3, "c")])


@pytest.mark.parametrize("tid", [2, -2])
def test_refid_outside_the_header(ctx, scratch, tid):
    refs = [("chr1", 5000), ("chr2", 900)]
    reads = [simple_read(0, 10 * k, f"a{k}") for k in range(30)]
    reads[17] = simple_read(tid, 5, "bad")
    with pytest.raises(ffi.PjbError) as e:
        ctx.bam_sort(bam_bytes(scratch, refs, reads))
    assert e.value.code == ERR_BGZF and re.search(r"alignment record 17\b", str(e.value)), str(e.value)
    good_case(ctx, scratch)


def test_pos_outside_the_target(ctx, scratch):
    refs = [("chr1", 5000), ("chr2", 900)]
    reads = [simple_read(0, 10 * k, f"a{k}") for k in range(30)] + [simple_read(1, 900, "bad"), simple_read(1, 899, "fine")]
    with pytest.raises(ffi.PjbError) as e:
        ctx.bam_sort(bam_bytes(scratch, refs, reads))
    assert e.value.code == ERR_BGZF and re.search(r"alignment record 30\b", str(e.value)), str(e.value)
    good_case(ctx, scratch)
    sort(ctx, scratch, refs, reads[:30] + reads[31:])  # (len - 1 is inside)


def test_data_that_ends_inside_a_record(ctx, scratch):
    refs = [("chr1", 5000)]
    reads = [simple_read(0, 4000 - 10 * k, f"a{k}") for k in range(30)]
    stream = bam_header(refs) + mm.record_stream(reads)
    path = os.path.join(scratch, "cut.bam")
    write_bgzf(path, stream[:-9], block_size=700)
    with pytest.raises(ffi.PjbError) as e:
        ctx.bam_sort(open(path, "rb").read(), piece_blocks=2)
    assert e.value.code == ERR_BGZF and "ends inside an alignment record" in str(e.value), str(e.value)
    good_case(ctx, scratch)


def test_calls_out_of_order(ctx, scratch):
    refs = [("chr1", 5000)]
    data = bam_bytes(scratch, refs, [simple_read(0, 9, "b"), simple_read(0, 3, "a")])
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as fresh:  # a context that has never begun a run
        fresh.set_refs([5000])
        with pytest.raises(ffi.PjbError) as e:
            fresh.bam_sort_piece(data, len(bam_header(refs)), True)
        assert e.value.code == ERR_STATE
        with pytest.raises(ffi.PjbError) as e:
            fresh.bam_sort_end()
        assert e.value.code == ERR_STATE
    res = ctx.bam_sort(data)
    assert res["n_records"] == 2
    with pytest.raises(ffi.PjbError) as e:
        ctx.bam_sort_end()
    assert e.value.code == ERR_STATE
    with pytest.raises(ffi.PjbError) as e:
        ctx.bam_sort_piece(data, len(bam_header(refs)), True)
    assert e.value.code == ERR_STATE
    good_case(ctx, scratch)


def test_a_first_record_longer_than_the_piece(ctx, scratch):
    refs = [("chr1", 5000)]
    reads = [simple_read(0, 4000 - 100 * k, f"long{k}", l=120) for k in range(12)]
    data = bam_bytes(scratch, refs, reads, src_block=64)
    starts = ffi.bgzf_block_starts(data)
    head = len(bam_header(refs))
    k0, u0 = head // 64, head % 64  # the first record's block
    ctx.set_refs([5000])
    ctx.bam_sort_begin()
    with pytest.raises(ffi.PjbError) as e:
        ctx.bam_sort_piece(data[starts[k0]:starts[k0 + 1]], u0, False)
    assert e.value.code == ERR_ARG and "longer than the piece" in str(e.value), str(e.value)
    nv, n = ctx.bam_sort_piece(data[starts[k0]:], u0, True)  # the run is as it was: the same blocks with more behind them
    assert n == 12 and nv >> 16 == len(data) - starts[k0]
    check(dict(ctx.bam_sort_end(), pieces=1), reads)
    res, _ = sort(ctx, scratch, refs, reads, piece_blocks=1, src_block=64)  # bam_sort widens the piece by itself
    assert res["pieces"] >= 6


def test_block_bytes_is_checked(ctx, scratch):
    refs = [("chr1", 5000)]
    data = bam_bytes(scratch, refs, [simple_read(0, 9, "b"), simple_read(0, 3, "a")])
    for bad in (0, 6, 0xFF04):
        with pytest.raises(ffi.PjbError) as e:
            ctx.bam_sort(data, block_bytes=bad)
        assert e.value.code == ERR_ARG
    good_case(ctx, scratch)


def test_memory_is_reported_as_staging(ctx, scratch):
    refs = [("chr1", 100000)]
    reads = [simple_read(0, (k * 7919) % 100000, f"m{k}", l=100) for k in range(3000)]
    data = bam_bytes(scratch, refs, reads)
    ctx.set_refs([100000])
    ctx.bam_sort_begin()
    before = ctx.memory_info()["staging"]
    ctx.bam_sort_piece(data, len(bam_header(refs)), True)
    held = ctx.memory_info()["staging"] - before
    assert held >= len(mm.record_stream(reads)), held  # the piece's inflated bytes stay until the end
    check(dict(ctx.bam_sort_end(), pieces=1), reads)
