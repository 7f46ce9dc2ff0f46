"""Several sorted files' records of one target merged on the device (pjb_bam_merge_begin / _file / _end through
ffi.Context.bam_merge) against tests/merge_model.py: the members are inflated with zlib, concatenated and compared byte for byte
with the stream the model's order gives."""
import os
import re

import numpy as np
import pytest

import merge_model as mm
from fuzzgen import make_reads
from portcullis_amd import ffi
from util_bam import bam_header, write_bam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_UNSORTED, ERR_ARG, ERR_STATE, ERR_BGZF = -14, -16, -19, -22


def rs_tile():
    src = open(os.path.join(ROOT, "portcullis_amd", "csrc", "pjb_device.hip.h")).read()
    items = int(re.search(r"constexpr int RS_ITEMS = (\d+);", src).group(1))
    return int(re.search(r"constexpr int RS_TILE = (\d+) \* RS_ITEMS;", src).group(1)) * items


@pytest.fixture(scope="module")
def ctx():
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as c:
        yield c


@pytest.fixture(scope="module")
def scratch(tmp_path_factory):
    return str(tmp_path_factory.mktemp("merge"))


def simple_read(tid, pos, name, l=20, aux=b""):
    return dict(tid=tid, pos=pos, cigar=f"{l}M", seq="ACGT" * (l // 4) + "A" * (l % 4), flag=0, mapq=60, xs=None, mtid=-1, mpos=-1, name=name, aux=aux)


def share_of(scratch, refs, reads, tid, src_block=0xFF00):
    """(BGZF bytes, first_uoffset) of target `tid` in the BAM write_bam writes from `reads` -- what BamReader::regionSpan describes --
    or, if the file has no record on the target, of whatever follows where they would be."""
    path = os.path.join(scratch, "in.bam")
    write_bam(path, refs, reads, block_size=src_block, write_index=False)
    data = open(path, "rb").read()
    before = [r for r in reads if mm.merge_key(r) < (tid, -1)]
    return mm.span_at(data, len(bam_header(refs)) + len(mm.record_stream(before)))


def check(res, tid, files, block_bytes):
    """A result against the model: files are the inputs' read lists (None: not handed over)."""
    want_reads = mm.merge_reads([[r for r in (f or []) if r["tid"] == tid] for f in files])
    want = mm.record_stream(want_reads)
    assert res["n_records"] == len(want_reads)
    assert res["raw_bytes"] == len(want)
    parts = mm.inflate_members(res["members"], res["member_size"])  # (also: sum(member_size) == member_bytes)
    assert len(parts) == (len(want) + block_bytes - 1) // block_bytes
    assert all(len(p) == block_bytes for p in parts[:-1])
    assert not parts or 0 < len(parts[-1]) <= block_bytes
    got = b"".join(parts)
    if got != want:
        k = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else min(len(got), len(want))
        raise AssertionError(f"merged stream differs from the model at byte {k} of {len(want)} (got {len(got)})")
    return want_reads


def merge(ctx, scratch, refs, tid, files, block_bytes=0xFF00, src_block=0xFF00):
    ctx.set_refs([l for _, l in refs])
    shares = [None if f is None else share_of(scratch, refs, f, tid, src_block) for f in files]
    res = ctx.bam_merge(tid, shares, block_bytes)
    return res, check(res, tid, files, block_bytes)


def good_case(ctx, scratch):
    refs = [("chr1", 5000)]
    a = [simple_read(0, 10 * k, f"a{k}") for k in range(40)]
    b = [simple_read(0, 10 * k + 5 * (k % 2), f"b{k}") for k in range(30)]
    merge(ctx, scratch, refs, 0, [a, b])


# ---- 1. one file: the identity
def test_one_file_is_the_identity(ctx, scratch):
    refs = [("chr1", 20000), ("chr2", 700)]
    reads = [simple_read(0, k * 66, f"id{k}" + "x" * (k % 5), l=20 + k % 31) for k in range(300)]
    reads += [simple_read(1, 7 * k, f"other{k}") for k in range(20)]
    res, want = merge(ctx, scratch, refs, 0, [reads], src_block=4096)
    assert res["n_records"] == 300 and [id(r) for r in want] == [id(r) for r in reads[:300]]


# ---- 2. stable splits of make_reads
@pytest.mark.parametrize("n_files", [2, 3])
def test_split_equals_model(ctx, scratch, n_files):
    genome, reads = make_reads(11 + n_files, n_reads=1500, paired=True)
    refs = [("chr0", 900), ("chr1", len(genome)), ("chr2", 1000)]
    for k, r in enumerate(reads):
        r["tid"] = 1
        r["pos"] = r["pos"] // 50 * 50  # (monotone: still sorted; many equal positions)
        r["name"] = f"q{k}" + "x" * (k % 7)
    rng = np.random.default_rng(5)
    files = mm.stable_split(reads, n_files, rng)
    for f, rs in enumerate(files):
        for r in rs:
            r["_file"] = f
    # at least a third of the records share their position with a record of another file and with one of their own
    by_pos = {}
    for r in reads:
        by_pos.setdefault(r["pos"], []).append(r["_file"])
    both = sum(1 for r in reads if by_pos[r["pos"]].count(r["_file"]) > 1 and len(set(by_pos[r["pos"]])) > 1)
    assert 3 * both >= len(reads), (both, len(reads))
    # (records of other targets around them: the run ends at the first record of another target)
    files[0] = [simple_read(0, 5 * k, f"pre{k}") for k in range(30)] + files[0]
    files[-1] = files[-1] + [simple_read(2, 9 * k, f"post{k}") for k in range(25)]
    res, want = merge(ctx, scratch, refs, 1, files, src_block=0xFF00 if n_files == 2 else 3000)
    assert res["n_records"] == len(reads)
    assert [r["pos"] for r in want] == sorted(r["pos"] for r in reads)


# ---- 3. files without a record on the target
def test_files_with_nothing_on_the_target(ctx, scratch):
    refs = [("chr1", 5000), ("chr2", 800)]
    a = [simple_read(0, 10 * k, f"a{k}") for k in range(40)]
    only_other = [simple_read(1, 3 * k, f"o{k}") for k in range(50)]
    res, _ = merge(ctx, scratch, refs, 0, [a, None, only_other])  # not handed over | a span that starts at another target's record
    assert res["n_records"] == 40
    res, _ = merge(ctx, scratch, refs, 0, [None, only_other, a])
    assert res["n_records"] == 40
    for files in ([only_other, only_other], [None, None], [[], only_other]):
        res, _ = merge(ctx, scratch, refs, 0, files)
        assert res["n_records"] == 0 and res["raw_bytes"] == 0 and len(res["member_size"]) == 0 and res["members"] == b""


def test_a_span_that_ends_inside_the_next_targets_first_record(ctx, scratch):
    """A span ends with the block in which the next target begins; of that target's first record it may hold fewer than the 36
    fixed bytes the walk asks for.  With the refID in reach (8 bytes) the record still ends the run; with fewer nobody can tell
    whose record is cut, and the call says so."""
    refs = [("chr1", 5000), ("chr2", 800)]
    a = [simple_read(0, 10 * k, f"a{k}") for k in range(40)]
    reads = a + [simple_read(1, 3 * k, f"o{k}") for k in range(5)]
    ctx.set_refs([l for _, l in refs])
    head = len(bam_header(refs))
    u = head + len(mm.record_stream(a))  # where target 1 begins
    path = os.path.join(scratch, "cut.bam")
    for keep in (35, 17, 8, 7):
        write_bam(path, refs, reads, block_size=u + keep, write_index=False)  # the first block ends `keep` bytes into that record
        data = open(path, "rb").read()
        first_block = data[:ffi.bgzf_block_starts(data)[1]]
        if keep >= 8:
            check(ctx.bam_merge(0, [(first_block, head)]), 0, [reads], 0xFF00)
        else:
            with pytest.raises(ffi.PjbError) as e:
                ctx.bam_merge(0, [(first_block, head)])
            assert e.value.code == ERR_BGZF and "ends inside" in str(e.value)


# ---- 4. the gather's alignments
def sweep_files():
    """Two files for the alignment sweep: names of 1..8 characters x aux of 0..3 bytes x with / without sequence, the shortest
    legal record among them, and one record longer than a BGZF block.  Every read knows its offset in its file (`_src`)."""
    refs = [("chr1", 200000)]
    files = [[], []]
    k = 0
    for rep in range(5):
        for l_name in range(1, 9):
            for n_aux in range(4):
                for with_seq in (False, True):
                    f = (k * 7 + rep) % 2 if k % 5 else k % 2
                    l = 1 + (k % 13)
                    r = dict(tid=0, pos=40 * k // 3, cigar=f"{l}M" if with_seq else np.zeros(0, np.uint32), seq=("ACGTN" * 3)[:l] if with_seq else None, flag=0, mapq=1,
                             xs=None, mtid=-1, mpos=-1, name="n" * l_name, aux=b"\x01\x02\x03"[:n_aux])
                    files[f].append(r)
                    k += 1
    shortest = [r for f in files for r in f if len(mm.record_bytes(r)) == 4 + 32 + 2]
    assert shortest  # no CIGAR, no sequence, a name of one character
    # a record longer than a BGZF block, straddling blocks of its source file
    big = dict(tid=0, pos=files[0][len(files[0]) // 2]["pos"], cigar="70001M", seq="ACGTTGCAT" * 7777 + "ACGTTGCA", flag=0, mapq=9, xs="+", mtid=-1, mpos=-1, name="big")
    files[0].insert(len(files[0]) // 2, big)
    assert len(mm.record_bytes(big)) > 0xFF00 + 30000  # (it spans three blocks of its file)
    for f, rs in enumerate(files):
        at = len(bam_header(refs))  # (each file's share starts with the file's first block: offsets in the share = in the file)
        for r in rs:
            r["_src"] = at
            at += len(mm.record_bytes(r))
    return refs, files


def test_gather_alignment_sweep(ctx, scratch):
    refs, files = sweep_files()
    res, want = merge(ctx, scratch, refs, 0, files)
    seen, at = set(), 0
    for r in want:
        n = len(mm.record_bytes(r))
        seen.add((r["_src"] % 4, at % 4, n % 4))
        at += n
    assert len(seen) == 64, sorted(set((a, b, c) for a in range(4) for b in range(4) for c in range(4)) - seen)
    merge(ctx, scratch, refs, 0, files, block_bytes=256, src_block=1000)


# ---- 5. edges: record counts around the wave, the block and the sort tile; the members' cut
@pytest.mark.parametrize("n_total", [1, 63, 64, 65, 255, 256, 257, "tile"])
def test_record_count_edges(ctx, scratch, n_total):
    n_total = rs_tile() * 3 + 1 if n_total == "tile" else n_total
    refs = [("chr1", 100000)]
    rng = np.random.default_rng(n_total)
    pos = np.sort(rng.integers(0, 100000, size=n_total) // 16 * 16)
    reads = [simple_read(0, int(p), f"e{k}", l=8 + k % 9) for k, p in enumerate(pos)]
    files = mm.stable_split(reads, 2, rng) if n_total > 1 else [[], reads]
    for bb in (256, 0xFF00):
        res, _ = merge(ctx, scratch, refs, 0, files, block_bytes=bb)
        assert res["n_records"] == n_total


@pytest.mark.parametrize("block_bytes", [256, 0xFF00])
@pytest.mark.parametrize("delta", [0, -4, 4])
def test_stream_length_against_the_cut(ctx, scratch, block_bytes, delta):
    refs = [("chr1", 100000)]
    n = 40 if block_bytes == 256 else 2400
    reads = [simple_read(0, 30 * k, f"c{k}", l=24) for k in range(n)]
    raw = len(mm.record_stream(reads))
    pad = (-raw) % block_bytes + delta
    pad += block_bytes if pad < 0 else 0
    reads[-1]["aux"] = b"\x07" * pad  # (the walk does not read aux bytes)
    assert (len(mm.record_stream(reads)) - delta) % block_bytes == 0
    files = [reads[0::2], reads[1::2]]
    res, _ = merge(ctx, scratch, refs, 0, files, block_bytes=block_bytes)
    assert res["raw_bytes"] % block_bytes == delta % block_bytes


# ---- 6. the sort's digits follow the target's length
@pytest.mark.parametrize("length", [1, 200, (1 << 29) - 1])
def test_digits_follow_the_target(ctx, scratch, length):
    refs = [("chr1", length)]
    rng = np.random.default_rng(length % 1000)
    if length <= 200:
        pos = rng.integers(0, length, size=400)
    else:  # near both ends, and apart in every digit
        pos = np.concatenate([rng.integers(0, 3000, size=150), length - 1 - rng.integers(0, 3000, size=150), rng.integers(0, 1 << 9, size=100) << 20,
                              [0, 1, length - 2, length - 1, length - 1, 0]])
    reads = [simple_read(0, int(p), f"d{k}", l=12) for k, p in enumerate(np.sort(pos))]
    files = mm.stable_split(reads, 3, rng)
    with ffi.Context(flags=ffi.FLAG_KERNEL_TIMING | ffi.FLAG_NO_CHAINS) as c:
        res, _ = merge(c, scratch, refs, 0, files)
        kt = c.kernel_timing()
    assert res["n_records"] == len(reads)
    passes = {1: 0, 200: 1, (1 << 29) - 1: 3}[length]  # 0, 8 and 29 bits of position in digits of at most 11
    assert kt.get("rs_scatter", (0, 0.0))[0] == passes and kt.get("rs_hist", (0, 0.0))[0] == passes, kt
    assert kt["mg_gather"][0] == 1 and kt["mg_keys"][0] == 3


def test_one_contributing_file_skips_the_sort(scratch):
    refs = [("chr1", 5000), ("chr2", 100)]
    a = [simple_read(0, 10 * k, f"a{k}") for k in range(40)]
    with ffi.Context(flags=ffi.FLAG_KERNEL_TIMING | ffi.FLAG_NO_CHAINS) as c:
        merge(c, scratch, refs, 0, [[simple_read(1, 3, "o")], a, None])
        assert "rs_scatter" not in c.kernel_timing()


# ---- 7. errors; the context merges a good case after each
def test_errors(ctx, scratch):
    refs = [("chr1", 5000), ("chr2", 800)]
    ctx.set_refs([l for _, l in refs])
    a = [simple_read(0, 10 * k, f"a{k}") for k in range(40)]
    b = [simple_read(0, p, f"b{k}") for k, p in enumerate([3, 10, 50, 40, 60, 20])]
    sa, sb = share_of(scratch, refs, a, 0), share_of(scratch, refs, b, 0)

    def fails(code, *words):
        def run(fn):
            with pytest.raises(ffi.PjbError) as e:
                fn()
            assert e.value.code == code, str(e.value)
            for w in words:
                assert w in str(e.value), str(e.value)
            with pytest.raises(ffi.PjbError) as e:  # the failing call dropped the merge
                ctx.bam_merge_end()
            assert e.value.code == ERR_STATE
            good_case(ctx, scratch)
            ctx.set_refs([l for _, l in refs])
        return run

    # pos goes back inside file 1, at its record 3
    fails(ERR_UNSORTED, "file 1", "record 3")(lambda: ctx.bam_merge(0, [sa, sb]))
    # the data ends inside a record of the target
    cut = share_of(scratch, refs, a, 0, src_block=700)
    starts = ffi.bgzf_block_starts(cut[0])
    ends = np.cumsum([len(mm.record_bytes(r)) for r in a]) + len(bam_header(refs))
    assert 1400 not in ends and ends[-1] > 1400  # (two blocks of 700 bytes end inside a record)
    fails(ERR_BGZF, "file 0", "ends inside")(lambda: ctx.bam_merge(0, [(cut[0][:starts[2]], cut[1]), sa]))
    # a position outside the target: an error, not the end of the run
    far = a[:10] + [simple_read(0, 5000, "far")]
    fails(ERR_BGZF, "file 1", "record 10", "outside")(lambda: ctx.bam_merge(0, [sa, share_of(scratch, refs, far, 0)]))

    def twice():
        ctx.bam_merge_begin(0, 2)
        ctx.bam_merge_file(1, *sa)
        ctx.bam_merge_file(1, *sa)
    fails(ERR_STATE, "file 1")(twice)

    def no_such_file():
        ctx.bam_merge_begin(0, 2)
        ctx.bam_merge_file(2, *sa)
    fails(ERR_ARG)(no_such_file)
    for bad in (0, 6, 0xFF04, 0x10000):
        fails(ERR_ARG, "block_bytes")(lambda: ctx.bam_merge(0, [sa], bad))
    # out of order: nothing begun (the last merge has ended)
    with pytest.raises(ffi.PjbError) as e:
        ctx.bam_merge_file(0, *sa)
    assert e.value.code == ERR_STATE
    with pytest.raises(ffi.PjbError) as e:
        ctx.bam_merge_begin(2, 1)  # no such target
    assert e.value.code == ERR_ARG
    good_case(ctx, scratch)


def test_end_without_begin():
    with ffi.Context(flags=ffi.FLAG_NO_CHAINS) as c:
        c.set_refs([1000])
        with pytest.raises(ffi.PjbError) as e:
            c.bam_merge_end()
        assert e.value.code == ERR_STATE
