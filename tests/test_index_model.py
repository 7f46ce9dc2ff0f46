"""tests/index_model.py -- the Python restatement of the BAI of an existing BAM that the device indexer is held to -- reproduces
the bytes `write_bam(..., write_index=True)` writes while it builds the file.  No GPU."""
import os

import pytest

import index_model as im
from util_bam import write_bam

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def mixed():
    return im.mixed_reads()


@pytest.mark.parametrize("block_size", [0xFF00, 4096, 777])
def test_model_reproduces_write_bam(tmp_path, mixed, block_size):
    p = str(tmp_path / "m.bam")
    write_bam(p, im.MIXED_REFS, mixed, block_size=block_size)
    want = open(p + ".bai", "rb").read()
    assert im.index_of(p) == want
    per_target, rest = im.parse_bai(want)
    assert rest == b""
    bins = per_target[0][0]
    levels = {next(l for l, first in ((5, 4681), (4, 585), (3, 73), (2, 9), (1, 1), (0, 0)) if b >= first) for b in bins}
    assert len(levels) >= 4, levels
    assert sum(len(c) > 1 for c in bins.values()) > 10
    assert per_target[1] == ({}, [], [])  # the target without reads


def test_model_on_runs(tmp_path):
    reads = im.run_reads()
    assert 69_000 < len(reads) < 76_000
    p = str(tmp_path / "r.bam")
    write_bam(p, [("one", 1_000_000)], reads)
    assert im.index_of(p) == open(p + ".bai", "rb").read()
    # the runs of equal bin have the lengths asked for
    runs, last = [], None
    for _, pos, end, _ in im.build(p)[3]:
        b = im._reg2bin(pos, end)
        if b == last:
            runs[-1] += 1
        else:
            runs.append(1)
            last = b
    assert runs[:20] == im.RUN_LENGTHS * 2


def test_model_on_degenerate_files(tmp_path):
    refs = [("a", 1000)]
    for name, reads in (("none", []), ("unplaced", [dict(tid=-1, pos=-1, cigar="", seq="ACGT")] * 3)):
        p = str(tmp_path / (name + ".bam"))
        write_bam(p, refs, reads)
        assert im.index_of(p) == open(p + ".bai", "rb").read()
    p, block = record_ending_on_a_block_end(tmp_path)
    assert im.index_of(p) == open(p + ".bai", "rb").read()


def record_ending_on_a_block_end(tmp_path):
    """A BAM whose single record ends exactly on its block's last byte (the block size is the whole stream's length)."""
    import gzip

    refs = [("a", 1000)]
    reads = [dict(tid=0, pos=5, cigar="10M", seq="ACGTACGTAC")]
    p = str(tmp_path / "edge.bam")
    write_bam(p, refs, reads)
    total = len(gzip.open(p, "rb").read())
    write_bam(p, refs, reads, block_size=total)
    assert len(im.bgzf_blocks(open(p, "rb").read())) == 3  # one data block, the EOF block, the sentinel
    return p, total


@pytest.mark.parametrize("name", ["sorted.bam", "clipped3.bam"])
def test_model_against_the_samtools_indexes(name):
    """The reference's fixtures carry indexes samtools wrote: they differ from this project's in the metadata pseudo-bin, the
    trailing count and the last chunk's end (samtools puts it behind the EOF block), and in nothing else that is asserted here."""
    p = os.path.join(GOLDEN, name)
    ours, rest = im.parse_bai(im.index_of(p))
    theirs, _ = im.parse_bai(open(p + ".bai", "rb").read())
    assert_same_where_it_counts(ours, theirs, im.build(p)[3])


def assert_same_where_it_counts(ours, theirs, records, merged_bins=False):
    """merged_bins: `theirs` comes straight from htslib's writer, which moves the chunks of a bin whose data lies within 64 KB of
    the file into the bin's parent before it saves (compress_binning, deps/htslib-1.3/hts.c); the samtools-made fixtures are too
    sparse for that to have happened.  Then a bin of ours may be found in its nearest ancestor that theirs holds -- which must hold
    nothing else -- and each of our chunks must lie inside one chunk of that bin; where nothing was moved this is the equality
    asked for without the flag."""
    assert len(ours) == len(theirs)
    touched = [set() for _ in ours]
    for tid, pos, end, _ in records:
        if tid >= 0:
            touched[tid].update(range(pos >> 14, ((end - 1) >> 14) + 1))
    for t, ((b1, l1, _), (b2, l2, _)) in enumerate(zip(ours, theirs)):
        b2 = {b: c for b, c in b2.items() if b != 37450}  # the pseudo-bin
        if merged_bins:
            def home(b):  # the nearest of b, its parent, its parent's parent ... that theirs holds
                while b not in b2 and b > 0:
                    b = (b - 1) >> 3
                return b
            assert {home(b) for b in b1} == set(b2), t
            for b, chunks in b1.items():
                for vs, ve in chunks:
                    assert any(u <= vs and ve <= v for u, v in b2[home(b)]), (t, b, vs, ve)
        else:
            assert set(b1) == set(b2), t
        if b1:
            assert min(c[0][0] for c in b1.values()) == min(c[0][0] for c in b2.values()), t
        assert len(l1) == len(l2), t
        for w in touched[t]:
            assert l1[w] == l2[w], (t, w)
