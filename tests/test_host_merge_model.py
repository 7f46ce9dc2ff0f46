"""tests/merge_model.py against the helpers it restates: record_bytes() gives the bytes write_bam emits for a read (so that a merged
stream can be compared byte for byte), span_at() finds the block and offset of a record as the reader's index would, and the
model's order is the one the issue defines -- one stable sort of the concatenation, unplaced records last."""
import gzip

import numpy as np

import merge_model as mm
from fuzzgen import aux_rich_targets
from util_bam import bam_header, write_bam


def test_record_bytes_are_write_bams(tmp_path):
    refs, _, reads = aux_rich_targets()  # every CIGAR op, SEQ '*', names of assorted lengths, aux fields before and behind XS
    reads = reads[::7] + [dict(tid=-1, pos=-1, cigar=np.zeros(0, np.uint32), seq="ACGT", flag=4, mapq=0, xs=None, mtid=-1, mpos=-1, name="u0")]
    path = str(tmp_path / "x.bam")
    write_bam(path, refs, reads, block_size=3000, write_index=False)
    raw = gzip.open(path, "rb").read()
    head = len(bam_header(refs))
    assert raw[head:] == mm.record_stream(reads)
    # span_at: the block that holds a record, and the record's offset in it
    data = open(path, "rb").read()
    for k in (0, 1, len(reads) // 2, len(reads) - 1):
        u = head + len(mm.record_stream(reads[:k]))
        comp, first = mm.span_at(data, u)
        assert u // 3000 * 3000 + first == u and gzip.decompress(comp)[first:] == raw[u:]
    comp, first = mm.span_at(data, len(raw))  # behind the last record: the EOF block
    assert first == 0 and gzip.decompress(comp) == b""


def test_the_order():
    def r(tid, pos, name):
        return dict(tid=tid, pos=pos, name=name)
    a = [r(0, 5, "a0"), r(0, 9, "a1"), r(2, 1, "a2"), r(-1, -1, "a3")]
    b = [r(0, 5, "b0"), r(0, 5, "b1"), r(1, 0, "b2"), r(2, 1, "b3"), r(-1, -1, "b4"), r(-1, -1, "b5")]
    names = [x["name"] for x in mm.merge_reads([a, b])]
    assert names == ["a0", "b0", "b1", "a1", "b2", "a2", "b3", "a3", "b4", "b5"]
    assert [x["name"] for x in mm.merge_reads([b, a])] == ["b0", "b1", "a0", "a1", "b2", "b3", "a2", "b4", "b5", "a3"]
    assert mm.merge_reads([a]) == a  # one file: the identity
    rng = np.random.default_rng(3)
    parts = mm.stable_split(a + b, 3, rng)
    assert sorted(x["name"] for p in parts for x in p) == sorted(x["name"] for x in a + b)
