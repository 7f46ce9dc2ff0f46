"""What the tests of `prep --sort` / pjb_bam_sort_* stand on, checked without a device: write_bam writes reads in whatever order
they come when it is not asked for an index, so an unsorted input is write_bam(shuffled, write_index=False); and the model of the
sorted file is sorted(reads, key=merge_model.merge_key), Python's stable sort by (refID as unsigned, pos)."""
import os
import zlib

import numpy as np

import merge_model as mm
from portcullis_amd.ffi import bgzf_block_starts
from util_bam import bam_header, write_bam


def read(tid, pos, name):
    return dict(tid=tid, pos=pos, cigar="20M", seq="ACGT" * 5, flag=0, mapq=60, xs=None, mtid=-1, mpos=-1, name=name)


def test_write_bam_takes_unsorted_reads_without_the_index(tmp_path):
    refs = [("chr1", 5000), ("chr2", 800)]
    reads = [read(1, 700, "a"), read(-1, -1, "u0"), read(0, 4000, "b"), read(0, 3, "c"), read(-1, -1, "u1"), read(1, 0, "d")]
    path = str(tmp_path / "unsorted.bam")
    write_bam(path, refs, reads, block_size=64, write_index=False)
    assert not os.path.exists(path + ".bai")
    data = open(path, "rb").read()
    starts = bgzf_block_starts(data)
    stream = b"".join(zlib.decompress(data[a:b], 31) for a, b in zip(starts, starts[1:]))
    assert stream == bam_header(refs) + mm.record_stream(reads)  # input order, byte for byte


def test_the_model_is_stable_and_puts_unplaced_records_last():
    rng = np.random.default_rng(3)
    reads = [read(int(t), int(p), f"n{k}") for k, (t, p) in enumerate(zip(rng.integers(0, 3, 200), rng.integers(0, 4, 200)))]
    reads += [read(-1, -1, f"u{k}") for k in range(20)]
    order = rng.permutation(len(reads))
    shuffled = [reads[k] for k in order]
    want = sorted(shuffled, key=mm.merge_key)
    keys = [mm.merge_key(r) for r in want]
    assert keys == sorted(keys) and all(r["tid"] == -1 for r in want[-20:]) and all(r["tid"] >= 0 for r in want[:-20])
    at = {id(r): k for k, r in enumerate(shuffled)}
    for a, b in zip(want, want[1:]):  # equal keys: input order
        if mm.merge_key(a) == mm.merge_key(b):
            assert at[id(a)] < at[id(b)]
