"""The launches behind prep's device calls, pinned: every label of Context.kernel_timing() with its launch count, for an index build
(BAI and CSI), a merge and a sort of four small fixed inputs.  bench.py does not run prep; a change to the host code behind
pjb_index_*, pjb_bam_merge_* or pjb_bam_sort_* that adds, drops or repeats a launch shows here.  The tables were recorded with the
library as it stood before these calls' drivers were given shared helpers and headers of their own."""
import os

import numpy as np
import pytest

from portcullis_amd import ffi
from util_bam import bam_header, write_bam

pytestmark = pytest.mark.gpu

REFS = [("chr1", 40000), ("chr2", 9000), ("chr3", 70000)]
BLOCK = 8000  # inflated bytes per BGZF block of the inputs


def simple_read(tid, pos, name, l=20):
    return dict(tid=tid, pos=pos, cigar=f"{l}M", seq="ACGT" * (l // 4) + "A" * (l % 4), flag=0, mapq=60, xs=None, mtid=-1, mpos=-1, name=name)


def sorted_reads():
    """300 records over the three targets, in coordinate order."""
    rng = np.random.default_rng(20240)
    reads = []
    for tid, (_, length) in enumerate(REFS):
        for k, p in enumerate(np.sort(rng.integers(0, length - 40, size=100))):
            reads.append(simple_read(tid, int(p), f"t{tid}r{k}" + "x" * (k % 5), l=20 + k % 23))
    return reads


def bam_bytes(tmp_path, refs, reads):
    path = str(tmp_path / "in.bam")
    write_bam(path, refs, reads, block_size=BLOCK, write_index=False)
    return open(path, "rb").read()


def table(run):
    """{label: launches} of what `run(context)` launches."""
    with ffi.Context(flags=ffi.FLAG_KERNEL_TIMING | ffi.FLAG_NO_CHAINS) as c:
        run(c)
        kt = {name: launches for name, (launches, _) in c.kernel_timing().items()}
    print(sorted(kt.items()))
    return kt


INFLATE = {"bgzf_decode": 2, "bgzf_resolve": 2}  # two pieces, or two files
WALK_ALL = {"bam_find_starts": 2, "bam_seg_reduce": 2, "bam_seg_apply": 2, "bam_walk_all_count": 2, "bam_walk_all_fill": 2,
            "bam_trim_segments": 1}  # (the first piece ends inside a record, the second on a record's end)
BAI_PIECES = {"bai_records": 2, "bai_head_reduce": 2, "bai_head_apply": 2, "bai_chunks": 2, "bai_win_apply": 2}
BAI_ORDER = {"bai_level_reduce": 3, "bai_level_apply": 3, "bai_tid_starts": 1, "bai_partition": 1}
SORT_PASSES = {"rs_hist": 2, "rs_panel_sums": 2, "rs_panel_scan": 2, "rs_scatter": 2}
DEFLATE = {"mg_gather": 1, "bgzf_deflate": 1, "bgzf_pack": 1}
EXPECTED = {
    "bai": {**INFLATE, **WALK_ALL, **BAI_PIECES, **BAI_ORDER, "bai_win_reduce": 2, "bai_win_tiles": 2},
    "csi": {**INFLATE, **WALK_ALL, **BAI_PIECES, **BAI_ORDER, "bai_win_reduce": 3, "bai_win_tiles": 3, "csi_seed": 1, "csi_fill_apply": 1, "csi_loffset": 1},
    "merge": {**INFLATE, "bam_find_starts": 2, "bam_seg_reduce": 2, "bam_seg_apply": 2, "bam_walk_count": 2, "bam_walk_fill": 2, "mg_keys": 2, **SORT_PASSES,
              "mg_off_reduce": 1, "mg_off_apply": 1, **DEFLATE},
    "sort": {**INFLATE, **WALK_ALL, "sr_keys": 2, **SORT_PASSES, "sr_off_reduce": 1, "sr_off_apply": 1, **DEFLATE},
}


@pytest.fixture(scope="module")
def sorted_file(tmp_path_factory):
    data = bam_bytes(tmp_path_factory.mktemp("launches"), REFS, sorted_reads())
    assert len(ffi.bgzf_block_starts(data)) - 1 == 5  # four blocks of records and the EOF block
    return data


def test_bai_in_two_pieces(sorted_file):
    def run(c):
        res = c.index_bam(sorted_file, piece_blocks=3)
        assert res["n_records"] == 300 and len(res["next_voffsets"]) == 2
    assert table(run) == EXPECTED["bai"]


def test_csi_of_depth_1_in_two_pieces(sorted_file):
    def run(c):
        res = c.index_bam(sorted_file, piece_blocks=3, csi_depth=1)
        assert res["n_records"] == 300 and res["depth"] == 1 and len(res["next_voffsets"]) == 2
    assert table(run) == EXPECTED["csi"]


def test_merge_of_two_files(tmp_path):
    refs = [("chr1", 5000)]
    a = [simple_read(0, 10 * k, f"a{k}") for k in range(40)]
    b = [simple_read(0, 10 * k + 5 * (k % 2), f"b{k}") for k in range(30)]
    shares = [(bam_bytes(tmp_path, refs, f), len(bam_header(refs))) for f in (a, b)]

    def run(c):
        c.set_refs([5000])
        assert c.bam_merge(0, shares)["n_records"] == 70
    assert table(run) == EXPECTED["merge"]


def test_sort_in_two_pieces(tmp_path):
    reads = sorted_reads()
    reads = [reads[k] for k in np.random.default_rng(7).permutation(len(reads))]
    data = bam_bytes(tmp_path, REFS, reads)
    assert len(ffi.bgzf_block_starts(data)) - 1 == 5

    def run(c):
        res = c.bam_sort(data, piece_blocks=3)
        assert res["n_records"] == 300 and res["was_sorted"] == 0 and res["pieces"] == 2
    assert table(run) == EXPECTED["sort"]
