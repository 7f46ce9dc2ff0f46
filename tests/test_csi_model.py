"""tests/csi_model.py, the definition of the CSI this project writes, held to the reference's own htslib-1.3
(oracle/_ref/hts_witness): htslib loads the model's files and answers region queries with them as with the BAI it builds
itself, and -- on a target of more than 2^30 bases, which no BAI can describe -- as the records themselves say.  No GPU."""
import os
import struct

import pytest

import csi_model as cm
import hts_witness as hts
import index_model as im
from test_oracle_htslib_witness import regions_for
from util_bam import write_bam


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("csi_mixed") / "m.bam")
    write_bam(p, im.MIXED_REFS, im.mixed_reads(), block_size=4096)
    return p


@pytest.fixture(scope="module")
def long_bam(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("csi_long") / "long.bam")
    cm.write_bam_long(p, cm.LONG_REFS, cm.long_reads(), block_size=cm.LONG_BLOCK)
    return p


def test_the_depth_rule():
    assert cm.depth_for([16_128]) == 0 and cm.depth_for([16_129]) == 1
    assert cm.depth_for([n for _, n in im.MIXED_REFS]) == 3
    assert cm.depth_for([248_956_422]) == 5  # human chr1
    assert cm.depth_for([2**29 - 256]) == 5 and cm.depth_for([2**29 - 255]) == 6
    assert cm.depth_for([2**31 - 1]) == 6
    assert cm.depth_for([]) == 0


# ---- (a) htslib answers with the model's .csi as with its own .bai
def test_htslib_answers_as_with_its_own_bai(tmp_path, mixed):
    assert cm.build(mixed)[1] == 3
    own = str(tmp_path / "htslib.bai")
    hts.index(mixed, own)
    regions = regions_for(im.MIXED_REFS, 300)
    want = cm.witness_query(mixed, own, regions)
    n = sum(len(h) for _, h in want)
    assert n > 50_000
    for depth in (3, 5, 6):
        f = str(tmp_path / f"d{depth}.csi")
        open(f, "wb").write(cm.container(cm.payload_of(mixed, depth)))
        got = cm.witness_query(mixed, f, regions)
        for (reg, a), (_, b) in zip(got, want):
            assert a == b, (depth, reg)


# ---- (b) depth 5 is the BAI's binning
def test_depth_5_agrees_with_the_bai_model(mixed):
    n_ref, depth, bins, loff, recs = cm.build(mixed, 5)
    b_ref, b_bins, b_lin, b_recs = im.build(mixed)
    assert (n_ref, bins, recs) == (b_ref, b_bins, b_recs) and depth == 5
    per_target, _ = im.parse_bai(im.serialise(b_ref, b_bins, b_lin))  # (the linear index filled as the file has it)
    checked = 0
    for t in range(n_ref):
        lin = per_target[t][1]
        first = min((vs for tid, _, _, vs in recs if tid == t), default=None)
        for b, v in loff[t].items():
            w = cm.first_window(b, 5)
            assert v == (lin[w] or first), (t, b)  # (leading untouched windows are 0 in the BAI, the first record's offset here)
            checked += 1
    assert checked > 50
    # the serialised form round-trips
    min_shift, d, parsed, rest = cm.parse(cm.serialise(n_ref, depth, bins, loff))
    assert (min_shift, d, rest) == (14, 5, b"")
    for t in range(n_ref):
        assert parsed[t][1] == sorted(bins[t])
        assert {b: [list(c) for c in cs] for b, (_, cs) in parsed[t][0].items()} == bins[t]


def test_depth_0_is_one_bin_per_target(mixed):
    """(No query goes to the witness at depth 0: htslib-1.3 walks below bin 0 on a target without bins and never returns.)"""
    _, _, parsed, rest = cm.parse(cm.payload_of(mixed, 0))
    assert rest == b""
    assert [order for _, order in parsed] == [[0], [], [0], [0]]
    recs = im.build(mixed)[3]
    for t in (0, 2, 3):
        loffset, chunks = parsed[t][0][0]
        assert loffset == chunks[0][0] == min(vs for tid, _, _, vs in recs if tid == t)
        assert len(chunks) == 1


def test_the_container(mixed):
    payload = cm.payload_of(mixed, 6) * 9  # more than one member
    assert len(payload) > 2 * 0xFF00
    assert cm.check_container(cm.container(payload)) == payload


# ---- (c) a target past 2^30
def test_a_long_target_is_served_as_brute_force_says(tmp_path, long_bam):
    assert os.path.getsize(long_bam) < 200_000
    n_ref, depth, bins, loff, recs = cm.build(long_bam)
    assert depth == 6 and n_ref == 2
    assert {cm.level_of(b) for b in bins[0]} >= {0, 3, 4, 5, 6}
    # bin 0 holds what straddles 2^29 (a level-1 boundary at depth 6), the read of two long introns among them; its loffset
    # is the target's first record's offset
    assert len(bins[0][0]) > 1 and loff[0][0] == recs[0][3]
    f = str(tmp_path / "long.csi")
    open(f, "wb").write(cm.container(cm.serialise(n_ref, depth, bins, loff)))
    regions = cm.long_regions()
    assert len(regions) == 612
    got = cm.witness_query(long_bam, f, regions)
    want = cm.brute_force(recs, regions)
    total = 0
    for (reg, hits), w in zip(got, want):
        assert [(p, e) for p, e, _ in hits] == w, reg
        total += len(w)
    assert total > 50_000


def test_the_long_input_is_what_the_issue_describes():
    reads = cm.long_reads()
    assert 3_200 < len(reads) < 3_400
    assert sum(r["tid"] == 1 for r in reads) == 300
    assert max(r["pos"] for r in reads if r["tid"] == 0) >= 2**30
    assert all(a["pos"] <= b["pos"] for a, b in zip(reads, reads[1:]) if a["tid"] == b["tid"])
    assert struct.calcsize("<H") == 2  # (the record's bin field: what write_bam_long truncates for)
