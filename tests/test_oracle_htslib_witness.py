"""What this project restates of htslib, held to the reference's own htslib-1.3 (oracle/_ref/hts_witness, tests/hts_witness.py):

  * the pileup and its 8000-node cap: orc.depth (the yardstick of `junc --extra`'s coverage) against bam_mplp_* driven as
    DepthParser drives it;
  * the record decode: util_bam.read_bam against sam_read1, bam_endpos, seq_nt16_str, bam_aux_get / bam_aux2A;
  * the BAI: tests/index_model.py and write_bam's own index against sam_index_build2, and sam_itr_queryi through either;
  * the FASTA index and fetch: GenomeMapper::buildFastaIndex and write_fasta against fai_build, the oracle's fetch_bases,
    GenomeMapper::fetchBases and the numpy restatement of the device's rule against faidx_fetch_seq.

Every comparison is exact.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import hts_witness as hts
import index_model as im
from oracle import oracle as orc
from portcullis_amd.records import CIGAR_CHARS, NT16, ReadBatch
from util_bam import _ref_span, read_bam, write_bam, write_fasta

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")


# =====================================================================================================================
# 1. the pileup
# =====================================================================================================================
def pile(tid, pos, n, cigar, **kw):
    return [{"tid": tid, "pos": pos, "cigar": cigar, "seq": None, **kw} for _ in range(n)]


def assert_pileup(tmp_path, refs, reads):
    """orc.depth of every target == what DepthParser would store from htslib's pileup of the same records, for every index
    below the target's length.  DepthParser stores the count of position p at depths[p + 1] (depth_parser.cc:131,149-153)
    without looking at the vector's size: for a record that covers the target's last base or leaves it htslib reports
    positions p with p + 1 >= length, which the reference writes out of bounds.  Those are not compared; every index the
    reference may write is.  Returns the vectors."""
    for k, r in enumerate(reads):
        r.setdefault("name", f"r{k}")
    assert all((a["tid"], a["pos"]) <= (b["tid"], b["pos"]) for a, b in zip(reads, reads[1:])), "not sorted"
    p = str(tmp_path / "pile.bam")
    write_bam(p, refs, reads, write_index=False)
    want = [np.zeros(ln, dtype=np.uint32) for _, ln in refs]
    for tid, pos, d in hts.depth(p):
        if pos + 1 < refs[tid][1]:
            want[tid][pos + 1] = d
    for tid, (_, ln) in enumerate(refs):
        got, _ = orc.depth(ln, ReadBatch.from_reads([r for r in reads if r["tid"] == tid]))
        bad = np.nonzero(got != want[tid])[0]
        assert bad.size == 0, (tid, [(int(x), int(got[x]), int(want[tid][x])) for x in bad[:10]])
    return want


def test_pileup_hand_worked_cap_case(tmp_path):
    """The case of test_oracle_extra_kat.py::test_pileup_cap_drops_only_ties_at_the_current_position."""
    reads = pile(0, 100, 9000, "50M") + pile(0, 101, 3, "50M") + pile(0, 200, 5, "10M")
    (d,) = assert_pileup(tmp_path, [("a", 400)], reads)
    assert d[101] == 7999 and d[102] == 8000 and d[151] == 1 and d[201] == 5


def test_pileup_near_ties_with_deletions(tmp_path):
    """12 000 records over six adjacent positions with lengths 40 .. 89, and 500 records that carry a deletion."""
    reads = []
    for k in range(12_000):
        reads.append(dict(tid=0, pos=300 + k // 2000, cigar=f"{40 + k % 50}M", seq=None))
    for k in range(500):
        reads.append(dict(tid=0, pos=300 + k % 6, cigar=f"{10 + k % 7}M{1 + k % 5}D{20 + k % 11}M", seq=None))
    reads.sort(key=lambda r: r["pos"])
    (d,) = assert_pileup(tmp_path, [("a", 1000)], reads)
    assert 7990 < d.max() <= 8010                # the cap was at work: 12 500 records, and no position holds many more than 8000


def test_pileup_churn_over_three_targets(tmp_path):
    """Per target piles of 10 / 3 000 / 8 500 records of 1 / 2 / 30 / 300 bases at positions 0, 1, 2, 50, 51 and 400, and
    records without a reference span (5S, 3I) between them."""
    sizes, lens = (10, 3000, 8500), (1, 2, 30, 300)
    refs, reads = [], []
    for tid in range(3):
        refs.append((f"t{tid}", 1000))
        for i, pos in enumerate((0, 1, 2, 50, 51, 400)):
            reads += pile(tid, pos, sizes[(i + tid) % 3], f"{lens[(i + 2 * tid) % 4]}M")
            if pos in (1, 50):
                reads += pile(tid, pos, 1, "5S", seq="ACGTA") + pile(tid, pos, 1, "3I", seq="ACG")
    want = assert_pileup(tmp_path, refs, reads)
    assert all(d.max() >= 7999 for d in want)


def test_pileup_spanless_records_ahead_of_a_capped_pile(tmp_path):
    """bam_endpos of a mapped record whose CIGAR spans nothing is pos itself (sam.c:336-342), so the pileup frees it before the
    next position: 50 such records at one position must not count against the cap of the pile that follows at the next."""
    reads = pile(0, 100, 25, "5S", seq="ACGTA") + pile(0, 100, 25, "3I", seq="ACG") + pile(0, 101, 9000, "20M") + pile(0, 102, 3, "4M")
    (d,) = assert_pileup(tmp_path, [("a", 400)], reads)
    assert d[102] == 7999


@pytest.mark.parametrize("ahead", [0, 1, 30])
def test_pileup_spanless_records_inside_a_capped_pile(tmp_path, ahead):
    """bam_plp_push links a kept record into its list only if the record's end lies behind the position the iterator stands on
    (sam.c:1930): of the records without a span at one position only one that is the first record there takes a node."""
    z = [r for k in range(15) for r in pile(0, 100, 1, "5S", seq="ACGTA") + pile(0, 100, 1, "3I", seq="ACG")]
    reads = pile(0, 99, 2, "1M") + z[:ahead] + pile(0, 100, 4000, "20M") + z + pile(0, 100, 5000, "20M") + z[:3] + pile(0, 101, 3, "4M")
    (d,) = assert_pileup(tmp_path, [("a", 400)], reads)
    # a record is dropped when it finds 7999 in the list: here the two of position 99, which end at 100, and one without a span
    # if it came first
    assert d[101] == 7999 - 2 - (1 if ahead else 0) and d[102] == 7999   # (at 101 the list fills up again: two of the three are kept)


def test_pileup_jump_between_two_piles(tmp_path):
    """Two piles of 9 000 records 4 900 bases apart, the first long enough to reach the second, and a few records one base
    behind the second pile."""
    reads = pile(0, 100, 9000, "5000M") + pile(0, 5000, 9000, "50M") + pile(0, 5001, 4, "50M")
    assert_pileup(tmp_path, [("a", 12_000)], reads)
    reads = pile(0, 100, 9000, "50M") + pile(0, 5000, 9000, "50M") + pile(0, 5001, 4, "50M")   # ... and one that ends long before
    (d,) = assert_pileup(tmp_path, [("a", 12_000)], reads)
    assert d[5001] == 7999 and d[5002] == 8000


def test_pileup_one_base_records_at_adjacent_positions(tmp_path):
    reads = pile(0, 10, 8500, "1M") + pile(0, 11, 8500, "1M")
    (d,) = assert_pileup(tmp_path, [("a", 100)], reads)
    assert d[11] == 7999 and d[12] == 1   # (a record of one base is still in the list when the next position's records arrive)


def test_pileup_mixed_flags(tmp_path):
    """Unmapped records are not pushed and do not count against the cap; every other flag counts (sam.c:1905)."""
    rng = np.random.default_rng(3)
    for n in (9000, 12_000):
        flags = rng.choice([0, 4, 0x100, 0x200, 0x400, 0x800, 16], size=n)
        reads = [dict(tid=0, pos=40, cigar="25M", seq=None, flag=int(f)) for f in flags] + pile(0, 41, 2, "25M")
        (d,) = assert_pileup(tmp_path, [("a", 200)], reads)
        mapped = int((flags != 4).sum())
        assert (mapped, d[41]) == ((mapped, mapped) if n == 9000 else (mapped, 7999)) and (mapped > 7999) == (n != 9000)


def test_pileup_ramp(tmp_path):
    """60 consecutive positions with 5 / 700 / 2 500 records of aMbDcM each."""
    reads = []
    for i in range(60):
        reads += pile(0, 500 + i, (5, 700, 2500)[i % 3], f"{3 + i % 17}M{1 + i % 4}D{5 + (7 * i) % 40}M")
    (d,) = assert_pileup(tmp_path, [("a", 1000)], reads)
    assert d.max() > 7000


@pytest.mark.parametrize("seed", [3, 41, 52])
def test_pileup_fuzz(tmp_path, seed):
    """fuzzgen reads: every CIGAR operation, spliced records (the reader skips them), soft clips at the target's ends."""
    from fuzzgen import make_reads

    genome, reads = make_reads(seed, n_reads=3000, paired=(seed == 41))
    for r in reads:
        r["tid"] = 0
        if r.get("mtid", -1) >= 0:
            r["mtid"] = 0
    (d,) = assert_pileup(tmp_path, [("chr1", len(genome))], reads)
    assert d.sum() > 0


def test_pileup_at_the_targets_end(tmp_path):
    """The edge the comparison leaves out (see assert_pileup): records that cover the last base and one that leaves the target."""
    reads = pile(0, 80, 3, "20M") + pile(0, 90, 2, "10M") + pile(0, 95, 1, "3M30D4M") + pile(0, 97, 1, "20M")
    d, _ = assert_pileup(tmp_path, [("a", 100), ("b", 50)], reads + pile(1, 0, 2, "50M") + pile(1, 49, 1, "1M"))
    assert d[99] == 6       # position 98, the last index the reference may write: 3 + 2 + 0 (in the deletion) + 1


# =====================================================================================================================
# 2. the record decode
# =====================================================================================================================
def assert_records(path):
    """Every field util_bam.read_bam reports == what htslib reads from the same file.  Returns read_bam's records."""
    refs, recs = read_bam(path)
    hrefs, hrecs = hts.records(path)
    assert refs == hrefs
    assert len(recs) == len(hrecs)
    for k, (r, h) in enumerate(zip(recs, hrecs)):
        cigar = "".join(f"{int(c) >> 4}{CIGAR_CHARS[int(c) & 15]}" for c in r["cigar"]) or "*"
        b = r["seq4"]
        seq = "".join(NT16[(b[i >> 1] >> 4) if (i & 1) == 0 else (b[i >> 1] & 15)] for i in range(r["l_qseq"])) or "*"
        mine = dict(tid=r["tid"], pos=r["pos"], flag=r["flag"], mapq=r["mapq"], l_qseq=r["l_qseq"], mtid=r["mtid"], mpos=r["mpos"],
                    cigar=cigar, seq=seq, name=r["name"], xs=r["xs"])
        theirs = {f: h[f] for f in mine}
        theirs["xs"] = None if h["xs"] is None else h["xs"][1]   # bam_aux2A's value: 0 for a type that is not 'A'
        assert mine == theirs, k
        if h["xs"] is not None:
            assert (h["xs"][0] == "A") == (r["xs"] != "\x00"), k
        # bam_endpos (sam.c:336-342): pos + span for a mapped record with a CIGAR, else pos + 1.  write_bam and index_model use
        # pos + max(1, span): the same wherever a mapped record's CIGAR spans a base
        span = _ref_span(r["cigar"])
        assert h["end"] == (r["pos"] + span if not (r["flag"] & 4) and len(r["cigar"]) else r["pos"] + 1), k
    return recs


@pytest.mark.parametrize("block_size", [0xFF00, 700])
def test_records_of_the_aux_rich_fuzz_bam(tmp_path, block_size):
    from fuzzgen import aux_rich_targets

    refs, _, reads = aux_rich_targets()
    p = str(tmp_path / "a.bam")
    write_bam(p, refs, reads, block_size=block_size, write_index=False)
    recs = assert_records(p)
    assert len(recs) == len(reads)
    assert sum(r["xs"] is None for r in recs) > 100 and sum(r["xs"] in ("+", "-") for r in recs) > 1000
    assert any(r["l_qseq"] == 0 for r in recs)


@pytest.mark.parametrize("name", ["bam1.bam", "bam2.bam", "clipped3.bam", "sorted.bam", "unsorted.bam"])
def test_records_of_the_golden_bams(name):
    recs = assert_records(os.path.join(GOLDEN, name))
    assert len(recs) >= 100
    if name == "bam1.bam":  # (aligners that write XS:i, the alignment score of the next-best hit: bam_aux2A gives 0 for it)
        assert any(r["xs"] == "\x00" for r in recs)


def test_records_xs_of_every_type(tmp_path):
    """XS as A, as an integer of every width, as Z, twice (the first counts), and absent."""
    import struct

    auxes = [b"", b"XSA+", b"XSA-", b"XSc\xff", b"XSC\x2b", b"XSs\x2b\x00", b"XSS\x2b\x00", b"XSi\x2b\x00\x00\x00", b"XSI\x2d\x00\x00\x00",
             b"XSf" + struct.pack("<f", 43.0), b"XSZ+\x00", b"NMC\x01XSA-XSA+", b"XSi\x01\x00\x00\x00XSA+", b"XTA+", b"XSA.",
             b"ZBBC" + struct.pack("<i", 2) + b"XS" + b"XSA-"]
    reads = [dict(tid=0, pos=10 + k, cigar="4M", seq="ACGT", aux=a) for k, a in enumerate(auxes)]
    p = str(tmp_path / "x.bam")
    write_bam(p, [("a", 100)], reads, write_index=False)
    recs = assert_records(p)
    assert [r["xs"] for r in recs] == [None, "+", "-"] + ["\x00"] * 8 + ["-", "\x00", None, ".", "-"]


# =====================================================================================================================
# 3. the BAI
# =====================================================================================================================
def regions_for(refs, per_target=300, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for t, (_, length) in enumerate(refs):
        for k in range(per_target):
            beg = int(rng.integers(0, length))
            out.append((t, beg, min(length, beg + (1, 50, 2_000, 40_000, 400_000)[k % 5])))
    return out


def assert_index_serves_htslib(tmp_path, bam, refs, candidates):
    """htslib loads each candidate index and answers region queries exactly as with the index it builds itself, and the
    candidate equals htslib's where test_index_model.assert_same_where_it_counts looks.  candidates: {label: bytes}.
    Returns the number of records the queries returned."""
    from test_index_model import assert_same_where_it_counts

    own = str(tmp_path / "htslib.bai")
    theirs, _ = im.parse_bai(hts.index(bam, own))
    regions = regions_for(refs)
    want = hts.query(bam, own, regions)
    records = im.build(bam)[3]
    for label, data in candidates.items():
        ours, rest = im.parse_bai(data)
        assert rest == b"", label
        assert_same_where_it_counts(ours, theirs, records, merged_bins=True)
        f = str(tmp_path / "candidate.bai")
        open(f, "wb").write(data)
        got = hts.query(bam, f, regions)
        for (reg, a), (_, b) in zip(got, want):
            assert a == b, (label, reg)
    # (the witness's own answers are complete: every record that overlaps a region, by the records themselves)
    by_tid = {}
    for tid, pos, end, _ in records:
        by_tid.setdefault(tid, []).append((pos, end))
    for (tid, beg, end), hits in want[::7]:
        assert len(hits) == sum(1 for pos, rend in by_tid.get(tid, []) if pos < end and rend > beg), (tid, beg, end)
    return sum(len(hits) for _, hits in want)


@pytest.mark.parametrize("block_size", [0xFF00, 4096, 700])
def test_index_of_mixed(tmp_path, block_size):
    p = str(tmp_path / "m.bam")
    write_bam(p, im.MIXED_REFS, im.mixed_reads(), block_size=block_size)
    n = assert_index_serves_htslib(tmp_path, p, im.MIXED_REFS, {"index_of": im.index_of(p), "write_bam": open(p + ".bai", "rb").read()})
    assert n > 50_000


def test_index_of_runs(tmp_path):
    reads = im.run_reads()[:10_000]
    refs = [("one", 1_000_000)]
    p = str(tmp_path / "r.bam")
    write_bam(p, refs, reads)
    runs, last = [], None
    for _, pos, end, _ in im.build(p)[3]:
        b = im._reg2bin(pos, end)
        if b == last:
            runs[-1] += 1
        else:
            runs.append(1)
            last = b
    assert runs[:10] == im.RUN_LENGTHS and len(runs) > 10      # the cut keeps a whole run of every length
    n = assert_index_serves_htslib(tmp_path, p, refs, {"index_of": im.index_of(p), "write_bam": open(p + ".bai", "rb").read()})
    assert n > 1000


def test_index_of_degenerate_files(tmp_path):
    from test_index_model import record_ending_on_a_block_end

    refs = [("a", 1000)]
    for name, reads in (("none", []), ("unplaced", [dict(tid=-1, pos=-1, cigar="", seq="ACGT")] * 3)):
        p = str(tmp_path / (name + ".bam"))
        write_bam(p, refs, reads)
        assert assert_index_serves_htslib(tmp_path, p, refs, {"index_of": im.index_of(p), "write_bam": open(p + ".bai", "rb").read()}) == 0
    p, _ = record_ending_on_a_block_end(tmp_path)
    n = assert_index_serves_htslib(tmp_path, p, refs, {"index_of": im.index_of(p), "write_bam": open(p + ".bai", "rb").read()})
    assert n > 0


@pytest.mark.parametrize("name", ["sorted.bam", "clipped3.bam"])
def test_htslib_reproduces_the_committed_indexes(tmp_path, name):
    """The two .bai fixtures are what this htslib writes, byte for byte: the witness is the library that made them."""
    p = os.path.join(GOLDEN, name)
    assert hts.index(p, str(tmp_path / "x.bai")) == open(p + ".bai", "rb").read()


# =====================================================================================================================
# 4. FASTA: the index and the fetch
# =====================================================================================================================
@pytest.fixture(scope="module")
def fasta_index_exe(tmp_path_factory):
    """tests/cpp/fasta_index.cc with GenomeMapper, which needs nothing of the device library."""
    host = os.path.join(ROOT, "portcullis_amd", "host")
    exe = str(tmp_path_factory.mktemp("fasta_index") / "fasta_index")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", f"-I{host}/include", f"-I{ROOT}/include", "-o", exe,
                           os.path.join(HERE, "cpp", "fasta_index.cc"), os.path.join(host, "src", "genome_mapper.cc"), "-lpthread"])
    return exe


def fasta_text(records, term="\n", last_newline=True):
    """records: [(header line without '>', sequence, width)]."""
    out = ""
    for head, seq, w in records:
        out += ">" + head + term + "".join(seq[k:k + w] + term for k in range(0, len(seq), w))
    return out if last_newline else out[:-len(term)]


def bases(n, seed=1):
    return np.random.default_rng(seed).choice(np.frombuffer(b"ACGTacgtNnRYKM", dtype=np.uint8), n).tobytes().decode()


RECORDS = [("full_last some description", bases(120, 1), 60), ("short_last", bases(61, 2), 60), ("seven\tx", bases(7, 3), 60),
           ("one_base", "G", 60), ("wide", bases(333, 4), 333), ("whole_lines", bases(50 * 9, 5), 50)]
ACCEPTED = {
    "lf": fasta_text(RECORDS),
    "crlf": fasta_text(RECORDS, term="\r\n"),
    "no_last_newline": fasta_text(RECORDS[:2], last_newline=False),
    "no_last_newline_full_width": fasta_text(RECORDS[:1], last_newline=False),
    "header_without_newline_but_a_blank": fasta_text(RECORDS[:1]) + ">tail ",
    "one_record_one_base": ">x\nA\n",
    "blank_lines_after_the_header": ">a\n\n\n" + bases(70, 6)[:60] + "\n" + bases(70, 6)[60:] + "\n>b\nACGT\n",
    "blank_lines_at_a_records_end": ">a\nACGTACGT\nACGT\n\n\n>b\nACGTACGT\nACGTACGT\n\n>c\nAC\n\n",
    "crlf_blank_line_at_the_end": ">a\r\nACGT\r\nAC\r\n\r\n",
    "blanks_inside_a_line": ">a\nAC GT\nAC GT\nA\n",
    "spaces_before_the_name": ">  a b\nACGT\n>\tc\nAC\n",
    "a_record_without_sequence": ">first\nACGTAC\nAC\n>empty\n>after\nACG\n",
    "an_empty_first_record": ">empty\n>after\nACG\n",
    "a_duplicated_name": ">a\nACGT\n>b\nAC\n>a\nACGTACGT\n",
    "a_header_without_a_name": ">a\nACGT\n>\nAC\n",
}
REFUSED = {
    "empty_file": "",
    "only_blank_lines": "\n\n",
    "ragged": ">ragged\n" + "A" * 60 + "\n" + "C" * 70 + "\n" + "G" * 10 + "\n",
    "longer_last_line": ">a\nACGT\nACGTA\nAC\n",
    "short_line_inside": ">a\nACGT\nAC\nACGT\n",
    "blank_inside_a_line": ">blank\n" + "A" * 60 + "\n" + "C" * 30 + " " + "C" * 29 + "\n" + "G" * 60 + "\n",
    "empty_line_inside": ">a\nACGT\n\nACGT\n",
    "empty_line_then_blank_line_then_more": ">a\nACGT\n\n \n\n",
    "crlf_empty_line_inside": ">a\r\nACGT\r\n\r\nACGT\r\n",
    "last_header_without_newline": ">a\nACGT\n>b",
    "second_record_ragged": ">a\nACGT\nACGT\n>b\nAC\nACGT\nAC\n",
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_fai_of_the_host_writer_is_htslibs(tmp_path, fasta_index_exe, case):
    for who in ("host", "hts"):
        os.makedirs(tmp_path / who)
        with open(tmp_path / who / "g.fa", "w", newline="") as f:
            f.write(ACCEPTED[case])
    assert hts.faidx(str(tmp_path / "hts" / "g.fa")) == 0
    want = open(tmp_path / "hts" / "g.fa.fai", "rb").read()
    assert want
    p = subprocess.run([fasta_index_exe, "build", str(tmp_path / "host" / "g.fa")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert open(tmp_path / "host" / "g.fa.fai", "rb").read() == want


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_fasta_that_htslib_refuses_is_refused(tmp_path, fasta_index_exe, case):
    fa = str(tmp_path / "g.fa")
    with open(fa, "w", newline="") as f:
        f.write(REFUSED[case])
    assert hts.faidx(fa) == 1 and not os.path.exists(fa + ".fai")
    p = subprocess.run([fasta_index_exe, "build", fa], capture_output=True, text=True)
    assert p.returncode == 1 and "Could not index genome file" in p.stderr, (p.returncode, p.stderr)
    assert not os.path.exists(fa + ".fai")


@pytest.mark.parametrize("width", [60, 7])
def test_fai_of_write_fasta_is_htslibs(tmp_path, width):
    fa = str(tmp_path / "g.fa")
    write_fasta(fa, [(h.split()[0], s) for h, s, _ in RECORDS] + [("none", ""), ("last", "ACGTACGTA")], width=width)
    ours = open(fa + ".fai", "rb").read()
    os.remove(fa + ".fai")
    assert hts.faidx(fa) == 0
    assert open(fa + ".fai", "rb").read() == ours
    fa2 = str(tmp_path / "h.fa")                      # a record without bases in front: htslib has no line width to repeat
    write_fasta(fa2, [("none", ""), ("x", "ACGT")], width=width)
    ours = open(fa2 + ".fai", "rb").read()
    os.remove(fa2 + ".fai")
    assert hts.faidx(fa2) == 0
    assert open(fa2 + ".fai", "rb").read() == ours


@pytest.mark.parametrize("term", ["\n", "\r\n"])
def test_fetch_clamp(tmp_path, fasta_index_exe, term):
    """Every (beg, end) in [-3, len + 3]^2 on records of 1, 7, 61 and 120 bases at line width 60: faidx_fetch_seq against the
    oracle's fetch_bases, the numpy restatement of the device's rule (test_host_fasta_raw.delinearize) under the same clamp,
    and GenomeMapper::fetchBases."""
    from test_host_fasta_raw import delinearize

    records = [(f"r{n}", bases(n, n), 60) for n in (1, 7, 61, 120)]
    fa = str(tmp_path / "g.fa")
    with open(fa, "w", newline="") as f:
        f.write(fasta_text(records, term=term))
    assert hts.faidx(fa) == 0
    whole = open(fa, "rb").read()
    fai = {l.split("\t")[0]: [int(x) for x in l.split("\t")[1:]] for l in open(fa + ".fai").read().splitlines()}
    queries, want_orc, want_np = [], [], []
    for name, seq, _ in records:
        n, off, lb, lw = fai[name]
        assert n == len(seq)
        flat, ok = delinearize(whole[off:off + (n - 1) // lb * lw + (n - 1) % lb + 1], n, lb, lw)
        assert ok and flat == seq.encode()
        for beg in range(-3, n + 4):
            for end in range(-3, n + 4):
                queries.append((name, beg, end))
                want_orc.append(orc.fetch_bases(seq, beg, end))
                want_np.append(orc.fetch_bases(flat, beg, end))
    got = hts.fetch(fa, queries)
    text = subprocess.run([fasta_index_exe, "fetch", fa], input="".join(f"{n} {b} {e}\n" for n, b, e in queries), capture_output=True, text=True,
                          check=True).stdout.split("\n")[:-1]
    assert len(text) == len(queries) == len(got)
    for q, (ln, s), a, b, host in zip(queries, got, want_orc, want_np, text):
        assert ln == len(s) and s.encode() == a == b, q
        assert host == f"{ln} {s}", q
