"""The catalogue of single-fault inputs: one malformed record (or one junction whose window leaves the contig) per entry, with
the code the reference's condition maps to, the index of the read at fault and the kernel that reports it on the device.  Plain
data and small builders -- no GPU import: tests/test_oracle_error_codes.py pins every entry against the CPU oracle, and
tests/test_gpu_error_parity.py runs them through the C ABI.

Every batch is well formed (offsets consistent, arrays of the stated lengths); only the record's meaning is off.

Codes without an entry, and why (oracle/portcullis_oracle.c beside anchor_side / k5_finalize of csrc/pjb_kernels.hip.h):

 -5  GENOME_RANGE      padded_genome asks for [rPos - start, + len) of the fetched anchor with start <= q_start <= rPos and
                       rPos + len - 1 <= q_end <= end: inside an anchor of the expected end - start + 1 letters.  A shorter
                       anchor (a window that leaves the contig) is ANCHOR_LEN in process_junction_window before any read is walked.
 -6  QREGION           q_start = max(position, start) >= start and q_end = min(rPos - 1, end) <= end by construction
                       (padded_query :400-401); the kernel says the same ("unreachable, kept for parity").
 -11 MIN_ANCHOR        orc_min_anchor's callers (add_junctions) pass left = lStart <= lEndExc = start, operation lengths being
                       unsigned, and right = rEndExc - 1 with rEndExc >= rStart = end + 1 before and after both clamps (an end
                       clamped to ref_len - 2 meets a right clamped to ref_len - 1).  A zero-length or back operation next
                       to the N adds 0 to either side.  Only positions past 2^31 (signed overflow in the reference) get there.
 -12 HAMMING_LEN       calc_match_stats compares strings it has just found equal in length (ANCHOR_MISMATCH otherwise);
                       orc_hamming_scores cuts both intron flanks (10 letters once INTRON_FLANK_LEN has passed) to the anchors'
                       min(10, length), so both pairs have equal lengths.
 -20 DIVERGENT         device only.  The query walk and the genome walk of anchor_side start at the same operation (q_start is
                       start unless the read begins inside the window, and then both begin at its first operation), stop at
                       the same one (the query walk stops where rPos > end or an N crosses end, which is where rPos > q_end),
                       and an operation between the two emits min(ln, end - rPos + 1) in both (q_end < end only when
                       the walk stopped before end, and then every emitting operation ends at or before q_end).  So qEmit == gEmit
                       operation by operation: no input reaches it, and the oracle's ANCHOR_MISMATCH is only ever "0 vs 0"
                       (FUZZ_FOUND_ONLY_EMPTY_ANCHORS in tests/test_oracle_error_codes.py searches for a counter-example).
"""
from collections import namedtuple

import numpy as np

from fixtures_micro import read_from_genome

G = "".join(np.random.default_rng(99).choice(list("ACGT"), size=6000))  # (the contig of tests/test_gpu_edge_cases.py)

# at: index of the read at fault in `reads` (they are in coordinate order), or "window" for a junction-level fault (k5_finalize
# reports those under a sentinel ordinal).  code: what the device reports.  oracle: what the oracle raises -- the same code, or
# None where the condition is the device's own (the oracle is not to be run on that input).
Fault = namedtuple("Fault", "name reads at code oracle kernel")
WINDOW = "window"
WINDOW_ORDINALS = tuple(0xffffff00 + k for k in range(4))  # k5_finalize: SPLICE_SITE_LEN, ANCHOR_LEN, INTRON_FLANK_LEN, HAMMING_LEN


def rd(pos, cigar, **kw):
    return read_from_genome(G, pos, cigar, **kw)


def _op(length, op):
    return (length << 4) | "MIDNSHP=XB".index(op)


def _f(name, reads, at, code, kernel, oracle="same"):
    return Fault(name, reads, at, code, code if oracle == "same" else oracle, kernel)


CLEAN = rd(900, "50M100N50M")  # a well-formed neighbour: the fault is then not the first read
K4B = "k4b_generic (anchor_side)"

CATALOGUE = [
    # ---- -1 BAD_XS: k1_count, both of its paths (the rounds path here, the whole-tile path in the position sweep)
    _f("bad_xs_value", [dict(pos=1000, cigar="50M100N50M", seq=G[1000:1050] + G[1150:1200], xs="*")], 0, -1, "k1_count"),
    _f("bad_xs_on_unspliced_read", [dict(pos=900, cigar="50M", seq=None, xs="x"), rd(1000, "50M100N50M")], 0, -1, "k1_count"),
    _f("bad_xs_behind_a_clean_read", [CLEAN, dict(pos=1010, cigar="50M", seq=None, xs="!")], 1, -1, "k1_count"),
    # ---- -2 NO_PRESENCE: an N operation with nothing aligned on one side, bam_alignment.cc:342
    _f("cigar_starts_with_refskip", [dict(pos=1000, cigar="100N50M", seq=G[1100:1150], xs="+")], 0, -2, K4B),
    _f("cigar_ends_with_refskip", [dict(pos=1000, cigar="50M100N", seq=G[1000:1050], xs="+")], 0, -2, K4B),
    _f("softclip_then_refskip", [rd(1000, "5S100N50M")], 0, -2, K4B),
    _f("refskip_then_softclip", [rd(1000, "50M100N5S")], 0, -2, K4B),
    _f("refskip_then_insertion", [CLEAN, rd(1000, "50M100N5I")], 1, -2, K4B),
    _f("refskip_then_back_op", [dict(pos=1000, cigar=np.array([_op(50, "M"), _op(100, "N"), _op(3, "B")], np.uint32), seq=G[1000:1050], xs="+")],
       0, -2, K4B),
    # ---- -3 ZERO_LEN_OP, bam_alignment.cc:363
    _f("zero_length_match_in_anchor", [rd(1000, "50M100N0M50M")], 0, -3, K4B),
    _f("zero_length_insertion_before_refskip", [CLEAN, rd(1000, "20M2D28M0I100N50M")], 1, -3, K4B),
    # ---- -4 QUERY_RANGE, bam_alignment.cc:376: the CIGAR asks for more bases than the record has
    _f("sequence_shorter_than_cigar", [dict(pos=1000, cigar="50M100N50M", seq="ACGT" * 10, xs="+")], 0, -4, K4B),  # M N M, off k1_emit's closed form (l_qseq)
    _f("sequence_shorter_than_cigar_with_deletion", [CLEAN, dict(pos=1000, cigar="20M2D28M100N50M", seq="ACGT" * 10, xs="+")], 1, -4, K4B),
    # ---- -7 ANCHOR_MISMATCH, junction.cc:192-223: an anchor without a single letter
    _f("read_runs_off_contig_end", [rd(5900, "50M100N60M")], 0, -7, K4B),
    _f("refskip_runs_off_contig_end", [rd(5900, "50M200N50M")], 0, -7, K4B),
    _f("two_introns_back_to_back", [CLEAN, rd(1000, "50M100N200N50M")], 1, -7, K4B),
    # ---- the window faults of Junction::processJunctionWindow (junction.cc:561-649), in the order it tests them.  The reads carry
    # no bases (calcMatchStats then takes its short branch, junction.cc:168-185) unless the name says otherwise.
    # -8 SPLICE_SITE_LEN: the two donor / acceptor letters reach over a contig end
    _f("acceptor_site_at_contig_start", [dict(pos=0, cigar="1N50M", seq=None, xs="+")], WINDOW, -8, "k5_finalize"),  # junction (0, 0)
    _f("donor_site_at_contig_end", [dict(pos=5949, cigar="50M100N50M", seq=None, xs="+")], WINDOW, -8, "k5_finalize"),  # junction (5999, 5998)
    # -9 ANCHOR_LEN: the left anchor starts before the contig (the library takes a negative position: such a chain runs on raw keys)
    _f("left_anchor_before_contig_start", [dict(pos=-5, cigar="50M100N50M", seq=None, xs="+")], WINDOW, -9, "k5_finalize"),  # junction (45, 144)
    # -10 INTRON_FLANK_LEN: a 3-base intron whose 10-base flank leaves the contig
    _f("intron_flank_past_contig_end", [dict(pos=5945, cigar="50M3N2M", seq=None, xs="+")], WINDOW, -10, "k5_finalize"),  # junction (5995, 5997)
    _f("intron_flank_before_contig_start", [dict(pos=0, cigar="2M3N50M", seq=None, xs="+")], WINDOW, -10, "k5_finalize"),  # junction (2, 4)
    _f("intron_flank_before_contig_start_with_bases", [rd(0, "2M3N50M")], WINDOW, -10, "k5_finalize"),
    # ---- -13 CLIP_RANGE, bam_alignment.cc:263
    _f("softclip_longer_than_read", [dict(pos=1000, cigar="60S50M100N50M", seq="ACGT" * 10, xs="+")], 0, -13, K4B),
    # ---- -14 UNSORTED: the input contract (k1_count; across batches and members in the position sweep)
    _f("read_before_its_predecessor", [rd(1000, "50M100N50M"), dict(pos=900, cigar="50M", seq=None)], 1, -14, "k1_count"),
    # ---- -21 NO_SEQ: the device's own -- a spliced record of l_qseq > 1 whose bases were not submitted (the oracle would read them)
    _f("spliced_read_without_bases", [dict(pos=1000, cigar="50M100N50M", seq=None, l_qseq=100, xs="+")], 0, -21, "k4b_generic", oracle=None),
    _f("spliced_read_without_bases_behind_a_clean_read", [CLEAN, dict(pos=1000, cigar="20M2D28M100N50M", seq=None, l_qseq=98, xs="+")], 1, -21,
       "k4b_generic", oracle=None),
]
BY_NAME = {f.name: f for f in CATALOGUE}
assert len(BY_NAME) == len(CATALOGUE)

NO_INPUT = {-5: "GENOME_RANGE", -6: "QREGION", -11: "MIN_ANCHOR", -12: "HAMMING_LEN", -20: "DIVERGENT"}  # (reasons: the module's docstring)


# ------------------------------------------------------------------ faults planted into a clean background
BACKGROUND_SEED, BACKGROUND_READS = 7100, 2048 + 300  # two whole tiles of K1_TILE = 1024 reads and a partial one
SWEEP_ORDINALS = (0, 1, 2, 3, 63, 64, 1023, 1024, 1025, 2047, BACKGROUND_READS - 1)


K1C_OPSW = 3072  # operations of a whole tile that k1_count's whole-tile path (k1_count_rows) keeps in LDS: a tile with more takes the rounds path


def background(seed=BACKGROUND_SEED, n=BACKGROUND_READS, paired=True):
    """(genome, reads): `n` clean fuzz reads in coordinate order (the oracle raises nothing on them).  Short reads with few
    indels: about 2 400 operations in 1024 reads, so that the whole tiles take k1_count_rows (whole_tile_ops checks it)."""
    from fuzzgen import make_reads
    genome, reads = make_reads(seed, glen=30000, n_reads=n + 60, paired=paired, L=(30, 100),
                               opts=dict(indel=0.02, eqx=0.01, pad=0.0, clip=0.05, hard=0.01))
    assert len(reads) >= n
    return genome, [dict(r) for r in reads[:n]]


def whole_tile_ops(batch, first=0):
    """Operations of every whole tile of 1024 reads of a batch that starts at read `first` of `batch`."""
    c = batch.cig_off
    return [int(c[k + 1024]) - int(c[k]) for k in range(first, batch.n - 1023, 1024)]


def _spliced_at(genome, pos, cigar, **kw):
    assert 0 <= pos and pos + 400 < len(genome), pos
    return read_from_genome(genome, pos, cigar, **kw)


def _plant_bad_xs(genome, reads, k):
    reads[k] = dict(reads[k], xs="*")


def _plant_unsorted(genome, reads, k):
    """Read k moves before its predecessor; no other pair becomes unsorted (read k + 1 still lies behind it)."""
    assert k > 0 and reads[k - 1]["pos"] > 0
    reads[k] = dict(pos=reads[k - 1]["pos"] - 1, cigar="30M", seq=None, flag=reads[k].get("flag", 0), mtid=reads[k].get("mtid", -1), mpos=reads[k].get("mpos", -1))


def _plant_query_range(genome, reads, k):  # M N M
    reads[k] = dict(pos=reads[k]["pos"], cigar="50M100N50M", seq="ACGT" * 10, xs="+")


def _plant_zero_len_op(genome, reads, k):  # a generic shape: a deletion in the left anchor
    reads[k] = _spliced_at(genome, reads[k]["pos"], "20M2D28M100N0M50M")


def _plant_no_seq(genome, reads, k):
    reads[k] = dict(pos=reads[k]["pos"], cigar="50M100N50M", seq=None, l_qseq=100, xs="+")


# name -> (planter, code, whether the oracle knows the condition, first ordinal it can stand at)
PLANTS = {
    "BAD_XS": (_plant_bad_xs, -1, True, 0),               # k1_count
    "UNSORTED": (_plant_unsorted, -14, True, 1),          # k1_count (the first read of a target has no predecessor)
    "QUERY_RANGE": (_plant_query_range, -4, True, 0),     # k4b_generic, M N M
    "ZERO_LEN_OP": (_plant_zero_len_op, -3, True, 0),     # k4b_generic, a generic shape
    "NO_SEQ": (_plant_no_seq, -21, False, 0),             # k4b_generic, before the walks
}
# (no MIN_ANCHOR plant: the catalogue has no input for it)


def plant(genome, reads, kind, k):
    """A copy of `reads` with the fault `kind` at ordinal k (same number of reads, still in coordinate order but for UNSORTED)."""
    out = list(reads)
    PLANTS[kind][0](genome, out, k)
    return out


def window_fault_read(genome_len):
    """A record for the END of a background whose junction window leaves the contig (INTRON_FLANK_LEN, k5_finalize): to be appended."""
    return dict(pos=genome_len - 55, cigar="50M3N2M", seq=None, xs="+")
