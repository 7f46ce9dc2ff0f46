"""Inputs at chromosome scale: one sparse target of 2^28 + 12 325 bases, reads copied from it, and the read sets of
test_gpu_coordinate_scale.py / test_oracle_scale_inputs.py.

The target is 'A' everywhere but for islands of seeded random ACGT under every read of every read set (300 bases either side of
each anchor), so the oracle and the device see real sequence wherever they look and the array costs nothing to build.  A read set is
a list of SPECS -- (pos, cigar, keywords) -- so that the islands can be planted before the first read copies its bases, and so
that the junctions a set must give are known from the CIGAR strings alone (expected()), independently of both implementations."""
import functools
import re
import time
from collections import Counter

import numpy as np

from parity import assert_rows_equal, region_equal
from portcullis_amd.records import ReadBatch

L_BIG = 2**28 + 3 * 4096 + 37   # 268 447 781: positions of 29 bits, a ragged last bitmap word (37 bases) and a ragged last page; below BAI's 2^29
L_ANCHOR = 2_300_000            # the anchor-edge genome: plain random ACGT
ISLAND = 300
KEYFMT = 2                      # pjb_timing.repeat_reasons: the chain's keys did not fit the digits planned (OVF_KEYFMT)
APART = 32                      # ... the group was taken apart

_OPS = re.compile(r"(\d+)([MIDNSHP=X])")


def spec(pos, cigar, **kw):
    return (int(pos), cigar, kw)


def blocks(pos, cigar):
    """-> (aligned blocks [(ref start, length)], introns [(start, end inclusive)]) of a CIGAR placed at pos."""
    r, m, n = pos, [], []
    for l, c in _OPS.findall(cigar):
        l = int(l)
        if c in "M=X":
            m.append((r, l))
            r += l
        elif c == "N":
            n.append((r, r + l - 1))
            r += l
        elif c == "D":
            r += l
    return m, n


def expected(specs):
    """{(start, end): nb_raw} the read set gives by construction: every N operation of every read is one alignment of its junction."""
    want = Counter()
    for pos, cigar, _ in specs:
        for se in blocks(pos, cigar)[1]:
            want[se] += 1
    return dict(want)


def cluster(base):
    """Five one-intron reads on two junctions that share their donor: (base + 50, base + 149) three times, (base + 50, base + 150) twice
    -- a start bit, two end slots of it."""
    return [spec(base + k, f"{50 - k}M{100 + k % 2}N50M") for k in range(5)]


def cluster_rows(base):
    return {(base + 50, base + 149): 3, (base + 50, base + 150): 2}


def long_intron(pos, nlen):
    return [spec(pos + k, f"{50 - k}M{nlen}N50M") for k in range(3)]


# ---- the read sets -------------------------------------------------------------------------------------------------------------------
# starts of the geometry clusters: bit 0 / bit 63 of a bitmap word, first / last base of a 4 096-base page, either side of the page
# ranks' scan tiles (2 048 pages = 8 388 608 bases), a start in the bitmap's first word, either side of 2^28
GEO_STARTS = [57, 64000, 64063, 5 * 4096 - 1, 5 * 4096, 8388607, 8388608, 16777215, 16777216, 2**28 - 1, 2**28 + 1]
LAST_WORD = [spec(L_BIG - 80 + k, f"{50 - k}M5N10M") for k in range(3)]   # (268447751, 268447755) three times: a start in the ragged last word
LAST_WORD_ROWS = {(L_BIG - 30, L_BIG - 26): 3}
CLUSTER_BASES = [1000, 2047 * 4096 - 30, 2048 * 4096 - 30, 2**28 - 200]
EXC_BASE = 2**28 - 200          # the cluster whose island carries letters outside ACGT (EXC_LETTERS)
# (position, letter): an anchor's first base, its last base, lower case, and the two sides of the boundary between the 64-base
# stretches 2^22 - 1 and 2^22 of the exception bitmap (2^28 - 1 is the last base of the even reads' right anchor, 2^28 of the odd ones')
EXC_LETTERS = [(EXC_BASE, "N"), (EXC_BASE + 2, "c"), (EXC_BASE + 49, "g"), (EXC_BASE + 150, "R"), (EXC_BASE + 151, "t"), (2**28 - 1, "Y"), (2**28, "N"),
               (2**28 - 64, "n"), (2**28 - 65, "K")]


def geometry():
    out = []
    for s in GEO_STARTS:
        out += cluster(s - 50)
    return out + LAST_WORD


def geometry_rows():
    want = dict(LAST_WORD_ROWS)
    for s in GEO_STARTS:
        want.update(cluster_rows(s - 50))
    return want


def clusters():
    out = []
    for b in CLUSTER_BASES:
        out += cluster(b)
    return out


def exception_reads():
    """The cluster under the planted letters, and reads of its junctions with an N of their own in an anchor: at its first base, at its
    last base, in its middle."""
    b = EXC_BASE
    return cluster(b) + [spec(b + 5, "45M100N50M", n_at=0), spec(b + 6, "44M100N50M", n_at=43), spec(b + 7, "43M101N50M", n_at=43),
                         spec(b + 8, "42M101N50M", n_at=91), spec(b + 9, "41M100N50M", n_at=20), spec(b + 9, "41M100N50M")]


KEY_B = long_intron(3000, 262143)                      # 18 bits: the width a fresh context plans
KEY_C = long_intron(4000, 262144)                      # 19 bits
KEY_E = long_intron(600000, 2**20) + long_intron(700000, 2**24 + 5) + long_intron(100, 2**28 - 1)   # 21, 25 and 28 bits (the last ends at 268 435 655)


def key_set(step):
    """The read sets of the key-width sequence: a = clusters, b = a + 262 143, c = b + 262 144, e = c + 2^20, 2^24 + 5, 2^28 - 1."""
    return clusters() + (KEY_B if step in "bce" else []) + (KEY_C if step in "ce" else []) + (KEY_E if step == "e" else [])


# alignments that leave the target (their chains run on raw keys).  test_gpu_groups' taken-apart member / test_gpu_edge_cases'
# read_runs_off_contig_end, 40 bases before the end: the target ends under its first anchor (the record has 40 bases for 110: QUERY_RANGE
# on its own) AND its intron starts behind the end (SPLICE_SITE_LEN on its own).  The same 100 bases before the end, as those tests
# place it (5900 of 6000): one fault.  And two that the reference clamps and accepts.
OFF_END = spec(L_BIG - 40, "50M100N60M")
OFF_END_NEAR = spec(L_BIG - 100, "50M100N60M")
OFF_END_OK = [spec(L_BIG - 30, "60M"), spec(L_BIG - 30, "20M5N40M")]


def unspliced_around(s):
    """Unspliced reads over the flanks and the inside of the introns that start at s (the coverage columns of junc --extra)."""
    return [spec(s - 70 + 9 * j, "60M") for j in range(6)] + [spec(s + 60 + 11 * j, "40M") for j in range(3)] + [spec(s + 105 + 12 * j, "40M") for j in range(3)]


def extra_set():
    out = geometry() + long_intron(600000, 2**20)
    for s in (64000, 5 * 4096, 8388608, 2**28 - 1):
        out += unspliced_around(s)
    return out + [spec(600000 + 2**20 - 20 + 13 * j, "60M") for j in range(5)]


def anchor_specs(a):
    """Anchors of `a` bases: left, right, and the closed middle block of a two-intron read; a copy of each with a substitution at the
    long anchor's first base and at its last base."""
    out = []
    for pos, cigar, first in ((1000, f"{a}M100N50M", 0), (2000, f"50M100N{a}M", 50), (3000, f"50M100N{a}M100N50M", 50)):
        out += [spec(pos, cigar), spec(pos + 1, cigar, sub=first), spec(pos + 2, cigar, sub=first + a - 1)]
    return out


ANCHORS = (0xfffff, 0x100000)

BIG_SETS = {  # name -> specs, on the big target, every alignment inside it
    "geometry": geometry, "clusters": clusters, "exceptions": exception_reads, "key_b": lambda: key_set("b"), "key_c": lambda: key_set("c"),
    "key_e": lambda: key_set("e"), "extra": extra_set,
}
RAW_OK = lambda: key_set("e") + OFF_END_OK   # (the oracle clamps and accepts: test_oracle_scale_inputs pins what it gives)


# ---- genomes -------------------------------------------------------------------------------------------------------------------------
def sparse_genome(length, spec_lists, seed, letters=()):
    """bytes: 'A' but for random ACGT from ISLAND bases before every aligned block of the specs to ISLAND bases behind it; then `letters`."""
    g = np.full(length, ord("A"), np.uint8)
    iv = sorted((max(0, s - ISLAND), min(length, s + l + ISLAND)) for specs in spec_lists for pos, cigar, _ in specs for s, l in blocks(pos, cigar)[0])
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    lo = hi = -1
    for a, b in iv + [(length + 1, length + 1)]:   # (merged: an island is drawn once, whatever overlaps it)
        if a > hi:
            if hi > lo:
                g[lo:hi] = acgt[rng.integers(0, 4, hi - lo)]
            lo, hi = a, b
        else:
            hi = max(hi, b)
    for p, ch in letters:
        g[p] = ord(ch)
    return g.tobytes()


@functools.lru_cache(maxsize=None)
def big_genome():
    """The big target's bytes: ONE object, handed to the oracle and to upload_contig alike."""
    return sparse_genome(L_BIG, [f() for f in BIG_SETS.values()] + [[OFF_END, OFF_END_NEAR] + OFF_END_OK], 20281, EXC_LETTERS)


@functools.lru_cache(maxsize=None)
def anchor_genome():
    rng = np.random.default_rng(20283)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L_ANCHOR)].tobytes()


def rd(pos, cigar, genome=None, **kw):
    """fixtures_micro.read_from_genome's record for a genome of any size (bytes; None: the big target): the bases are copied from
    slices of it and upper-cased, inserted / soft-clipped bases are 'A', sub= substitutes one read base; n_at= puts an N there."""
    view = memoryview(big_genome() if genome is None else genome)
    seq, r = [], pos
    for l, c in _OPS.findall(cigar):
        l = int(l)
        if c in "M=X":
            seq.append(bytes(view[max(r, 0):max(r + l, 0)]))
            r += l
        elif c in "IS":
            seq.append(b"A" * l)
        elif c in "DN":
            r += l
    seq = b"".join(seq).decode().upper()
    sub = kw.pop("sub", None)
    if sub is not None:
        seq = seq[:sub] + ("C" if seq[sub] != "C" else "G") + seq[sub + 1:]
    n_at = kw.pop("n_at", None)
    if n_at is not None:
        seq = seq[:n_at] + "N" + seq[n_at + 1:]
    d = dict(pos=pos, cigar=cigar, seq=seq, flag=0, mapq=60, xs="+", mtid=-1, mpos=-1)
    d.update(kw)
    return d


def reads_of(genome, specs):
    """The specs' records in BAM order (a stable sort: reads of one position keep their order)."""
    return sorted((rd(pos, cigar, genome, **kw) for pos, cigar, kw in specs), key=lambda r: r["pos"])


def rows_by_key(rows):
    return {(int(r["start"]), int(r["end"])): int(r["nb_raw"]) for r in rows}


# ---- the oracle's rows, once per read set --------------------------------------------------------------------------------------------
_ORACLE = {}


def oracle_rows(orc, name, genome, specs, tid=0, orientation="UNKNOWN"):
    """(batch, rows, region) of a read set: computed once per (name, tid) and shared by the tests; nobody writes to it."""
    key = (name, tid, orientation)
    if key not in _ORACLE:
        b = ReadBatch.from_reads(reads_of(genome, specs))
        rows, reg = orc.find_juncs(tid, len(genome), genome, b, orientation)
        rows.setflags(write=False)
        _ORACLE[key] = (b, rows, reg)
    return _ORACLE[key]


def run_variants(ffi, orc, name, genome, specs, variants, flags=0, check=None):
    """routes() of test_gpu_run_sort for a genome that is expensive to upload: every variant -- a dict of pjb_set_option values -- runs
    the read set on a fresh context (upload through the host route), rows and region must equal the oracle's, and the variants'
    collect() bytes each other's.  check(ctx, variant, timing, rows), if given, is called before the context closes.
    -> [timing per variant], each with "wall_s"."""
    b, orows, oreg = oracle_rows(orc, name, genome, specs)
    out, raw = [], []
    for v in variants:
        t0 = time.perf_counter()
        with ffi.Context(0, "UNKNOWN", flags=flags) as ctx:
            for k, val in v.items():
                ctx.set_option(k, val)
            ctx.set_refs([len(genome)])
            drows, dreg = ffi.run_contig(ctx, 0, genome, [b])
            t = ctx.timing()
            region_equal(dreg, oreg)
            assert_rows_equal(drows, orows)
            raw.append(drows.tobytes())
            if check:
                check(ctx, v, t, drows)
        t["wall_s"] = time.perf_counter() - t0
        out.append(t)
    for k in range(1, len(raw)):
        assert raw[k] == raw[0], (variants[k], variants[0])
    return out
