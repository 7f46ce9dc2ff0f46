"""The BAI of an EXISTING coordinate-sorted BAM in plain Python: the yardstick of the device indexer (pjb_index_*).

`index_of(path)` restates the definition `write_bam(..., write_index=True)` and BamWriter::indexRecord share, for a
file somebody else wrote: the blocks' file offsets and ISIZEs give the virtual offsets, the records of the
gzip-inflated stream give bins, chunks and the linear index, and the serialisation is write_bam's.
tests/test_index_model.py pins it to write_bam's bytes without a GPU.

Per record with refID >= 0: beg = pos, end = pos + max(1, reference span of the CIGAR), bin = reg2bin(beg, end),
vs = its virtual offset, ve = the next record's (the start of the block behind the last data for the last one).
A record that starts where a block ends belongs to the block behind it.  Chunks per (tid, bin), a record joining the
bin's last chunk when that chunk ends at its vs; lin[tid][w] = vs of the first record overlapping window w.
No pseudo-bin, no trailing count; records with refID < 0 add nothing.
"""
import bisect
import gzip
import struct

from util_bam import _reg2bin


def bgzf_blocks(data):
    """[(file offset, inflated offset)] of every BGZF block + the sentinel (end of file, end of data)."""
    out, o, u = [], 0, 0
    while o < len(data):
        assert data[o:o + 4] == b"\x1f\x8b\x08\x04", o
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        x, bsize = o + 12, None
        while x < o + 12 + xlen:
            si, slen = data[x:x + 2], struct.unpack_from("<H", data, x + 2)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", data, x + 4)[0] + 1
            x += 4 + slen
        out.append((o, u))
        u += struct.unpack_from("<I", data, o + bsize - 4)[0]
        o += bsize
    out.append((o, u))
    return out


def walk_records(stream):
    """(n_ref, [(tid, pos, end, ustart)]) of an inflated BAM stream."""
    assert stream[:4] == b"BAM\x01"
    o = 8 + struct.unpack_from("<i", stream, 4)[0]
    (n_ref,) = struct.unpack_from("<i", stream, o)
    o += 4
    for _ in range(n_ref):
        o += 4 + struct.unpack_from("<i", stream, o)[0] + 4
    recs = []
    while o < len(stream):
        (bs,) = struct.unpack_from("<i", stream, o)
        tid, pos, l_name = struct.unpack_from("<iiB", stream, o + 4)
        (n_cig,) = struct.unpack_from("<H", stream, o + 16)
        span = 0
        for c in struct.unpack_from(f"<{n_cig}I", stream, o + 36 + l_name):
            if (c & 15) in (0, 2, 3, 7, 8):  # M D N = X
                span += c >> 4
        recs.append((tid, pos, pos + max(1, span), o))
        o += 4 + bs
    assert o == len(stream)
    return n_ref, recs


def build(path):
    """-> (n_ref, bins [per target {bin: [[vs, ve]]}], lin [per target {window: vs}], records [(tid, pos, end, vs)])."""
    data = open(path, "rb").read()
    blocks = bgzf_blocks(data)
    ustarts = [u for _, u in blocks]
    with gzip.open(path, "rb") as f:
        stream = f.read()
    assert len(stream) == ustarts[-1]

    def voff(u):
        b = bisect.bisect_left(ustarts, u)  # the first block that starts at u, else the one u lies in
        if b == len(ustarts) or ustarts[b] > u:
            b -= 1
        return (blocks[b][0] << 16) | (u - ustarts[b])

    n_ref, recs = walk_records(stream)
    bins = [dict() for _ in range(n_ref)]
    lin = [dict() for _ in range(n_ref)]
    out = []
    for k, (tid, pos, end, us) in enumerate(recs):
        vs = voff(us)
        ve = voff(recs[k + 1][3] if k + 1 < len(recs) else len(stream))
        out.append((tid, pos, end, vs))
        if tid < 0:
            continue
        ch = bins[tid].setdefault(_reg2bin(pos, end), [])
        if ch and ch[-1][1] == vs:
            ch[-1][1] = ve
        else:
            ch.append([vs, ve])
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            lin[tid].setdefault(w, vs)
    return n_ref, bins, lin, out


def serialise(n_ref, bins, lin):
    o = bytearray(b"BAI\x01" + struct.pack("<i", n_ref))
    for t in range(n_ref):
        o += struct.pack("<i", len(bins[t]))
        for b in sorted(bins[t]):
            o += struct.pack("<Ii", b, len(bins[t][b]))
            for vs, ve in bins[t][b]:
                o += struct.pack("<QQ", vs, ve)
        n_intv = (max(lin[t]) + 1) if lin[t] else 0
        o += struct.pack("<i", n_intv)
        last = 0
        for w in range(n_intv):
            last = lin[t].get(w, last)
            o += struct.pack("<Q", last)
    return bytes(o)


def index_of(path):
    """The .bai bytes of the BAM at `path`."""
    n_ref, bins, lin, _ = build(path)
    return serialise(n_ref, bins, lin)


def serialise_result(n_ref, res):
    """The .bai bytes of a device result (ffi.Context.index_end): chunks are in (tid, bin, file order) already, so this only
    groups them; untouched windows (0) repeat the entry before them."""
    ch = res["chunks"]
    lin_off, lin = res["lin_off"], res["lin"]
    o = bytearray(b"BAI\x01" + struct.pack("<i", n_ref))
    k = 0
    for t in range(n_ref):
        groups = []
        while k < len(ch) and int(ch[k]["tid"]) == t:
            b = int(ch[k]["bin"])
            if not groups or groups[-1][0] != b:
                groups.append((b, []))
            groups[-1][1].append((int(ch[k]["vbeg"]), int(ch[k]["vend"])))
            k += 1
        o += struct.pack("<i", len(groups))
        for b, cs in groups:
            o += struct.pack("<Ii", b, len(cs))
            for vs, ve in cs:
                o += struct.pack("<QQ", vs, ve)
        a, e = int(lin_off[t]), int(lin_off[t + 1])
        o += struct.pack("<i", e - a)
        last = 0
        for w in range(a, e):
            last = int(lin[w]) or last
            o += struct.pack("<Q", last)
    assert k == len(ch), "chunks are not grouped by ascending target"
    return bytes(o)


def parse_bai(d):
    """-> [per target (bins {bin: [(vs, ve)]} in file order of the bins, lin [n_intv], bin order list)]."""
    assert d[:4] == b"BAI\x01"
    (n_ref,) = struct.unpack_from("<i", d, 4)
    o, out = 8, []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", d, o)
        o += 4
        bins, order = {}, []
        for _b in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", d, o)
            o += 8
            bins[b] = [struct.unpack_from("<QQ", d, o + 16 * k) for k in range(n_chunk)]
            order.append(b)
            o += 16 * n_chunk
        (n_intv,) = struct.unpack_from("<i", d, o)
        o += 4
        lin = list(struct.unpack_from(f"<{n_intv}Q", d, o))
        o += 8 * n_intv
        out.append((bins, lin, order))
    return out, d[o:]


def reg2bins(beg, end):
    """SAM spec 5.3: the bins that may hold records overlapping [beg, end)."""
    end -= 1
    out = [0]
    for off, sh in ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14)):
        out += range(off + (beg >> sh), off + (end >> sh) + 1)
    return out


# ---- the inputs the CPU and GPU tests share ---------------------------------------------------------------------
MIXED_REFS = [("big", 1_300_000), ("empty", 5_000), ("mid", 70_000), ("tiny", 40)]


def mixed_reads(seed=11):
    """~4 600 sorted records on MIXED_REFS (one target without reads, one of 40 bases): 100M, introns of 70 .. 300 000 bases,
    a soft clip, an empty CIGAR, 30 unplaced records at the end.  Reaches bins on levels 2 to 5."""
    import numpy as np

    rng = np.random.default_rng(seed)
    reads = []

    def add(tid, pos, cigar):
        n = sum(int(x) for x, op in _ops(cigar) if op in "MIS=X") if cigar != "*" else 0
        reads.append(dict(tid=tid, pos=int(pos), cigar=("" if cigar == "*" else cigar), seq=("A" * n if n else None)))

    introns = [70, 3_000, 20_000, 150_000, 300_000]
    for pos in np.sort(rng.integers(0, 900_000, size=4_000)):
        r = rng.random()
        if r < 0.55:
            add(0, pos, "100M")
        elif r < 0.9:
            add(0, pos, f"50M{introns[int(rng.integers(0, 5))]}N50M")
        elif r < 0.97:
            add(0, pos, "20S30M")
        else:
            add(0, pos, "*")
    for pos in np.sort(rng.integers(0, 69_000, size=560)):
        add(2, pos, "100M" if rng.random() < 0.6 else "50M3000N50M" if pos < 60_000 else "20S30M")
    for pos in (0, 0, 3, 5, 9):
        add(3, pos, "20S30M" if pos < 9 else "*")
    for _ in range(30):
        reads.append(dict(tid=-1, pos=-1, cigar="", seq="ACGT"))
    return reads


def _ops(cigar):
    import re

    return re.findall(r"(\d+)([MIDNSHP=X])", cigar)


RUN_LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def run_reads(n_target=70_000):
    """~70 000 tiny records on one 1 Mb target whose runs of equal bin have the lengths of RUN_LENGTHS, repeated: a run of
    10-base reads inside one 16 kb window (a level-5 bin) alternates with a run of 4-base reads that straddle the window's
    boundary (2M16384N2M: a level-4 bin, or a higher one where the boundary is a larger bin's too).  Three such pairs per window."""
    reads, w, k = [], 0, 0
    while len(reads) < n_target:
        for off in (100, 5_500, 11_000):
            n = RUN_LENGTHS[k % len(RUN_LENGTHS)]
            base = w * 16384 + off
            for j in range(n):
                reads.append(dict(tid=0, pos=base + (j * 4000) // n, cigar="10M", seq="ACGTACGTAC"))
            n = RUN_LENGTHS[(k + 1) % len(RUN_LENGTHS)]
            for j in range(n):
                reads.append(dict(tid=0, pos=base + 4_500 + (j * 300) // n, cigar="2M16384N2M", seq="ACGT"))
            k += 2
        w += 1
    assert (w + 2) * 16384 < 1_000_000
    return reads
