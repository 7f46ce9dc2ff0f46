"""The CSI of an EXISTING coordinate-sorted BAM in plain Python: the yardstick of the device indexer's CSI mode
(pjb_index_begin_csi / pjb_index_end_csi, `prep --build_csi`) and of BamWriter's `.csi`.

min_shift is 14.  The depth is htslib's choice (sam.c bam_index): the smallest n with 2^(14 + 3 n) >= (longest target) + 256,
unless one is passed.  Per record with refID >= 0: beg = pos, end = pos + max(1, reference span of the CIGAR) -- the span
rule of index_model.py -- and bin = hts_reg2bin(beg, end, 14, depth).  Chunks exactly as the BAI has them: per (tid, bin)
in file order, a record joining the bin's last chunk when that chunk ends at its virtual offset.  The 16 kb linear index is
built as for the BAI, untouched windows are filled from the left (leading ones with the virtual offset of the target's
first record), and loffset(bin) is the filled entry at the bin's first window: htslib's update_loff.

Layout: "CSI\\1", min_shift, depth, l_aux = 0, n_ref; per target n_bin, then the bins ascending as (bin u32, loffset u64,
n_chunk i32, chunks).  No metadata pseudo-bin, no trailing count of unplaced records.  The file is that payload in BGZF
members of at most 0xFF00 inflated bytes with the EOF block behind them.
tests/test_csi_model.py pins all of it to the reference's htslib without a GPU.
"""
import bisect
import gzip
import struct

import index_model as im
import util_bam

MIN_SHIFT = 14


def depth_for(ref_lens):
    longest = max(list(ref_lens) + [0]) + 256
    n, s = 0, 1 << MIN_SHIFT
    while longest > s:
        n, s = n + 1, s << 3
    return n


def level_first(level):
    return ((1 << (3 * level)) - 1) // 7


def reg2bin(beg, end, depth, min_shift=MIN_SHIFT):
    """hts_reg2bin: end exclusive."""
    end -= 1
    s = min_shift
    for level in range(depth, 0, -1):
        if beg >> s == end >> s:
            return level_first(level) + (beg >> s)
        s += 3
    return 0


def level_of(b):
    level = 0
    while level_first(level + 1) <= b:
        level += 1
    return level


def first_window(b, depth):
    """hts_bin_bot: the first 16 kb window of the bin's interval."""
    level = level_of(b)
    return (b - level_first(level)) << (3 * (depth - level))


def reg2bins(beg, end, depth):
    """The bins that may hold records overlapping [beg, end)."""
    end -= 1
    out = []
    for level in range(depth + 1):
        s = MIN_SHIFT + 3 * (depth - level)
        out += range(level_first(level) + (beg >> s), level_first(level) + (end >> s) + 1)
    return out


def ref_lens_of(stream):
    o = 8 + struct.unpack_from("<i", stream, 4)[0]
    (n_ref,) = struct.unpack_from("<i", stream, o)
    o += 4
    lens = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, o)[0]
        lens.append(struct.unpack_from("<i", stream, o + 4 + l_name)[0])
        o += 8 + l_name
    return lens


def build(path, depth=None):
    """-> (n_ref, depth, bins [per target {bin: [[vs, ve]]}], loff [per target {bin: loffset}], records [(tid, pos, end, vs)])."""
    data = open(path, "rb").read()
    blocks = im.bgzf_blocks(data)
    ustarts = [u for _, u in blocks]
    with gzip.open(path, "rb") as f:
        stream = f.read()
    assert len(stream) == ustarts[-1]

    def voff(u):
        b = bisect.bisect_left(ustarts, u)  # the first block that starts at u, else the one u lies in
        if b == len(ustarts) or ustarts[b] > u:
            b -= 1
        return (blocks[b][0] << 16) | (u - ustarts[b])

    if depth is None:
        depth = depth_for(ref_lens_of(stream))
    n_ref, recs = im.walk_records(stream)
    bins = [dict() for _ in range(n_ref)]
    lin = [dict() for _ in range(n_ref)]
    first = [None] * n_ref
    out = []
    for k, (tid, pos, end, us) in enumerate(recs):
        vs = voff(us)
        ve = voff(recs[k + 1][3] if k + 1 < len(recs) else len(stream))
        out.append((tid, pos, end, vs))
        if tid < 0:
            continue
        if first[tid] is None:
            first[tid] = vs
        ch = bins[tid].setdefault(reg2bin(pos, end, depth), [])
        if ch and ch[-1][1] == vs:
            ch[-1][1] = ve
        else:
            ch.append([vs, ve])
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            lin[tid].setdefault(w, vs)
    loff = []
    for t in range(n_ref):
        touched = sorted(lin[t])
        d = {}
        for b in bins[t]:
            k = bisect.bisect_right(touched, first_window(b, depth))  # the last touched window at or before the bin's first
            d[b] = lin[t][touched[k - 1]] if k else first[t]
        loff.append(d)
    return n_ref, depth, bins, loff, out


def serialise(n_ref, depth, bins, loff):
    o = bytearray(b"CSI\x01" + struct.pack("<iiii", MIN_SHIFT, depth, 0, n_ref))
    for t in range(n_ref):
        o += struct.pack("<i", len(bins[t]))
        for b in sorted(bins[t]):
            o += struct.pack("<IQi", b, loff[t][b], len(bins[t][b]))
            for vs, ve in bins[t][b]:
                o += struct.pack("<QQ", vs, ve)
    return bytes(o)


def payload_of(path, depth=None):
    """The inflated .csi bytes of the BAM at `path`."""
    n_ref, depth, bins, loff, _ = build(path, depth)
    return serialise(n_ref, depth, bins, loff)


def container(payload):
    """The .csi file: the payload in BGZF members of at most 0xFF00 bytes, the EOF block last."""
    return b"".join(util_bam._bgzf_block(payload[u:u + 0xFF00]) for u in range(0, len(payload), 0xFF00)) + util_bam.BGZF_EOF


def serialise_result(n_ref, res):
    """The inflated .csi bytes of a device result (ffi.Context.index_end_csi): chunks are in (tid, bin, file order) already
    and carry their bin's loffset, so this only groups them."""
    ch, lo = res["chunks"], res["loffset"]
    o = bytearray(b"CSI\x01" + struct.pack("<iiii", int(res["min_shift"]), int(res["depth"]), 0, n_ref))
    k = 0
    for t in range(n_ref):
        groups = []
        while k < len(ch) and int(ch[k]["tid"]) == t:
            b = int(ch[k]["bin"])
            if not groups or groups[-1][0] != b:
                groups.append((b, int(lo[k]), []))
            assert int(lo[k]) == groups[-1][1], "chunks of one bin disagree about its loffset"
            groups[-1][2].append((int(ch[k]["vbeg"]), int(ch[k]["vend"])))
            k += 1
        o += struct.pack("<i", len(groups))
        for b, loffset, cs in groups:
            o += struct.pack("<IQi", b, loffset, len(cs))
            for vs, ve in cs:
                o += struct.pack("<QQ", vs, ve)
    assert k == len(ch), "chunks are not grouped by ascending target"
    return bytes(o)


def parse(payload):
    """-> (min_shift, depth, [per target ({bin: (loffset, [(vs, ve)])}, bin order list)], rest)."""
    assert payload[:4] == b"CSI\x01"
    min_shift, depth, l_aux, n_ref = struct.unpack_from("<iiii", payload, 4)
    assert l_aux == 0
    o, out = 20, []
    for _ in range(n_ref):
        (n_bin,) = struct.unpack_from("<i", payload, o)
        o += 4
        bins, order = {}, []
        for _b in range(n_bin):
            b, loffset, n_chunk = struct.unpack_from("<IQi", payload, o)
            o += 16
            bins[b] = (loffset, [struct.unpack_from("<QQ", payload, o + 16 * k) for k in range(n_chunk)])
            order.append(b)
            o += 16 * n_chunk
        out.append((bins, order))
    return min_shift, depth, out, payload[o:]


def check_container(data):
    """The BGZF container of a .csi file: members of at most 64 KB, the EOF block last, gzip inflates it.  -> the payload."""
    blocks = im.bgzf_blocks(data)
    assert len(blocks) >= 2
    for (o0, u0), (o1, u1) in zip(blocks, blocks[1:]):
        assert o1 - o0 <= 0x10000 and u1 - u0 <= 0xFF00
    assert data[blocks[-2][0]:] == util_bam.BGZF_EOF
    return gzip.decompress(data)


# ---- the long input the CPU and GPU tests share -----------------------------------------------------------------------
LONG_REFS = [("huge", 2**30 + 5000), ("small", 70_000)]
LONG_BLOCK = 4096


def long_reads():
    """~3 300 sorted records on LONG_REFS: around the start, around 2^29 (where reg2bin ends) and up to the end of a target of
    2^30 + 5000 bases, one read of two 2^28 - 1 introns that lands in bin 0, 300 reads on a small second target."""
    import numpy as np

    rng = np.random.default_rng(3)
    length = LONG_REFS[0][1]
    pos = np.concatenate([rng.integers(0, 2_000_000, size=600), rng.integers(2**29 - 1_000_000, 2**29 + 1_000_000, size=1500),
                          rng.integers(2**30 - 600_000, 2**30 + 4000, size=900)])
    introns = [70, 3_000, 20_000, 150_000, 300_000]
    reads = []
    for p in pos:
        p, r = int(p), rng.random()
        if r < 0.55:
            cig = [(100, "M")]
        elif r < 0.9:
            cig = [(50, "M"), (introns[int(rng.integers(0, 5))], "N"), (50, "M")]
        elif r < 0.97:
            cig = [(20, "S"), (30, "M")]
        else:
            cig = []
        # shortened at the target's end: reference-consuming operations are cut where the target stops
        room, kept = length - p, []
        for n, op in cig:
            if op in "MN":
                n = min(n, room)
                room -= n
            if n > 0:
                kept.append((n, op))
        if kept and kept[-1][1] == "N":
            kept.pop()
        cigar = "".join(f"{n}{op}" for n, op in kept)
        n_seq = sum(n for n, op in kept if op in "MS")
        reads.append(dict(tid=0, pos=p, cigar=cigar, seq=("A" * n_seq if n_seq else None)))
    reads.append(dict(tid=0, pos=2**29 - 40, cigar="30M268435455N268435455N30M", seq="A" * 60))
    reads.sort(key=lambda r: r["pos"])
    for p in np.sort(rng.integers(0, 69_900, size=300)):
        reads.append(dict(tid=1, pos=int(p), cigar="100M", seq="A" * 100))
    return reads


def write_bam_long(path, refs, reads, block_size=0xFF00):
    """util_bam.write_bam without its .bai, the records' 16-bit `bin` field truncated as htslib truncates it: reg2bin of a
    position of 2^29 or more does not fit the field."""
    orig = util_bam._reg2bin
    util_bam._reg2bin = lambda b, e: orig(b, e) & 0xFFFF
    try:
        util_bam.write_bam(path, refs, reads, block_size=block_size, write_index=False)
    finally:
        util_bam._reg2bin = orig


def long_regions():
    """612 regions on LONG_REFS: 606 around 1 000, 2^29 and 2^30 with lengths 1 .. 5 000 000, and six edges."""
    import numpy as np

    rng = np.random.default_rng(7)
    length = LONG_REFS[0][1]
    out = []
    for k in range(606):
        centre = (1_000, 2**29, 2**30)[k % 3]
        beg = max(0, centre + int(rng.integers(-1_000_000, 1_000_000)))
        beg = min(beg, length - 1)
        out.append((0, beg, min(length, beg + (1, 50, 2_000, 40_000, 400_000, 5_000_000)[(k // 3) % 6])))
    out += [(0, 0, length), (0, 2**29 - 1, 2**29), (0, 2**29, 2**29 + 1), (0, length - 1, length), (1, 0, 70_000), (1, 16384, 16385)]
    return out


def brute_force(records, regions):
    """[[(pos, end)]] of the records overlapping each region, in file order."""
    return [[(pos, end) for tid, pos, end, _ in records if tid == t and pos < e and end > b] for t, b, e in regions]


def witness_query(bam, idx, regions, timeout=60):
    """hts_witness.query under a time limit (htslib-1.3 never returns from some queries on a depth-0 CSI):
    [((tid, beg, end), [(pos, end, qname)])]."""
    import subprocess

    import hts_witness as hts

    p = subprocess.run([hts.program(), "query", bam, idx], input="".join(f"{t} {b} {e}\n" for t, b, e in regions), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out, cur = [], None
    for line in p.stdout.splitlines():
        if line.startswith("#"):
            cur = []
            out.append((tuple(int(x) for x in line.split()[1:]), cur))
        elif line.startswith("!"):
            cur.append(line)
        else:
            pos, end, name = line.split(" ", 2)
            cur.append((int(pos), int(end), name))
    assert [k for k, _ in out] == [tuple(r) for r in regions]
    return out
