"""The model of `prep --merge` / pjb_bam_merge_*: what several coordinate-sorted files' records are once merged.

The order ("prep --merge"): records ascend by (refID as unsigned, so -1 comes last; then pos); ties go to the
file given earlier, then to the order inside the file.  With the files concatenated in command-line order that is ONE stable sort
-- Python's sorted() is stable -- and the merge of a single file is the identity.

Reads are util_bam-style dicts (what write_bam takes: tid, pos, cigar, seq, flag, mapq, xs, mtid, mpos, name, aux); record_bytes()
restates write_bam's encoding of one of them, so that a merged stream can be compared byte for byte (tests/test_host_merge_model.py
holds the restatement to write_bam itself).
"""
import struct
import zlib

import numpy as np

from portcullis_amd.ffi import bgzf_block_starts
from portcullis_amd.records import encode_cigar, encode_seq
from util_bam import _ref_span, _reg2bin, bam_header


def merge_key(r):
    return (r["tid"] & 0xFFFFFFFF, r["pos"])


def merge_reads(files):
    """files: one list of reads per input, command-line order, each coordinate sorted -> the merged list."""
    return sorted((r for f in files for r in f), key=merge_key)


def stable_split(reads, n_files, rng, weights=None):
    """Deals a sorted list of reads to n_files files at random, keeping the order inside every file."""
    which = rng.choice(n_files, size=len(reads), p=weights)
    return [[r for r, w in zip(reads, which) if w == k] for k in range(n_files)]


def record_bytes(r):
    """The bytes write_bam emits for one read: the 4-byte block_size and the body.  (The read must carry its name.)"""
    cig = r["cigar"]
    cig = encode_cigar(cig) if isinstance(cig, str) else np.asarray(cig, np.uint32)
    seq = r.get("seq")
    if seq is None or seq == "*":
        l_seq, sb, qb = 0, b"", b""
    else:
        l_seq = len(seq)
        sb = encode_seq(seq).tobytes()
        qb = b"\xff" * l_seq
    name = r["name"].encode() + b"\x00"
    pos = r["pos"]
    span = _ref_span(cig)
    end = pos + (span if span > 0 else 1)
    aux = b""
    if r.get("xs") is not None:
        aux += b"XSA" + r["xs"].encode()
    aux += r.get("aux", b"")
    body = struct.pack("<iiBBHHHiiii", r["tid"], pos, len(name), r.get("mapq", 60), _reg2bin(pos, end), len(cig), r.get("flag", 0), l_seq,
                       r.get("mtid", -1), r.get("mpos", -1), 0)
    body += name + cig.astype("<u4").tobytes() + sb + qb + aux
    return struct.pack("<i", len(body)) + body


def record_stream(reads):
    return b"".join(record_bytes(r) for r in reads)


def inflate_members(members, sizes):
    """The packed BGZF members of a result (their lengths in `sizes`) -> list of each member's inflated bytes."""
    assert int(np.sum(sizes, dtype=np.int64)) == len(members)
    out, o = [], 0
    for s in sizes:
        s = int(s)
        m = members[o:o + s]
        assert m[:4] == b"\x1f\x8b\x08\x04" and int.from_bytes(m[16:18], "little") + 1 == s  # BSIZE
        d = zlib.decompress(m, 31)
        assert int.from_bytes(m[-4:], "little") == len(d) and int.from_bytes(m[-8:-4], "little") == zlib.crc32(d)
        out.append(d)
        o += s
    return out


def span_at(data, u):
    """What BamReader::regionSpan describes, for the bytes `data` of a BAM file and the offset `u` of a target's first record in
    the file's inflated stream: (the BGZF bytes from the block that holds the record to the end of the file, the record's offset
    in that block's inflated bytes)."""
    starts = bgzf_block_starts(data)
    at = 0  # inflated offset of block k
    for k in range(len(starts) - 1):
        isize = int.from_bytes(data[starts[k + 1] - 4:starts[k + 1]], "little")
        if u < at + isize:
            return data[starts[k]:], u - at
        at += isize
    return data[starts[-2]:], 0  # (behind the last record: the EOF block, nothing in it)
