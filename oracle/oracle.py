"""ctypes loader for the CPU oracle (oracle/portcullis_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg -- never by the product package.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

CIGAR_CHARS = "MIDNSHP=XB"
NT16 = "=ACMGRSVTWYHKDBN"

ORIENTATION = {"SE": 0, "FR": 1, "RF": 2, "FF": 3, "UNKNOWN": 4}


class OrcReads(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("pos", C.c_void_p),
        ("flag", C.c_void_p),
        ("mapq", C.c_void_p),
        ("xs", C.c_void_p),
        ("l_qseq", C.c_void_p),
        ("mtid", C.c_void_p),
        ("mpos", C.c_void_p),
        ("cig_off", C.c_void_p),
        ("cigar", C.c_void_p),
        ("seq_off", C.c_void_p),
        ("seq4", C.c_void_p),
    ]


ROW_DTYPE = np.dtype(
    [
        ("id", "<u4"),
        ("refid", "<i4"),
        ("start", "<i4"),
        ("end", "<i4"),
        ("left", "<i4"),
        ("right", "<i4"),
        ("read_strand", "u1"),
        ("ss_strand", "u1"),
        ("cons_strand", "u1"),
        ("canonical", "u1"),
        ("da1", "u1", (2,)),
        ("da2", "u1", (2,)),
        ("suspicious", "u1"),
        ("pfp", "u1"),
        ("uniq", "u1"),
        ("primary", "u1"),
        ("nb_raw", "<u4"),
        ("nb_dist", "<u4"),
        ("nb_ms", "<u4"),
        ("nb_um", "<u4"),
        ("nb_bpp", "<u4"),
        ("nb_ppp", "<u4"),
        ("nb_rel", "<u4"),
        ("r1pos", "<u4"),
        ("r1neg", "<u4"),
        ("r2pos", "<u4"),
        ("r2neg", "<u4"),
        ("entropy", "<f8"),
        ("mean_mismatches", "<f8"),
        ("mean_readlen", "<f8"),
        ("max_min_anc", "<u4"),
        ("maxmmes", "<u4"),
        ("hamming5p", "<u4"),
        ("hamming3p", "<u4"),
        ("nb_up_juncs", "<u4"),
        ("nb_down_juncs", "<u4"),
        ("dist_up", "<u4"),
        ("dist_down", "<u4"),
        ("dist_nearest", "<u4"),
        ("jad", "<u4", (20,)),
        ("_pad1", "<u4"),
        ("sum_mismatches", "<u8"),
        ("mm_score", "<f8"),
        ("coverage", "<f8"),
        ("up_aln", "<u4"),
        ("down_aln", "<u4"),
    ],
    align=False,
)


class OrcRegion(C.Structure):
    _fields_ = [
        ("spliced", C.c_uint64),
        ("unspliced", C.c_uint64),
        ("sum_len", C.c_uint64),
        ("min_len", C.c_int32),
        ("max_len", C.c_int32),
    ]


class OracleError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"oracle error {code}: {msg}")
        self.code = code


def build(force=False):
    """Compile liborc.so with gcc (building the checker is not using it)."""
    so = os.path.join(_HERE, "liborc.so")
    src = os.path.join(_HERE, "portcullis_oracle.c")
    hdr = os.path.join(_HERE, "portcullis_oracle.h")
    if (
        force
        or not os.path.exists(so)
        or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr))
    ):
        subprocess.check_call(["make", "-C", _HERE, "liborc.so"], stdout=subprocess.DEVNULL)
    return so


def lib():
    global _LIB
    if _LIB is None:
        so = build()
        L = C.CDLL(so)
        L.orc_last_error.restype = C.c_char_p
        L.orc_entropy.restype = C.c_double
        L.orc_entropy.argtypes = [C.c_void_p, C.c_size_t]
        L.orc_min_anchor.restype = C.c_int64
        L.orc_min_anchor.argtypes = [C.c_int32] * 4
        L.orc_hamming.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.orc_revcomp.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p]
        L.orc_find_juncs.argtypes = [
            C.c_int32,
            C.c_int32,
            C.c_char_p,
            C.POINTER(OrcReads),
            C.c_int,
            C.POINTER(C.c_void_p),
            C.POINTER(C.c_int64),
            C.POINTER(OrcRegion),
        ]
        L.orc_free_rows.argtypes = [C.c_void_p]
        L.orc_finalize.argtypes = [C.c_void_p, C.c_int64, C.c_double]
        for f in ("orc_write_tab", "orc_write_bed", "orc_write_intron_gff", "orc_write_exon_gff"):
            getattr(L, f).restype = C.c_void_p
        L.orc_free_text.argtypes = [C.c_void_p]
        assert C.sizeof(OrcRegion) == 32
        L.orc_sizeof_row.restype = C.c_size_t
        assert L.orc_sizeof_row() == ROW_DTYPE.itemsize, (L.orc_sizeof_row(), ROW_DTYPE.itemsize)
        L.orc_name_hash.restype = C.c_uint64
        L.orc_name_hash.argtypes = [C.c_char_p, C.c_size_t, C.c_uint16]
        L.orc_depth.restype = C.c_int64
        L.orc_depth.argtypes = [C.c_int32, C.POINTER(OrcReads), C.c_void_p]
        L.orc_calc_coverage.restype = C.c_double
        L.orc_calc_coverage.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]
        L.orc_fetch_bases.restype = C.c_int64
        L.orc_fetch_bases.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_size_t]
        L.orc_extra.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
        _LIB = L
    return _LIB


def _err(code):
    raise OracleError(code, lib().orc_last_error().decode(errors="replace"))


# ---------------------------------------------------------------- encoders
def encode_cigar(s):
    """'5S65M200N30M2S' -> uint32 array of BAM-native ops."""
    out = []
    num = ""
    for ch in s:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num) << 4) | CIGAR_CHARS.index(ch))
            num = ""
    return np.array(out, dtype=np.uint32)


def encode_seq(s):
    """letters -> BAM 4-bit packed bytes (high nibble first)."""
    codes = [NT16.index(c) for c in s]
    if len(codes) % 2:
        codes.append(0)
    return np.array([(codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2)], dtype=np.uint8)


# ---------------------------------------------------------------- unit level
def padded_query_seq(cigar, position, aligned_len, query, start, end):
    L = lib()
    cg = encode_cigar(cigar) if isinstance(cigar, str) else np.asarray(cigar, dtype=np.uint32)
    buf = C.create_string_buffer(max(1 << 16, 4 * (end - start + 10)))
    a_s, a_e = C.c_int32(start), C.c_int32(end)
    rc = L.orc_padded_query_seq(
        cg.ctypes.data_as(C.c_void_p), len(cg), C.c_int32(position), C.c_int32(aligned_len), query.encode(),
        C.c_int32(start), C.c_int32(end), C.byref(a_s), C.byref(a_e), buf, C.c_size_t(len(buf)),
    )
    if rc < 0:
        _err(rc)
    return buf.value.decode(), a_s.value, a_e.value


def padded_genome_seq(cigar, position, aligned_len, genome, start, end, q_start, q_end):
    L = lib()
    cg = encode_cigar(cigar) if isinstance(cigar, str) else np.asarray(cigar, dtype=np.uint32)
    buf = C.create_string_buffer(max(1 << 16, 4 * (end - start + 10)))
    rc = L.orc_padded_genome_seq(
        cg.ctypes.data_as(C.c_void_p), len(cg), C.c_int32(position), C.c_int32(aligned_len), genome.encode(),
        C.c_int32(start), C.c_int32(end), C.c_int32(q_start), C.c_int32(q_end), buf, C.c_size_t(len(buf)),
    )
    if rc < 0:
        _err(rc)
    return buf.value.decode()


def hamming(a, b):
    rc = lib().orc_hamming(a.encode(), len(a), b.encode(), len(b))
    if rc < 0:
        _err(rc)
    return rc


def revcomp(s):
    out = C.create_string_buffer(len(s) + 1)
    lib().orc_revcomp(s.encode(), len(s), out)
    return out.raw[: len(s)]


def fetch_bases(genome, beg, end):
    """The oracle's faidx_fetch_seq on an in-memory sequence (0-based inclusive, clamped): the bases as bytes."""
    g = genome.encode() if isinstance(genome, str) else bytes(genome)
    out = C.create_string_buffer(len(g) + 2)
    n = lib().orc_fetch_bases(g, len(g), beg, end, out, len(out))
    if n < 0:
        _err(int(n))
    return out.raw[:n]


def min_anchor(start, end, left, right):
    rc = lib().orc_min_anchor(start, end, left, right)
    if rc < 0:
        _err(rc)
    return rc


def donor_acceptor(seq1, seq2, read_strand=2):
    ss, cons = C.c_int(), C.c_int()
    da1 = (C.c_uint8 * 2)()
    da2 = (C.c_uint8 * 2)()
    rc = lib().orc_donor_acceptor(
        seq1.encode(), C.c_size_t(len(seq1)), seq2.encode(), C.c_size_t(len(seq2)), C.c_int(read_strand),
        C.byref(ss), C.byref(cons), da1, da2,
    )
    if rc < 0:
        _err(rc)
    return rc, ss.value, cons.value, bytes(da1), bytes(da2)


def entropy(positions):
    p = np.ascontiguousarray(np.sort(np.asarray(positions, dtype=np.int32)))
    return lib().orc_entropy(p.ctypes.data_as(C.c_void_p), len(p))


def hamming_scores(la, li, ri, ra, cons_strand):
    h5, h3 = C.c_uint32(), C.c_uint32()
    rc = lib().orc_hamming_scores(
        la.encode(), C.c_size_t(len(la)), li.encode(), C.c_size_t(len(li)), ri.encode(), C.c_size_t(len(ri)),
        ra.encode(), C.c_size_t(len(ra)), C.c_int(cons_strand), C.byref(h5), C.byref(h3),
    )
    if rc < 0:
        _err(rc)
    return h5.value, h3.value


# ---------------------------------------------------------------- path level
def as_soa(x):
    """The records as the oracle's C struct takes them: a dict of numpy arrays with byte-granular uint64 sequence
    offsets.  Accepts such a dict, or a batch in the product's layout (attributes pos, flag, ..., seq_off counted in
    4-byte words: portcullis_amd.records.ReadBatch)."""
    if isinstance(x, dict):
        return x
    return dict(pos=x.pos, flag=x.flag, mapq=x.mapq, xs=x.xs, l_qseq=x.l_qseq, mtid=x.mtid, mpos=x.mpos, cig_off=x.cig_off,
                cigar=x.cigar, seq_off=np.asarray(x.seq_off).astype(np.uint64) * 4, seq4=x.seq4)


def _reads_struct(soa):
    """soa: dict of numpy arrays or a ReadBatch (see as_soa)."""
    soa = as_soa(soa)
    keep = {}
    r = OrcReads()
    r.n = int(len(soa["pos"]))
    spec = [
        ("pos", np.int32), ("flag", np.uint16), ("mapq", np.uint8), ("xs", np.uint8), ("l_qseq", np.int32),
        ("mtid", np.int32), ("mpos", np.int32), ("cig_off", np.uint32), ("cigar", np.uint32),
        ("seq_off", np.uint64), ("seq4", np.uint8),
    ]
    for name, dt in spec:
        a = np.ascontiguousarray(soa[name], dtype=dt)
        if a.size == 0:
            a = np.zeros(1, dtype=dt)
        keep[name] = a
        setattr(r, name, a.ctypes.data)
    return r, keep


def find_juncs(tid, ref_len, genome, soa, orientation="UNKNOWN"):
    """Run the per-contig path.  Returns (rows ndarray[ROW_DTYPE], region dict)."""
    L = lib()
    assert C.sizeof(C.c_double) == 8
    r, keep = _reads_struct(soa)
    rows_p = C.c_void_p()
    n = C.c_int64()
    reg = OrcRegion()
    if isinstance(genome, str):
        genome = genome.encode()
    gbuf = bytes(genome)
    ori = ORIENTATION[orientation] if isinstance(orientation, str) else int(orientation)
    rc = L.orc_find_juncs(tid, ref_len, gbuf, C.byref(r), ori, C.byref(rows_p), C.byref(n), C.byref(reg))
    if rc < 0:
        _err(rc)
    nrows = n.value
    if nrows:
        buf = (C.c_char * (nrows * ROW_DTYPE.itemsize)).from_address(rows_p.value)
        rows = np.frombuffer(buf, dtype=ROW_DTYPE, count=nrows).copy()
    else:
        rows = np.zeros(0, dtype=ROW_DTYPE)
    L.orc_free_rows(rows_p)
    region = dict(spliced=reg.spliced, unspliced=reg.unspliced, sum_len=reg.sum_len, min_len=reg.min_len, max_len=reg.max_len)
    return rows, region


def name_hash(qname, flag):
    """std::hash<std::string>()(deriveName()) of one record (bytes / str name without the NUL)."""
    q = qname.encode() if isinstance(qname, str) else bytes(qname)
    return lib().orc_name_hash(q, len(q), int(flag) & 0xffff)


def depth(ref_len, soa):
    """DepthParser's vector for one target's records (unspliced.bam view); returns (uint32[ref_len], records kept)."""
    r, keep = _reads_struct(soa)
    out = np.zeros(max(ref_len, 1), dtype=np.uint32)
    n = lib().orc_depth(ref_len, C.byref(r), out.ctypes.data_as(C.c_void_p))
    if n < 0:
        _err(int(n))
    return out[:ref_len], int(n)


def calc_coverage(start, end, levels):
    lv = np.ascontiguousarray(levels, dtype=np.uint32)
    return lib().orc_calc_coverage(start, end, lv.ctypes.data_as(C.c_void_p), len(lv))


def extra(ref_lens, soa_by_tid, name_hash_by_tid, rows, max_query_len):
    """calcExtraMetrics on finalised rows.  soa_by_tid / name_hash_by_tid: {tid: soa dict} / {tid: uint64 array}."""
    n = len(ref_lens)
    structs = (OrcReads * n)()
    keep = []
    hp = (C.c_void_p * n)()
    for t in range(n):
        if t in soa_by_tid and len(as_soa(soa_by_tid[t])["pos"]):
            r, k = _reads_struct(soa_by_tid[t])
            h = np.ascontiguousarray(name_hash_by_tid[t], dtype=np.uint64)
            assert len(h) == r.n
            keep += [k, h]
            structs[t] = r
            hp[t] = h.ctypes.data
        else:
            structs[t].n = 0
    lens = np.ascontiguousarray(ref_lens, dtype=np.int32)
    rows = np.ascontiguousarray(rows)
    rc = lib().orc_extra(n, lens.ctypes.data_as(C.c_void_p), C.cast(structs, C.c_void_p), C.cast(hp, C.c_void_p),
                         rows.ctypes.data_as(C.c_void_p), len(rows), int(max_query_len))
    if rc < 0:
        _err(rc)
    return rows


ORIENTATION_LONG = {0: "Single-End (SE)", 1: "Paired-End (FR): Forward Reverse (-> <-)", 2: "Paired-End (RF): Reverse Forward (<- ->)",
                    3: "Paired-End (FF): Forward Forward (-> ->)", 4: "Unknown"}                 # bam_master.hpp:166-175
STRANDEDNESS_LONG = {0: "Unstranded - can't determine transcript strand from read strand", 1: "Firststrand - R1 is not on transcript strand",
                     2: "Secondstrand - R1 is on transcript strand", 3: "Unknown strand protocol"}  # bam_master.hpp:115-123


def determine_strandedness(rows):
    """JunctionSystem::determineStrandedness -> (orientation code, strandedness code)."""
    rows = np.ascontiguousarray(rows)
    o, s = C.c_int(), C.c_int()
    lib().orc_determine_strandedness(rows.ctypes.data_as(C.c_void_p), C.c_int64(len(rows)), C.byref(o), C.byref(s))
    return o.value, s.value


def bamfilt_flags(soa, js_start, js_end, clip_mode="HARD"):
    """BamFilter::filter's decision per record of one target (0 drop, 1 unspliced, 2 spliced kept, 3 MSR kept)."""
    r, keep = _reads_struct(soa)
    S = np.ascontiguousarray(js_start, dtype=np.int32)
    E = np.ascontiguousarray(js_end, dtype=np.int32)
    out = np.zeros(max(int(r.n), 1), dtype=np.uint8)
    mode = {"HARD": 0, "SOFT": 1, "COMPLETE": 2}[clip_mode]
    lib().orc_bamfilt_flags(C.byref(r), S.ctypes.data_as(C.c_void_p), E.ctypes.data_as(C.c_void_p), C.c_int64(len(S)), C.c_int(mode),
                            out.ctypes.data_as(C.c_void_p))
    return out[: int(r.n)]


N_FEATURES, KMER_TABLE, PW_LEN = 34, 3125 * 5, 32


def filt_features(ref_lens, genomes, rows, l95_idx, cp_idx, pass_idx, fail_idx):
    """ModelFeatures: train (L95, coding potential, splicing models) and one feature row per junction.
    genomes: {tid: str/bytes}.  Returns (features [n, 34], models dict in the layout pjb_filt_features takes, L95)."""
    L = lib()
    n = len(ref_lens)
    lens = np.ascontiguousarray(ref_lens, dtype=np.int32)
    bufs = [(genomes[t].encode() if isinstance(genomes.get(t), str) else bytes(genomes.get(t, b""))) for t in range(n)]
    gp = (C.c_char_p * n)(*bufs)
    rows = np.ascontiguousarray(rows)

    def idx(a):
        a = np.ascontiguousarray(a, dtype=np.int64)
        return a, a.ctypes.data_as(C.c_void_p), C.c_int64(len(a))

    a1, p1, n1 = idx(l95_idx)
    a2, p2, n2 = idx(cp_idx)
    a3, p3, n3 = idx(pass_idx)
    a4, p4, n4 = idx(fail_idx)
    F = np.zeros((max(len(rows), 1), N_FEATURES), dtype=np.float64)
    M = np.zeros(6 * KMER_TABLE + 2 * PW_LEN * 5 + 8, dtype=np.float64)
    l95 = C.c_uint32()
    rc = L.orc_filt_features(C.c_int32(n), lens.ctypes.data_as(C.c_void_p), gp, rows.ctypes.data_as(C.c_void_p), C.c_int64(len(rows)),
                             p1, n1, p2, n2, p3, n3, p4, n4, F.ctypes.data_as(C.c_void_p), M.ctypes.data_as(C.c_void_p), C.byref(l95))
    if rc < 0:
        _err(rc)
    names = ["exon", "intron", "donor_t", "donor_f", "acceptor_t", "acceptor_f"]
    models = {nm: M[k * KMER_TABLE:(k + 1) * KMER_TABLE].copy() for k, nm in enumerate(names)}
    o = 6 * KMER_TABLE
    models["donor_pw"] = M[o:o + PW_LEN * 5].copy()
    models["acceptor_pw"] = M[o + PW_LEN * 5:o + 2 * PW_LEN * 5].copy()
    tail = M[o + 2 * PW_LEN * 5:]
    models.update(exon_size=int(tail[0]), intron_size=int(tail[1]), donor_pw_size=int(tail[2]), acceptor_pw_size=int(tail[3]))
    return F[: len(rows)], models, int(l95.value)


def finalize(rows, mean_query_len):
    rows = np.ascontiguousarray(rows)
    lib().orc_finalize(rows.ctypes.data_as(C.c_void_p), len(rows), C.c_double(mean_query_len))
    return rows


def _names(ref_names):
    arr = (C.c_char_p * len(ref_names))(*[n.encode() for n in ref_names])
    return arr


def _text(fn, *args):
    L = lib()
    ln = C.c_size_t()
    p = getattr(L, fn)(*args, C.byref(ln))
    data = C.string_at(p, ln.value)
    L.orc_free_text(p)
    return data


def write_tab(rows, ref_names, ref_lens):
    rows = np.ascontiguousarray(rows)
    lens = np.ascontiguousarray(ref_lens, dtype=np.int32)
    return _text("orc_write_tab", rows.ctypes.data_as(C.c_void_p), C.c_int64(len(rows)), _names(ref_names), lens.ctypes.data_as(C.c_void_p))


def write_bed(rows, ref_names, source="portcullis", version=""):
    rows = np.ascontiguousarray(rows)
    return _text("orc_write_bed", rows.ctypes.data_as(C.c_void_p), C.c_int64(len(rows)), _names(ref_names), source.encode(), version.encode())


def write_intron_gff(rows, ref_names, source="portcullis"):
    rows = np.ascontiguousarray(rows)
    return _text("orc_write_intron_gff", rows.ctypes.data_as(C.c_void_p), C.c_int64(len(rows)), _names(ref_names), source.encode())


def write_exon_gff(rows, ref_names, source="portcullis"):
    rows = np.ascontiguousarray(rows)
    return _text("orc_write_exon_gff", rows.ctypes.data_as(C.c_void_p), C.c_int64(len(rows)), _names(ref_names), source.encode())


def run_prep_like(refs, genomes, batches_by_tid, orientation="UNKNOWN"):
    """The whole junc stage on in-memory inputs: per-contig find_juncs, merge, finalize.
    refs: [(name, len)], genomes: {tid: bytes/str}, batches_by_tid: {tid: ReadBatch-like with to_oracle()}.
    Returns (rows, totals dict)."""
    all_rows = []
    spliced = unspliced = sum_len = 0
    mn, mx = 2**31 - 1, 0
    for tid, (name, ln) in enumerate(refs):
        b = batches_by_tid.get(tid)
        if b is None or b.n == 0:
            continue
        rows, reg = find_juncs(tid, ln, genomes[tid], b, orientation)
        all_rows.append(rows)
        spliced += reg["spliced"]
        unspliced += reg["unspliced"]
        sum_len += reg["sum_len"]
        mn = min(mn, reg["min_len"])
        mx = max(mx, reg["max_len"])
    rows = np.concatenate(all_rows) if all_rows else np.zeros(0, dtype=ROW_DTYPE)
    total = spliced + unspliced
    mean = (sum_len / total) if total else float("nan")
    rows = finalize(rows, mean)
    return rows, dict(spliced=spliced, unspliced=unspliced, sum_len=sum_len, min_len=mn, max_len=mx, mean=mean)
