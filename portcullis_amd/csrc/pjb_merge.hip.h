// pjb_merge.hip.h -- several coordinate-sorted BAM files' records of ONE target merged into one stream, on the device
// (`portcullis_amd prep --merge`, pjb_bam_merge_begin / _file / _end; DESIGN.md section 5, "prep").  Included by pjb_ingest_api.hip only.
//
// The order: pos ascending; equal positions by the file's index, then by the order inside the file.  Every file is sorted already, so
// with the records numbered file after file (the "global ordinal") that is the STABLE sort of the ordinals by pos -- and the identity
// when one file contributed.  The inflated bytes of every file stay where the inflate put them; between inflate and deflate the records
// move once (mg_gather), and nothing but the packed BGZF members crosses to the host.
//
//   bgzf_decode / bgzf_resolve, bam_find_starts / bam_walk : per file, as pjb_submit_bam (pjb_ingest.hip.h): inflated bytes + rec_off
//   mg_keys        : a thread per record of a file: key = pos, size = 4 + block_size, where the record lies; pos inside the target,
//                    pos not below its predecessor's in the same file
//   rs_hist, rs_panel_sums, rs_panel_scan, rs_scatter : the stable LSD passes of pjb_k2_sort.hip.h over (pos, global ordinal), only over
//                    the digits the target's length occupies; skipped when one file contributed.  (Launched by sort_u32_pairs in
//                    the chains' unit: two of them are no templates and can be compiled into one unit of the library only.)
//   mg_off scan    : run_scan over the sizes in sorted order: every record's offset in the merged stream, and the stream's length
//   mg_gather      : a wavefront per record copies it to its place (the one pass over the record bytes)
//   bgzf_deflate / bgzf_pack : the merged stream cut every block_bytes bytes, straight from device memory (pjb_deflate.hip.h)
//
// `prep --sort` (pjb_bam_sort_begin / _piece / _end) orders the records of ALL targets of an unsorted file's run with the same passes,
// scan, gather and deflate; what it adds is sr_keys, which puts target and pos into one key.
#pragma once
#include "pjb_ingest.hip.h"

namespace pjb {

// ctl words (u64) of a file's mg_keys
enum : int {
    MG_CTL_UNSORTED = 0, // smallest ordinal (within the file's records on the target) of a record that goes back in pos, ~0 if none
    MG_CTL_BAD = 1,      // ... of a record whose pos lies outside the target
    MG_CTL_TOTAL = 2,    // the offset scan's total: bytes of the merged stream
    MG_CTL_WORDS = 4,
};

// A thread per record of one file.  U: the file's inflated bytes, rec_off: its records on the target (bam_walk: each has refID == tid
// and lies completely inside U).
__global__ __launch_bounds__(256) void mg_keys(const uint8_t *U, const iu64 *rec_off, iu64 n, int32_t ref_len, iu32 *key, iu32 *size, iu64 *src,
                                               iu64 *ctl) {
    const iu64 i = (iu64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const iu64 off = rec_off[i];
    const int32_t pos = (int32_t)ld32u(U + off + 8);
    if (pos < 0 || pos >= ref_len) atomicMin(&ctl[MG_CTL_BAD], i);
    if (i && pos < (int32_t)ld32u(U + rec_off[i - 1] + 8)) atomicMin(&ctl[MG_CTL_UNSORTED], i);
    key[i] = (iu32)pos;
    size[i] = 4u + ld32u(U + off);
    src[i] = (iu64)(uintptr_t)(U + off);
}

// ctl words (u64) of a piece's sr_keys
enum : int {
    SR_CTL_DESCENT = 0, // smallest ordinal (within the piece) of a record whose key lies below its predecessor's, ~0 if none
    SR_CTL_BAD_TID = 1, // ... of a record whose refID lies outside [-1, n_ref)
    SR_CTL_BAD_POS = 2, // ... of a placed record whose pos lies outside its target
    SR_CTL_LAST = 3,    // the key of the piece's last record
    SR_CTL_UNPLACED = 4, // records with refID == -1 (a count; zeroed, not ~0)
    SR_CTL_TOTAL = 5,   // the offset scan's total: bytes of the sorted stream
    SR_CTL_N = 6,       // the passes' record count (u32)
    SR_CTL_WORDS = 8,
};

// The key of the record at p: (target << pos_bits) | pos, unplaced records (refID -1) behind every target with pos 0.  A record the
// header has no place for gets a key as well (its target or pos clamped): the caller fails the piece, the key only has to stay inside
// the bits the sort runs over.
__device__ __forceinline__ iu64 sr_key_of(const uint8_t *p, const int32_t *ref_len, int32_t n_ref, int pos_bits, bool &bad_tid, bool &bad_pos) {
    const int32_t tid = (int32_t)ld32u(p + 4), pos = (int32_t)ld32u(p + 8);
    bad_tid = tid < -1 || tid >= n_ref;
    bad_pos = false;
    if (tid < 0 || tid >= n_ref) return (iu64)(iu32)n_ref << pos_bits;
    const int32_t len = ref_len[tid];
    bad_pos = pos < 0 || pos >= len;
    return (iu64)(iu32)tid << pos_bits | (bad_pos ? 0u : (iu32)pos);
}

// A thread per record of one piece of a run.  U: the piece's inflated bytes, rec_off: its complete records (bam_walk_all), prev: the key
// of the run's last record before the piece (0 for the first: no key lies below it).  K: u32 where pos_bits + bits_of(n_ref) <= 32.
template <typename K>
__global__ __launch_bounds__(256) void sr_keys(const uint8_t *U, const iu64 *rec_off, iu64 n, const int32_t *ref_len, int32_t n_ref, int pos_bits, iu64 prev,
                                               K *key, iu32 *size, iu64 *src, iu64 *ctl) {
    const iu64 i = (iu64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const iu64 off = rec_off[i];
    bool bad_tid, bad_pos, b0, b1;
    const iu64 k = sr_key_of(U + off, ref_len, n_ref, pos_bits, bad_tid, bad_pos);
    if (i) prev = sr_key_of(U + rec_off[i - 1], ref_len, n_ref, pos_bits, b0, b1);
    if (k < prev) atomicMin(&ctl[SR_CTL_DESCENT], i);
    if (bad_tid) atomicMin(&ctl[SR_CTL_BAD_TID], i);
    if (bad_pos) atomicMin(&ctl[SR_CTL_BAD_POS], i);
    if ((int32_t)ld32u(U + off + 4) == -1) atomicAdd(&ctl[SR_CTL_UNPLACED], 1ull);
    if (i == n - 1) ctl[SR_CTL_LAST] = k;
    key[i] = (K)k;
    size[i] = 4u + ld32u(U + off);
    src[i] = (iu64)(uintptr_t)(U + off);
}

// the sizes in sorted order (order == nullptr: the identity) -> the records' offsets in the merged stream
struct MgSizeFn {
    const iu32 *size, *order;
    __device__ iu64 operator()(iu64 j) const { return size[order ? order[j] : j]; }
};
struct MgOffsetSink {
    iu64 *dst;
    __device__ void operator()(iu64 j, iu64, iu64 ex) const { dst[j] = ex; }
};

// A wavefront per record of the merged stream: record j (global ordinal order[j]) goes from src[] to out + dst[j], size[] bytes.
// Source and destination have byte alignments of their own.  The stores are the destination's aligned dwords, 256 contiguous bytes
// a round; each is put together from the two aligned source dwords it straddles (v_alignbyte); the up to three bytes before the
// destination's first aligned dword and behind its last go one lane each.  Nothing outside [out + dst, out + dst + size) is written.
// Loads: the aligned dword that holds the first source byte begins at most 3 bytes before it -- inside the inflate buffer, whose
// start is aligned --; the last round's second dword ends at most 3 bytes behind the record, within the 64 zeroed bytes every
// inflate output carries behind its data (the "+ 64" of b_inf_out).  A source that is aligned too is copied dword by dword and
// reads nothing outside the record.
__global__ __launch_bounds__(256) void mg_gather(const iu64 *src, const iu32 *size, const iu32 *order, const iu64 *dst, iu64 n, uint8_t *out) {
    const iu64 j = (iu64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    const iu32 lane = threadIdx.x & 63u;
    const iu64 g = order ? order[j] : j;
    const uint8_t *s = (const uint8_t *)(uintptr_t)src[g];
    uint8_t *d = out + dst[j];
    const iu32 len = size[g];
    const iu32 head = (iu32)(-(intptr_t)d) & 3u; // (len >= 36: a record has its 32 fixed bytes)
    if (lane < head) d[lane] = s[lane];
    s += head;
    d += head;
    const iu32 body = len - head, nd = body >> 2, tail = body & 3u;
    const iu32 sa = (iu32)((uintptr_t)s & 3u);
    const iu32 *S = (const iu32 *)(s - sa);
    iu32 *D = (iu32 *)d;
    if (sa == 0) {
        for (iu32 k = lane; k < nd; k += 64) D[k] = S[k];
    } else {
        for (iu32 k = lane; k < nd; k += 64) D[k] = __builtin_amdgcn_alignbyte(S[k + 1], S[k], sa);
    }
    if (lane < tail) d[4 * (size_t)nd + lane] = s[4 * (size_t)nd + lane];
}

} // namespace pjb
