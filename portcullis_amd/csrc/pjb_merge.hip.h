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
