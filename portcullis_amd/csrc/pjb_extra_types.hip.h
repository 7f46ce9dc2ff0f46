// pjb_extra_types.hip.h -- what other units need from the `--extra` family (pjb_extra.hip.h): the name hash (the ingest transcoder computes it),
// the counters and the structures a context keeps of a finished target.
#pragma once

#include "pjb_device.hip.h"

namespace pjb {

// ---- std::hash<std::string> (libstdc++ _Hash_bytes, 64-bit: a MurmurHash64A variant, seed 0xc70f6907) of
// BamAlignment::deriveName() (lib/src/bam_alignment.cc:233-242; lib/include/portcullis/junction.hpp:158).
// `name` has `len` bytes without the NUL.  Used by the device record transcoder; the host transcoder has the
// same function (portcullis/bam/name_hash.hpp).
__host__ __device__ inline u64 std_hash_shift_mix(u64 v) { return v ^ (v >> 47); }
__host__ __device__ inline u64 derive_name_hash(const uint8_t *name, u32 len, u32 flag) {
    const u64 mul = (((u64)0xc6a4a793UL) << 32) + (u64)0x5bd1e995UL;
    uint8_t suf[3] = {'_', 'R', '?'};
    u32 total = len;
    if (flag & 0x1u) {
        suf[2] = (flag & 0x40u) ? '1' : (flag & 0x80u) ? '2' : '?';
        total += 3;
    }
    auto at = [&](u32 i) -> u64 { return i < len ? name[i] : suf[i - len]; };
    u64 hash = 0xc70f6907ULL ^ ((u64)total * mul);
    const u32 aligned = total & ~7u;
    for (u32 p = 0; p < aligned; p += 8) {
        u64 w = 0;
        for (int k = 7; k >= 0; k--) w = (w << 8) | at(p + (u32)k); // little-endian unaligned load
        const u64 data = std_hash_shift_mix(w * mul) * mul;
        hash ^= data;
        hash *= mul;
    }
    if (total & 7u) {
        u64 data = 0;
        for (int n = (int)(total & 7u) - 1; n >= 0; n--) data = (data << 8) + at(aligned + (u32)n);
        hash ^= data;
        hash *= mul;
    }
    hash = std_hash_shift_mix(hash) * mul;
    hash = std_hash_shift_mix(hash);
    return hash;
}

constexpr u32 PLP_MAXCNT = 8000; // bam_plp_init, deps/htslib-1.3/sam.c:1622

struct ExtraCounters { // one per contig, device memory
    u32 n_zero;       // unspliced mapped records with no reference-consuming op (zlist entries)
    u32 n_spliced;    // spliced records appended to the name-code list
    u32 max_buffered; // max over unspliced records of the pileup's buffered-record upper bound (cap detection)
    u32 n_unspliced;  // unspliced mapped records with a reference span
    u32 hot_first, hot_last; // first / last record ordinal whose bound reaches the cap
    u32 n_dropped;
    u32 _pad;
};

// A group of targets finished as one chain keeps its unspliced records in the coordinates of the group's virtual sequence
// (member m at voff[m], GroupTab): what the kernels that convert between a member's own coordinates and those need
struct XMembers {
    int32_t n;
    int32_t tid[GROUP_MAX], voff[GROUP_MAX], len[GROUP_MAX];
};
struct GroupCounters { // behind a slot's SparseCounters and ExtraCounters
    u32 has_spans; // bit m: member m has unspliced records with a span (the coverage hand-over asks per target)
    u32 _pad;
};

struct ExtraRow { // what pjb_extra_finish hands back, parallel to the junction rows
    double mm_score, coverage;
    u32 up_aln, down_aln;
    u32 m_sum; // sum of name multiplicities (uint32 arithmetic as in junction.cc:916-919)
    u32 _pad;
};

struct Gap {
    int32_t start, end; // [start, end)
};

// what a target keeps for pjb_extra_finish (device pointers): the records with a span in rank order, their gaps (record
// order = rank order) and the number of gaps before every 256th of them
struct SparseDepth {
    const int32_t *s_pos, *s_end;
    const Gap *gaps;
    const u32 *gapoff;
    u32 n_reads, n_gaps, max_span, max_gap;
};

} // namespace pjb
