// pjb_device.hip.h -- what more than one translation unit needs on the device side: the types the units share (batches, control block,
// pairs, groups, key format), the wave / block primitives, the generic multi-block scan (pjb_host.hip.h launches it for every unit) and the
// constants that two units size buffers from -- and what more than one stage of the junc chain uses (the end of this file).  The kernels
// themselves are in the headers of their family: pjb_kernels.hip.h (the junc chain; its stages K2d, K2, K2s and K4 in pjb_k2d_ids.hip.h,
// pjb_k2_sort.hip.h, pjb_k2s_runs.hip.h and pjb_k4_pairs.hip.h, which include this file and no other stage), pjb_extra.hip.h, pjb_features.hip.h / pjb_forest.hip.h / pjb_grow.hip.h / pjb_knn.hip.h (filt and train), pjb_ingest.hip.h / pjb_deflate.hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/portcullis_amd.h"

namespace pjb {

typedef unsigned long long u64;
typedef unsigned int u32;

// ---------------------------------------------------------------------------------------------
// device-side structures
// ---------------------------------------------------------------------------------------------
struct DevBatch {
    const int32_t *pos;
    const uint16_t *flag;
    const uint8_t *mapq;
    const uint8_t *xs;
    const int32_t *l_qseq;
    const int32_t *mtid;
    const int32_t *mpos;
    const uint32_t *cig_off;
    const uint32_t *cigar;
    const uint32_t *seq_off;
    const uint8_t *seq4;
    const u64 *name_hash; // --extra only (nullptr otherwise)
    int64_t n;
    uint32_t base;      // global read ordinal of record 0 within the contig
    uint32_t tile_base; // first K1 tile index of this batch
    int32_t prev_pos;   // pos of the last record of the previous batch (sortedness across batches)
    int32_t member;     // the batch's target: its index among the chain's members (GroupTab)
    const int32_t *prev_pos_ptr; // where that position is, when only the device knows it (nullptr: prev_pos holds it)
    const uint32_t *seq2;        // pjb_batch.seq2 seen as words (two 16-bit granules each; nullptr: the batch has 4-bit bases only)
    const uint32_t *seq_exc;     // pjb_batch.seq_exc
};

// error word: min over (ordinal << 8 | -code); ~0 = no error
__device__ inline void set_error(u64 *err, u32 ordinal, int code) {
    atomicMin(err, ((u64)ordinal << 8) | (u64)(u32)(-code));
}

struct TileStats { // per K1 tile
    u32 spliced, unspliced;
    u64 sum_len;
    int32_t min_len, max_len;
    int32_t max_end;   // max(pos + alignedLength)
    int32_t max_nlen;  // longest N op
    int32_t min_pos;
    u32 max_span;      // longest alignment without its N operations (aligned length - sum of N lengths, saturating): see ContigStats::max_span
};
static_assert(sizeof(TileStats) == 40, "TileStats layout");

// Per-contig control block in device memory.  The host sizes buffers and grids from LIMITS it chooses before anything
// runs (pairs, junctions, key format); the kernels read the actual counts from here, and a count that exceeds its limit
// raises an overflow bit and zeroes the count so that everything downstream does nothing.  pjb_finish_contig reads the
// block back once, at the end, and repeats the contig with larger limits if a bit is set.
enum : u32 { OVF_PAIRS = 1u, OVF_KEYFMT = 2u, OVF_JUNC = 4u, OVF_DENSE = 8u, OVF_LISTS = 16u, OVF_RUNS = 64u /* (32: the host's "group taken apart") */ };
struct ContigStats {
    u64 spliced, unspliced, sum_len;
    int32_t min_len, max_len;
    int32_t max_end, max_nlen, min_pos;
    u32 n_tiles;
    u64 n_pairs;   // pairs found (whatever the limit)
    u64 err;
    u32 n_junc, n_runs; // junctions / position runs found (whatever the limit)
    u32 P;         // pairs the pipeline works on: n_pairs, or 0 after an overflow
    u32 J, R;      // junctions / runs the pipeline works on
    u32 n_slots;   // fragment slots: J + the ranges of the sorted pair array (frag_slots)
    u32 overflow;  // OVF_*
    u32 n_cand;    // K2d: keys in the candidate list (every junction at least once, few of them more often)
    u32 n_slices;  // ceil(P / 64): 64-pair slices of the sorted pair array (fragments, run masks)
    u32 list_need; // OVF_LISTS: the fullest sub-list of the read lists (EmitLists) wanted this many entries
    u32 max_span;  // B: the chain's longest alignment without its N operations.  No pair of the chain has istart - lStart or rEnd - iend above
                   // it (a pair's anchors are blocks of one read: junction_system.cc:140-210; the clamps only shorten them), so no junction's
                   // window reaches further than B beyond its intron: k1_emit / k1_generic list a closed read for k4b_generic's window check
                   // only where that can reach a neighbouring intron (window_reach).  All-ones: pjb_set_option("window_skip", 0), list them all
};
static_assert(sizeof(ContigStats) == 112, "ContigStats layout");

// The fragment rule (k4_pairs writes the slots, k5_frag_reduce folds them).  A RANGE is 2^range_shift consecutive 64-pair slices of the
// sorted pair array (pjb_set_option("pair_range", n)); a fragment is a maximal run of one junction inside one range.  Ids ascend along the
// array in steps of 0 or 1 and every id occurs, so id + range index is unique and strictly increasing from fragment to fragment: that is
// the fragment's slot.  One slot is skipped where a junction begins exactly at a range's start, and the last slot is never reached; whoever
// sees either marks it unused (frag_j = -1), nothing is initialised.  Host and device, values in, values out: tests/cpp/pair_range_slots.cc.
constexpr int PAIR_RANGE_SHIFT_MAX = 5; // 32 slices, 2 048 pairs a range
constexpr int PAIR_RANGE_SHIFT_DEFAULT = 3;
__host__ __device__ inline u32 frag_ranges(u32 n_pairs, int range_shift) { // ranges that hold a pair
    return (u32)(((u64)n_pairs + ((u64)64 << range_shift) - 1) >> (6 + range_shift));
}
__host__ __device__ inline u32 frag_slot(u32 jid, u32 pair, int range_shift) { return jid + (pair >> (6 + range_shift)); }
__host__ __device__ inline u32 frag_slots(u32 n_junc, u32 n_pairs, int range_shift) { return n_junc + frag_ranges(n_pairs, range_shift); }
// the slot a pair leaves unused: the one before its own if it begins both a junction and a range (never the array's first pair), the one
// behind its own if it is the array's last pair; -1: none
__host__ __device__ inline int64_t frag_unused_before(u32 jid, u32 pair, bool junction_head, int range_shift) {
    const bool range_head = (pair & (((u32)64 << range_shift) - 1u)) == 0;
    return pair != 0 && range_head && junction_head ? (int64_t)frag_slot(jid, pair, range_shift) - 1 : -1;
}
__host__ __device__ inline int64_t frag_unused_behind(u32 jid, u32 pair, u32 n_pairs, int range_shift) {
    return pair + 1 == n_pairs ? (int64_t)frag_slot(jid, pair, range_shift) + 1 : -1;
}
// room for the slots of any chain within its limits (one to spare: the grids that follow it divide it up)
__host__ __device__ inline u32 frag_slots_limit(u32 junc_limit, u32 pair_limit, int range_shift) {
    return frag_slots(junc_limit, pair_limit, range_shift) + 1;
}
// A closed read [S] B (N B)+ [S]: can some junction's window reach over the intron before / behind the block of `blk` reference positions
// that lies between two of its introns (nl_prev, nl_next long)?  k4b_generic's tests: prev_istart >= anc_l[j], where prev_istart = istart -
// blk - nl_prev and anc_l[j] >= istart - B; next_iend + 1 <= anc_r[j], where next_iend = iend + blk + nl_next and anc_r[j] <= iend + B.
__device__ __forceinline__ bool window_reach(u32 blk, u32 nl_prev, u32 nl_next, u32 B) {
    const u32 l = __builtin_elementwise_add_sat(blk, nl_prev), r = __builtin_elementwise_add_sat(__builtin_elementwise_add_sat(blk, nl_next), 1u);
    return l <= B || r <= B; // (a sum that saturates: only an all-ones B lists the read, and that lists every read)
}

// A pair = one N operation walked (JunctionSystem::addJunctions, junction_system.cc:140-210).  k1_emit writes, in BAM order,
// the pair's intron key (its own array: kd_assign and the sort's first pass stream over the keys alone) and ONE 32-byte record
// with everything the per-junction reductions need; every later kernel that works in sorted order fetches a pair with one
// 32-byte gather (two 16-byte loads from one sector).
struct __attribute__((aligned(16))) PairRec {
    u64 aux;         // per-pair match statistics (pack_res): written by k1_emit for the [S] M N M [S] shape, by k4b_generic for the rest
    int32_t lstart;  // lStart  (left anchor start of this pair)
    int32_t rend;    // rEndExc-1
    int32_t pos;     // read position   (entropy / distinct-alignment runs)
    int32_t aend;    // read end = pos + alignedLength - 1
    u32 meta;        // bit field, see META_*
    u32 updown;      // upjuncs | downjuncs << 16
};
static_assert(sizeof(PairRec) == 32, "PairRec is one 32-byte sector");
struct Pairs {
    u64 *key;     // packed intron key (see make_key), BAM order
    PairRec *rec; // BAM order
    u32 *g;       // global read ordinal of the pair's record -- written for PJB_FLAG_EXTRA contexts only (nullptr otherwise)
};
__device__ __forceinline__ void rec_store(PairRec *dst, const PairRec &r) {
    uint4 *q = reinterpret_cast<uint4 *>(dst);
    q[0] = make_uint4((u32)r.aux, (u32)(r.aux >> 32), (u32)r.lstart, (u32)r.rend);
    q[1] = make_uint4((u32)r.pos, (u32)r.aend, r.meta, r.updown);
}
__device__ __forceinline__ PairRec rec_load(const PairRec *src) {
    const uint4 *q = reinterpret_cast<const uint4 *>(src);
    const uint4 a = q[0], b = q[1];
    PairRec r;
    r.aux = (u64)a.x | ((u64)a.y << 32);
    r.lstart = (int32_t)a.z;
    r.rend = (int32_t)a.w;
    r.pos = (int32_t)b.x;
    r.aend = (int32_t)b.y;
    r.meta = b.z;
    r.updown = b.w;
    return r;
}

enum : u32 {
    META_CAT_MASK = 3u,      // 0 r1pos, 1 r1neg, 2 r2pos, 3 r2neg   (junction.cc:483-498)
    META_MULTI = 1u << 2,    // read has > 1 N op                    (junction.cc:499)
    META_XS_SHIFT = 3,       // 2 bits: 0 unknown, 1 '+', 2 '-'
    META_UM = 1u << 5,       // mapq >= 30                           (junction.cc:773)
    META_BPP = 1u << 6,      // BAM proper-pair flag                 (junction.cc:780)
    META_PPP = 1u << 7,      // calcIfProperPair                     (junction.cc:784)
    META_REL = 1u << 8,      // reliable                             (junction.cc:792)
    META_SIMPLE = 1u << 9,   // CIGAR is [S] M N M [S] and l_qseq matches it: both anchors are single contiguous compares
                             // that do not depend on the junction-level window (k1_emit compares them itself)
};
// per-pair match statistics packed in 64 bits: minMatch | mmes << 20 | mismatches << 40
__device__ __forceinline__ u64 pack_res(u32 minMatch, u32 mmes, u32 mis) {
    return (u64)(minMatch & 0xfffffu) | ((u64)(mmes & 0xfffffu) << 20) | ((u64)mis << 40);
}
constexpr u32 RES_FIELD_MAX = 0xfffffu; // anchors longer than this take the generic path

// ---------------------------------------------------------------------------------------------
// Target GROUPS ("super-chains").  A chain of 45 kernels over one 8 M-read target leaves most of the chip idle in most of
// its kernels; several targets finished together are ONE chain over a virtual sequence in which member i occupies
// [voff_i, voff_i + len_i) (offsets 64-aligned, a gap between members).  k1_emit adds the offset to every coordinate it
// emits, so keys, sort, grouping, anchors and reductions never see the difference -- an intron key still names one
// junction of one target, and key order is (member, start, end).  Only what touches a target's OWN data converts back:
// the genome of a pair / junction (k1_generic, k4b_generic, k5_finalize look the member up by index / position) and the rows
// (refid, local coordinates).  A single target is a group of one with offset 0.
// ---------------------------------------------------------------------------------------------
constexpr int GROUP_MAX = 32;
constexpr int32_t GROUP_GAP = 4096;
struct GroupTab {
    int32_t n;
    int32_t voff[GROUP_MAX]; // ascending
    int32_t len[GROUP_MAX];
    int32_t tid[GROUP_MAX];
    const uint8_t *d[GROUP_MAX];   // upper-cased bases
    const u32 *codes[GROUP_MAX];   // 4-bit codes (nullptr: exotic member)
    const u32 *codes2[GROUP_MAX];  // 2-bit codes and, behind them, the bitmap of the 64-base stretches that hold a character outside ACGT
                                   // (k0_encode2; nullptr with codes)
    u32 exc_members;               // bit m: member m's bitmap has a bit set at all (else k1_emit does not look at it)
};
struct Member {
    int32_t idx, voff, len, tid;
    const uint8_t *d;
    const u32 *codes;
};
__device__ __forceinline__ Member member_of(const GroupTab &T, int32_t vpos) {
    int m = 0;
    if (T.n > 1) {
#pragma unroll
        for (int s = GROUP_MAX / 2; s >= 1; s >>= 1)
            if (m + s < T.n && T.voff[m + s] <= vpos) m += s;
    }
    Member M;
    M.idx = m;
    M.voff = T.voff[m];
    M.len = T.len[m];
    M.tid = T.tid[m];
    M.d = T.d[m];
    M.codes = T.codes[m];
    return M;
}
// per-member counters of a group (what pjb_region_result reports per target)
struct MemberStats {
    u64 spliced, unspliced, sum_len, n_pairs;
    int32_t min_len, max_len;
    u32 n_junc, _pad;
};

// key packing: normal case (start << lbits) | intron_len, fallback raw (start << 32) | (u32)end
struct KeyFmt {
    int raw;   // 1 = raw 64-bit (weird coordinates present)
    int lbits; // bits of intron length
    int total_bits;
};
__device__ __host__ inline u64 make_key(const KeyFmt &f, int32_t istart, int32_t iend) {
    if (f.raw) return ((u64)(u32)istart << 32) | (u64)(u32)iend;
    return ((u64)(u32)istart << f.lbits) | (u64)(u32)(iend - istart + 1);
}
__device__ __host__ inline void unpack_key(const KeyFmt &f, u64 k, int32_t &istart, int32_t &iend) {
    if (f.raw) {
        istart = (int32_t)(u32)(k >> 32);
        iend = (int32_t)(u32)k;
    } else {
        istart = (int32_t)(u32)(k >> f.lbits);
        iend = istart + (int32_t)(u32)(k & ((1ull << f.lbits) - 1)) - 1;
    }
}

// CIGAR op classes by BAM op code "MIDNSHP=XB" (bam_alignment.hpp:75-99)
__device__ __forceinline__ bool op_consumes_ref(u32 op) { return (0x18Du >> op) & 1u; }   // M D N = X
__device__ __forceinline__ bool op_consumes_query(u32 op) { return (0x193u >> op) & 1u; } // M I S = X
enum : u32 { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_H = 5, OP_P = 6, OP_EQ = 7, OP_X = 8 };

// ---------------------------------------------------------------------------------------------
// wave / block primitives (wave = 64 lanes)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
// A barrier that orders LDS traffic only.  __syncthreads() is a workgroup-scope fence as well: hipcc drains vmcnt before it, which
// makes a wave wait for every load it has in flight and for its STORES to be acknowledged -- k1_emit keeps the next trip's loads in
// flight across its barriers on purpose.  Nothing that other waves of the block read from global memory may depend on this.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// A pointer that was READ from memory (a batch descriptor, a pair's sequence address) is a generic pointer to the compiler:
// its loads are flat_load, which count against the LDS counter too and are waited for one by one.  Everything such pointers
// name here is device memory: gload reads through a global pointer.
template <class T>
__device__ __forceinline__ T gload(const T *p) {
    T v;
    __builtin_memcpy(&v, (const __attribute__((address_space(1))) void *)p, sizeof(T));
    return v;
}
// A batch descriptor fetched from device memory (one launch per chain: the block looks its batch up): the same fields as
// pointers into GLOBAL memory, so that what is read through them are global_load / s_load instructions.
#define PJB_GLOBAL __attribute__((address_space(1)))
#define PJB_LDS __attribute__((address_space(3)))
template <class T>
__device__ __forceinline__ const PJB_GLOBAL T *as_global(const T *p) {
    return (const PJB_GLOBAL T *)p;
}
template <class T, class U>
__device__ __forceinline__ T gload_as(const PJB_GLOBAL U *p) { // a T at a global address
    T v;
    __builtin_memcpy(&v, (const PJB_GLOBAL void *)p, sizeof(T));
    return v;
}
struct GBatch {
    const PJB_GLOBAL int32_t *pos;
    const PJB_GLOBAL uint16_t *flag;
    const PJB_GLOBAL uint8_t *mapq;
    const PJB_GLOBAL uint8_t *xs;
    const PJB_GLOBAL int32_t *l_qseq;
    const PJB_GLOBAL int32_t *mtid;
    const PJB_GLOBAL int32_t *mpos;
    const PJB_GLOBAL uint32_t *cig_off;
    const PJB_GLOBAL uint32_t *cigar;
    const PJB_GLOBAL uint32_t *seq_off;
    const PJB_GLOBAL uint8_t *seq4;
    int64_t n;
    uint32_t base, tile_base;
    int32_t prev_pos, member;
    const PJB_GLOBAL int32_t *prev_pos_ptr;
    const PJB_GLOBAL uint32_t *seq2, *seq_exc;
};
#define PJB_CONSTANT __attribute__((address_space(4)))
__device__ __forceinline__ GBatch load_batch(const DevBatch *d) { // (through the constant address space: a uniform index gives scalar loads)
    const PJB_CONSTANT DevBatch *g = (const PJB_CONSTANT DevBatch *)d;
    GBatch b;
    b.pos = as_global(g->pos);
    b.flag = as_global(g->flag);
    b.mapq = as_global(g->mapq);
    b.xs = as_global(g->xs);
    b.l_qseq = as_global(g->l_qseq);
    b.mtid = as_global(g->mtid);
    b.mpos = as_global(g->mpos);
    b.cig_off = as_global(g->cig_off);
    b.cigar = as_global(g->cigar);
    b.seq_off = as_global(g->seq_off);
    b.seq4 = as_global(g->seq4);
    b.n = g->n;
    b.base = g->base;
    b.tile_base = g->tile_base;
    b.prev_pos = g->prev_pos;
    b.member = g->member;
    b.prev_pos_ptr = as_global(g->prev_pos_ptr);
    b.seq2 = as_global(g->seq2);
    b.seq_exc = as_global(g->seq_exc);
    return b;
}
// four consecutive words at a 4-byte aligned address (global_load_dwordx4 accepts that)
struct __attribute__((packed, aligned(4))) Words4 {
    u32 x, y, z, w;
};

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        T t = __shfl_down(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        T t = __shfl_down(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}
// inclusive scan across the wave
template <typename T>
__device__ __forceinline__ T wave_iscan(T v) {
    int l = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        T t = __shfl_up(v, o, 64);
        if (l >= o) v += t;
    }
    return v;
}

// Whole-wave reductions on the DPP path (no LDS traffic, one VALU instruction per step; __shfl_* goes through
// ds_bpermute): quads, half rows, rows of 16, then row_bcast:15 / row_bcast:31 carry the row totals up -- the result
// is in lane 63 and is read back as a scalar.  `IDENT` is what lanes that a step does not write contribute.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ u32 dpp_move(u32 ident, u32 v) {
    return (u32)__builtin_amdgcn_update_dpp((int)ident, (int)v, CTRL, ROW_MASK, 0xf, false);
}
struct DppAdd {
    static constexpr u32 ident = 0u;
    __device__ __forceinline__ static u32 op(u32 a, u32 b) { return a + b; }
};
struct DppMax {
    static constexpr u32 ident = 0u;
    __device__ __forceinline__ static u32 op(u32 a, u32 b) { return a > b ? a : b; }
};
struct DppMin {
    static constexpr u32 ident = 0xffffffffu;
    __device__ __forceinline__ static u32 op(u32 a, u32 b) { return a < b ? a : b; }
};
template <typename Op>
__device__ __forceinline__ u32 wave_fold(u32 v) { // the result where the steps leave it: in lane 63 (the other lanes: partial results)
    v = Op::op(v, dpp_move<0xB1, 0xf>(Op::ident, v));  // quad_perm [1,0,3,2]
    v = Op::op(v, dpp_move<0x4E, 0xf>(Op::ident, v));  // quad_perm [2,3,0,1]
    v = Op::op(v, dpp_move<0x141, 0xf>(Op::ident, v)); // row_half_mirror
    v = Op::op(v, dpp_move<0x140, 0xf>(Op::ident, v)); // row_mirror: every lane of a row holds the row's result
    v = Op::op(v, dpp_move<0x142, 0xa>(Op::ident, v)); // row_bcast:15 into rows 1 and 3
    v = Op::op(v, dpp_move<0x143, 0xc>(Op::ident, v)); // row_bcast:31 into rows 2 and 3
    return v;
}
template <typename Op>
__device__ __forceinline__ u32 wave_total(u32 v) { return (u32)__builtin_amdgcn_readlane((int)wave_fold<Op>(v), 63); }

// exclusive scan over the 256 threads of a block in thread order; returns exclusive prefix, total in *total.
// smem: at least 4 elements of T.  Contains __syncthreads (call uniformly).
template <typename T>
__device__ __forceinline__ T block_escan_256(T v, T *smem, T *total) {
    T inc = wave_iscan(v);
    int w = threadIdx.x >> 6, l = lane_id();
    __syncthreads();
    if (l == 63) smem[w] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        T s = smem[i];
        if (i < w) base += s;
        tot += s;
    }
    *total = tot;
    return base + inc - v;
}

// the same over NW wavefronts (NW = 1: no barrier, no shared memory traffic)
template <int NW, typename T, bool LDS_ONLY = false>
__device__ __forceinline__ T block_escan(T v, T *smem, T *total) {
    T inc = wave_iscan(v);
    if constexpr (NW == 1) {
        *total = __shfl(inc, 63, 64);
        return inc - v;
    } else {
        int w = threadIdx.x >> 6, l = lane_id();
        if constexpr (LDS_ONLY) lds_barrier();
        else __syncthreads();
        if (l == 63) smem[w] = inc;
        if constexpr (LDS_ONLY) lds_barrier();
        else __syncthreads();
        T base = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < NW; i++) {
            T s = smem[i];
            if (i < w) base += s;
            tot += s;
        }
        *total = tot;
        return base + inc - v;
    }
}

// segmented (by key) reduce towards the segment's FIRST lane; equal keys are contiguous across the lanes
template <typename T, typename OP>
__device__ __forceinline__ T seg_reduce_to_head(T v, u32 segkey, OP op) {
    const int l = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        T t = __shfl_down(v, o, 64);
        u32 k = __shfl_down(segkey, o, 64);
        if (l + o < 64 && k == segkey) v = op(v, t);
    }
    return v;
}
struct OpMin { template <typename T> __device__ T operator()(T a, T b) const { return a < b ? a : b; } };
struct OpMax { template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct OpAdd { template <typename T> __device__ T operator()(T a, T b) const { return a + b; } };

// ---------------------------------------------------------------------------------------------
// generic multi-block exclusive scan of u64 values produced by a functor (3 kernels)
// ---------------------------------------------------------------------------------------------
constexpr int SCAN_TILE = 2048; // 256 threads x 8

template <typename F>
__global__ __launch_bounds__(256) void scan_reduce_kernel(F f, u64 n, u64 *tile_sums, const u32 *np) {
    __shared__ u64 sm[4];
    if (np) { // length known on the device only: the grid covers the host's limit, and a count beyond it (there is none) must not reach past the buffers
        const u64 d = *np;
        n = d < n ? d : n;
    }
    u64 base = (u64)blockIdx.x * SCAN_TILE;
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        u64 i = base + (u64)k * 256 + threadIdx.x;
        if (i < n) s += f(i); // (fetching all eight terms first, unconditionally, as k1_count does, changed nothing here: 49 vs 45 us)
    }
    s = wave_sum(s);
    if (lane_id() == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = sm[0] + sm[1] + sm[2] + sm[3];
}

// single block: in-place exclusive scan of tile sums; writes grand total to *total
// (a template only so that every translation unit that scans -- chain, extra, ingest -- instantiates it for itself)
template <int UNUSED = 0>
__global__ __launch_bounds__(1024) void scan_tiles_kernel(u64 *tile_sums, u32 n_tiles, u64 *total) {
    __shared__ u64 wsum[16];
    __shared__ u64 carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (u32 base = 0; base < n_tiles; base += 1024) {
        u32 i = base + threadIdx.x;
        u64 v = i < n_tiles ? tile_sums[i] : 0;
        u64 inc = wave_iscan(v);
        int w = threadIdx.x >> 6;
        if (lane_id() == 63) wsum[w] = inc;
        __syncthreads();
        u64 wb = 0, tot = 0;
        for (int k = 0; k < 16; k++) {
            u64 s = wsum[k];
            if (k < w) wb += s;
            tot += s;
        }
        u64 carry = carry_s;
        if (i < n_tiles) tile_sums[i] = carry + wb + inc - v;
        __syncthreads();
        if (threadIdx.x == 0) carry_s = carry + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}

// third kernel: recompute values, exclusive prefix handed to the sink g(i, value, exclusive_prefix)
template <typename F, typename G>
__global__ __launch_bounds__(256) void scan_apply_kernel(F f, G g, u64 n, const u64 *tile_sums, const u32 *np) {
    __shared__ u64 sm[4];
    if (np) {
        const u64 d = *np;
        n = d < n ? d : n;
    }
    if ((u64)blockIdx.x * SCAN_TILE >= n) return;
    u64 base = (u64)blockIdx.x * SCAN_TILE;
    u64 run = tile_sums[blockIdx.x];
    // thread order within the tile must equal element order: round k covers [base+k*256, +256)
#pragma unroll
    for (int k = 0; k < 8; k++) {
        u64 i = base + (u64)k * 256 + threadIdx.x;
        u64 v = i < n ? f(i) : 0;
        u64 tot;
        u64 ex = block_escan_256<u64>(v, sm, &tot);
        if (i < n) g(i, v, run + ex);
        run += tot;
    }
}

// ---------------------------------------------------------------------------------------------
// The same scan in TWO kernels for contig-sized inputs: every block of the apply kernel adds up the sums of the
// tiles before it itself (at most SCAN2_MAX_TILES plain loads from an L2-resident array, 16 per thread) instead of
// waiting for a single-block kernel in between -- one dependent launch less per scan.  (A one-kernel scan with
// decoupled look-back was built and measured: 2 600 resident tiles polling each other's granules through the fabric
// cost 47-76 us against 29 us for three kernels, with or without fences; it is in the history, not in the tree.)
// ---------------------------------------------------------------------------------------------
constexpr u32 SCAN2_MAX_TILES = 4096;
template <typename F, typename G>
__global__ __launch_bounds__(256) void scan_apply2_kernel(F f, G g, u64 n, const u64 *tile_sums, const u32 *np, u64 *total) {
    __shared__ u64 sm[4];
    __shared__ u64 s_pref[4];
    if (np) {
        const u64 d = *np;
        n = d < n ? d : n;
    }
    const u64 n_tiles = n == 0 ? 1 : (n + SCAN_TILE - 1) / SCAN_TILE; // (an empty input still gets its total written)
    if (blockIdx.x >= n_tiles) return;
    u64 acc = 0;
    for (u32 t = threadIdx.x; t < blockIdx.x; t += 256) acc += tile_sums[t];
    acc = wave_sum(acc);
    if (lane_id() == 0) s_pref[threadIdx.x >> 6] = acc;
    __syncthreads();
    u64 run = s_pref[0] + s_pref[1] + s_pref[2] + s_pref[3];
    if (blockIdx.x == n_tiles - 1 && threadIdx.x == 0) *total = run + tile_sums[blockIdx.x];
    const u64 base = (u64)blockIdx.x * SCAN_TILE;
    // thread order within the tile must equal element order: round k covers [base+k*256, +256)
#pragma unroll
    for (int k = 0; k < 8; k++) {
        u64 i = base + (u64)k * 256 + threadIdx.x;
        u64 v = i < n ? f(i) : 0;
        u64 tot;
        u64 ex = block_escan_256<u64>(v, sm, &tot);
        if (i < n) g(i, v, run + ex);
        run += tot;
    }
}

// scan functors -----------------------------------------------------------------------------------------------
struct ArrU32Fn {
    const u32 *a;
    __device__ u64 operator()(u64 i) const { return a[i]; }
};
struct ArrU8Fn {
    const uint8_t *a;
    __device__ u64 operator()(u64 i) const { return a[i]; }
};
struct ArrU8Bit0Fn { // bit 0 of every byte
    const uint8_t *a;
    __device__ u64 operator()(u64 i) const { return a[i] & 1u; }
};
struct ArrI32Fn { // signed terms, summed modulo 2^64
    const int32_t *a;
    __device__ u64 operator()(u64 i) const { return (u64)(int64_t)a[i]; }
};
struct ExclusiveU32Sink { // out[i] = sum of the terms before i (may alias the input)
    u32 *out;
    __device__ void operator()(u64 i, u64, u64 ex) const { out[i] = (u32)ex; }
};
struct InclusiveU32Sink { // out[i] = sum of the terms up to and including i (may alias the input)
    u32 *out;
    __device__ void operator()(u64 i, u64 v, u64 ex) const { out[i] = (u32)(ex + v); }
};

// a K1 tile: 1024 consecutive reads (k1_count; the host sizes the tiles' arrays from it)
constexpr int K1_TILE = 1024;

// --extra by-products of the first pass (pjb_extra.hip.h, "the sparse path"): which records belong to unspliced.bam and what
// they span -- k1_count has every record's CIGAR in registers anyway
struct SparseCounters { // one per target, device memory (zeroed)
    u32 n_zero;       // unspliced mapped records with no reference-consuming op (zlist entries)
    u32 max_span;     // longest reference span of an unspliced mapped record
    u32 max_gap;      // longest D operation among them
    u32 need_dense;   // bit 0: the pileup cap may bite; bit 1: a record with more than 126 gaps; bit 2: gap list full;
                      // bit 3: a span leaves its member (chains of several members only)
    u64 total;        // written by the scan: unspliced records with a span | gaps << 32
};
constexpr u32 SPARSE_GAP_MAX = 126;
struct XOut {
    int32_t *s_pos, *s_end; // per record (global ordinal): position, exclusive end of the span (= pos: no span / not unspliced.bam)
    uint8_t *q;             // bit 0: has a span, bits 1-7: D operations
    u32 *zlist;             // the unspliced records without a span, two words an entry: its position in its member at [z], the member at
    u32 zcap;               // [zcap + z] (two plain word stores: as one 8-byte store they cost k1_count<true> 16 more spilled registers)
    SparseCounters *cnt;
};
// The one classification of the sparse path: a record's part in unspliced.bam (junction_builder.cc:168-186).  Record `g` of its
// chain starts at `pos`, covers `aligned` bases of the reference and has `ngap` D operations, the longest of `gapmax` bases; it
// belongs to member `member`, which lies at `voff` in the chain's virtual sequence and has `len` bases (a lone target: member 0
// at 0).  Positions and ends are written in virtual coordinates, so that the spans of a whole chain are one position-sorted list; a
// record without a span keeps its own position beside its member.  With several members (`many_members`, uniform) a span that
// leaves its member would reach into the gap behind it or into the next member and is reported; a lone target's may leave it.
struct XLane { // what a lane's records add to the SparseCounters (x_counters)
    u32 span = 0, gapmax = 0; // longest span, longest D operation of a record with a span
    bool many = false;        // a record with more than SPARSE_GAP_MAX gaps
    bool leaves = false;      // a span that leaves its member
};
__device__ __forceinline__ void x_classify(const XOut &X, u32 g, int32_t pos, int32_t aligned, u32 ngap, u32 gapmax, bool spliced, u32 flag,
                                           int32_t voff, int32_t len, u32 member, bool many_members, XLane &a) {
    const bool unspliced = !spliced && !(flag & 0x4u);
    const bool spans = unspliced && aligned > 0 && pos >= 0;
    const int32_t vpos = (int32_t)((u32)pos + (u32)voff);
    X.s_pos[g] = vpos;
    X.s_end[g] = spans ? vpos + aligned : vpos;
    if (!spans) ngap = 0, gapmax = 0;
    if (ngap > SPARSE_GAP_MAX) a.many = true, ngap = SPARSE_GAP_MAX;
    X.q[g] = (uint8_t)((spans ? 1u : 0u) | (ngap << 1));
    if (spans) a.span = max(a.span, (u32)aligned);
    a.gapmax = max(a.gapmax, gapmax);
    if (many_members && spans && (int64_t)pos + aligned > (int64_t)len) a.leaves = true;
    if (unspliced && aligned == 0) { // getEnd() == pos - 1: tested one by one by the flank kernels (practically never)
        const u32 z = atomicAdd(&X.cnt->n_zero, 1u);
        if (z < X.zcap) X.zlist[z] = (u32)pos, X.zlist[X.zcap + z] = member;
    }
}
// the lanes' contributions into the counters; every lane of the wavefront calls this
__device__ __forceinline__ void x_counters(SparseCounters *cnt, const XLane &a) {
    const u32 span = wave_max(a.span), gapmax = wave_max(a.gapmax);
    if (lane_id() == 0) { // (look first: the maxima settle after a few waves)
        if (span > cnt->max_span) atomicMax(&cnt->max_span, span);
        if (gapmax > cnt->max_gap) atomicMax(&cnt->max_gap, gapmax);
    }
    if (a.many) atomicOr(&cnt->need_dense, 2u);
    if (a.leaves) atomicOr(&cnt->need_dense, 8u);
}

// what k5_finalize and kg_features (pjb_features.hip.h) both do to a target's bases
__device__ __forceinline__ uint8_t revcomp_char(uint8_t c) { // REVCOMP_LOOKUP seq_utils.hpp:33-40 (NUL outside A-Z)
    switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'D': return 'H';
    case 'G': return 'C';
    case 'H': return 'D';
    case 'M': return 'K';
    case 'N': return 'N';
    case 'R': return 'Y';
    case 'S': return 'W';
    case 'T': return 'A';
    case 'U': return 'A';
    case 'V': return 'B';
    case 'W': return 'S';
    case 'X': return 'X';
    case 'Y': return 'R';
    default: return 0;
    }
}

// faidx_fetch_seq clamping (deps/htslib-1.3/faidx.c:453-457): returns clamped [b,e]
__device__ __forceinline__ void fetch_clamp(int32_t glen, int32_t &b, int32_t &e) {
    if (e < b) b = e;
    if (b < 0) b = 0;
    else if (glen <= b) b = glen - 1;
    if (e < 0) e = 0;
    else if (glen <= e) e = glen - 1;
}

// byte offsets in the control block that publish_chain (pjb_kernels.hip.h) writes to page-locked host memory
constexpr int PUB_BASE_AT = 240, PUB_ERR_AT = 256, PUB_XCNT_AT = 320 /* --extra: the target's counters, 64 bytes */, PUB_CHECKED_AT = 384 /* reads on k4b_generic's second list */, PUB_GEN_AT = 512, PUB_MEMBERS_AT = 1536, PUB_GREADS_AT = 3072, PUB_BYTES = 4096; // byte offsets in the published block
static_assert(PUB_MEMBERS_AT + GROUP_MAX * sizeof(MemberStats) <= PUB_BYTES && sizeof(MemberStats) % 8 == 0, "control block layout");

// the read lists of a chain (EmitLists, below): sub-lists, and the words of a sub-list's line of counters
constexpr u32 GEN_SHARDS = 256, GEN_CNT_STRIDE = 32;
// Room of a sub-list (before anything says otherwise): k1_emit deals its chunks of 256 spliced reads round-robin to the sub-lists
// (up to 256 entries a chunk on list 2 and on list 3), k1_generic its chunks of 256 items of list 3 (up to 256 entries on list 1
// or 2).  A sub-list that several full chunks of both kernels hit can want more than this: the appends count on, nothing is
// written past the room, the chain is closed (OVF_LISTS, ContigStats::list_need) and repeated with the room it asked for.
__host__ __device__ inline u32 gen_list_cap(u32 pair_limit) {
    const u32 chunks = pair_limit / 256u + 2u;
    return ((chunks + GEN_SHARDS - 1) / GEN_SHARDS) * 256u;
}

// ---------------------------------------------------------------------------------------------
// What more than one stage of the junc chain uses (a stage header includes this file and no other stage): each definition
// stands here once, beside the stages that share it
// ---------------------------------------------------------------------------------------------
// What k1_emit and k1_generic leave beside the pairs: the candidate keys with their start bitmap for K2d (kd_*), the read lists for k1_generic and
// k4b_generic; kd_table and k2_close ask lists_over whether every sub-list stayed within its room
constexpr u64 KD_EMPTY = ~0ull; // no key: a packed key has fewer than 64 bits
constexpr int KD_PAGE_SHIFT = 6; // a page of the start bitmap: 64 words, one wavefront
struct EmitLists {
    u64 *cand;      // candidate keys (nullptr: the chain sorts the full keys and wants none); their count is ContigStats::n_cand
    u64 *bitmap;    // K2d's bitmap of intron starts (all-clear at rest): every candidate sets its start's bit as it is listed
    u32 *page_cnt;  // starts per PAGE of the bitmap (64 words = 4 096 bases; all-zero at rest): counted as their bits are set for the first time
    u64 *cand_anc;  // per candidate: min lStart | max rEnd << 32 over the pairs it stands for (the junction anchors' first level)
    u64 *gen_list;  // [3][GEN_SHARDS][gen_cap], every entry the read's slot in the tiles' spliced lists (spl_idx, spl_rec: what k1_count kept of it)
                    // | index of its first pair << 32.  Lists 1 and 2, for k4b_generic: the reads whose pairs need the generic walks; the reads
                    // whose closed form waits for the window check.  List 3, for k1_generic.
    u32 *gen_cnt;   // [GEN_SHARDS][GEN_CNT_STRIDE]: words 2 l - 2, 2 l - 1 = entries of list l's sub-list, pairs of those reads -- a cache
                    // line per shard: atomics on one line are served one after the other, whatever the address in it
    u32 gen_cap;    // room of one sub-list
    u32 pack_nn;    // 1 (chains of fewer than 2^28 slots): entries of the second list carry min(N operations, 15) in bits 28-31 of the slot
};
// the fullest sub-list of the three lists' sub-lists `shard` (0: all within their room)
__device__ __forceinline__ u32 lists_over(const u32 *gen_cnt, u32 shard, u32 cap) {
    const u32 a = gen_cnt[shard * GEN_CNT_STRIDE], b = gen_cnt[shard * GEN_CNT_STRIDE + 2], c = gen_cnt[shard * GEN_CNT_STRIDE + 4];
    // (the entries of list 3 that found no room were not walked by k1_generic: each of them would have gone on list 1 or 2 -- an
    // upper bound, so that ONE repeat settles the lists)
    const u32 dropped = c > cap ? c - cap : 0u;
    const u32 ab = (a > b ? a : b) + dropped;
    const u32 m = ab > c ? ab : c;
    return m > cap ? m : 0u;
}

// The sort's tile and its digit counter (pjb_k2_sort.hip.h); kd_assign (pjb_k2d_ids.hip.h) works on the same tiles and counts the first digit
// of the ids it hands out
constexpr int RS_ITEMS = 16;
constexpr int RS_TILE = 256 * RS_ITEMS; // 4096 keys per block
constexpr int RS_MAX_BITS = 12;
constexpr int RS_MAX_BINS = 1 << RS_MAX_BITS;
constexpr int KDA_TILE = RS_TILE; // kd_assign's tile is the sort's
static_assert(RS_MAX_BINS <= 4096, "kd_assign counts the sort's first digit tile by tile"); // (its table in LDS: s_h[4096])

// Histogram add of one digit per lane.  Keys arrive nearly sorted and deep junctions repeat one key
// thousands of times, so most lanes of a wave often hold the same digit: the two most common
// leading digits are counted by one lane each (no 64-way same-address LDS conflict), the rest
// with plain LDS atomics.
__device__ __forceinline__ void wave_hist_add(u32 *h, u32 d, bool valid) {
    u64 rem = __ballot(valid);
    const int lane = lane_id();
#pragma unroll
    for (int it = 0; it < 2; it++) {
        if (rem == 0) return;
        const int first = __ffsll((long long)rem) - 1;
        const u32 d0 = __shfl(d, first, 64);
        const u64 m = __ballot(valid && d == d0) & rem;
        if (lane == first) atomicAdd(&h[d0], (u32)__popcll(m));
        rem &= ~m;
    }
    if ((rem >> lane) & 1ull) atomicAdd(&h[d], 1u);
}

// The id runs of the tiles (the run route of the sort, see rs_place): pairs arrive in BAM order and ids are handed out in (start, end)
// order, so the 4 096 ids of a tile lie in a window of a few dozen consecutive ids.  kd_assign counts them in a table indexed by
// id & (RUN_W - 1) -- exact while max - min < RUN_W -- and appends one entry per (tile, id) to the chain's run list: the key
// id << tile_bits | tile and the number of pairs.  Sorted by key, the exclusive prefix sum of the counts is where the run's first
// pair belongs in the sorted pair array.
constexpr u32 RUN_W = 2048;
struct RunOut {
    u64 *key;         // [cap] id << tile_bits | tile, in the order the tiles reserved their room
    u32 *cnt;         // [cap] pairs of the run
    u32 *tile_first;  // [tiles] the tile's first entry,
    u32 *tile_n;      //         and how many it has (ascending ids)
    u32 *n_runs;      // entries reserved so far (kd_table zeroes it)
    u32 cap;
    u32 window;       // 0: the radix route (nothing of the above is touched); else a tile's ids must span less than this (<= RUN_W)
    int tile_bits;
};

// fragment record of the per-junction reductions: 48 words (see k4_pairs)
enum {
    F_N = 0, F_R1P, F_R1N, F_R2P, F_R2N, F_MS, F_XSP, F_XSN, F_UM, F_BPP, F_PPP, F_REL, F_DIST, // sums
    F_MAXMINANC, F_UP, F_DOWN, F_MAXMMES, F_MAXMINMATCH,                                       // max
    F_FIRSTMIS,                                                                                 // min
    F_PAD19,                                                                                    // keeps the next pair 8-byte aligned
    F_MISM_LO, F_MISM_HI,                                                                       // 64-bit sum
    F_JAD0,                                                                                     // 20 sums
    F_WORDS = 48
};
__device__ __forceinline__ void acc_rest_state(u32 *acc, u64 n_junc) { // what k5_frag_reduce's atomics start from: sums 0, max 0, min 100000000
    const u64 n = n_junc * F_WORDS, step = (u64)gridDim.x * blockDim.x;
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += step) acc[t] = (t % F_WORDS) == F_FIRSTMIS ? 100000000u : 0u;
}

} // namespace pjb
