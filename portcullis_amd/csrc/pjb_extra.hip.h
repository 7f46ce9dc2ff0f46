// pjb_extra.hip.h -- `junc --extra` on the device: the three metric families the
// reference computes after the main pass, single-threaded, by re-reading BAM files it has just split off
// (src/junction_builder.cc:152-226,293-312):
//   mm_score          Junction::calcMultipleMappingScore              lib/src/junction.cc:914-921
//   up_aln, down_aln  Junction::processJunctionVicinity               lib/src/junction.cc:651-677
//   coverage          DepthParser::loadNextBatch + Junction::calcCoverage
//                                                                     lib/src/depth_parser.cc:112-164, junction.cc:923-951
// Here they come from the alignment records that are already in HBM for the main pass:
//   * "unspliced.bam" = records without an N operation that are mapped (junction_builder.cc:168-186);
//   * per-base depth = difference array over their M / = / X runs + one scan (replaces htslib's pileup,
//     deps/htslib-1.3/sam.c:1853-1975, including its 8000-record cap -- see kx_cap_*);
//   * flanking counts = two rank queries: records starting before the intron minus records ending before
//     the left anchor; records starting inside the right anchor;
//   * name multiplicities = one open-addressing table over the 64-bit codes of every spliced record.
#pragma once

#include "pjb_extra_types.hip.h"

namespace pjb {

// a record's M / = / X runs, clipped to the target, into the depth difference array (sign -1: out of it again)
__device__ __forceinline__ void depth_runs(const u32 *cigar, u32 c0, u32 c1, int32_t pos, int32_t ref_len, int32_t *dd, int32_t sign) {
    int32_t x = pos;
    for (u32 k = c0; k < c1; k++) {
        const u32 op = cigar[k];
        const u32 ty = op & 15u;
        const int32_t ln = (int32_t)(op >> 4);
        if (ty == OP_M || ty == OP_EQ || ty == OP_X) {
            int32_t a = x, bb = x + ln;
            if (a < 0) a = 0;
            if (bb > ref_len) bb = ref_len;
            if (a < bb) {
                atomicAdd(&dd[a], sign);
                atomicAdd(&dd[bb], -sign);
            }
        }
        if (op_consumes_ref(ty)) x += ln;
    }
}

// KX1: one thread per record (every record of the contig).  Classifies the record as the reference's
// separateBams does, records its position / exclusive end for the rank queries, counts its end in `ce`
// and adds its M / = / X runs to the depth difference array; the name codes of spliced records are appended
// (order is irrelevant: they only feed a multiset).
__global__ __launch_bounds__(256) void kx_classify(DevBatch b, int32_t ref_len, int32_t *x_pos,
                                                    int32_t *x_endx, uint8_t *q_flag, u32 *ce, int32_t *dd, u32 *zlist,
                                                    u32 zcap, ExtraCounters *cnt) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool on = r < b.n;
    bool spliced = false;
    if (on) {
        const u32 g = b.base + (u32)r;
        const u32 c0 = b.cig_off[r], c1 = b.cig_off[r + 1];
        const int32_t pos = b.pos[r];
        int32_t aligned = 0;
        for (u32 k = c0; k < c1; k++) {
            const u32 op = b.cigar[k];
            const u32 ty = op & 15u;
            if (ty == OP_N) spliced = true;
            if (op_consumes_ref(ty)) aligned += (int32_t)(op >> 4);
        }
        const bool mapped = !(b.flag[r] & 0x4u);
        const bool unspliced = !spliced && mapped; // a record of unspliced.bam
        const bool spans = unspliced && aligned > 0 && pos >= 0;
        x_pos[g] = pos;
        // bam_endpos (sam.c:336-342): pos + span with a CIGAR -- pos itself where it spans nothing --, pos + 1 without one
        x_endx[g] = c1 > c0 ? pos + aligned : pos + 1;
        // bit 0: a record with a span (depth, rank queries); bit 1: one without, which the pileup still holds in its list while
        // it stands on the record's position (kx_cap_*)
        q_flag[g] = spans ? 1 : (unspliced && aligned == 0 && pos >= 0 ? 2 : 0);
        if (unspliced && aligned == 0) { // getEnd() == pos - 1: handled one by one in kx_flank (practically never)
            const u32 z = atomicAdd(&cnt->n_zero, 1u);
            if (z < zcap) zlist[z] = (u32)pos;
        }
        if (spans) {
            int32_t e = pos + aligned - 1; // getEnd()
            if (e > ref_len) e = ref_len;
            atomicAdd(&ce[e], 1u);
            depth_runs(b.cigar, c0, c1, pos, ref_len, dd, 1);
        }
    }
}

// The name codes of the spliced records, in BAM order, without a single atomic: k1_count left, per 1024-record tile,
// the ordered list of its spliced records (spl_idx) and their number (tile_stats); one block scans the tile counts,
// then a block per tile copies its records' codes to the tile's place.  (A wave-aggregated atomicAdd on one counter
// per wavefront of records cost 1.1 ms per 10 M records: 156 k returning atomics on ONE address.)
__global__ __launch_bounds__(1024) void kx_spliced_offsets(const TileStats *ts, u32 n_tiles, u32 *off, ExtraCounters *cnt) {
    __shared__ u32 wsum[16];
    __shared__ u32 carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (u32 base = 0; base < n_tiles; base += 1024) {
        const u32 i = base + threadIdx.x;
        const u32 v = i < n_tiles ? ts[i].spliced : 0u;
        const u32 inc = wave_iscan(v);
        const int w = threadIdx.x >> 6;
        if (lane_id() == 63) wsum[w] = inc;
        __syncthreads();
        u32 wb = 0, tot = 0;
        for (int k = 0; k < 16; k++) {
            const u32 t = wsum[k];
            if (k < w) wb += t;
            tot += t;
        }
        const u32 carry = carry_s;
        if (i < n_tiles) off[i] = carry + wb + inc - v;
        __syncthreads();
        if (threadIdx.x == 0) carry_s = carry + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) cnt->n_spliced = carry_s;
}
__global__ __launch_bounds__(256) void kx_spliced_codes(DevBatch b, const TileStats *ts, const u32 *spl_idx, const u32 *off, u64 *spl_codes) {
    const u32 tile = b.tile_base + blockIdx.x;
    const u32 nspl = ts[tile].spliced, o = off[tile];
    for (u32 ks = threadIdx.x; ks < nspl; ks += 256) spl_codes[o + ks] = b.name_hash[spl_idx[(size_t)tile * K1_TILE + ks]];
}

// KX3: the pileup's record cap.  bam_plp_push (sam.c:1906) drops a record that starts where the iterator
// stands -- the start of the last record it kept -- while more than maxcnt list nodes exist: the kept records
// with bam_endpos >= that position, plus two.  An upper bound for record i: every earlier unspliced record with
// endpos >= pos_i, kept or not = (unspliced records before i) - (unspliced records with endpos < pos_i).  If
// the bound stays below maxcnt - 1 everywhere, nothing is dropped and the difference array already holds the
// reference's depth (the normal case: it takes 8000-fold coverage of unspliced records).
//   prefix_q and pe count the records with a span.  One without a span (q_flag 2: its bam_endpos is its own position, or
// the next where it has no CIGAR) is in the list only for the records that follow it there; there are at most n_zero of
// them (a target with more than X_ZCAP is refused), so the bound is this one plus n_zero, and the replay counts them one by one.
__global__ __launch_bounds__(256) void kx_cap_bound(const int32_t *x_pos, const uint8_t *q_flag, const u32 *prefix_q,
                                                     const u32 *pe, u32 n, int32_t ref_len, u32 *bound, ExtraCounters *cnt) {
    const u32 g = blockIdx.x * 256 + threadIdx.x;
    u32 u = 0;
    bool hot = false;
    if (g < n && q_flag[g]) {
        const int32_t p = x_pos[g];
        // records with endpos < p  <=>  getEnd() < p - 1
        const int32_t idx = p - 1 < 0 ? 0 : (p - 1 > ref_len + 1 ? ref_len + 1 : p - 1);
        u = prefix_q[g] - pe[idx];
        if (bound) bound[g] = u;
        hot = u + cnt->n_zero + 2 > PLP_MAXCNT; // (n_zero: written by kx_classify, the launch before)
    }
    // (one counter for every wavefront of records: look first -- the maximum settles after a few waves, and 156 k
    // atomics on one address are served one at a time; a stale look only costs an atomic)
    const u32 wm = wave_max(u);
    if (lane_id() == 0 && wm > cnt->max_buffered) atomicMax(&cnt->max_buffered, wm);
    if (hot) {
        atomicMin(&cnt->hot_first, g);
        atomicMax(&cnt->hot_last, g);
    }
}

// KX3b: exact replay of the cap over the span of records whose bound reaches it (outside the span every record
// is kept whatever happened before: its list is at most its bound).  Sequential by nature -- whether a record is
// kept depends on which earlier ones were -- so one lane walks the span; `de` (zeroed, ref_len + 2 entries)
// counts dropped records by endpos.  Kept records inside the list = bound - dropped records still inside.
//   The bound leaves out the records without a span (q_flag 2).  bam_plp_push links a kept record into the list only if its
// endpos lies behind the position the iterator stands on (sam.c:1930) -- every record with a span; one without a CIGAR, whose
// endpos is pos + 1; and one whose CIGAR spans nothing only where it is the first record kept at its position.  Such a record is
// in the list up to its endpos like any other, so it goes into `de` with the opposite sign (the sums are modulo 2^32): "dropped and
// still inside" minus "without a span, linked and still inside".  Those in front of the walked span that are still inside where it
// begins -- kept, like everything in front of it -- start at its first position or one base before it.
__global__ void kx_cap_replay(const int32_t *x_pos, const int32_t *x_endx, const uint8_t *q_flag, const u32 *bound, u32 n,
                              int32_t ref_len, u32 *de, uint8_t *dropped, ExtraCounters *cnt) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const u32 g0 = cnt->hot_first, g1 = cnt->hot_last;
    if (g0 > g1 || g0 >= n) return;
    auto slot = [&](int32_t e, int32_t sweep) { // where endpos e is counted: at or behind the sweep, inside the array
        if (e < sweep) e = sweep;
        return e > ref_len + 1 ? ref_len + 1 : e;
    };
    u32 dtotal = 0, dgone = 0, n_dropped = 0;
    int32_t sweep = x_pos[g0];
    // the records in front of the span that start at most one base before it, and the start of the last unspliced record
    // before them (kept: nothing before the span is dropped)
    u32 gs = g0;
    while (gs > 0 && x_pos[gs - 1] >= sweep - 1) gs--;
    int32_t last_kept_pos = -1;
    for (u32 g = gs; g-- > 0;)
        if (q_flag[g]) {
            last_kept_pos = x_pos[g];
            break;
        }
    for (u32 g = gs; g < g0; g++) {
        if (!q_flag[g]) continue;
        if (q_flag[g] == 2 && x_endx[g] > last_kept_pos && x_endx[g] >= sweep) de[slot(x_endx[g], sweep)]--, dtotal--;
        last_kept_pos = x_pos[g];
    }
    for (u32 g = g0; g <= g1; g++) {
        if (!q_flag[g]) continue;
        const int32_t p = x_pos[g];
        while (sweep < p && sweep <= ref_len + 1) dgone += de[sweep++];
        const u32 in_list = bound[g] - (dtotal - dgone);
        const bool spanless = q_flag[g] == 2;
        if (p == last_kept_pos && in_list + 2 > PLP_MAXCNT) {
            dropped[g] = 1; // (one without a span has no run to take back: kx_undo_dropped finds none)
            n_dropped++;
            if (!spanless) de[slot(x_endx[g], sweep)]++, dtotal++; // (the bound never held one without a span)
        } else {
            if (spanless && x_endx[g] > last_kept_pos) de[slot(x_endx[g], sweep)]--, dtotal--;
            last_kept_pos = p;
        }
    }
    cnt->n_dropped = n_dropped;
}

// KX3c: take the dropped records' M / = / X runs back out of the difference array (before the scan).
__global__ __launch_bounds__(256) void kx_undo_dropped(DevBatch b, int32_t ref_len, const uint8_t *dropped, int32_t *dd) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= b.n || !dropped[b.base + (u32)r]) return;
    depth_runs(b.cigar, b.cig_off[r], b.cig_off[r + 1], b.pos[r], ref_len, dd, -1);
}

__device__ __forceinline__ u32 lower_bound_i32(const int32_t *a, u32 n, int32_t v) { // first index with a[i] >= v
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// KX4: flanking alignment counts, one thread per junction (processJunctionVicinity, junction.cc:651-677):
//   up   = unspliced records with  intron.start > pos  and  leftAncStart <= getEnd()
//   down = unspliced records with  rightAncEnd >= pos  and  intron.end < pos
// A record with a reference span has getEnd() >= pos, so "getEnd() < left" implies "pos < intron.start" and
//   up = #{pos < start} - #{getEnd() < left};  down = #{pos <= right} - #{pos <= end}.
// prefix_q[i] = such records among the first i records (all records are position sorted); pe[x] = such records
// with getEnd() < x.  The reference's region query (sam_itr_queryi over [left - maxQueryLength - 1, right +
// maxQueryLength + 1), its end clamped to ref_len - 1: junction.cc:654-659) takes records with pos < its end, so it
// excludes one record the tests accept: a record that starts on the target's LAST base, when the right anchor reaches
// it -- `down` counts positions up to min(right, ref_len - 2) (flank_right).  Records without a reference span
// (getEnd() == pos - 1) are tested one by one from `zlist`.
__device__ __forceinline__ int32_t flank_right(int32_t r, int32_t ref_len) { return r < ref_len - 2 ? r : ref_len - 2; }
__global__ __launch_bounds__(256) void kx_flank(const pjb_junction_row *rows, u32 n_rows, const int32_t *x_pos, u32 n_reads,
                                                 const u32 *prefix_q, const u32 *pe, int32_t ref_len, const u32 *zlist,
                                                 const ExtraCounters *cnt, u32 zcap, ExtraRow *out) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_rows) return;
    const int32_t s = rows[j].start, e = rows[j].end, l = rows[j].left, r = rows[j].right;
    auto before = [&](int32_t v) -> u32 { return prefix_q[lower_bound_i32(x_pos, n_reads, v)]; }; // #{pos < v}
    auto clampx = [&](int32_t v) -> int32_t { return v < 0 ? 0 : (v > ref_len + 1 ? ref_len + 1 : v); };
    const int32_t rr = flank_right(r, ref_len);
    u32 up = before(s) - pe[clampx(l)];
    u32 down = rr > e ? before(rr + 1) - before(e + 1) : 0u;
    u32 nz = cnt->n_zero;
    if (nz > zcap) nz = zcap;
    for (u32 k = 0; k < nz; k++) {
        const int32_t pos = (int32_t)zlist[k], end = pos - 1;
        if (s > pos && l <= end) up++;
        if (rr >= pos && e < pos) down++;
    }
    out[j].up_aln = up;
    out[j].down_aln = down;
}

// KX5: per sorted pair, the name code of its record and the global row it belongs to (kept until pjb_extra_finish)
__global__ __launch_bounds__(256) void kx_pair_codes(const u32 *sidx, const u32 *jid_of, const u32 *pair_g, const DevBatch *batches,
                                                      int n_batches, u32 n, u32 row_base,
                                                      u64 *pair_code, u32 *pair_row) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u32 g = pair_g[sidx[i]];
    int bi = n_batches - 1;
    while (bi > 0 && g < batches[bi].base) bi--;
    pair_code[i] = batches[bi].name_hash[g - batches[bi].base];
    pair_row[i] = row_base + jid_of[i];
}

// ---- the sparse path (round 3): no array of the target's length --------------------------------------------------
// The depth of the unspliced records is only ever READ at 42 positions per junction (Junction::calcCoverage,
// junction.cc:935-951) and the ends histogram at one position per junction (processJunctionVicinity) -- while building
// them costs two memsets, 3 atomics per record and two scans over the target's LENGTH (0.5 ms each per 100 Mb).  The
// records are sorted by position, and a record that covers x starts within max_span bases before x: so both questions
// are answered from the records themselves, by a thread per junction that walks the few records starting in
// (x - max_span, x].  What is kept of a target until pjb_extra_finish: the unspliced records with a span, compacted --
// pos[k], end[k] (exclusive) in file order -- and the list of their D operations ("gaps": inside the span, not counted by
// the pileup) with one offset per 256 records.  (The spliced records are left out: a junction's own alignments start
// right before it, 300 k of them at the deepest junction of configs[1], and would all be walked for nothing.)
//   htslib's 8000-record cap (kx_cap_*) is only possible where 7999 consecutive unspliced records start within max_span
// bases (kx_cap_check); such a target -- and one with more gaps than the list holds -- goes through the dense path
// above instead.
//   A chain of several targets (a group, pjb_finish_group_begin) is ONE such target in the coordinates of its virtual sequence: member m
// lies at voff[m] there, positions and ends are kept in virtual coordinates, and the spans of the whole chain are one position-sorted
// list (members in the order of their offsets, records in file order inside a member).  A lone target is the chain of one member at 0.
//   The classification itself is x_classify (pjb_device.hip.h).  A lone target's records get it inside the chain's k1_count, which has
// every CIGAR in registers anyway; kx_classify_sparse does the same for the batches of a chain of several members, whose k1_count does
// not.  There a span that leaves its member's sequence takes the group apart (need_dense bit 3): its members then go one by one.
__global__ __launch_bounds__(256) void kx_classify_sparse(DevBatch b, int32_t voff, int32_t len, bool many_members, XOut X) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    XLane a;
    if (r < b.n) {
        int32_t aligned = 0;
        u32 ngap = 0, gapmax = 0;
        bool spliced = false;
        for (u32 k = b.cig_off[r]; k < b.cig_off[r + 1]; k++) {
            const u32 op = b.cigar[k];
            const u32 ty = op & 15u;
            if (ty == OP_N) spliced = true;
            if (op_consumes_ref(ty)) aligned += (int32_t)(op >> 4);
            if (ty == OP_D && (op >> 4)) { // inside the span, no depth
                ngap++;
                gapmax = max(gapmax, op >> 4);
            }
        }
        x_classify(X, b.base + (u32)r, b.pos[r], aligned, ngap, gapmax, spliced, b.flag[r], voff, len, (u32)b.member, many_members, a);
    }
    x_counters(X.cnt, a);
}

// one scan over the records: (records with a span) | (gaps) << 32
struct SparseFn {
    const uint8_t *q;
    __device__ u64 operator()(u64 i) const {
        const u32 v = q[i];
        return (u64)(v & 1u) | ((u64)(v >> 1) << 32);
    }
};
struct SparseSink { // the records with a span, compacted in rank order; gaps before every 256th record and every 256th rank
    int32_t *comp_pos, *comp_end;
    u32 *gapoff_rec, *gapoff_rank;
    const int32_t *s_pos, *s_end;
    const uint8_t *q;
    __device__ void operator()(u64 i, u64, u64 ex) const {
        const u32 rank = (u32)ex, gbefore = (u32)(ex >> 32);
        if ((i & 255u) == 0) gapoff_rec[i >> 8] = gbefore;
        if (q[i] & 1u) {
            comp_pos[rank] = s_pos[i];
            comp_end[rank] = s_end[i];
            if ((rank & 255u) == 0) gapoff_rank[rank >> 8] = gbefore;
        }
    }
};
// the gaps (D operations) of the unspliced records in record order: a block per 256 records (global ordinals, so that
// gapoff[block] is the block's first entry), an exclusive scan of the records' gap counts inside the block.  `voff`: where the batch's
// target lies in its group's virtual sequence (0: a target finished alone) -- the gaps are in the coordinates of the spans.
__global__ __launch_bounds__(256) void kx_gaps(DevBatch b, int32_t voff, const uint8_t *q, u32 n_total, const u32 *gapoff, Gap *gaps, u32 gap_cap,
                                                SparseCounters *cnt, u32 n_blocks) {
    __shared__ u32 wsum[4];
    if ((cnt->total >> 32) == 0) return; // (no gap in the whole target: the usual case for short reads; the grid is small for that)
    const u32 first_block = b.base >> 8;
    for (u32 blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) { // (uniform per block: the barriers are safe)
        const u64 g = ((u64)(first_block + blk) << 8) + threadIdx.x; // global record ordinal
        const u32 ngap = g < n_total ? (u32)(q[g] >> 1) : 0u;
        const u32 inc = wave_iscan(ngap);
        const int w = threadIdx.x >> 6;
        __syncthreads();
        if (lane_id() == 63) wsum[w] = inc;
        __syncthreads();
        u32 before = gapoff[first_block + blk] + inc - ngap;
        for (int k = 0; k < w; k++) before += wsum[k];
        if (!ngap || g < b.base || g >= (u64)b.base + (u64)b.n) continue; // (a neighbouring batch's record: it only counts)
        if (before + ngap > gap_cap) {
            atomicOr(&cnt->need_dense, 4u);
            continue;
        }
        const u32 r = (u32)g - b.base;
        int32_t x = b.pos[r] + voff;
        u32 k_out = 0;
        for (u32 k = b.cig_off[r]; k < b.cig_off[r + 1] && k_out < ngap; k++) {
            const u32 op = b.cigar[k], ty = op & 15u;
            const int32_t ln = (int32_t)(op >> 4);
            if (ty == 2u && ln) gaps[before + k_out++] = Gap{x, x + ln};
            if (op_consumes_ref(ty)) x += ln;
        }
    }
}

// the pileup's cap can only bite where PLP_MAXCNT - 1 records start within max_span bases of each other; those without a span
// are not in the list walked here, so each of them may stand for one that is
__global__ __launch_bounds__(256) void kx_cap_check(const int32_t *comp_pos, SparseCounters *cnt) {
    const u32 n = (u32)cnt->total, K = PLP_MAXCNT - 1 - min(cnt->n_zero, PLP_MAXCNT - 2);
    const u32 r = blockIdx.x * 256 + threadIdx.x + K;
    if (r >= n) return;
    if ((int64_t)comp_pos[r] - (int64_t)comp_pos[r - K] <= (int64_t)cnt->max_span) atomicOr(&cnt->need_dense, 1u);
}

__device__ __forceinline__ u32 lower_bound_i64(const int32_t *a, u32 n, int64_t v) { // first index with a[i] >= v
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if ((int64_t)a[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Every lane has a range [i0, i1) of its own and wants acc(i, p) summed over it, p being the lane's parameters.  The ranges are
// a handful of records where coverage is ordinary -- the lane walks them itself -- and thousands in a pile-up: those are taken
// one after the other by the whole wavefront.  (A wavefront per junction was tried first: its 64-wide searches touched 64 cache
// lines per probe, 0.8 ms per 50 k junctions; a search per lane shares its upper levels with the neighbouring junctions'.)
// Every lane of the wavefront must call this.
constexpr u32 RANGE_SHORT = 48;
struct Win { // two windows of positions, [p1lo, p1hi] and [p2lo, p2hi] (empty: hi < lo)
    int32_t p1lo, p1hi, p2lo, p2hi;
};
template <class F>
__device__ __forceinline__ void ranges_sum2(u32 i0, u32 i1, const Win w, F acc, u32 &s1, u32 &s2) {
    const bool big = i1 > i0 && i1 - i0 > RANGE_SHORT;
    if (!big)
        for (u32 i = i0; i < i1; i++) acc(i, w, s1, s2);
    u64 m = __ballot(big);
    const int lane = lane_id();
    while (m) {
        const int src = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const u32 j0 = (u32)__shfl((int)i0, src, 64), j1 = (u32)__shfl((int)i1, src, 64);
        Win ws;
        ws.p1lo = __shfl(w.p1lo, src, 64);
        ws.p1hi = __shfl(w.p1hi, src, 64);
        ws.p2lo = __shfl(w.p2lo, src, 64);
        ws.p2hi = __shfl(w.p2hi, src, 64);
        u32 t1 = 0, t2 = 0;
        for (u32 i = j0 + (u32)lane; i < j1; i += 64) acc(i, ws, t1, t2);
        t1 = wave_total<DppAdd>(t1); // (every lane gets the sum)
        t2 = wave_total<DppAdd>(t2);
        if (lane == src) {
            s1 += t1;
            s2 += t2;
        }
    }
}

// The spans of a group's members per member, from the compacted list: member m's records are those whose virtual position lies in
// [voff[m], voff[m + 1]) -- a record with a span starts inside its member (a group with one that does not goes
// through its members one by one: need_dense bit 3).  One wavefront, a lane per member.
__global__ __launch_bounds__(64) void kx_member_spans(const int32_t *s_pos, const SparseCounters *cnt, XMembers M, GroupCounters *out) {
    const u32 n_reads = (u32)cnt->total;
    const int m = (int)threadIdx.x;
    bool has = false;
    if (m < M.n) {
        const u32 lo = lower_bound_i64(s_pos, n_reads, (int64_t)M.voff[m]);
        const u32 hi = m + 1 < M.n ? lower_bound_i64(s_pos, n_reads, (int64_t)M.voff[m + 1]) : n_reads;
        has = hi > lo;
    }
    const u64 mask = __ballot(has);
    if (m == 0) {
        out->has_spans = (u32)mask;
        out->_pad = 0;
    }
}

// KX4 without the ends histogram: a thread per junction, for the rows of a whole chain.
//   #{getEnd() < x} = (records with a span that start before x - max_span: all of them) + (those among the records starting
//   in [x - max_span, x) whose last base lies before x); a record starting at or after x ends at or after x.
// s_pos / s_end hold the spans of every member in the coordinates of the chain's virtual sequence, the rows carry their target (refid)
// and its own coordinates.  A row finds its member in M, applies the reference's clamps in the member's coordinates and searches in
// virtual ones.  A row lies inside its target (a junction that reaches past the end stops the chain: PJB_ERR_SPLICE_SITE_LEN), so the
// positions searched for -- start, end + 1, flank_right + 1 -- are inside [0, len + 1] already; the clamp only says so.
//   The records of EARLIER members start before every position of this one and end inside their own member: they are counted by
// before(s) and by `ended` alike -- among the records before the search window, or inside it with their last base before the anchor --
// and cancel in `up`; in `down` they are in both terms.  A LATER member's records start behind voff + len + 1 (the gap between members
// is 4096 bases) and are in neither.  max_span is the chain's maximum: a larger one only widens the window that is walked.  A lone
// target is the chain with M.n == 1: no other member, offset 0 -- and its records may start or end past its end, which no searched
// position reaches.
__global__ __launch_bounds__(256) void kx_flank_sparse(const pjb_junction_row *rows, u32 n_rows, const int32_t *s_pos, const int32_t *s_end, XMembers M,
                                                       const u32 *zlist, const SparseCounters *cnt, u32 zcap, ExtraRow *out) {
    const u32 n_reads = (u32)cnt->total;
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    const bool on = j < n_rows;
    int32_t s = 0, e = 0, l = 0, r = 0, refid = -1;
    if (on) s = rows[j].start, e = rows[j].end, l = rows[j].left, r = rows[j].right, refid = rows[j].refid;
    u32 member = 0;
    int32_t voff = M.voff[0], ref_len = M.len[0];
    for (int k = 1; k < M.n; k++) // (k is uniform: the table is read with scalar loads)
        if (M.tid[k] == refid) member = (u32)k, voff = M.voff[k], ref_len = M.len[k];
    auto before = [&](int64_t v) -> u32 { // #{records of earlier members} + #{this member's records with pos < v}
        const int64_t vc = v < 0 ? 0 : (v > (int64_t)ref_len + 1 ? (int64_t)ref_len + 1 : v);
        return lower_bound_i64(s_pos, n_reads, (int64_t)voff + vc);
    };
    const int32_t lc = l < 0 ? 0 : (l > ref_len + 1 ? ref_len + 1 : l);
    const int32_t vlc = voff + lc;
    u32 ended = 0, i0 = 0, i1 = 0;
    if (on) {
        if (lc == ref_len + 1) ended = before(lc); // (the histogram clamps every end to ref_len: every record of the member)
        else {
            i0 = lower_bound_i64(s_pos, n_reads, (int64_t)vlc - (int64_t)cnt->max_span);
            i1 = lower_bound_i32(s_pos, n_reads, vlc);
            ended = i0;
        }
    }
    u32 part = 0, unused = 0;
    ranges_sum2(i0, i1, Win{vlc, 0, 0, 0}, [&](u32 i, const Win w, u32 &a, u32 &) {
        if (s_end[i] - 1 < w.p1lo) a++;
    }, part, unused);
    if (!on) return;
    const int32_t rr = flank_right(r, ref_len);
    u32 up = before(s) - (ended + part);
    u32 down = rr > e ? before((int64_t)rr + 1) - before((int64_t)e + 1) : 0u;
    u32 nz = cnt->n_zero;
    if (nz > zcap) nz = zcap;
    for (u32 k = 0; k < nz; k++) {
        if (zlist[zcap + k] != member) continue;
        const int32_t pos = (int32_t)zlist[k], end = pos - 1;
        if (s > pos && l <= end) up++;
        if (rr >= pos && e < pos) down++;
    }
    out[j].up_aln = up;
    out[j].down_aln = down;
}

__device__ __forceinline__ u32 span_overlap(int64_t x0, int64_t x1, int32_t plo, int32_t phi) { // |[x0, x1) n [plo, phi]|
    const int64_t lo = x0 > plo ? x0 : (int64_t)plo, hi = (x1 - 1) < phi ? (x1 - 1) : (int64_t)phi;
    return hi >= lo ? (u32)(hi - lo + 1) : 0u;
}
// sum over i in [a, b], 1 <= i < len, of the depth at position i - 1 -- for two windows [a1, b1], [a2, b2] at once; every lane of
// the wavefront calls this (`on`: the lane has a junction).  D may hold the records of a whole group in virtual coordinates, the
// source target lying at `voff` in them: the windows are clipped to the target in its own coordinates and then moved there.  The
// records of its neighbours that the search also meets lie inside their own members and overlap nothing of the windows.
__device__ __forceinline__ void sparse_cov2(const SparseDepth D, int32_t len, int32_t voff, bool on, int32_t a1, int32_t b1, int32_t a2, int32_t b2,
                                            u32 &sum1, u32 &sum2) {
    // window [a, b] in i -> positions [max(a, 1) - 1, min(b, len - 1) - 1]
    auto lo_of = [&](int32_t a) -> int32_t { return (a < 1 ? 1 : a) - 1; };
    auto hi_of = [&](int32_t b) -> int32_t { return b < 0 ? -1 : (b > len - 1 ? len - 1 : b) - 1; };
    const Win w{lo_of(a1) + voff, hi_of(b1) + voff, lo_of(a2) + voff, hi_of(b2) + voff};
    const bool e1 = w.p1hi >= w.p1lo, e2 = w.p2hi >= w.p2lo;
    int64_t lo = 0, hi = -1;
    if (e1) lo = w.p1lo, hi = w.p1hi;
    if (e2) {
        lo = e1 && lo < w.p2lo ? lo : (int64_t)w.p2lo;
        hi = e1 && hi > w.p2hi ? hi : (int64_t)w.p2hi;
    }
    u32 i0 = 0, i1 = 0, g0 = 0, g1 = 0;
    if (on && hi >= lo) {
        i0 = lower_bound_i64(D.s_pos, D.n_reads, lo - (int64_t)D.max_span + 1);
        i1 = lower_bound_i64(D.s_pos, D.n_reads, hi + 1);
        if (D.n_gaps && i1 > i0) { // a gap that covers a position of the window belongs to a record starting in (lo - max_span, hi]
            const u32 k1 = (i1 + 255u) >> 8;
            g0 = D.gapoff[i0 >> 8];
            g1 = (u64)k1 * 256u < (u64)D.n_reads ? D.gapoff[k1] : D.n_gaps;
        }
    }
    u32 s1 = 0, s2 = 0, m1 = 0, m2 = 0;
    ranges_sum2(i0, i1, w, [&](u32 i, const Win ww, u32 &a, u32 &b) {
        const int64_t x0 = D.s_pos[i], x1 = D.s_end[i];
        a += span_overlap(x0, x1, ww.p1lo, ww.p1hi);
        b += span_overlap(x0, x1, ww.p2lo, ww.p2hi);
    }, s1, s2);
    ranges_sum2(g0, g1, w, [&](u32 k, const Win ww, u32 &a, u32 &b) {
        const Gap g = D.gaps[k];
        a += span_overlap(g.start, g.end, ww.p1lo, ww.p1hi);
        b += span_overlap(g.start, g.end, ww.p2lo, ww.p2hi);
    }, m1, m2);
    sum1 = s1 - m1;
    sum2 = s2 - m2;
}
// Junction::calcCoverage (junction.cc:923-951) from a target's records instead of its depth vector: a thread per junction
__global__ __launch_bounds__(256) void kx_coverage_sparse(const pjb_junction_row *rows, u32 row0, u32 n, SparseDepth D, int32_t len_src, int32_t voff_src,
                                                           ExtraRow *out) {
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    const bool on = k < n;
    const u32 j = row0 + (on ? k : 0u);
    int32_t s = 0, e = 0;
    if (on) s = rows[j].start, e = rows[j].end;
    u32 d1, d2, a1, a2;
    sparse_cov2(D, len_src, voff_src, on, s - 20, s - 11, s - 10, s, d1, d2);
    sparse_cov2(D, len_src, voff_src, on, e + 10, e + 20, e, e + 9, a1, a2);
    if (!on) return;
    const double donor = (1.0 / 9.0) * (double)d1 - (1.0 / 10.0) * (double)d2;
    const double acceptor = (1.0 / 10.0) * (double)a1 - (1.0 / 9.0) * (double)a2;
    out[j].coverage = donor + acceptor;
}

// ---- phase 2 (all contigs done) ---------------------------------------------------------------------------
constexpr u64 NAME_EMPTY = ~0ull;
__device__ __forceinline__ u64 name_slot_key(u64 code) { return code == NAME_EMPTY ? code - 1 : code; }
// (any number of slots, not a power of two: the table of a file is sized to its names, and 144 MB stay in the 256 MB of
// Infinity Cache where 268 MB do not)
__device__ __forceinline__ u32 name_slot_of(u64 key, u32 slots) { return (u32)((((key * 0x9e3779b97f4a7c15ULL) >> 32) * (u64)slots) >> 32); }
__device__ __forceinline__ u32 name_next(u32 h, u32 slots) { return h + 1 == slots ? 0u : h + 1; }

// splicedAlignmentMap[code]++ (junction_builder.cc:173-174) for every spliced record of the file.  One 16-byte slot per
// name: key and count share a sector (a lookup is one random access, not two); the table is filled with 0xff, so an empty
// slot's key is NAME_EMPTY and a slot's count is `count + 1` in 32-bit arithmetic.
struct NameSlot {
    u64 key;
    u32 count, _pad;
};
__device__ __forceinline__ void name_add(NameSlot *tab, u32 slots, u64 key, u32 n) {
    u32 h = name_slot_of(key, slots);
    for (;;) {
        u64 cur = tab[h].key;
        if (cur == NAME_EMPTY) cur = atomicCAS((unsigned long long *)&tab[h].key, (unsigned long long)NAME_EMPTY, (unsigned long long)key);
        if (cur == NAME_EMPTY || cur == key) {
            atomicAdd(&tab[h].count, n);
            return;
        }
        h = name_next(h, slots);
    }
}
// the table has grown: every name of the old one into the new one
__global__ __launch_bounds__(256) void kx_name_rehash(const NameSlot *old_tab, u32 old_slots, NameSlot *tab, u32 slots) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= old_slots) return;
    const NameSlot o = old_tab[i];
    if (o.key != NAME_EMPTY) name_add(tab, slots, o.key, o.count + 1u);
}
// M of every junction: sum over its alignments of the map entry of their code (junction.cc:916-919, uint32).  Four pairs
// per thread, a wavefront's 256 consecutive pairs in four rounds: the four random probes of a thread are in flight together.
__global__ __launch_bounds__(256) void kx_name_sum(const u64 *pair_code, const u32 *pair_row, u32 n, const NameSlot *tab, u32 slots, ExtraRow *out) {
    const u32 base = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 256 + (u32)lane_id();
    u64 key[4];
    u32 h[4], row[4], c[4];
    NameSlot sl[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { // (unconditional loads from a clamped index, masked after: they travel together)
        const u32 i = base + 64 * k, ic = i < n ? i : n - 1;
        const u64 code = pair_code[ic];
        const u32 rw = pair_row[ic];
        key[k] = i < n ? name_slot_key(code) : 0ull;
        row[k] = i < n ? rw : 0xffffffffu;
        h[k] = name_slot_of(key[k], slots);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) sl[k] = tab[h[k]];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u32 i = base + 64 * k;
        while (i < n && sl[k].key != key[k] && sl[k].key != NAME_EMPTY) {
            h[k] = name_next(h[k], slots);
            sl[k] = tab[h[k]];
        }
        c[k] = i < n && sl[k].key == key[k] ? sl[k].count + 1u : 0u;
    }
    // pairs are stored junction by junction: fold equal rows inside the wave before the atomic
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u32 i = base + 64 * k;
        const u32 cc = seg_reduce_to_head(c[k], row[k], OpAdd());
        const u32 prev = __shfl_up(row[k], 1, 64);
        if (i < n && (lane_id() == 0 || prev != row[k])) atomicAdd(&out[row[k]].m_sum, cc);
    }
}
// four codes per thread into the table (the probes of a thread in flight together)
__global__ __launch_bounds__(256) void kx_name_insert4(const u64 *codes, u32 n, NameSlot *tab, u32 slots) {
    const u32 base = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 256 + (u32)lane_id();
    u64 key[4];
    u32 h[4];
    u64 cur[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u32 i = base + 64 * k;
        const u64 code = codes[i < n ? i : n - 1];
        key[k] = i < n ? name_slot_key(code) : 0ull;
        h[k] = name_slot_of(key[k], slots);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) cur[k] = tab[h[k]].key; // (a plain look first: most codes of a deep file are in the table already)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (base + 64 * k >= n) continue;
        if (cur[k] == key[k]) atomicAdd(&tab[h[k]].count, 1u);
        else name_add(tab, slots, key[k], 1u);
    }
}

// Junction::calcCoverage (junction.cc:923-951) for the rows [row0, row0 + n) against the depth vector of one
// target: levels[i] = cover[i - 1] (DepthParser stores a position's depth at pos + 1, depth_parser.cc:127,147),
// entries outside [0, len_src) are skipped as the reference's bounds test does.
__device__ __forceinline__ double cov_window(const u32 *cover, int32_t len, int32_t a, int32_t b) {
    const double multiplier = 1.0 / (double)(b - a);
    u32 readCount = 0;
    for (int32_t i = a; i <= b; i++)
        if (i >= 1 && i < len) readCount += cover[i - 1];
    return multiplier * (double)readCount;
}
__global__ __launch_bounds__(256) void kx_coverage(const pjb_junction_row *rows, u32 row0, u32 n, const u32 *cover, int32_t len_src, ExtraRow *out) {
    const u32 k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const u32 j = row0 + k;
    const int32_t s = rows[j].start, e = rows[j].end;
    const double donor = cov_window(cover, len_src, s - 20, s - 11) - cov_window(cover, len_src, s - 10, s);
    const double acceptor = cov_window(cover, len_src, e + 10, e + 20) - cov_window(cover, len_src, e, e + 9);
    out[j].coverage = donor + acceptor;
}
// the finished columns of every junction, in the layout pjb_extra_finish hands out (mm_score = N / M, junction.cc:920)
__global__ __launch_bounds__(256) void kx_rows_out(const pjb_junction_row *rows, const ExtraRow *x, u32 n, pjb_extra_row *out) {
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    pjb_extra_row o;
    o.mm_score = (double)rows[j].nb_raw / (double)x[j].m_sum;
    o.coverage = x[j].coverage;
    o.up_aln = x[j].up_aln;
    o.down_aln = x[j].down_aln;
    out[j] = o;
}

// ---- bamfilt: BamFilter::filter's decision per alignment, src/bam_filter.cc:75-150,190-225.
// The walk is the reference's, including that it does not advance over an N operation (only the else-branch of
// :86-96 adds to lEnd): the introns after a read's first one are looked up short of the earlier introns' lengths.
__global__ __launch_bounds__(256) void kf_filter(const int32_t *pos, const u32 *cig_off, const u32 *cigar, u32 n, const u64 *keys, u32 n_keys,
                                                  int clip_mode, uint8_t *codes) {
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int32_t lEnd = pos[i];
    u32 nN = 0;
    bool good = false;
    for (u32 k = cig_off[i]; k < cig_off[i + 1]; k++) {
        const u32 op = cigar[k];
        const u32 ty = op & 15u;
        const int32_t ln = (int32_t)(op >> 4);
        if (ty == OP_N) {
            nN++;
            const u64 key = ((u64)(u32)lEnd << 32) | (u64)(u32)(lEnd + ln - 1);
            u32 lo = 0, hi = n_keys; // JunctionSystem::getJunction: is the intron in the set?
            while (lo < hi) {
                const u32 mid = lo + ((hi - lo) >> 1);
                if (keys[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            good |= lo < n_keys && keys[lo] == key;
        } else if (op_consumes_ref(ty)) {
            lEnd += ln;
        }
    }
    uint8_t code = 1;                                    // not spliced: written as is (:221-224)
    if (nN) {
        if (clip_mode == PJB_CLIP_COMPLETE || nN <= 1) code = good ? 2 : 0;   // containsJunctionInSystem (:196-202)
        else code = good ? 3 : 0;                         // clipMSR: !allBad (:204-218)
    }
    codes[i] = code;
}

} // namespace pjb
