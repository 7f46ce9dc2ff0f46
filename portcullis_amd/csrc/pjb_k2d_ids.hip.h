// pjb_k2d_ids.hip.h -- K2d of the junc chain: ordered dense junction ids (kd_*).
// Reads the candidate keys, their partial anchors, the start bitmap and its page counts (k1_emit / k1_generic) and the pairs' keys;
// leaves the junction table (jkey, anc_l, anc_r), every pair's id in BAM order (jid_bam), the accumulators' rest state, and for the sort
// either the tiles' counts of the ids' first digit or the tiles' id runs (RunOut); wipes the bitmap, page counts and end slots it used.
#pragma once

#include "pjb_device.hip.h"

namespace pjb {

// ---------------------------------------------------------------------------------------------
// K2d: ordered dense junction ids.  The intron key is 46-48 bits wide (contig coordinate + intron length): five radix
// passes, the first of them over digits that differ for every junction of a tile.  But a contig has 10^4-10^5
// distinct introns, and their RANK in (start, end) order needs 15-19 bits: two passes -- and because the ranks of
// the junctions a tile touches are neighbours (pairs arrive in BAM order, ranks are ordered by start), both passes
// scatter into a few long runs per tile.  The rank comes without sorting anything:
//   k1_emit    pairs -> candidate keys (distinct per block residency; see there)
//   (k1_emit / k1_generic also set one bit per contig base where an intron of a listed candidate starts)
//   scan       prefix popcount over the bitmap words  -> rank of a start among the distinct starts
//   kd_ends    per start rank, the distinct intron ends seen (alternative acceptors: a handful; DENSE_ENDS slots)
//   scan       number of ends per start rank           -> first junction id of every start (+ the anchors' rest state)
//   kd_table   junction id -> intron key and the junction's anchors (min lStart, max rEnd over its pairs, junction.cc:477-529),
//              from the candidates; closes the chain if a limit was exceeded
//   kd_assign  id of a pair = first id of its start + number of that start's ends below its own end
// Grouping by id is grouping by (start, end), id order is (start, end) order, so everything downstream -- segment
// heads, fragments, row order -- works on the ids as it did on the keys.  A start with more than DENSE_ENDS different
// ends raises OVF_DENSE and the contig is repeated with the full-key sort.
// ---------------------------------------------------------------------------------------------
constexpr int DENSE_ENDS = 8;
constexpr u32 DENSE_EMPTY = 0xffffffffu;

__device__ __forceinline__ u32 start_rank(const u64 *bitmap, const u32 *wrank, int32_t start) {
    const u32 w = (u32)start >> 6;
    return wrank[w] + (u32)__popcll(bitmap[w] & ((1ull << (start & 63)) - 1ull));
}
// Pairs arrive in BAM order, so the pairs of a junction sit close together, and a deep junction is one key repeated 10^5
// times.  Operations on device memory that many waves aim at one address (or one cache line: the bitmap words of
// neighbouring starts) are served one after the other by a single L2 channel -- measured, 0.5 ns each, 1.4 ms for the
// pairs of one contig.  So only the CANDIDATE list (1-3x the number of junctions) touches the bitmap and the end slots.
// candidates -> one bit per contig base: an intron starts here
struct PopcFn {
    const u64 *words;
    __device__ u64 operator()(u64 i) const { return (u64)__popcll(words[i]); }
};
__global__ __launch_bounds__(256) void kd_ends(const u64 *cand, KeyFmt kf, const u64 *bitmap, const u32 *wrank, u32 junc_limit, u32 *ends,
                                               u32 *cand_rank, ContigStats *cs) {
    const u32 n = cs->n_cand; // (a few candidates per junction: the grid is small and strides)
    for (u32 p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        int32_t s, e;
        unpack_key(kf, cand[p], s, e);
        const u32 rs = start_rank(bitmap, wrank, s);
        cand_rank[p] = rs;
        if (rs >= junc_limit) {
            atomicOr(&cs->overflow, OVF_JUNC);
            continue;
        }
        u32 *slot = ends + (size_t)rs * DENSE_ENDS;
        const u32 ue = (u32)e;
        bool placed = false;
        for (int k = 0; k < DENSE_ENDS && !placed; k++) {
            const u32 cur = atomicCAS(&slot[k], DENSE_EMPTY, ue);
            placed = cur == DENSE_EMPTY || cur == ue; // else: the slot holds another end (slots never change once set)
        }
        if (!placed) atomicOr(&cs->overflow, OVF_DENSE);
    }
}
// The ranks of the bitmap's words, page by page: the starts are few (a third of the pages of a human-sized chain hold one, fewer
// where genes cluster), so the prefix sum runs over the PAGES' counts (k1_emit / k1_generic count a start when its bit is set for
// the first time) and only the pages that hold a start are read: a wavefront per page, lane = word, the word's rank = the page's
// rank + the popcounts of the page's words before it.  Words of pages without a start keep whatever rank they had: nobody asks
// for it (kd_ends, kd_assign look up the words of their own starts).  (Until round 5 a three-kernel scan read all of the bitmap
// twice and wrote every word's rank: 320 MB and 90 us a 1-Gb chain.)
__global__ __launch_bounds__(256) void kd_rank_pages(const u64 *bitmap, const u32 *page_cnt, const u32 *page_rank, u32 *wrank, u32 n_pages, u32 n_words) {
    const u32 page = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (page >= n_pages) return;
    if (page_cnt[page] == 0) return; // (uniform per wavefront)
    const u32 w = (page << KD_PAGE_SHIFT) + (u32)lane_id();
    const u32 c = w < n_words ? (u32)__popcll(bitmap[w]) : 0u;
    const u32 inc = wave_iscan(c);
    if (w < n_words) wrank[w] = page_rank[page] + inc - c;
}
// Bitmap, page counts and end slots are all-clear at rest: instead of memsets over contig-sized buffers per contig, the
// candidates wipe exactly what they set (after kd_assign has read it).
__global__ __launch_bounds__(256) void kd_reset(const u64 *cand, const u32 *cand_rank, KeyFmt kf, u32 junc_limit, const ContigStats *cs,
                                                u64 *bitmap, u32 *ends, u32 *page_cnt) {
    const u32 n = cs->n_cand;
    for (u32 p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
        int32_t s, e;
        unpack_key(kf, cand[p], s, e);
        bitmap[(u32)s >> 6] = 0;
        page_cnt[(u32)s >> (6 + KD_PAGE_SHIFT)] = 0;
        const u32 rs = cand_rank[p];
        if (rs < junc_limit) {
            uint4 *q = reinterpret_cast<uint4 *>(ends + (size_t)rs * DENSE_ENDS);
            q[0] = q[1] = make_uint4(DENSE_EMPTY, DENSE_EMPTY, DENSE_EMPTY, DENSE_EMPTY);
        }
    }
}
struct EndsCountFn {
    const u32 *ends;
    __device__ u64 operator()(u64 rs) const {
        const uint4 *q = reinterpret_cast<const uint4 *>(ends + rs * DENSE_ENDS);
        const uint4 a = q[0], b = q[1];
        return (u64)((a.x != DENSE_EMPTY) + (a.y != DENSE_EMPTY) + (a.z != DENSE_EMPTY) + (a.w != DENSE_EMPTY) + (b.x != DENSE_EMPTY) +
                     (b.y != DENSE_EMPTY) + (b.z != DENSE_EMPTY) + (b.w != DENSE_EMPTY));
    }
};
// sink of the scan over the start ranks (junc_limit entries): first junction id of the start, and -- entry i of the
// junction-sized anchor arrays -- the rest state kd_assign's atomics start from
struct FirstIdSink {
    u32 *first_id;
    int32_t *anc_l, *anc_r;
    __device__ void operator()(u64 i, u64, u64 ex) const {
        first_id[i] = (u32)ex;
        anc_l[i] = INT32_MAX;
        anc_r[i] = INT32_MIN;
    }
};
__device__ __forceinline__ u32 ends_below(const u32 *ends, u32 rs, u32 ue) { // (DENSE_EMPTY slots compare as larger than any end)
    const uint4 *q = reinterpret_cast<const uint4 *>(ends + (size_t)rs * DENSE_ENDS);
    const uint4 a = q[0], b = q[1];
    return (a.x < ue) + (a.y < ue) + (a.z < ue) + (a.w < ue) + (b.x < ue) + (b.y < ue) + (b.z < ue) + (b.w < ue);
}

// junction id -> intron key (every candidate writes its junction's entry: duplicates write the same value) and the junction's
// anchors from the candidates' partial ones; thread 0 closes the chain -- P = 0, nothing downstream runs, the host repeats the
// contig -- if a limit was exceeded while the ids were built
__global__ __launch_bounds__(256) void kd_table(const u64 *cand, const u64 *cand_anc, const u32 *cand_rank, KeyFmt kf, u32 junc_limit, const u32 *ends,
                                                const u32 *first_id, const u64 *total, u64 *jkey, int32_t *anc_l, int32_t *anc_r, ContigStats *cs,
                                                const u32 *gen_cnt, u32 gen_cap, u32 sort_limit, u32 *n_runs, int range_shift) {
    const u32 p = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0) { // (the read lists: every sub-list within its room?)
        static_assert(GEN_SHARDS == 256, "a shard per thread of the first block");
        const u32 over = lists_over(gen_cnt, threadIdx.x, gen_cap);
        if (over) atomicMax(&cs->list_need, over);
        if (__syncthreads_or((int)over) && threadIdx.x == 0) cs->overflow |= OVF_LISTS;
    }
    if (p == 0) {
        if (n_runs) *n_runs = 0; // (the run list kd_assign fills: see RunOut)
        const u64 J = *total;
        u32 ovf = cs->overflow;
        // (sort_limit: the ids the sort's digits were planned for -- what chains of this context have had so far, with room; junc_limit:
        // what the buffers hold)
        if (cs->P != 0 && (J > (u64)junc_limit || J > (u64)sort_limit)) {
            ovf |= OVF_JUNC;
            cs->overflow = ovf;
            cs->n_junc = (u32)(J < 0xffffffffull ? J : 0xffffffffull);
        }
        if (ovf) cs->P = 0;
        else if (cs->P) { // the ids ARE the junctions: their number and the fragment slots are known from here on
            const u32 n_pairs = cs->P;
            cs->n_junc = cs->J = (u32)J;
            cs->n_slices = (n_pairs + 63) / 64;
            cs->n_slots = frag_slots((u32)J, n_pairs, range_shift);
        }
    }
    const u32 n = cs->n_cand;
    for (u32 base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
        const u32 q = base + threadIdx.x;
        const bool on = q < n;
        const u32 pc = on ? q : n - 1;
        const u32 rs = cand_rank[pc];
        const u64 k = cand[pc], a = cand_anc[pc];
        bool valid = on && rs < junc_limit;
        u32 id = 0xffffffffu;
        if (valid) {
            int32_t s, e;
            unpack_key(kf, k, s, e);
            id = first_id[rs] + ends_below(ends, rs, (u32)e);
            valid = id < junc_limit;
            if (valid) jkey[id] = k;
        }
        // (a junction has a candidate or two: the lanes of a wavefront hold different junctions, there is nothing to fold -- each lane
        // moves its junction's anchors itself, and only if its value would move them)
        if (valid) {
            const int32_t lo = (int32_t)(u32)a, hi = (int32_t)(u32)(a >> 32);
            if (lo < __hip_atomic_load(&anc_l[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&anc_l[id], lo);
            if (hi > __hip_atomic_load(&anc_r[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&anc_r[id], hi);
        }
    }
}

// (kd_assign's tile KDA_TILE is the sort's, and it counts the first digit of the ids it hands out with the sort's wave_hist_add; on the run route it
// fills the sort's RunOut, RUN_W counters a tile -- all four stand in pjb_device.hip.h, beside each other)
constexpr int KDA_PER = 4;
static_assert(RUN_W == 256 * 8, "kd_assign compacts eight table entries a thread");
// a tile's ids span more than the window, or the run list is full: the chain is closed (as kd_table closes it) and repeated on the radix route
__device__ __forceinline__ void runs_close_chain(ContigStats *cs) {
    atomicOr(&cs->overflow, OVF_RUNS);
    cs->P = 0;
    cs->J = 0;
    cs->n_slots = 0;
    cs->n_slices = 0;
}
__global__ __launch_bounds__(256) void kd_assign(const u64 *key, const u32 *np, KeyFmt kf, const u64 *bitmap, const u32 *wrank, const u32 *ends,
                                                 const u32 *first_id, u32 junc_limit, const u64 *total, u32 *jid_bam, u32 *acc, const u64 *jkey,
                                                 const int32_t *anc_l, const int32_t *anc_r, u64 *err, ContigStats *cs_chk, int hist_bits, u32 *hist,
                                                 RunOut ro) {
    // A block takes one TILE of the sort (4 096 pairs, four chunks of 1 024) and leaves the tile's counts of the ids' first digit
    // where rs_hist would have put them (hist_bits > 0): the sort's first pass starts at its scan -- the ids are not read a second
    // time to be counted.  On the run route (ro.window, hist_bits = 0) it leaves the tile's id runs instead.
    __shared__ u32 s_h[4096]; // (RS_MAX_BINS; the run route: RUN_W counters)
    __shared__ u32 s_run[4];  // the tile's least and largest id, its first entry in the run list
    __shared__ u32 s_rscan[4];
    const u32 n = *np;
    if (n == 0) { // (a chain without pairs, or closed by an overflow: the tile's counts are still this kernel's to write -- zeros --, the
                  // panel kernels behind it read them)
        if (hist_bits > 0)
            for (u32 d = threadIdx.x; d < (1u << hist_bits); d += 256) hist[(size_t)blockIdx.x * (1u << hist_bits) + d] = 0;
        return;
    }
    {
        const u64 J = *total;
        acc_rest_state(acc, J < (u64)junc_limit ? J : (u64)junc_limit);
    }
    const u32 nb = hist_bits > 0 ? 1u << hist_bits : 0u;
    for (u32 d = threadIdx.x; d < (ro.window ? RUN_W : nb); d += 256) s_h[d] = 0;
    if (threadIdx.x == 0) {
        s_run[0] = 0xffffffffu;
        s_run[1] = 0u;
    }
    if (nb || ro.window) __syncthreads();
    u32 id_lo = 0xffffffffu, id_hi = 0u; // (this thread's pairs)
    for (u32 chunk = blockIdx.x * (KDA_TILE / (KDA_PER * 256)); chunk < (blockIdx.x + 1) * (KDA_TILE / (KDA_PER * 256)); chunk++) {
    if (chunk * (KDA_PER * 256) >= n) break;
    // KDA_PER pairs a thread, their loads side by side: a pair is a chain of three dependent look-ups (key -> bitmap word and rank ->
    // end slots and first id), and a wavefront with one pair per lane (651 k of them a chain) spent its life waiting for them one
    // after the other -- 134 us a chain (round 4) for 267 MB
    // Pairs arrive in BAM order: the lanes of a wavefront mostly hold the pairs of one or two junctions.  Only the first lane of a run
    // of equal keys (a "leader") looks its junction up -- the look-ups are gathers of 56 bytes a pair, and their cost follows the
    // lanes that take part -- the others take the leader's answer (one ds_bpermute).
    u64 kk[KDA_PER];
    u32 pp[KDA_PER];
#pragma unroll
    for (int q = 0; q < KDA_PER; q++) {
        pp[q] = (chunk * KDA_PER + q) * 256 + threadIdx.x;
        kk[q] = key[pp[q] < n ? pp[q] : n - 1];
    }
    bool lead[KDA_PER];
    int32_t ss[KDA_PER], ee[KDA_PER];
    u64 bw[KDA_PER];
    u32 wr[KDA_PER];
#pragma unroll
    for (int q = 0; q < KDA_PER; q++) {
        const u32 plo = (u32)__builtin_amdgcn_update_dpp(0, (int)(u32)kk[q], 0x138, 0xf, 0xf, false);         // wave_shr:1
        const u32 phi = (u32)__builtin_amdgcn_update_dpp(0, (int)(u32)(kk[q] >> 32), 0x138, 0xf, 0xf, false);
        lead[q] = lane_id() == 0 || plo != (u32)kk[q] || phi != (u32)(kk[q] >> 32);
        unpack_key(kf, kk[q], ss[q], ee[q]);
        bw[q] = 0;
        wr[q] = 0;
        if (lead[q]) {
            bw[q] = bitmap[(u32)ss[q] >> 6];
            wr[q] = wrank[(u32)ss[q] >> 6];
        }
    }
    u32 rs_[KDA_PER], fi[KDA_PER], eb[KDA_PER];
#pragma unroll
    for (int q = 0; q < KDA_PER; q++) {
        rs_[q] = wr[q] + (u32)__popcll(bw[q] & ((1ull << (ss[q] & 63)) - 1ull));
        fi[q] = eb[q] = 0;
        if (lead[q]) {
            fi[q] = first_id[rs_[q]];
            eb[q] = ends_below(ends, rs_[q], (u32)ee[q]);
        }
    }
#pragma unroll
    for (int q = 0; q < KDA_PER; q++) {
        const u64 lm = __ballot(lead[q]) & ((2ull << lane_id()) - 1ull); // (lane 0 always leads)
        const u32 id = (u32)__shfl((int)(fi[q] + eb[q]), 63 - __clzll((long long)lm), 64);
        fi[q] = id;
        eb[q] = 0;
        if (pp[q] < n) jid_bam[pp[q]] = id; // (the sort's first pass reads the ids from here; k4b_generic looks its pairs' junctions up)
        if (nb) wave_hist_add(s_h, id & (nb - 1u), pp[q] < n);
        if (ro.window) {
            wave_hist_add(s_h, id & (RUN_W - 1u), pp[q] < n);
            if (pp[q] < n) {
                id_lo = id < id_lo ? id : id_lo;
                id_hi = id > id_hi ? id : id_hi;
            }
        }
    }
#ifdef PJB_SELFCHECK
    const u32 p = pp[0];
    if (p < n) {
    const int32_t s = ss[0], e = ee[0];
    const u32 rs = rs_[0], id = fi[0] + eb[0]; // (debug builds: the junction table kd_table made must know this pair's junction -- its start bit, its end slot, its key,
                     // anchors that enclose the intron; a failure stops the chain (P = 0) so that the report gets out)
    {
        int bad = 0;
        const uint4 *q = reinterpret_cast<const uint4 *>(ends + (size_t)rs * DENSE_ENDS);
        const uint4 a = q[0], b = q[1];
        const u32 ue = (u32)e;
        if (!((bitmap[(u32)s >> 6] >> (s & 63)) & 1ull)) bad = 6;
        else if (!(a.x == ue || a.y == ue || a.z == ue || a.w == ue || b.x == ue || b.y == ue || b.z == ue || b.w == ue)) bad = 7;
        else if (id >= junc_limit || id >= (u32)*total) bad = 1;
        else if (jkey[id] != key[p]) bad = 2;
        else if (anc_l[id] > s || anc_r[id] < e) bad = 3;
        if (bad) {
            set_error(err, 0xfffff000u + (u32)bad, PJB_ERR_HIP);
            cs_chk->P = 0;
        }
    }
    }
#endif
    } // chunks
    if (nb) {
        __syncthreads();
        for (u32 d = threadIdx.x; d < nb; d += 256) hist[(size_t)blockIdx.x * nb + d] = s_h[d];
    }
    if (ro.window) {
        // the tile's runs: the non-zero counters of [least id, largest id], in id order
        id_lo = wave_total<DppMin>(id_lo);
        id_hi = wave_total<DppMax>(id_hi);
        if (lane_id() == 0) {
            atomicMin(&s_run[0], id_lo);
            atomicMax(&s_run[1], id_hi);
        }
        __syncthreads();
        const u32 lo = s_run[0], hi = s_run[1];
        if (lo > hi) { // (a tile past the pairs)
            if (threadIdx.x == 0) ro.tile_n[blockIdx.x] = 0;
            return;
        }
        if (hi - lo >= ro.window) {
            if (threadIdx.x == 0) {
                ro.tile_n[blockIdx.x] = 0;
                runs_close_chain(cs_chk);
            }
            return;
        }
        const u32 span = hi - lo + 1u; // (<= RUN_W)
        u32 c[8], nz = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const u32 o = threadIdx.x * 8u + (u32)k;
            c[k] = o < span ? s_h[(lo + o) & (RUN_W - 1u)] : 0u;
            nz += c[k] != 0u;
        }
        u32 tot;
        u32 at = block_escan_256<u32>(nz, s_rscan, &tot);
        if (threadIdx.x == 0) { // room in the chain's run list (a reservation that does not fit is taken back: the count never stays above the room)
            u32 b = atomicAdd(ro.n_runs, tot);
            if (b > ro.cap || tot > ro.cap - b) {
                atomicSub(ro.n_runs, tot);
                b = 0xffffffffu;
                runs_close_chain(cs_chk);
            }
            s_run[2] = b;
            ro.tile_first[blockIdx.x] = b == 0xffffffffu ? 0u : b;
            ro.tile_n[blockIdx.x] = b == 0xffffffffu ? 0u : tot;
        }
        __syncthreads();
        const u32 first = s_run[2];
        if (first == 0xffffffffu) return;
        at += first;
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (c[k]) {
                ro.key[at] = ((u64)(lo + threadIdx.x * 8u + (u32)k) << ro.tile_bits) | (u64)blockIdx.x;
                ro.cnt[at] = c[k];
                at++;
            }
    }
}

} // namespace pjb
