// pjb_k4_pairs.hip.h -- K4 of the junc chain: per-pair match statistics and their fold to fragments.
// k4b_generic reads lists 1 and 2 and jid_bam, walks or window-checks those reads' pairs and fills their records in (side stream).
// k4_pairs reads the pairs in sorted order; leaves one 48-word fragment per junction and range, the head / run masks for k2_expand and
// the junctions' anchors.  k5_frag_reduce folds the fragments into the junction accumulators that k5_finalize reads.
#pragma once

#include "pjb_device.hip.h"
#include "pjb_basecmp.hip.h"
#include "pjb_readops.hip.h"

namespace pjb {

// ---------------------------------------------------------------------------------------------
// K4: per-pair match statistics (AlignmentInfo::calcMatchStats junction.cc:147-240 on top of
// BamAlignment::getPaddedQuerySeq / getPaddedGenomeSeq bam_alignment.cc:341-462), computed by
// counting instead of building strings: the query walk and the genome walk are advanced in
// lock-step over the CIGAR and their emissions compared op by op.
// ---------------------------------------------------------------------------------------------
constexpr int GENERIC_NW = 8; // (as the closed form: two 16-byte loads per stream and round, loads may run to the buffers' ends)
struct Side {
    int32_t len, mism, first_mis, last_mis;
    int err;
};

// (k0, r0, q0): the operation the walks start at and the reference / query position there -- (0, position, 0), or, from the
// pair's hint, the first operation that starts inside the window: everything before it the walks only step over
__device__ Side anchor_side(const OpsView cig, u32 n, int32_t position, int32_t aligned, const uint8_t *seq, int32_t lq,
                            const uint8_t *genome, int32_t glen, bool genome_has_x, const u32 *gcodes, int32_t start,
                            int32_t end, u32 k0, int32_t r0, int32_t q0, int32_t q_limit /* last word behind seq that may be read */) {
    Side S;
    S.len = 0;
    S.mism = 0;
    S.first_mis = -1;
    S.last_mis = -1;
    S.err = 0;
    const int32_t get_end = position + aligned - 1;
    if (start > get_end || end < position) { // bam_alignment.cc:342
        S.err = PJB_ERR_NO_PRESENCE;
        return S;
    }
    // getQuerySeqAfterClipping, bam_alignment.cc:256-264 (size_t arithmetic incl. the "+1")
    int32_t dS = 0, dE = 0;
    if ((cig[0] & 15u) == OP_S) dS = (int32_t)(cig[0] >> 4);
    if ((cig[n - 1] & 15u) == OP_S) dE = (int32_t)(cig[n - 1] >> 4);
    if (dS > lq) {
        S.err = PJB_ERR_CLIP_RANGE;
        return S;
    }
    const u64 cnt = (u64)(int64_t)lq - (u64)(int64_t)dS - (u64)(int64_t)dE + 1ull;
    const u64 avail = (u64)(lq - dS);
    const int32_t clen = (int32_t)(cnt < avail ? cnt : avail);
    // ---- pass A: query walk over ops only -> where it stops (actual_start / actual_end)
    int32_t rPos = r0, qPos = q0;
    for (u32 k = k0; k < n; k++) {
        const u32 op = cig[k], ty = op & 15u;
        const int32_t ln = (int32_t)(op >> 4);
        const bool cRef = op_consumes_ref(ty);
        const bool cQry = op_consumes_query(ty) && ty != OP_S;
        if (rPos < start) {
            if (cRef) rPos += ln;
            if (cQry) qPos += ln;
            continue;
        }
        if ((rPos > end && ty != OP_I) || (ty == OP_N && rPos + ln > end)) break; // :359
        if (cQry) {
            const int32_t l = (rPos + ln > end && ty != OP_I) ? end - rPos + 1 : ln;
            if (l == 0) {
                S.err = PJB_ERR_ZERO_LEN_OP;
                return S;
            }
            if (qPos < 0 || qPos + l > clen) {
                S.err = PJB_ERR_QUERY_RANGE;
                return S;
            }
        }
        if (cRef) rPos += ln;
        if (cQry) qPos += ln;
    }
    const int32_t q_start = position > start ? position : start; // :400
    const int32_t q_end = rPos <= end ? rPos - 1 : end;          // :401
    if (q_start - start < 0 || end - q_end < 0) {                // :414-421 (unreachable, kept for parity)
        S.err = PJB_ERR_QREGION;
        return S;
    }
    const int32_t gsize = end - start + 1; // length of the fetched anchor string
    // ---- pass B: both walks in lock-step, comparing emissions
    rPos = r0;
    qPos = q0;
    bool qDone = false, gDone = false, diverged = false;
    int32_t qTot = 0, gTot = 0, mism = 0, first_mis = -1, last_mis = -1;
    for (u32 k = k0; k < n; k++) {
        const u32 op = cig[k], ty = op & 15u;
        const int32_t ln = (int32_t)(op >> 4);
        const bool cRef = op_consumes_ref(ty);
        const bool cQry = op_consumes_query(ty) && ty != OP_S;
        int32_t qEmit = 0, gEmit = 0;
        int qKind = 0, gKind = 0; // 1 = bases, 2 = 'X' padding
        if (!qDone && rPos >= start) {
            if ((rPos > end && ty != OP_I) || (ty == OP_N && rPos + ln > end)) qDone = true;
            else if (cQry) {
                qEmit = (rPos + ln > end && ty != OP_I) ? end - rPos + 1 : ln;
                qKind = 1;
            } else if (cRef) {
                qEmit = rPos + ln > end ? end - rPos + 1 : ln;
                qKind = 2;
            }
        }
        if (!gDone && rPos >= q_start) {
            if (rPos > q_end && ty != OP_I) gDone = true;
            else if (cRef) {
                const int32_t so = rPos - start;
                gEmit = rPos + ln > q_end ? q_end - rPos + 1 : ln;
                if (so < 0 || so + gEmit > gsize) { // :437
                    S.err = PJB_ERR_GENOME_RANGE;
                    return S;
                }
                gKind = 1;
            } else if (cQry) {
                gEmit = ln;
                gKind = 2;
            }
        }
        if (qEmit != gEmit) diverged = true;
        if (!diverged && qEmit > 0) {
            if (qKind == 1 && gKind == 1 && gcodes != nullptr && rPos >= 0 && rPos + qEmit <= glen) {
                cmp_words<GENERIC_NW, true>(reinterpret_cast<const u32 *>(seq), dS + qPos, q_limit, gcodes, rPos, (glen + 7) / 8 + 1, qEmit, qTot,
                                      mism, first_mis, last_mis);
            } else if (qKind == 1 && gKind == 1) {
                const int32_t qb = dS + qPos;
                for (int32_t t = 0; t < qEmit; t++) {
                    const int32_t qi = qb + t;
                    const u32 byte = gload(seq + (qi >> 1));
                    const u32 code = (qi & 1) ? (byte & 15u) : (byte >> 4);
                    const int32_t gi = rPos + t;
                    const u32 gc = (gi >= 0 && gi < glen) ? (u32)gload(genome + gi) : 0u;
                    if (nt16_ascii(code) != gc) {
                        mism++;
                        if (first_mis < 0) first_mis = qTot + t;
                        last_mis = qTot + t;
                    }
                }
            } else if (qKind == 1) { // read letters vs 'X' (insertion): never equal
                mism += qEmit;
                if (first_mis < 0) first_mis = qTot;
                last_mis = qTot + qEmit - 1;
            } else if (!genome_has_x) { // 'X' padding (deletion / enclosed intron) vs genome bases without any 'X'
                mism += qEmit;
                if (first_mis < 0) first_mis = qTot;
                last_mis = qTot + qEmit - 1;
            } else { // contig really contains 'X' characters: compare byte by byte
                for (int32_t t = 0; t < qEmit; t++) {
                    const int32_t gi = rPos + t;
                    const u32 gc = (gi >= 0 && gi < glen) ? (u32)gload(genome + gi) : 0u;
                    if (gc != (u32)'X') {
                        mism++;
                        if (first_mis < 0) first_mis = qTot + t;
                        last_mis = qTot + t;
                    }
                }
            }
        }
        qTot += qEmit;
        gTot += gEmit;
        if (cRef) rPos += ln;
        if (cQry) qPos += ln;
        if (qDone && gDone) break;
    }
    if (qTot != gTot || qTot == 0) { // junction.cc:192,208
        S.err = PJB_ERR_ANCHOR_MISMATCH;
        return S;
    }
    if (diverged) {
        S.err = PJB_ERR_DIVERGENT;
        return S;
    }
    S.len = qTot;
    S.mism = mism;
    S.first_mis = first_mis;
    S.last_mis = last_mis;
    return S;
}

// per-pair match statistics through the generic lock-step walks (any CIGAR)
__device__ __forceinline__ u64 pair_stats_generic(const OpsView cig, u32 nc, int32_t pos, int32_t aligned, const uint8_t *seq,
                                                  int32_t lq, const uint8_t *genome, int32_t glen, bool has_x, const u32 *gcodes,
                                                  int32_t left, int32_t istart, int32_t iend, int32_t right, u32 g, u64 *err, u32 opi,
                                                  int32_t qN, int32_t q_limit) {
    if (lq <= 1) { // junction.cc:168-185
        const u32 totUp = (u32)((istart - 1) - left + 1);
        const u32 totDown = (u32)(right - (iend + 1) + 1);
        return pack_res(0, totUp < totDown ? totUp : totDown, 0);
    }
    // Where the walks start.  The pair's N operation is operation `opi`; it starts at istart, qN query bases into the read.  The
    // left side walks BACK from it to the first operation that starts inside the window -- an operation that starts before the
    // window is stepped over whole by the walks, and so is everything before it --, the right side starts at the operation
    // behind the N.  (A read of 95 operations and 15 introns walked all 95 four times per pair.)
    u32 kL = opi, kR = 0;
    int32_t rL = istart, qL = qN, rR = pos, qR = 0;
    while (kL > 0) {
        const u32 op = cig[kL - 1], ty = op & 15u;
        const int32_t ln = (int32_t)(op >> 4);
        const int32_t rp = rL - (op_consumes_ref(ty) ? ln : 0);
        if (rp < left) break; // (it starts before the window: stepped over, like all before it)
        kL--;
        rL = rp;
        if (op_consumes_query(ty) && ty != OP_S) qL -= ln;
    }
    const int32_t after = istart + (int32_t)(cig[opi] >> 4); // the walks' position behind the N (iend + 1 unless it was clamped)
    if (after == iend + 1) {
        kR = opi + 1;
        rR = after;
        qR = qN;
    }
    const Side L = anchor_side(cig, nc, pos, aligned, seq, lq, genome, glen, has_x, gcodes, left, istart - 1, kL, rL, qL, q_limit);
    if (L.err) {
        set_error(err, g, L.err);
        return 0;
    }
    const Side R = anchor_side(cig, nc, pos, aligned, seq, lq, genome, glen, has_x, gcodes, iend + 1, right, kR, rR, qR, q_limit);
    if (R.err) {
        set_error(err, g, R.err);
        return 0;
    }
    const u32 upM = L.last_mis < 0 ? (u32)L.len : (u32)(L.len - 1 - L.last_mis);  // getNbMatchesFromEnd :272
    const u32 downM = R.first_mis < 0 ? (u32)R.len : (u32)R.first_mis;            // getNbMatchesFromStart :263
    const u32 tu = (u32)(L.len - L.mism), td = (u32)(R.len - R.mism);
    return pack_res(upM < downM ? upM : downM, tu < td ? tu : td, (u32)(L.mism + R.mism));
}

// K4b: every pair that is not of the simple shape (multi-junction reads, indels, = X P H ops, exotic contigs, SEQ '*'), one
// thread per READ of the lists k1_emit and k1_generic compacted -- the second list holds only the closed reads whose window check
// the chain's bound B could not rule out (ContigStats::max_span) --: the read's fields come from the record k1_count kept of it
// (spl_rec), its batch from the block's table, its operations are fetched once (two 16-byte loads into an LDS column) and
// walked once; at every N operation the pair's junction-level anchors (kd_assign) are looked up and the two lock-step
// walks start right there (op index and query offset are at hand: no hint has to travel with the pair).  The result
// goes into the pair's record.  Runs on the side stream, beside the sort.
__global__ __launch_bounds__(256) void k4b_generic(const u64 *list, const u32 *gen_cnt, u32 cap, const u64 *key, PairRec *rec, const u32 *jid_bam,
                                                    KeyFmt kf, const DevBatch *batches, int n_batches, const int32_t *anc_l, const int32_t *anc_r,
                                                    GroupTab G, int genome_has_x, int use_codes, u64 *err, const ContigStats *cs, u32 pack_nn,
                                                    const u32 *spl_idx, const uint4 *spl_rec) {
    __shared__ u32 s_ops[OPS_LDS][256];
    __shared__ u32 s_first[2 * GEN_SHARDS + 1]; // item index of every sub-list's first entry (both lists, one index space)
    __shared__ u32 s_wsum[4];
    __shared__ BatchTab s_bt;
    if (cs->P == 0) return; // (a limit was exceeded while the junction ids were built: there are no ids, the chain is repeated)
    // The sub-lists are filled to different heights (sub-list `shard` of list `l` occupies [(l GEN_SHARDS + shard) cap, ... + its
    // count)): every block numbers their entries -- an exclusive scan over the 512 counts -- and the grid strides over the items.
    {
        const u32 i0 = threadIdx.x * 2;
        const u32 c0 = gen_cnt[(i0 % GEN_SHARDS) * GEN_CNT_STRIDE + (i0 / GEN_SHARDS) * 2];
        const u32 c1 = gen_cnt[((i0 + 1) % GEN_SHARDS) * GEN_CNT_STRIDE + ((i0 + 1) / GEN_SHARDS) * 2];
        const u32 n0 = c0 < cap ? c0 : cap, n1 = c1 < cap ? c1 : cap;
        s_bt.fill(batches, n_batches);
        u32 total;
        const u32 ex = block_escan<4>(n0 + n1, s_wsum, &total);
        s_first[i0] = ex;
        s_first[i0 + 1] = ex + n0;
        if (threadIdx.x == 255) s_first[2 * GEN_SHARDS] = total;
        __syncthreads();
    }
    static_assert(GEN_SHARDS == 256, "two sub-lists per thread of the block");
    const u32 n_items = s_first[2 * GEN_SHARDS];
    for (u32 item0 = blockIdx.x * 256; item0 < n_items; item0 += gridDim.x * 256) {
    const u32 item = item0 + threadIdx.x;
    if (item >= n_items) continue; // (no barrier below)
    u32 sub = 0; // the last sub-list with s_first[sub] <= item
#pragma unroll
    for (u32 step = GEN_SHARDS; step > 0; step >>= 1)
        if (sub + step < 2 * GEN_SHARDS && s_first[sub + step] <= item) sub += step;
    const bool check_only = sub >= GEN_SHARDS;
    const u64 entry = list[(size_t)sub * cap + (item - s_first[sub])];
    const u32 p0 = (u32)(entry >> 32);
    const u32 slot = check_only && pack_nn ? (u32)entry & 0x0fffffffu : (u32)entry; // the read's place in the tiles' spliced lists
    if (check_only) {
        // A read [S] M (N M)+ [S] whose pairs k1_emit finished with the M blocks as anchors.  That is what the walks produce
        // unless the junction's window reaches over a neighbouring intron of the read: on the left the walk starts at the
        // first operation that begins inside the window (the previous N begins at its istart), on the right it stops at an N
        // that ends outside it (bam_alignment.cc:359).  A read that fails the test takes the walks below -- all its pairs.
        // N operations of the read: in the entry, or from its first pair's record (no junction of the read ends before that pair, one is its own)
        const u32 code = pack_nn ? (u32)entry >> 28 : 15u;
        const u32 nN = code < 15u ? code : (reinterpret_cast<const uint4 *>(rec + p0)[1].w >> 16) + 1u;
        bool ok = true;
        int32_t prev_istart = 0, is, ie;
        unpack_key(kf, key[p0], is, ie);
        for (u32 k = 0; k < nN; k++) {
            const u32 j = jid_bam[p0 + k];
            int32_t nis = 0, nie = 0;
            if (k + 1 < nN) unpack_key(kf, key[p0 + k + 1], nis, nie);
            if (k > 0 && prev_istart >= anc_l[j]) ok = false;
            if (k + 1 < nN && nie + 1 <= anc_r[j]) ok = false;
            prev_istart = is;
            is = nis;
            ie = nie;
        }
        if (ok) continue;
    }
    // what k1_count kept of the read (spl_rec: first operation, position, first word of the bases, operations | bases present | l_qseq --
    // no gathers of cig_off, l_qseq, seq_off) and its batch, from the slot's tile
    const int bi = s_bt.find(batches, n_batches, slot / (u32)K1_TILE);
    const DevBatch &b = batches[bi];
    const u32 r = spl_idx[slot];
    const uint4 sr = spl_rec[slot];
    const u32 g = gload(&b.base) + r;
    const u32 c0 = sr.x;
    u32 nc = sr.w & 0x7fffu;
    if (nc == 0x7fffu) nc = gload(b.cig_off + r + 1) - c0; // (a count that did not fit the record)
    OpsView cig;
    cig.g = b.cigar + c0;
    cig.lds = &s_ops[0][threadIdx.x];
    {
        u32 w[OPS_LDS];
        fetch_ops8(as_global(b.cigar), c0, s_bt.cig_words(b, bi), w);
#pragma unroll
        for (int k = 0; k < OPS_LDS; k++) s_ops[k][threadIdx.x] = (u32)k < nc ? w[k] : 0u;
    }
    const uint4 rb = reinterpret_cast<const uint4 *>(rec + p0)[1]; // pos | aend | meta | updown of the read's first pair
    const int32_t vpos = (int32_t)rb.x, aend = (int32_t)rb.y;
    const Member M = member_of(G, vpos); // the read's target: everything below is in the target's own coordinates
    const int32_t pos = vpos - M.voff;
    int32_t lq = (int32_t)(sr.w >> 16);
    if (lq == 0xffff) lq = gload(b.l_qseq + r);
    const u32 so0 = sr.z;
    if (lq > 1 && !(sr.w & 0x8000u)) { // (the record carries fewer than lq bases)
        set_error(err, g, PJB_ERR_NO_SEQ);
        continue; // (the records keep aux = 0)
    }
    const uint8_t *seq = b.seq4 + (size_t)so0 * 4;
    const int32_t q_limit = (int32_t)min(s_bt.seq_words(b, bi) - 1u - so0, 0x7fffffffu); // (to the end of the batch's bases: chunk_load)
    u32 k = 0;
    int32_t qsum = 0; // query bases before the operation, soft clips not counted (anchor_side's qPos)
    for (u32 i = 0; i < nc; i++) {
        const u32 op = cig[i], ty = op & 15u;
        if (ty == OP_N) {
            const u32 p = p0 + k;
            const u32 j = jid_bam[p];
            int32_t istart, iend;
            unpack_key(kf, key[p], istart, iend);
            const u64 res = pair_stats_generic(cig, nc, pos, aend - vpos + 1, seq, lq, M.d, M.len, genome_has_x != 0, use_codes ? M.codes : (const u32 *)nullptr,
                                               anc_l[j] - M.voff, istart - M.voff, iend - M.voff, anc_r[j] - M.voff, g, err, i, qsum, q_limit);
            *reinterpret_cast<u64 *>(rec + p) = res; // PairRec::aux
            k++;
        }
        if (op_consumes_query(ty) && ty != OP_S) qsum += (int32_t)(op >> 4);
    }
    } // items
}

// how two values of word k of a fragment record combine (k4_pairs over a range's slices, k5_frag_reduce over a junction's fragments)
__device__ __forceinline__ u32 frag_combine(int k, u32 a, u32 b) {
    if (k >= F_MAXMINANC && k <= F_MAXMINMATCH) return a > b ? a : b;
    if (k == F_FIRSTMIS) return a < b ? a : b;
    return a + b; // sums; F_MISM_LO/HI are handled as one 64-bit add by the caller
}
// A slice's totals for one junction, from the lane that holds them to one word of the fragment record a lane: the sixteen words (13 + 20
// byte counters packed in nine, five maxima, the minimum, a zero) go through the wavefront's own 64 bytes of LDS, and lane k reads the one
// its field lies in.  (Selecting among sixteen registers by lane number costs 30 compares whose masks the compiler keeps in SGPRs: the
// kernel then spills.)  Wavefront-local: no barrier, the LDS unit serves a wavefront's instructions in order.
// the sixteen words in LDS order: the four words of the first thirteen counters | the maxima | the last maximum, the minimum, the first
// two words of the twenty JAD counters | their other three, a zero
enum { FW_CNT = 0, FW_MAX = 4, FW_MIN = 9, FW_JAD = 10 };
struct FragWordOf {
    u32 word, shift, mask; // of lane k's field: the word among the sixteen, the byte's shift in it, all-ones / 0xff / 0 (no field)
    __device__ __forceinline__ explicit FragWordOf(int k) {
        const bool c = k <= F_DIST, a = k >= F_JAD0 && k < F_JAD0 + 20, m = k >= F_MAXMINANC && k <= F_FIRSTMIS;
        const int q = a ? k - F_JAD0 : k;
        word = c ? FW_CNT + (u32)(q >> 2) : a ? FW_JAD + (u32)(q >> 2) : m ? FW_MAX + (u32)(k - F_MAXMINANC) : 15u;
        shift = c || a ? 8u * (u32)(q & 3) : 0u;
        mask = c || a ? 0xffu : m ? 0xffffffffu : 0u;
    }
    // four of the sixteen words at a time, as soon as they are folded (all sixteen results held back at once cost sixteen registers)
    __device__ __forceinline__ static void put(u32 *tot, int quad, bool holder, u32 a, u32 b, u32 c, u32 d) {
        if (holder) reinterpret_cast<uint4 *>(tot)[quad] = make_uint4(a, b, c, d);
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ u32 get(const u32 *tot) const {
        __builtin_amdgcn_wave_barrier();
        const u32 w = (tot[word] >> shift) & mask;
        __builtin_amdgcn_wave_barrier();
        return w;
    }
};

// K4: gather the pairs in sorted order -- one 32-byte record each -- and fold predicates and match statistics to fragments
// (junction.cc:862-909 accumulators, :755-814 counters).
// Fragments.  A wavefront owns a RANGE of 2^range_shift consecutive 64-pair slices of the sorted pair array and walks them in order.  A
// fragment is a maximal run of one junction inside one range; its slot is jid + range index (frag_slot, pjb_device.hip.h, with the rule
// for the slots that stay unused).  Per slice the 33 counters are folded in packed 8-bit form -- whole-wave reductions on the DPP path
// where the slice holds one junction, a segmented reduce otherwise --; the fragment that is open across slices lives one word a lane
// (lane k: word k, k5_frag_reduce's layout), takes each slice's totals with frag_combine and leaves with one coalesced 192-byte store
// when its junction or the range ends.  While a slice is folded the next one's records and keys and the indices of the one after are on
// their way; the pair before a slice is lane 63 of the slice before -- only a range's first slice fetches it.
// A second small kernel reduces slots -> junctions (segmented again, then one atomic per wave and junction), so a
// junction with 10^6 pairs costs a few dozen same-address atomics, not 10^6.
// masks (nullptr: the chain that sorted the full keys has its runs from the head scan): per 64-pair slice, the lanes where a
// junction starts and the lanes where a run of equal read positions starts (entropy, junction.cc:730-749) -- this kernel holds
// every pair's record anyway, k2_expand turns the bits into seg_off / run_first / run_start without touching a pair.
__global__ __launch_bounds__(256) void k4_pairs(const u32 *sidx, const u32 *jid_of, const PairRec *rec, const u64 *jkey, KeyFmt kf, const u32 *np,
                                                 u32 *frag, int32_t *frag_j, u64 *head_mask, u64 *run_mask, const ContigStats *cs_chk, u64 *err_chk,
                                                 int range_shift) {
    __shared__ __attribute__((aligned(16))) u32 s_tot[4][16];
    const u32 n = *np;
    const int lane = lane_id();
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); // (in an SGPR: the range, its loop and its branches are scalar)
    const u32 range = blockIdx.x * 4 + wave;
    u32 *tot = s_tot[wave];
    const FragWordOf word_of(lane);
    const u64 first = (u64)range << (6 + range_shift);
    if (first >= n) return;
    const u32 i0 = (u32)first;
    const u32 n_sl = min(1u << range_shift, (n - i0 + 63) >> 6); // slices of this range that hold a pair
    // (loads unconditional, index clamped to n - 1, masked after: see k1_count.  Nothing behind the pairs is touched.)
    // (32 bits do: n <= 0xffffff00 and at() is asked for the slice behind the range's last at the most)
    auto at = [&](u32 s) { return min(i0 + 64u * s + (u32)lane, n - 1); };
    auto key_of = [&](u32 jl) { // a slice of one junction (most are) asks for its key once
        const u32 jf = (u32)__builtin_amdgcn_readfirstlane((int)jl);
        return __ballot(jl != jf) == 0 ? jkey[jf] : jkey[jl];
    };
    u32 jv = jid_of[at(0)];
    const u32 p0 = sidx[at(0)];
    u32 j_nx = jid_of[at(1)], p_nx = sidx[at(1)];
    // the pair before the range: j, pos, aend of the last pair a slice saw go to the next one's lane 0
    u32 jprev_c = 0xffffffffu;
    int32_t pos_c = 0, aend_c = 0;
    if (i0 > 0) {
        jprev_c = jid_of[i0 - 1];
        const uint4 q = reinterpret_cast<const uint4 *>(rec + sidx[i0 - 1])[1];
        pos_c = (int32_t)q.x;
        aend_c = (int32_t)q.y;
    }
    PairRec Rc = rec_load(rec + p0);
    u64 jk = key_of(jv);
    // the open fragment: its junction, word `lane` of its record, the 64-bit sum of F_MISM_LO / F_MISM_HI
    u32 open_j = 0xffffffffu, fv = 0;
    u64 fm = 0;
    auto flush = [&]() {
        if (open_j == 0xffffffffu) return;
        const u32 slot = open_j + range;
        if (lane < F_WORDS) frag[(size_t)slot * F_WORDS + lane] = lane == F_MISM_LO ? (u32)fm : lane == F_MISM_HI ? (u32)(fm >> 32) : fv;
        if (lane == 0) frag_j[slot] = (int32_t)open_j;
    };
    auto absorb = [&](u32 jh, u32 w, u64 m64) { // a slice's totals for junction jh (wave-uniform), this lane's word of them
        if (jh != open_j) {
            flush();
            open_j = jh;
            fv = w;
            fm = m64;
        } else {
            fv = frag_combine(lane, fv, w);
            fm += m64;
        }
    };
    for (u32 s = 0; s < n_sl; s++) {
        PairRec Rn = Rc;
        u64 jkn = jk;
        u32 j_n2 = j_nx, p_n2 = p_nx;
        if (s + 1 < n_sl) {
            Rn = rec_load(rec + p_nx);
            jkn = key_of(j_nx);
        }
        if (s + 2 < n_sl) {
            j_n2 = jid_of[at(s + 2)];
            p_n2 = sidx[at(s + 2)];
        }
        const u32 i = i0 + 64u * s + (u32)lane; // (the slice's first pair lies below n <= 0xffffff00)
        const bool valid = i < n;
#ifdef PJB_SELFCHECK // (debug builds: what the sort hands over must be a permutation of the pairs with ids below J that ascend in steps of 0 or 1)
        {
            const u32 ic = valid ? i : n - 1;
            const u32 Jc = cs_chk->J;
            const u32 jb = ic ? jid_of[ic - 1] : jv;
            int bad = 0;
            if (sidx[ic] >= n) bad = 1;
            else if (jv >= Jc) bad = 2;
            else if (jv != jb && jv != jb + 1) bad = 3;
            else if (ic == 0 && jv != 0) bad = 4;
            else if (ic == n - 1 && jv != Jc - 1) bad = 5;
            else if (frag_slot(jv, ic, range_shift) + 1 >= cs_chk->n_slots) bad = 6;
            else if ((ic >> 6) >= cs_chk->n_slices) bad = 7;
            else if (cs_chk->n_slots != frag_slots(Jc, n, range_shift)) bad = 8;
            if (__ballot(bad != 0)) {
                if (bad) set_error(err_chk, 0xffffe000u + (u32)bad, PJB_ERR_HIP);
                return;
            }
        }
#endif
        // the pair before this one in sorted order: the neighbouring lane's -- lane 0 has it from the slice before
        u32 jprev_v = __shfl_up(jv, 1, 64);
        int32_t pos_prev = __shfl_up(Rc.pos, 1, 64), aend_prev = __shfl_up(Rc.aend, 1, 64);
        if (lane == 0) {
            jprev_v = jprev_c;
            pos_prev = pos_c;
            aend_prev = aend_c;
        }
        u32 j = 0xffffffffu;
        u32 cnt[4] = {0, 0, 0, 0}, jadp[5] = {0, 0, 0, 0, 0}, mx[5] = {0, 0, 0, 0, 0};
        u32 first_mis = 100000000u; // junction.cc:864
        u32 nb_mis = 0;
        if (valid) {
            j = jv;
            int32_t istart, iend;
            unpack_key(kf, jk, istart, iend);
            const u64 rs = Rc.aux;
            const u32 minMatch = (u32)(rs & 0xfffffu), mmes = (u32)((rs >> 20) & 0xfffffu), nbMis = (u32)(rs >> 40);
            const u32 meta = Rc.meta;
            const u32 cat = meta & META_CAT_MASK;
            const u32 xs = (meta >> META_XS_SHIFT) & 3u;
            // distinct alignment runs in BAM order (junction.cc:763-771): compare with the previous pair of the junction
            const bool dist_head = i == 0 || jprev_v != j || pos_prev != Rc.pos || aend_prev != Rc.aend;
            // 8-bit lanes: a slice adds at most 64 per field
            cnt[0] = 1u | ((u32)(cat == 0) << 8) | ((u32)(cat == 1) << 16) | ((u32)(cat == 2) << 24);
            cnt[1] = (u32)(cat == 3) | ((u32)((meta & META_MULTI) != 0) << 8) | ((u32)(xs == 1) << 16) | ((u32)(xs == 2) << 24);
            cnt[2] = (u32)((meta & META_UM) != 0) | ((u32)((meta & META_BPP) != 0) << 8) | ((u32)((meta & META_PPP) != 0) << 16) |
                     ((u32)((meta & META_REL) != 0) << 24);
            cnt[3] = (u32)dist_head;
#pragma unroll
            for (int w = 0; w < 5; w++) // junction.cc:875-877: JAD[k]++ for k < min(20, minMatch)
                jadp[w] = (u32)((u32)(4 * w) < minMatch) | ((u32)((u32)(4 * w + 1) < minMatch) << 8) |
                          ((u32)((u32)(4 * w + 2) < minMatch) << 16) | ((u32)((u32)(4 * w + 3) < minMatch) << 24);
            const int32_t la = istart - Rc.lstart, ra = Rc.rend - iend; // Intron::minAnchorLength intron.cc:81-83
            mx[0] = (u32)(la < ra ? la : ra);
            mx[1] = Rc.updown & 0xffffu;
            mx[2] = Rc.updown >> 16;
            mx[3] = mmes;
            mx[4] = minMatch;
            first_mis = minMatch > 0 ? minMatch : 100000000u;
            nb_mis = nbMis;
            // unused fragment slots: the one skipped when a junction starts with the range, and the last one
            if (s == 0 && lane == 0) {
                const int64_t u = frag_unused_before(j, i, jprev_v != j, range_shift);
                if (u >= 0) frag_j[u] = -1;
            }
            const int64_t u = frag_unused_behind(j, i, n, range_shift);
            if (u >= 0) frag_j[u] = -1;
        }
        const bool hj = valid && (i == 0 || jprev_v != j);
        if (head_mask) {
            const bool hr = valid && (hj || pos_prev != Rc.pos);
            const u64 mj = __ballot(hj), mr = __ballot(hr);
            if (lane == 0) { // (a slice word per 64 pairs: the arrays hold ceil(n / 64) words, and s < n_sl)
                head_mask[i >> 6] = mj;
                run_mask[i >> 6] = mr;
            }
        }
        // (a slice with a successor is full: lane 63 holds a pair)
        jprev_c = (u32)__builtin_amdgcn_readlane((int)jv, 63);
        pos_c = __builtin_amdgcn_readlane(Rc.pos, 63);
        aend_c = __builtin_amdgcn_readlane(Rc.aend, 63);
        // ---- the slice's segments -- one, usually: a junction has a few hundred pairs -- in order.  Lane 0 heads the first whether or
        // not its junction began there: that one may continue the open fragment.  Each is folded by whole-wave reductions on the DPP
        // path over its own lanes (16 x 6 VALU steps; the lanes outside contribute the identities, as the lanes past the end do);
        // lane 63 ends up with the totals and hands them on.
        u64 heads = __ballot(valid && (lane == 0 || jprev_v != j));
        while (heads) {
            const int h = __ffsll((unsigned long long)heads) - 1;
            heads &= heads - 1;
            const int e = heads ? __ffsll((unsigned long long)heads) - 1 : 64;
            const bool in = lane >= h && lane < e;
            const bool last = lane == 63;
            auto add = [&](u32 v) { return wave_fold<DppAdd>(in ? v : 0u); };
            auto top = [&](u32 v) { return wave_fold<DppMax>(in ? v : 0u); };
            __builtin_amdgcn_wave_barrier(); // (the lanes' reads of the segment before are done)
            FragWordOf::put(tot, FW_CNT / 4, last, add(cnt[0]), add(cnt[1]), add(cnt[2]), add(cnt[3]));
            FragWordOf::put(tot, FW_MAX / 4, last, top(mx[0]), top(mx[1]), top(mx[2]), top(mx[3]));
            FragWordOf::put(tot, 2, last, top(mx[4]), wave_fold<DppMin>(in ? first_mis : 100000000u), add(jadp[0]), add(jadp[1]));
            FragWordOf::put(tot, 3, last, add(jadp[2]), add(jadp[3]), add(jadp[4]), 0u);
            // (a pair has fewer than 2^24 mismatches: 64 of them fit 32 bits)
            const u32 mis = wave_total<DppAdd>(in ? nb_mis : 0u);
            absorb((u32)__builtin_amdgcn_readlane((int)j, h), word_of.get(tot), (u64)mis);
        }
        Rc = Rn;
        jk = jkn;
        jv = j_nx;
        j_nx = j_n2;
        p_nx = p_n2;
    }
    flush();
}

// K5a: fragment slots -> junction accumulators (acc pre-initialised: sums 0, max 0, min 100000000).
// One wavefront walks FRAG_SLOTS_PER_WAVE consecutive slots; lane k owns word k of the 48-word record, so every
// load is one coalesced 192-byte row and a junction's run of slots is folded in registers; the run
// is flushed with one atomic per word when the junction changes.
constexpr int FRAG_SLOTS_PER_WAVE = 16; // short per-wave chains keep enough wavefronts in flight
__global__ __launch_bounds__(256) void k5_frag_reduce(const u32 *frag, const int32_t *frag_j, const u32 *n_slots_p, u32 *acc) {
    const u32 n_slots = *n_slots_p;
    const u32 wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int k = lane_id();
    const u32 s0 = wave * FRAG_SLOTS_PER_WAVE;
    if (s0 >= n_slots) return;
    const int32_t myj = (k < FRAG_SLOTS_PER_WAVE && s0 + k < n_slots) ? frag_j[s0 + k] : -1;
    int32_t cur = -1;
    u32 v = 0, carry_lo = 0; // lane F_MISM_HI also keeps the low word to do the 64-bit add
    auto flush = [&](int32_t j) {
        if (j < 0 || k >= F_JAD0 + 20) return;
        u32 *dst = acc + (size_t)j * F_WORDS + k;
        if (k == F_MISM_LO) return; // done by lane F_MISM_HI as one 64-bit atomic
        if (k == F_MISM_HI) {
            atomicAdd(reinterpret_cast<u64 *>(dst - 1), ((u64)v << 32) | carry_lo);
        } else if (k >= F_MAXMINANC && k <= F_MAXMINMATCH) atomicMax(dst, v);
        else if (k == F_FIRSTMIS) atomicMin(dst, v);
        else if (v) atomicAdd(dst, v);
    };
    // (the rows of all sixteen slots are asked for before the first is folded: sixteen loads on their way at once, not a chain of
    // sixteen round trips)
    u32 row[FRAG_SLOTS_PER_WAVE];
#pragma unroll
    for (int q = 0; q < FRAG_SLOTS_PER_WAVE; q++) {
        const int32_t jq = __shfl(myj, q, 64);
        row[q] = (jq >= 0 && k < F_WORDS) ? frag[(size_t)(s0 + (u32)q) * F_WORDS + k] : 0u;
    }
#pragma unroll
    for (int q = 0; q < FRAG_SLOTS_PER_WAVE; q++) { // (no break / continue: the loop unrolls and row[] stays in registers)
        const int32_t j = __shfl(myj, q, 64);
        if (j >= 0) { // (unused slots and those past the last have -1)
            const u32 w = row[q];
            const u32 wlo = __shfl(w, F_MISM_LO, 64);
            if (j != cur) {
                flush(cur);
                cur = j;
                v = w;
                carry_lo = wlo;
            } else if (k == F_MISM_HI) {
                const u64 sum = (((u64)v << 32) | carry_lo) + (((u64)w << 32) | wlo);
                v = (u32)(sum >> 32);
                carry_lo = (u32)sum;
            } else {
                v = frag_combine(k, v, w);
            }
        }
    }
    flush(cur);
}

} // namespace pjb
