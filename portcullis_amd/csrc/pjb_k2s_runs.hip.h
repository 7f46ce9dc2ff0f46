// pjb_k2s_runs.hip.h -- K2s of the junc chain: where junctions and position runs begin in the sorted pair array (k2_*), and the full-key chain's
// catch-up (kf_*).  Reads the sorted ids with k4_pairs' head / run masks (k2_expand), or the sorted full keys (HeadFn, HeadSink, k2_close);
// leaves seg_off, run_first, run_start and the counts J, R in ContigStats for K5.  kf_init / kf_anchors give the full-key chain what
// kd_assign gives the usual one: rest states, jid_bam, the anchors.
#pragma once

#include "pjb_device.hip.h"

namespace pjb {

// ---------------------------------------------------------------------------------------------
// K2s: segment heads.  For sorted position i:  head_j = new intron key; head_r = head_j or read
// position differs from the previous pair of the junction (entropy runs, junction.cc:730-749).
// One u64 scan carries both counters (junction count << 32 | run count).
// ---------------------------------------------------------------------------------------------
struct HeadFn {
    const u64 *skey;
    const u32 *sidx;
    const PairRec *rec;
    __device__ u64 operator()(u64 i) const {
        const u64 im = i ? i - 1 : 0; // (every load unconditional)
        const u64 ka = skey[i], kb = skey[im];
        const u32 sa = sidx[i], sb = sidx[im];
        const int32_t pa = rec[sa].pos, pb = rec[sb].pos;
        const bool hj = i == 0 || ka != kb;
        const bool hr = hj || pa != pb;
        return ((u64)hj << 32) | (u64)hr;
    }
};
struct HeadSink {
    u32 *jid_of;    // [P]   junction id per sorted pair
    u32 *seg_off;   // [J+1] first sorted pair of junction
    u32 *run_first; // [J+1] first run of junction
    u32 *run_start; // [R+1] first sorted pair of run
    const u64 *skey;
    u64 *jkey;      // [J]   intron key of the junction -- when the sort ran on the full keys (nullptr: K2d left the table)
    u32 junc_limit; //       entries jkey has (the other arrays are pair-sized; k2_close stops the chain when there are more heads)
    __device__ void operator()(u64 i, u64 v, u64 ex) const {
        const u32 j = (u32)(ex >> 32) + (u32)(v >> 32) - 1; // inclusive count - 1
        const u32 r = (u32)ex + (u32)v - 1;
        jid_of[i] = j;
        if (v >> 32) {
            seg_off[j] = (u32)i;
            run_first[j] = r;
            if (jkey && j < junc_limit) jkey[j] = skey[i];
        }
        if ((u32)v) run_start[r] = (u32)i;
    }
};
__global__ void k2_close(u64 *total, u32 *seg_off, u32 *run_first, u32 *run_start, ContigStats *cs, u32 junc_limit, const u32 *gen_cnt, u32 gen_cap,
                         int range_shift) {
    const u32 n_pairs = cs->P;
    if (n_pairs == 0) return;
    {
        u32 need = 0;
        for (u32 sh = 0; sh < GEN_SHARDS; sh++) need = max(need, lists_over(gen_cnt, sh, gen_cap));
        if (need) { // a read list overflowed: the chain is repeated with more room
            cs->list_need = need;
            cs->overflow |= OVF_LISTS;
            cs->P = 0;
            return;
        }
    }
    const u32 J = (u32)(*total >> 32), R = (u32)*total;
    cs->n_junc = J;
    cs->n_runs = R;
    if (J > junc_limit) { // the junction-sized buffers are too small: everything downstream stands still
        cs->overflow |= OVF_JUNC;
        cs->P = 0;
        return;
    }
    seg_off[J] = n_pairs;
    run_first[J] = R;
    run_start[R] = n_pairs;
    cs->J = J;
    cs->R = R;
    cs->n_slots = frag_slots(J, n_pairs, range_shift);
}

// K2s for the chain on dense ids: k4_pairs left two bits per sorted pair (junction starts / position run starts), a scan over the
// slices' popcounts numbers the runs, and this kernel writes what HeadSink writes -- from the masks and the sorted ids alone.
struct Popc64Fn {
    const u64 *words;
    __device__ u64 operator()(u64 i) const { return (u64)__popcll(words[i]); }
};
constexpr int K2E_PER = 4;
__global__ __launch_bounds__(256) void k2_expand(const u32 *sid, const u64 *head_mask, const u64 *run_mask, const u32 *run_base, const u64 *total,
                                                 u32 *seg_off, u32 *run_first, u32 *run_start, ContigStats *cs) {
    const u32 n = cs->P;
#pragma unroll
    for (int q = 0; q < K2E_PER; q++) { // (a wavefront takes K2E_PER slices: their mask words' loads travel together)
        const u32 i = (blockIdx.x * K2E_PER + q) * 256 + threadIdx.x;
        if (i >= n) continue;
        const u32 sl = i >> 6, bit = i & 63u;
        const u64 mr = run_mask[sl], mj = head_mask[sl];
        if ((mr >> bit) & 1ull) {
            const u32 r = run_base[sl] + (u32)__popcll(mr & ((1ull << bit) - 1ull));
            run_start[r] = i;
            if ((mj >> bit) & 1ull) {
                const u32 j = sid[i];
                seg_off[j] = i;
                run_first[j] = r;
            }
        }
    }
    if (n > 0 && (n - 1) / (256u * K2E_PER) == blockIdx.x && threadIdx.x == 0) { // (k2_close's part: once, by the block that holds the last pair)
        const u32 R = (u32)*total, J = cs->J;
        seg_off[J] = n;
        run_first[J] = R;
        run_start[R] = n;
        cs->n_runs = cs->R = R;
    }
}

// Junction anchors from pairs that sit in the lanes of a wavefront (any order): leftAncStart = min lStart, rightAncEnd = max
// rEnd (junction.cc:477-529).  In BAM order the pairs of the two or three junctions of a locus alternate from lane to lane, so
// the wavefront takes its DISTINCT junctions one after the other -- all lanes of one junction are folded on the DPP path,
// whatever lies between them -- and one lane per junction touches the arrays, and only if the value would move them (a
// read at L2 first: the arrays only ever move one way, so an older value errs on the side of one atomic too many).  (Folding
// neighbouring lanes only left one atomic per lane wherever junctions alternate: 1.4 ms per chain on one L2 channel.)
__device__ __forceinline__ void anchors_fold(bool valid, u32 j, int32_t l, int32_t r, int32_t *anc_l, int32_t *anc_r) {
    const u32 lk = (u32)l ^ 0x80000000u, rk = (u32)r ^ 0x80000000u; // (signed order through the sign bit)
    u64 todo = __ballot(valid);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const u32 jc = (u32)__builtin_amdgcn_readlane((int)j, first);
        const bool mine = valid && j == jc;
        const u64 m = __ballot(mine);
        const int32_t lo = (int32_t)(wave_total<DppMin>(mine ? lk : 0xffffffffu) ^ 0x80000000u);
        const int32_t hi = (int32_t)(wave_total<DppMax>(mine ? rk : 0u) ^ 0x80000000u);
        if (lane_id() == first) { // (the look goes to L2, where the atomics are done: a CU's L1 would keep showing it the line it fetched first)
            if (lo < __hip_atomic_load(&anc_l[jc], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&anc_l[jc], lo);
            if (hi > __hip_atomic_load(&anc_r[jc], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&anc_r[jc], hi);
        }
        todo &= ~m;
    }
}

// ---------------------------------------------------------------------------------------------
// The chain that sorted the FULL keys (PJB_DENSE_IDS off, raw keys, or a donor with more acceptors than K2d keeps) has its
// junction ids only now: two small kernels give it what kd_assign gives the usual chain -- the rest state of anchors and
// accumulators, the junction id of every pair in BAM order (k4b_generic works in BAM order) and the anchors.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kf_init(u32 *acc, const u32 *n_junc_p, int32_t *anc_l, int32_t *anc_r) {
    const u32 n_junc = *n_junc_p;
    acc_rest_state(acc, n_junc);
    for (u64 t = (u64)blockIdx.x * 256 + threadIdx.x; t < n_junc; t += (u64)gridDim.x * 256) {
        anc_l[t] = INT32_MAX;
        anc_r[t] = INT32_MIN;
    }
}
__global__ __launch_bounds__(256) void kf_anchors(const u32 *sidx, const u32 *jid_of, const PairRec *rec, const u32 *np, u32 *jid_bam, int32_t *anc_l,
                                                   int32_t *anc_r) {
    const u32 n = *np;
    if (blockIdx.x * 256u >= n) return;
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    const u32 ic = valid ? i : n - 1;
    const u32 p = sidx[ic], j = jid_of[ic];
    const uint4 ra = *reinterpret_cast<const uint4 *>(rec + p);
    if (valid) jid_bam[p] = j;
    anchors_fold(valid, j, (int32_t)ra.z, (int32_t)ra.w, anc_l, anc_r);
}

} // namespace pjb
