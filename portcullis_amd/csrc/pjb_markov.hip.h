// pjb_markov.hip.h -- `filt --self_train` / `train --markov`: the eight Markov models trained on the device (km_*), behind
// pjb_markov_train (pjb_model_api.hip).  KmerMarkovModel::train / PosMarkovModel::train (lib/src/markov_model.cc:31-54, 80-98) over the
// windows of ModelFeatures::trainCodingPotentialModel / trainSplicingModels (lib/src/model_features.cc:77-158).  Every count is an
// integer add (LDS u32, then global u64), so the tables do not depend on how the work was scheduled; the one floating-point step is
// km_normalise's division, count / row sum, as the host does it.
#pragma once

#include "pjb_features.hip.h"

namespace pjb {

// A window is cut into segments of this many positions; a wavefront takes a segment, its lanes consecutive bases.
constexpr int32_t MARKOV_SEG = 4096;
// The k-mer models in the order pjb_markov_models lists them; which index list trains which.
enum { MK_EXON = 0, MK_INTRON, MK_DONOR_T, MK_DONOR_F, MK_ACCEPTOR_T, MK_ACCEPTOR_F, MK_KMER_MODELS };
enum { MK_LIST_CP = 0, MK_LIST_PASS, MK_LIST_FAIL, MK_LISTS };

struct MarkovJob {
    const pjb_junction_row *rows;
    const GenomeRef *genomes;
    int n_refs;
    const int64_t *idx[MK_LISTS];      // checked by the host: every entry is a row
    u32 n_idx[MK_LISTS];
    u32 win_off[MK_KMER_MODELS + 1];   // model m owns the windows win_off[m] .. win_off[m + 1]: two per entry of `cp` for exon, else one per entry
};
struct MarkovWindow {
    const uint8_t *g;
    int32_t b, e, n; // clamped, inclusive; n bases (0: no genome)
    int neg;
};

// the junction's genome and strand; false: it lies on a target without an uploaded genome
__device__ __forceinline__ bool markov_genome(const MarkovJob &J, const pjb_junction_row &j, MarkovWindow &w) {
    w.neg = j.cons_strand == PJB_STRAND_NEG;
    w.g = nullptr;
    w.b = w.e = w.n = 0;
    return j.refid >= 0 && j.refid < J.n_refs && J.genomes[j.refid].d;
}
__device__ __forceinline__ void markov_clamp(const MarkovJob &J, const pjb_junction_row &j, int32_t beg, int32_t end, MarkovWindow &w) {
    const int32_t gl = J.genomes[j.refid].len;
    w.g = J.genomes[j.refid].d;
    w.b = beg;
    w.e = end;
    fetch_clamp(gl, w.b, w.e);
    w.n = gl > 0 ? w.e - w.b + 1 : 0;
}
// donor / acceptor windows, model_features.cc:118-131: left = [start-3, start+20], right = [end-20, end+2]; on the negative strand
// `right` is the donor and `left` the acceptor
__device__ __forceinline__ void markov_splice_window(const MarkovJob &J, const pjb_junction_row &j, bool donor, MarkovWindow &w) {
    const bool left = donor != (w.neg != 0);
    if (left) markov_clamp(J, j, j.start - 3, j.start + 20, w);
    else markov_clamp(J, j, j.end - 20, j.end + 2, w);
}
// window k of k-mer model m
__device__ bool markov_window(const MarkovJob &J, int m, u32 k, MarkovWindow &w) {
    const int list = m <= MK_INTRON ? MK_LIST_CP : (m == MK_DONOR_T || m == MK_ACCEPTOR_T) ? MK_LIST_PASS : MK_LIST_FAIL;
    const pjb_junction_row &j = J.rows[J.idx[list][m == MK_EXON ? k >> 1 : k]];
    if (!markov_genome(J, j, w)) return false;
    if (m == MK_EXON) { // model_features.cc:86-100: the 200 bases before the intron and the 200 behind it, each a string of its own
        if (k & 1) markov_clamp(J, j, j.end + 1, j.end + 201, w);
        else markov_clamp(J, j, j.start - 202, j.start - 2, w);
    } else if (m == MK_INTRON)
        markov_clamp(J, j, j.start, j.end, w);
    else
        markov_splice_window(J, j, m == MK_DONOR_T || m == MK_DONOR_F, w);
    return true;
}

// segments of every window: 0 unless the window trains -- markov_model.cc:36, `(uint16_t)s.size() > order + 1`, the length cut to 16 bits
// for the gate alone.  *bad: a junction on a target without a genome.
__global__ __launch_bounds__(256) void km_windows(MarkovJob J, u32 *nseg, int *bad) {
    const u32 w = blockIdx.x * 256 + threadIdx.x;
    if (w >= J.win_off[MK_KMER_MODELS]) return;
    int m = 0;
    while (w >= J.win_off[m + 1]) m++;
    MarkovWindow win;
    if (!markov_window(J, m, w - J.win_off[m], win)) {
        atomicOr(bad, 1);
        nseg[w] = 0;
        return;
    }
    nseg[w] = (uint16_t)win.n > PJB_KMER_ORDER + 1 ? ((u32)win.n + (u32)MARKOV_SEG - 1) / (u32)MARKOV_SEG : 0u;
}

// the sink of the prefix sum over the windows' segments (run_scan): off[w] = the segments of the windows before w
struct MarkovOffSink {
    u64 *off;
    __device__ void operator()(u64 i, u64, u64 ex) const { off[i] = ex; }
};

// One k-mer model's transitions: the block owns the segments [first, last) of the model's windows -- gridDim.x equal shares --, its four
// wavefronts take them in turn.  A segment starts PJB_KMER_ORDER bases early for its context and counts only its own positions; position
// i of a window adds 1 to count[context of i-5 .. i-1][base i] for i >= 5.  The counters are the block's static LDS (62 500 B: two
// blocks share a CU's 160 KiB), added to with LDS atomics that return nothing; what is not zero goes to the model's global u64 table.
// The host keeps a block's share at 2^31 bases or fewer (MARKOV_MAX_SEGS, pjb_model_api.hip), so no LDS counter wraps.
__global__ __launch_bounds__(256) void km_count(MarkovJob J, int m, const u64 *seg_off, u64 *counts) {
    __shared__ u32 cnt[PJB_KMER_TABLE];
    const u32 w0 = J.win_off[m], w1 = J.win_off[m + 1];
    const u64 g0 = seg_off[w0], g1 = seg_off[w1];
    const u64 share = (g1 - g0 + gridDim.x - 1) / gridDim.x;
    const u64 first = g0 + share * blockIdx.x, last = first + share < g1 ? first + share : g1;
    if (first >= last) return; // (the whole block)
    for (u32 k = threadIdx.x; k < (u32)PJB_KMER_TABLE; k += 256) cnt[k] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 g = first + wave; g < last; g += 4) {
        u32 lo = w0, hi = w1; // the last window that starts at or before segment g (windows without segments share their start with the next)
        while (hi - lo > 1) {
            const u32 mid = lo + (hi - lo) / 2;
            if (seg_off[mid] <= g) lo = mid;
            else hi = mid;
        }
        MarkovWindow win;
        if (!markov_window(J, m, lo - w0, win)) continue; // (km_windows gave it no segment)
        const u32 i0 = (u32)(g - seg_off[lo]) * (u32)MARKOV_SEG; // (unsigned: i0 + MARKOV_SEG may pass 2^31 in the last segment of a window that long)
        const u32 i1 = (u32)win.n - i0 < (u32)MARKOV_SEG ? (u32)win.n : i0 + (u32)MARKOV_SEG;
        for (u32 i = i0 + lane; i < i1; i += 64) {
            if (i < (u32)PJB_KMER_ORDER) continue;
            u32 ctx = 0;
#pragma unroll
            for (int k = PJB_KMER_ORDER; k >= 1; k--) ctx = ctx * 5u + (u32)window_code(win.g, win.b, win.e, win.neg, (int32_t)i - k);
            const u32 c = (u32)window_code(win.g, win.b, win.e, win.neg, (int32_t)i);
            (void)__hip_atomic_fetch_add(&cnt[ctx * 5u + c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    unsigned long long *out = (unsigned long long *)counts + (size_t)m * PJB_KMER_TABLE;
    for (u32 k = threadIdx.x; k < (u32)PJB_KMER_TABLE; k += 256) {
        const u32 v = cnt[k];
        if (v) (void)__hip_atomic_fetch_add(&out[k], (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The two position models (order 1) from `pass`: position i of the donor / acceptor window adds 1 to count[i][base i] for
// i in 1 .. min(n, PJB_PW_LEN) - 1.  One lane per junction, a block's counts in LDS first.
__global__ __launch_bounds__(256) void km_pos(MarkovJob J, u64 *counts, int *bad) {
    __shared__ u32 cnt[2 * PJB_PW_LEN * 5];
    for (u32 k = threadIdx.x; k < 2u * PJB_PW_LEN * 5; k += 256) cnt[k] = 0;
    __syncthreads();
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r < J.n_idx[MK_LIST_PASS]) {
        const pjb_junction_row &j = J.rows[J.idx[MK_LIST_PASS][r]];
        MarkovWindow win;
        if (!markov_genome(J, j, win)) atomicOr(bad, 1);
        else
            for (int side = 0; side < 2; side++) { // donor, acceptor
                markov_splice_window(J, j, side == 0, win);
                for (int32_t i = 1; i < win.n && i < PJB_PW_LEN; i++)
                    (void)__hip_atomic_fetch_add(&cnt[(side * PJB_PW_LEN + i) * 5 + window_code(win.g, win.b, win.e, win.neg, i)], 1u, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_WORKGROUP);
            }
    }
    __syncthreads();
    unsigned long long *out = (unsigned long long *)counts + (size_t)MK_KMER_MODELS * PJB_KMER_TABLE;
    for (u32 k = threadIdx.x; k < 2u * PJB_PW_LEN * 5; k += 256)
        if (cnt[k]) (void)__hip_atomic_fetch_add(&out[k], (unsigned long long)cnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// markov_model.cc:43-53 / 90-98: every context (position) whose five counts sum to more than 0 is divided by that sum -- count and sum are
// integers below 2^53, exact as doubles, so the quotient is the host's; sizes[model] counts those rows, *transitions sums the k-mer models'.
constexpr u32 MARKOV_ROWS = MK_KMER_MODELS * 3125 + 2 * PJB_PW_LEN;
__global__ __launch_bounds__(256) void km_normalise(const u64 *counts, double *tables, int *sizes, unsigned long long *transitions) {
    const u32 r = blockIdx.x * 256 + threadIdx.x;
    if (r >= MARKOV_ROWS) return;
    const u32 model = r < MK_KMER_MODELS * 3125u ? r / 3125u : MK_KMER_MODELS + (r - MK_KMER_MODELS * 3125u) / PJB_PW_LEN;
    u64 sum = 0;
    for (int k = 0; k < 5; k++) sum += counts[(size_t)r * 5 + k];
    for (int k = 0; k < 5; k++) tables[(size_t)r * 5 + k] = sum ? __ddiv_rn((double)counts[(size_t)r * 5 + k], (double)sum) : 0.0;
    if (sum) {
        atomicAdd(&sizes[model], 1);
        if (model < MK_KMER_MODELS) (void)__hip_atomic_fetch_add(transitions, (unsigned long long)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

} // namespace pjb
