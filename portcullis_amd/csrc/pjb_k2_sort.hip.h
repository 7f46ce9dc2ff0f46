// pjb_k2_sort.hip.h -- K2 of the junc chain: the stable sort of (junction id or full key, pair index) (rs_*).
// Reads the keys in BAM order (jid_bam, or the full keys) and either the tiles' digit counts or the tiles' id runs that kd_assign left;
// leaves the sorted keys and the pair indices in sorted order, which k4_pairs gathers by.  Radix passes (rs_hist, rs_panel_*, rs_scatter),
// or on the run route one counting pass (rs_place).
#pragma once

#include "pjb_device.hip.h"

namespace pjb {

// ---------------------------------------------------------------------------------------------
// K2: stable LSD radix sort of (key, pair index).  Classic 3-step passes: per-tile digit
// histogram -> exclusive scan of the bin-major count matrix -> ranked scatter.  Stability comes
// from ranking in memory order: wave w of a tile owns a contiguous 1/4 of it, rounds are
// contiguous 64-element slices, and equal digits inside a round are ranked by lane with a
// ballot-based match-any.
// ---------------------------------------------------------------------------------------------

template <typename K>
__global__ __launch_bounds__(256) void rs_hist(const K *keys, const u32 *np, int shift, int bits, u32 *hist, u32 n_tiles) {
    __shared__ u32 h[RS_MAX_BINS];
    const u32 n = *np; // the grid covers the host's limit; tiles past the data count nothing
    const u32 nb = 1u << bits;
    for (u32 d = threadIdx.x; d < nb; d += 256) h[d] = 0;
    __syncthreads();
    const u32 base = blockIdx.x * RS_TILE;
    const u32 mask = nb - 1;
    K kk[RS_ITEMS];
#pragma unroll
    for (int k = 0; k < RS_ITEMS; k++) {
        const u32 i = base + k * 256 + threadIdx.x;
        kk[k] = i < n ? keys[i] : (K)0;
    }
#pragma unroll
    for (int k = 0; k < RS_ITEMS; k++) {
        const u32 i = base + k * 256 + threadIdx.x;
        wave_hist_add(h, (u32)(kk[k] >> shift) & mask, i < n);
    }
    __syncthreads();
    // tile-major: a tile's counts are one contiguous run (bin-major, every 4-byte store was a write granule of its own:
    // twice the algorithmic traffic, PMC round 2), and rs_scatter reads its tile's scanned counts the same way
    for (u32 d = threadIdx.x; d < nb; d += 256) hist[(size_t)blockIdx.x * nb + d] = h[d];
}

// Exclusive scan over the tiles of every digit's counts (tile order) and the digit totals, on the tile-major matrix, in two
// small kernels over PANELS of RSP_TILES tiles x 64 digits (one wavefront each, lane = digit, so every load is 256
// contiguous bytes of a tile's row): rs_panel_sums adds up each panel's columns; rs_panel_scan lets every panel add the
// sums of the panels before it itself (a few hundred at most) and writes its tiles' exclusive counts; the last panel
// also leaves the digit totals.  (One block per digit walking all tiles -- round 2 -- took 8 us for one chromosome's 650
// tiles and 144 us for a 0.5 Gb chain's 4 400.)  The scatter adds the number of keys with a smaller digit itself (a
// block scan of the 2^bits totals), so the pass needs neither a scan of the whole matrix nor global atomics.
constexpr u32 RSP_TILES = 64;
__global__ __launch_bounds__(256) void rs_panel_sums(const u32 *hist, u32 n_tiles, u32 nb, u32 *psum) {
    const u32 d = blockIdx.y * 256 + threadIdx.x;
    if (d >= nb) return;
    const u32 t0 = blockIdx.x * RSP_TILES, t1 = t0 + RSP_TILES < n_tiles ? t0 + RSP_TILES : n_tiles;
    u32 sum = 0;
    for (u32 t = t0; t < t1; t += 8) { // eight loads in flight per lane
        u32 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = t + k < t1 ? hist[(size_t)(t + k) * nb + d] : 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) sum += v[k];
    }
    psum[(size_t)blockIdx.x * nb + d] = sum;
}
__global__ __launch_bounds__(256) void rs_panel_scan(const u32 *hist, const u32 *psum, u32 n_tiles, u32 nb, u32 *hist_scan, u32 *row_total) {
    const u32 d = blockIdx.y * 256 + threadIdx.x;
    if (d >= nb) return;
    const u32 panel = blockIdx.x;
    u32 run = 0;
    for (u32 q = 0; q < panel; q += 8) {
        u32 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = q + k < panel ? psum[(size_t)(q + k) * nb + d] : 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) run += v[k];
    }
    const u32 t0 = panel * RSP_TILES, t1 = t0 + RSP_TILES < n_tiles ? t0 + RSP_TILES : n_tiles;
    for (u32 t = t0; t < t1; t += 8) {
        u32 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = t + k < t1 ? hist[(size_t)(t + k) * nb + d] : 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (t + k < t1) hist_scan[(size_t)(t + k) * nb + d] = run;
            run += v[k];
        }
    }
    if (t1 == n_tiles) row_total[d] = run; // (the last panel)
}

// LDS of one rs_scatter block: the tile's keys in digit order (reused for the pair indices), the offset
// "global position - tile-local position" of every digit, and the digit counters of the 4 waves
// (16 bit: a wave owns 1024 keys, a tile 4096).
__host__ __device__ constexpr size_t rs_scatter_lds_bytes(int bits, size_t key_bytes = 8) {
    return (size_t)RS_TILE * key_bytes + ((size_t)4 << bits) + ((size_t)8 << bits);
}
constexpr int RS_PF = 2; // digits per thread whose scan entries are prefetched (9-bit digits: all of them)

// Lanes of the wave holding the same digit as this lane ("match any"), one ballot per digit bit:
// peers &= bit set ? ballot : ~ballot, written as peers &= ~(ballot ^ m) with m = 0 / -1 from a signed
// bit-field extract.  BITS > 0 unrolls the loop; BITS == 0 takes the width at run time.
template <int BITS>
__device__ __forceinline__ u64 wave_match_digit(u32 d, bool valid, int bits) {
    u64 peers = __ballot(valid);
    u32 lo = (u32)peers, hi = (u32)(peers >> 32);
    auto step = [&](int bit) {
        const int m = __builtin_amdgcn_sbfe((int)d, bit, 1); // -1 if the bit is set
        const u64 bb = __ballot(m != 0);
        lo &= ~((u32)bb ^ (u32)m);
        hi &= ~((u32)(bb >> 32) ^ (u32)m);
    };
    if constexpr (BITS > 0) {
#pragma unroll
        for (int bit = 0; bit < BITS; bit++) step(bit);
    } else {
        for (int bit = 0; bit < bits; bit++) step(bit);
    }
    return ((u64)hi << 32) | lo;
}

// One radix pass over a 4096-key tile: rank (stable, in memory order), exchange through LDS so that
// the tile leaves in digit order, write out with consecutive lanes on consecutive addresses inside a
// digit run.  The first output slot of (digit, tile) = keys of the whole array with a smaller digit
// (block scan over row_total) + keys with that digit in earlier tiles (hist_scan, bin-major).
// A single-launch variant (digit totals up front, earlier tiles' counts by decoupled look-back over
// 8-byte {epoch, count} granules) was measured at 0.064 ms per pass against 0.058 ms for
// hist + rowscan + scatter: with every tile resident at once the look-back chain costs more than the
// two small kernels, so it was dropped.
// K: u64 (full intron keys) or u32 (dense junction ids: half the key traffic, half the key registers)
template <int BITS, typename K>
__global__ __launch_bounds__(256, 3) void rs_scatter(const K *kin, const u32 *vin, K *kout, u32 *vout, const u32 *np, int shift,
                                                      int bits, const u32 *hist_scan, const u32 *row_total, u32 n_tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_smem[];
    __shared__ u64 s_scan[4];
    const u32 n = *np;
    if ((u64)blockIdx.x * RS_TILE >= n) return; // the grid covers the host's limit
    if (BITS > 0) bits = BITS;
    const u32 nb = 1u << bits;
    const u32 mask = nb - 1;
    K *kbuf = (K *)rs_smem;
    u32 *ibuf = (u32 *)rs_smem;
    u32 *delta = (u32 *)(rs_smem + (size_t)RS_TILE * sizeof(K));
    unsigned short *wcnt = (unsigned short *)(delta + nb); // [4][nb]
    for (u32 d = threadIdx.x; d < 2 * nb; d += 256) ((u32 *)wcnt)[d] = 0;
    __syncthreads();
    const u32 tile = blockIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id(); // w in an SGPR: scalar base addresses
    unsigned short *wc = wcnt + (size_t)w * nb;
    const u32 base = tile * RS_TILE + w * (RS_TILE / 4);
    const u64 lt = (1ull << lane) - 1;
    K key[RS_ITEMS];
    u32 val[RS_ITEMS];
    u32 rkp[RS_ITEMS / 2]; // tile-local ranks (< 4096), two per register: the kernel must stay under 128 VGPRs
    // the key / index buffers are allocated with one tile of slack, so the last tile loads unguarded too
    // (lanes past n are masked below): 16 independent loads from one scalar base
    const K *kp = kin + base;
#pragma unroll
    for (int r = 0; r < RS_ITEMS; r++) key[r] = kp[r * 64 + lane];
    // digits [d0, d0 + per) belong to this thread in the digit phase (consecutive, so that one block
    // scan orders them); their row totals / scanned counts are fetched now, behind the ranking
    const u32 per = (nb + 255) / 256;
    const u32 d0 = threadIdx.x * per;
    u32 pf_rt[RS_PF], pf_hs[RS_PF];
#pragma unroll
    for (int k = 0; k < RS_PF; k++) {
        const u32 d = d0 + k;
        const bool on = (u32)k < per && d < nb;
        pf_rt[k] = on ? row_total[d] : 0u;
        pf_hs[k] = on ? hist_scan[(size_t)tile * nb + d] : 0u;
    }
#pragma unroll
    for (int r = 0; r < RS_ITEMS; r++) {
        const u32 i = base + r * 64 + lane;
        const bool valid = i < n;
        const u32 d = (u32)(key[r] >> shift) & mask;
        const u64 peers = wave_match_digit<BITS>(d, valid, bits);
        // only scalars of the peer mask stay live across the LDS round trip
        const u32 lower = (u32)__popcll(peers & lt), group = (u32)__popcll(peers);
        const int leader = valid ? __ffsll((long long)peers) - 1 : lane;
        u32 before = 0;
        if (valid && lane == leader) {
            before = wc[d];
            wc[d] = (unsigned short)(before + group);
        }
        const u32 rank = __shfl(before, leader, 64) + lower;
        rkp[r >> 1] = (r & 1) ? (rkp[r >> 1] | (rank << 16)) : rank;
    }
    // the pair indices are not needed before the second exchange: their latency hides behind the digit phase
    if (vin) {
        const u32 *vp = vin + base;
#pragma unroll
        for (int r = 0; r < RS_ITEMS; r++) val[r] = vp[r * 64 + lane];
    } else {
#pragma unroll
        for (int r = 0; r < RS_ITEMS; r++) val[r] = base + r * 64 + lane;
    }
    __syncthreads();
    u32 mine = 0, below = 0;
    for (u32 k = 0; k < per; k++) {
        const u32 d = d0 + k;
        if (d < nb) {
            mine += (u32)wcnt[d] + wcnt[nb + d] + wcnt[2 * nb + d] + wcnt[3 * nb + d];
            below += k < RS_PF ? pf_rt[k < RS_PF ? k : 0] : row_total[d];
        }
    }
    u64 tot; // one scan carries both: tile-local start of the digit | keys of the whole array with a smaller digit
    const u64 both = block_escan_256<u64>((u64)mine | ((u64)below << 32), s_scan, &tot);
    u32 tstart = (u32)both, dbase = (u32)(both >> 32);
    for (u32 k = 0; k < per; k++) {
        const u32 d = d0 + k;
        if (d >= nb) break;
        const u32 c0 = wcnt[d], c1 = wcnt[nb + d], c2 = wcnt[2 * nb + d], c3 = wcnt[3 * nb + d];
        // first output slot of this tile's keys with digit d
        const u32 gfirst = dbase + (k < RS_PF ? pf_hs[k < RS_PF ? k : 0] : hist_scan[(size_t)tile * nb + d]);
        dbase += k < RS_PF ? pf_rt[k < RS_PF ? k : 0] : row_total[d];
        delta[d] = gfirst - tstart;
        wcnt[d] = (unsigned short)tstart;
        wcnt[nb + d] = (unsigned short)(tstart + c0);
        wcnt[2 * nb + d] = (unsigned short)(tstart + c0 + c1);
        wcnt[3 * nb + d] = (unsigned short)(tstart + c0 + c1 + c2);
        tstart += c0 + c1 + c2 + c3;
    }
    __syncthreads();
    // exchange: keys to their tile-local sorted position
#pragma unroll
    for (int r = 0; r < RS_ITEMS; r++) {
        const u32 i = base + r * 64 + lane;
        const u32 lp = ((rkp[r >> 1] >> ((r & 1) * 16)) & 0xffffu) + wc[(u32)(key[r] >> shift) & mask];
        rkp[r >> 1] = (r & 1) ? ((rkp[r >> 1] & 0xffffu) | (lp << 16)) : ((rkp[r >> 1] & 0xffff0000u) | lp);
        if (i < n) kbuf[lp] = key[r];
    }
    __syncthreads();
    const u32 cnt = min((u32)RS_TILE, n - tile * RS_TILE);
    u32 digp[RS_ITEMS / 2]; // digit of the key in slot j, two per register (for the second write-out)
#pragma unroll
    for (int r = 0; r < RS_ITEMS; r++) {
        const u32 j = r * 256 + threadIdx.x;
        const K kk = j < cnt ? kbuf[j] : (K)0;
        const u32 d = (u32)(kk >> shift) & mask;
        digp[r >> 1] = (r & 1) ? (digp[r >> 1] | (d << 16)) : d;
        if (j < cnt) kout[delta[d] + j] = kk;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ITEMS; r++) {
        const u32 i = base + r * 64 + lane;
        if (i < n) ibuf[(rkp[r >> 1] >> ((r & 1) * 16)) & 0xffffu] = val[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ITEMS; r++) {
        const u32 j = r * 256 + threadIdx.x;
        if (j < cnt) vout[delta[(digp[r >> 1] >> ((r & 1) * 16)) & 0xffffu] + j] = ibuf[j];
    }
}

// ---------------------------------------------------------------------------------------------
// The run route of the dense-id sort: a stable counting sort in ONE pass over the pairs.  kd_assign left one entry per
// (tile, id) run; the run list -- about as many entries as the chain has junctions -- is sorted by id << tile_bits | tile with
// the radix kernels above, and a scan of the counts in that order gives every run the place of its first pair (RunDestSink
// writes it back at the run's own index).  rs_place then ranks the pairs of a tile within their runs -- wave w owns the w-th
// quarter of the tile, rounds are contiguous 64-pair slices, equal ids inside a round are ranked by lane: memory order, as in
// rs_scatter, so the result is the stable sort's, bit for bit -- and writes id and pair index straight to their places.  A
// slice holds one or two distinct ids: the lanes of an id write consecutive addresses without an exchange through LDS, and
// instead of one ballot per digit bit the wavefront takes its distinct ids one after the other.
// ---------------------------------------------------------------------------------------------
struct RunCountFn { // counts in sorted order
    const u32 *cnt, *order;
    __device__ u64 operator()(u64 i) const { return cnt[order[i]]; }
};
struct RunDestSink {
    u32 *dest;
    const u32 *order;
    __device__ void operator()(u64 i, u64, u64 ex) const { dest[order[i]] = (u32)ex; }
};
__global__ __launch_bounds__(256) void rs_place(const u32 *jid_bam, const u32 *np, const u64 *run_key, const u32 *run_dest, const u32 *tile_first,
                                                const u32 *tile_n, u32 run_cap, int tile_bits, u32 *kout, u32 *vout) {
    __shared__ u32 s_dest[RUN_W];               // first place of the tile's pairs of id d, at d & (RUN_W - 1)
    __shared__ unsigned short s_wcnt[4][RUN_W]; // pairs of that id per wave (16 bit: a wave owns 1 024 pairs)
    const u32 n = *np;
    const u32 tile = blockIdx.x;
    if ((u64)tile * RS_TILE >= n) return; // the grid covers the host's limit (and a closed chain has no pairs)
    for (u32 d = threadIdx.x; d < 2 * RUN_W; d += 256) ((u32 *)&s_wcnt[0][0])[d] = 0;
    const u32 tf = tile_first[tile], tn = tf < run_cap ? min(tile_n[tile], min(RUN_W, run_cap - tf)) : 0u;
    for (u32 e = threadIdx.x; e < tn; e += 256) s_dest[(u32)(run_key[tf + e] >> tile_bits) & (RUN_W - 1u)] = run_dest[tf + e];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    unsigned short *wc = s_wcnt[w];
    const u32 base = tile * RS_TILE + w * (RS_TILE / 4);
    const u64 lt = (1ull << lane) - 1;
    u32 id[RS_ITEMS];
    u32 rkp[RS_ITEMS / 2]; // ranks within the wave's quarter (< 1 024), two per register
    // (the id buffer has one tile of slack: the last tile loads unguarded, lanes past n are masked below)
    const u32 *kp = jid_bam + base;
#pragma unroll
    for (int r = 0; r < RS_ITEMS; r++) id[r] = kp[r * 64 + lane];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ITEMS; r++) {
        const bool valid = base + r * 64 + lane < n;
        const u32 d = id[r] & (RUN_W - 1u);
        u32 rank = 0;
        u64 todo = __ballot(valid);
        while (todo) {
            const int first = __ffsll((long long)todo) - 1;
            const u32 idc = (u32)__builtin_amdgcn_readlane((int)id[r], first);
            const bool mine = valid && id[r] == idc;
            const u64 m = __ballot(mine);
            u32 before = 0;
            if (lane == first) {
                before = wc[d];
                wc[d] = (unsigned short)(before + (u32)__popcll(m));
            }
            before = (u32)__builtin_amdgcn_readlane((int)before, first);
            if (mine) rank = before + (u32)__popcll(m & lt);
            todo &= ~m;
        }
        rkp[r >> 1] = (r & 1) ? (rkp[r >> 1] | (rank << 16)) : rank;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_ITEMS; r++) {
        const u32 i = base + r * 64 + lane;
        const u32 d = id[r] & (RUN_W - 1u);
        u32 dst = s_dest[d] + ((rkp[r >> 1] >> ((r & 1) * 16)) & 0xffffu);
        for (int q = 0; q < w; q++) dst += s_wcnt[q][d]; // the id's pairs in the waves before this one
        if (i < n && dst < n) { // (dst < n always: every id of the tile has its entry)
            kout[dst] = id[r];
            vout[dst] = i;
        }
    }
}

} // namespace pjb
