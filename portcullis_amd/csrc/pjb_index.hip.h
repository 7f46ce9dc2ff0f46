// pjb_index.hip.h -- the BAM index (.bai) of a coordinate-sorted BAM, built on the device from the inflated records
// (`portcullis_amd prep`, pjb_index_begin / _piece / _end; DESIGN.md section 5, "prep").  Included by pjb_ingest_api.hip only.
//
// The index is the one BamWriter::indexRecord builds record by record on the host (SAM spec 5.2 / 5.3: bins of reg2bin with
// their chunks, a linear index of 16 kb windows).  The file is sorted, and three consequences of that make every step here a
// scan instead of a sort or an atomic per bin:
//   - a chunk is a maximal run of consecutive records of one (target, bin): a flag per record, a prefix sum, a compaction;
//   - within a target the bins of one LEVEL never decrease in file order and bin numbers ascend with the level, so the order
//     (target, bin, file order) the file format wants is a stable partition of the chunks by (target, level): six prefix
//     sums and the targets' boundaries;
//   - the windows record k is the first to overlap are max(w0, M + 1) .. w1, M the largest last window of the earlier records
//     of the target: a running maximum, and every window is stored once.
//
//   bam_walk_all   : bam_walk over the records of every target (the walk of pjb_ingest.hip.h with its end test off)
//   bai_records    : a thread per record: span of the CIGAR, bin, windows, virtual offset, order against its predecessor
//   bai_head scan  : run_scan over the run heads (chunk number of every record)
//   bai_chunks     : run heads open a chunk, the record behind a run closes it
//   bai_win_*      : the running maximum in three kernels (tile maxima, their scan, apply), the last storing the windows
//   bai_level scan, bai_tid_starts, bai_partition : the stable partition of the finished chunk list (pjb_index_end)
//
// The CSI mode (pjb_index_begin_csi / pjb_index_end_csi) shares all of it: bai_records bins by hts_reg2bin(beg, end, 14, depth)
// for a depth of 0 .. 6 and keeps windows for targets of any length, the partition has depth + 1 levels, and three kernels
// turn the windows into the `loffset` every bin carries instead of a linear index:
//   csi_seed       : window 0 of every target with records takes its first record's virtual offset
//   csi_fill_apply : untouched windows take the entry before them (a running maximum: virtual offsets ascend through the file;
//                    the tile maxima are bai_win_reduce's and bai_win_tiles')
//   csi_loffset    : every chunk of the ordered list reads the filled entry at its bin's first 16 kb window
#pragma once
#include "pjb_ingest.hip.h"

namespace pjb {

template <bool FILL>
__global__ __launch_bounds__(256) void bam_walk_all(BamRegion R, iu32 n_seg, const iu64 *seg_start, BamWalkOut O) {
    bam_walk_body<FILL, true>(R, n_seg, seg_start, O);
}

constexpr iu64 BAI_NOKEY = ~0ull;       // run key of a record without a target
constexpr int32_t BAI_MAX_LEN = 1 << 29; // reg2bin's range: targets of this many bases cannot be indexed
constexpr int CSI_MIN_SHIFT = 14;        // the CSI's smallest bins are the BAI's: 16 kb
constexpr int CSI_MAX_DEPTH = 6;         // 2^(14 + 3 * 6) covers every int32 position
constexpr iu32 BAI_SLICE = 512;         // block-table entries a workgroup of bai_records keeps in LDS

struct BaiChunk { // = pjb_index_chunk
    iu64 vbeg, vend;
    int32_t tid;
    iu32 bin;
};

// ctl words (u64) of a piece
enum : int {
    BAI_CTL_UNSORTED = 0, // smallest ordinal (within the piece) of a record that goes back, ~0 if none
    BAI_CTL_BAD = 1,      // ... of a record whose refID / pos cannot be (refID >= n_ref, pos outside the target)
    BAI_CTL_LONG = 2,     // ... of a record on a target reg2bin cannot cover
    BAI_CTL_LASTSORT = 3, // (refID unsigned) << 32 | pos of the piece's last record
    BAI_CTL_LASTKEY = 4,  // its run key
    BAI_CTL_HEADS = 5,    // total of the head scan
    BAI_CTL_WINMAX = 6,   // running window maximum behind the piece
    BAI_CTL_WORDS = 8,
};

__device__ __forceinline__ iu32 bai_reg2bin(iu32 beg, iu32 end) { // SAM spec 5.3; end exclusive, > beg
    end--;
    if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
    return 0u;
}
// hts_reg2bin(beg, end, 14, depth); end exclusive, > beg, at most 2^(14 + 3 * depth).  Level l's first bin is (8^l - 1) / 7
// whatever the depth, so depth 5 numbers the bins as bai_reg2bin does.
__device__ __forceinline__ iu32 csi_level_first(int l) { return ((1u << (3 * l)) - 1u) / 7u; }
__device__ __forceinline__ iu32 csi_reg2bin(iu32 beg, iu32 end, int depth) {
    end--;
    int s = CSI_MIN_SHIFT;
    for (int l = depth; l > 0; l--, s += 3)
        if (beg >> s == end >> s) return csi_level_first(l) + (beg >> s);
    return 0u;
}
__device__ __forceinline__ iu32 bai_level(iu32 bin) {
    return bin >= 37449u ? 6u : bin >= 4681u ? 5u : bin >= 585u ? 4u : bin >= 73u ? 3u : bin >= 9u ? 2u : bin >= 1u ? 1u : 0u;
}
// the first 16 kb window of a bin's interval
__device__ __forceinline__ iu32 csi_first_window(iu32 bin, int depth) {
    const int l = (int)bai_level(bin);
    return l > depth ? 0u : (bin - csi_level_first(l)) << (3 * (depth - l));
}

// The block an inflated offset belongs to, in a table of block starts [lo, hi) that ends with the sentinel "end of the data, next
// block of the file": the first entry that starts AT u (a record that starts where a block ends belongs to the block behind it,
// as bgzf_tell says it after reading up to there -- also when that block is empty, the EOF block), else the last that starts before u.
template <typename P>
__device__ __forceinline__ iu32 bai_block_of(P out_off, iu32 lo, iu32 hi, iu64 u) {
    const iu32 first = lo, end = hi;
    while (lo < hi) {
        const iu32 mid = lo + (hi - lo) / 2;
        if (out_off[mid] < u) lo = mid + 1;
        else hi = mid;
    }
    if ((lo == end || out_off[lo] > u) && lo > first) lo--;
    return lo;
}

struct BaiTable { // the piece's blocks + the sentinel
    const iu64 *out_off; // inflated offset of each block's first byte
    const iu64 *cstart;  // its offset in the file
    iu32 n;              // entries, sentinel included
};
struct BaiRecOut {
    iu64 *key;  // (tid << 32 | bin), BAI_NOKEY
    iu64 *vs;   // virtual offset
    iu64 *win;  // (tid + 1) << 32 | (last window + 1); 0 without a target: the running maximum's terms
    iu32 *w0;   // first window
    iu64 *ctl;
};

__device__ __forceinline__ iu64 bai_sort_key(const uint8_t *U, iu64 off) { return (iu64)ld32u(U + off + 4) << 32 | ld32u(U + off + 8); }

// csi_depth < 0: the BAI (reg2bin, targets of 2^29 bases or more refused); 0 .. 6: the CSI of that depth
__global__ __launch_bounds__(256) void bai_records(const uint8_t *U, const iu64 *rec_off, iu64 n, BaiTable T, const int32_t *ref_len, int32_t n_ref,
                                                   iu64 prev_sort, int csi_depth, BaiRecOut O) {
    __shared__ iu64 s_off[BAI_SLICE];
    __shared__ iu32 s_b0, s_nb;
    const iu64 i0 = (iu64)blockIdx.x * 256;
    if (i0 >= n) return;
    // the blocks this workgroup's records start in: a short slice of the table (records follow each other in the file)
    if (threadIdx.x == 0) {
        const iu64 i1 = i0 + 255 < n ? i0 + 255 : n - 1;
        const iu32 b0 = bai_block_of(T.out_off, 0u, T.n, rec_off[i0]), b1 = bai_block_of(T.out_off, 0u, T.n, rec_off[i1]);
        s_b0 = b0;
        s_nb = b1 - b0 + 1;
    }
    __syncthreads();
    const iu32 b0 = s_b0, nb = s_nb;
    const bool in_lds = nb <= BAI_SLICE;
    if (in_lds)
        for (iu32 k = threadIdx.x; k < nb; k += 256) s_off[k] = T.out_off[b0 + k];
    __syncthreads();
    const iu64 i = i0 + threadIdx.x;
    if (i >= n) return;
    const iu64 off = rec_off[i];
    const uint8_t *r = U + off + 4;
    const int32_t tid = (int32_t)ld32u(r), pos = (int32_t)ld32u(r + 4);
    const iu32 l_name = r[8], n_cig = ld16u(r + 12);
    const iu32 b = in_lds ? b0 + bai_block_of((const iu64 *)s_off, 0u, nb, off) : bai_block_of(T.out_off, b0, b0 + nb, off);
    const iu64 vs = T.cstart[b] << 16 | (off - T.out_off[b]);
    O.vs[i] = vs;
    // order: (refID as unsigned, pos) must not go back
    const iu64 sk = (iu64)(iu32)tid << 32 | (iu32)pos;
    const iu64 before = i ? bai_sort_key(U, rec_off[i - 1]) : prev_sort;
    if (sk < before) atomicMin(&O.ctl[BAI_CTL_UNSORTED], i);
    iu64 key = BAI_NOKEY, win = 0;
    iu32 w0 = 0;
    if (tid >= n_ref || tid < -1) atomicMin(&O.ctl[BAI_CTL_BAD], i);
    else if (tid >= 0) {
        const int32_t len = ref_len[tid];
        if (csi_depth < 0 && len >= BAI_MAX_LEN) atomicMin(&O.ctl[BAI_CTL_LONG], i);
        else if (pos < 0 || pos >= len) atomicMin(&O.ctl[BAI_CTL_BAD], i);
        else {
            const uint8_t *cg = r + 32 + l_name;
            iu64 span = 0;
            for (iu32 k = 0; k < n_cig; k++) { // M D N = X consume reference
                const iu32 op = ld32u(cg + 4 * (size_t)k);
                if ((0x18Du >> (op & 15u)) & 1u) span += op >> 4;
            }
            iu64 end = (iu64)pos + (span ? span : 1);
            if (end > (iu64)len) end = (iu64)len; // (what hangs over the target's end is not indexed; pos < len)
            const iu32 bin = csi_depth < 0 ? bai_reg2bin((iu32)pos, (iu32)end) : csi_reg2bin((iu32)pos, (iu32)end, csi_depth);
            key = (iu64)(iu32)tid << 32 | bin;
            w0 = (iu32)pos >> 14;
            win = (iu64)((iu32)tid + 1u) << 32 | ((((iu32)end - 1u) >> 14) + 1u);
        }
    }
    O.key[i] = key;
    O.win[i] = win;
    O.w0[i] = w0;
    if (i == n - 1) {
        O.ctl[BAI_CTL_LASTSORT] = sk;
        O.ctl[BAI_CTL_LASTKEY] = key;
    }
}

// run heads: a record with a target whose (target, bin) is not its predecessor's
struct BaiHeadFn {
    const iu64 *key;
    iu64 prev_key;
    __device__ iu64 operator()(iu64 i) const {
        const iu64 k = key[i];
        return k != BAI_NOKEY && k != (i ? key[i - 1] : prev_key);
    }
};

// heads[i]: run heads before record i.  A head opens chunk base + heads[i]; a record whose key differs from its predecessor's
// closes the predecessor's chunk, base + heads[i] - 1 -- the last chunk of the piece before when the run came from there.
// The last run's end stays open: the next piece's first boundary, or pjb_index_end, writes it.
__global__ __launch_bounds__(256) void bai_chunks(const iu64 *key, const iu64 *vs, const iu32 *heads, iu64 n, iu64 prev_key, BaiChunk *chunks, iu64 base, iu64 cap) {
    const iu64 i = (iu64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const iu64 k = key[i], before = i ? key[i - 1] : prev_key;
    if (k == before) return;
    const iu64 at = base + heads[i];
    const iu64 v = vs[i];
    if (before != BAI_NOKEY && at >= 1 && at - 1 < cap) chunks[at - 1].vend = v;
    if (k != BAI_NOKEY && at < cap) {
        chunks[at].vbeg = v;
        chunks[at].tid = (int32_t)(k >> 32);
        chunks[at].bin = (iu32)k;
    }
}

// ---- the running maximum (exclusive) of O.win, in tiles of 2048 as the sum scan of pjb_device.hip.h
__device__ __forceinline__ iu64 wave_imax(iu64 v) {
    const int l = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const iu64 t = __shfl_up(v, o, 64);
        if (l >= o && t > v) v = t;
    }
    return v;
}
__global__ __launch_bounds__(256) void bai_win_reduce(const iu64 *win, iu64 n, iu64 *tile_max) {
    __shared__ iu64 sm[4];
    const iu64 base = (iu64)blockIdx.x * SCAN_TILE;
    iu64 m = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const iu64 i = base + (iu64)k * 256 + threadIdx.x;
        if (i < n) {
            const iu64 v = win[i];
            m = v > m ? v : m;
        }
    }
    m = wave_imax(m);
    if (lane_id() == 63) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        iu64 t = sm[0];
        for (int k = 1; k < 4; k++) t = sm[k] > t ? sm[k] : t;
        tile_max[blockIdx.x] = t;
    }
}
// single block: tile_max[t] <- maximum of `carry` and the tiles before t; *total <- the maximum of all
__global__ __launch_bounds__(1024) void bai_win_tiles(iu64 *tile_max, iu32 n_tiles, iu64 carry, iu64 *total) {
    __shared__ iu64 wmax[16];
    __shared__ iu64 carry_s;
    if (threadIdx.x == 0) carry_s = carry;
    __syncthreads();
    for (iu32 base = 0; base < n_tiles; base += 1024) {
        const iu32 i = base + threadIdx.x;
        const iu64 v = i < n_tiles ? tile_max[i] : 0;
        const iu64 inc = wave_imax(v);
        iu64 ex = __shfl_up(inc, 1, 64);
        if (lane_id() == 0) ex = 0;
        const int w = threadIdx.x >> 6;
        if (lane_id() == 63) wmax[w] = inc;
        __syncthreads();
        iu64 before = carry_s, all = carry_s;
        for (int k = 0; k < 16; k++) {
            const iu64 s = wmax[k];
            if (k < w && s > before) before = s;
            if (s > all) all = s;
        }
        if (i < n_tiles) tile_max[i] = ex > before ? ex : before;
        __syncthreads();
        if (threadIdx.x == 0) carry_s = all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}
// every record stores the windows it is the first to overlap
__global__ __launch_bounds__(256) void bai_win_apply(const iu64 *win, const iu32 *w0, const iu64 *vs, iu64 n, const iu64 *tile_max, const iu64 *lin_off,
                                                     iu64 *lin, iu64 lin_total) {
    __shared__ iu64 sm[4];
    const iu64 base = (iu64)blockIdx.x * SCAN_TILE;
    if (base >= n) return;
    iu64 run = tile_max[blockIdx.x];
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const iu64 i = base + (iu64)k * 256 + threadIdx.x;
        const iu64 v = i < n ? win[i] : 0;
        const iu64 inc = wave_imax(v);
        iu64 ex = __shfl_up(inc, 1, 64);
        if (lane_id() == 0) ex = 0;
        __syncthreads();
        if (lane_id() == 63) sm[w] = inc;
        __syncthreads();
        iu64 all = run;
        if (run > ex) ex = run;
        for (int j = 0; j < 4; j++) {
            const iu64 s = sm[j];
            if (j < w && s > ex) ex = s;
            if (s > all) all = s;
        }
        run = all;
        if (i < n && v) {
            const iu32 t1 = (iu32)(v >> 32), last = (iu32)v - 1u; // target + 1, last window
            iu32 from = w0[i];
            if ((iu32)(ex >> 32) == t1 && (iu32)ex > from) from = (iu32)ex; // (largest last window before) + 1
            const iu64 at = lin_off[t1 - 1];
            const iu64 voff = vs[i];
            for (iu32 x = from; x <= last; x++)
                if (at + x < lin_total) lin[at + x] = voff;
        }
    }
}

// ---- the finished chunk list (file order) -> (target, bin, file order)
struct BaiLevelFn { // chunks of level 2p in the low half, of level 2p + 1 in the high half (p = 3: level 6 alone, the deepest CSI's)
    const BaiChunk *chunks;
    iu64 n;
    iu32 p;
    __device__ iu64 operator()(iu64 j) const {
        if (j >= n) return 0; // (the scan runs over n + 1 terms: the sink's last entry is the total)
        const iu32 l = bai_level(chunks[j].bin);
        return (l >> 1) == p ? ((l & 1u) ? 1ull << 32 : 1ull) : 0ull;
    }
};
struct BaiLevelSink {
    iu64 *q;
    __device__ void operator()(iu64 j, iu64, iu64 ex) const { q[j] = ex; }
};
// tid_start[t] = first chunk of a target >= t (targets ascend in the list); n_ref + 1 entries, the last is n
__global__ __launch_bounds__(256) void bai_tid_starts(const BaiChunk *chunks, iu64 n, int32_t n_ref, iu32 *tid_start) {
    const iu64 j = (iu64)blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    const int32_t before = j ? chunks[j - 1].tid : -1, cur = j < n ? chunks[j].tid : n_ref;
    for (int32_t t = before + 1; t <= cur && t <= n_ref; t++) tid_start[t] = (iu32)j;
}
// q3 (level 6) is read only where a chunk of level 6 exists: a CSI of depth 6
__global__ __launch_bounds__(256) void bai_partition(const BaiChunk *chunks, iu64 n, int32_t n_ref, const iu32 *tid_start, const iu64 *q0, const iu64 *q1,
                                                     const iu64 *q2, const iu64 *q3, BaiChunk *out) {
    const iu64 j = (iu64)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const BaiChunk ch = chunks[j];
    if (ch.tid < 0 || ch.tid >= n_ref) return;
    const iu32 s = tid_start[ch.tid], e = tid_start[ch.tid + 1];
    const iu32 lvl = bai_level(ch.bin);
    const iu64 *q[4] = {q0, q1, q2, q3};
    iu64 dest = s;
    for (iu32 l = 0; l <= lvl; l++) {
        const iu64 *a = q[l >> 1];
        const iu32 sh = (l & 1u) * 32u;
        const iu32 ps = (iu32)(a[s] >> sh);
        dest += l < lvl ? (iu32)(a[e] >> sh) - ps : (iu32)(a[j] >> sh) - ps;
    }
    if (dest < n) out[dest] = ch;
}

// ---- the CSI's loffset: the windows filled from the left, read at every bin's first window
// window 0 of a target with records <- its first record's virtual offset (the first chunk of the target in the file-order list):
// what its leading untouched windows take.  Where the first record lies in window 0 the value is the one already there.
__global__ __launch_bounds__(256) void csi_seed(const BaiChunk *chunks, const iu32 *tid_start, int32_t n_ref, const iu64 *lin_off, iu64 *lin, iu64 lin_total) {
    const int32_t t = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    if (t >= n_ref) return;
    const iu32 s = tid_start[t], e = tid_start[t + 1];
    const iu64 at = lin_off[t];
    if (s < e && at < lin_off[t + 1] && at < lin_total) lin[at] = chunks[s].vbeg;
}
// lin[i] <- the maximum of lin[0 .. i]: virtual offsets ascend through a sorted file, target by target and window by window, so the
// maximum is the last touched entry at or before i, and csi_seed keeps it inside the target.  tile_max as for bai_win_apply.
__global__ __launch_bounds__(256) void csi_fill_apply(iu64 *lin, iu64 n, const iu64 *tile_max) {
    __shared__ iu64 sm[4];
    const iu64 base = (iu64)blockIdx.x * SCAN_TILE;
    if (base >= n) return;
    iu64 run = tile_max[blockIdx.x];
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const iu64 i = base + (iu64)k * 256 + threadIdx.x;
        const iu64 v = i < n ? lin[i] : 0;
        iu64 inc = wave_imax(v);
        __syncthreads();
        if (lane_id() == 63) sm[w] = inc;
        __syncthreads();
        iu64 all = run;
        if (run > inc) inc = run;
        for (int j = 0; j < 4; j++) {
            const iu64 s = sm[j];
            if (j < w && s > inc) inc = s;
            if (s > all) all = s;
        }
        run = all;
        if (i < n) lin[i] = inc;
    }
}
__global__ __launch_bounds__(256) void csi_loffset(const BaiChunk *sorted, iu64 n, int32_t n_ref, int depth, const iu64 *lin_off, const iu64 *lin, iu64 lin_total,
                                                   iu64 *loff) {
    const iu64 j = (iu64)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const BaiChunk ch = sorted[j];
    iu64 v = 0;
    if (ch.tid >= 0 && ch.tid < n_ref) {
        const iu64 at = lin_off[ch.tid] + csi_first_window(ch.bin, depth);
        if (at < lin_off[ch.tid + 1] && at < lin_total) v = lin[at];
    }
    loff[j] = v;
}

} // namespace pjb
