// pjb_kernels.hip.h -- hand-written HIP kernels (gfx950 / CDNA4, wave64) for the
// Portcullis `junc` hot path.  Integer / byte work bounded by HBM bandwidth; no MFMA.
//
//   K2d, K2, K2s and K4 have a header each, included below where their text stood, so that the unit's kernels keep their order.  A stage
// header includes pjb_device.hip.h -- where what two stages use stands: constants, wave primitives, the layouts of buffers that pass from
// stage to stage --, the helpers pjb_basecmp.hip.h / pjb_readops.hip.h where it compares bases or walks reads, and no other stage header;
// each compiles on its own (tests/test_kernel_headers_standalone.py).  K0, K1 and K5 / K6 stand in this file.
//
// The chain of one target or group of targets (DESIGN.md section 4 has the table, the data layout and the byte counts):
//   K1   k1_count, k1_scan_tiles   per-read CIGAR walk: N-op count, length stats, sortedness, the block-span bound B;
//                                  the tiles' spliced lists                                                               (a1,a2)
//        k1_emit                   the spliced reads of the closed-form shapes: pairs (key, 32-byte record) complete       (a3,a5,a8,a12)
//        k1_generic                every other spliced read: its operations walked, pairs, closed form where possible      (a3,a5,a8,a12)
//   K2d  kd_*                      ordered dense junction ids from candidate keys; junction keys and anchors               (a3,a5)
//   K4b  k4b_generic               window check of the closed forms / the padded query-genome walks (side stream)          (a12,a13)
//   K2   rs_*                      stable LSD radix sort of (junction id, pair index)                                       (a3 grouping)
//   K4   k4_pairs                  sorted pairs -> fragment heads; head / run masks                                         (a8,a13)
//   K2s  k2_runs, k2_expand        position runs per junction (or k2_heads + kf_* on full keys)                             (a3,a7)
//   K5   k5_*                      fragment -> junction reduce, entropy, splice motif, hamming -> rows                      (a6,a7,a9-a11,a13)
//   K6   k6_rows_out               rows to the table; control block to the host
// References in comments are file:line in the reference checkout.
#pragma once

#include "pjb_device.hip.h"
#include "pjb_basecmp.hip.h"
#include "pjb_readops.hip.h"

namespace pjb {

// ---------------------------------------------------------------------------------------------
// K0: upper-case contig bases in place (boost::to_upper on fetched strings, junction.cc:586-587,635-638)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k0_upper(uint8_t *g, int64_t n, int do_upper, int *has_x) {
    int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    bool x = false;
    for (int64_t j = i; j < n && j < i + 16; j++) {
        uint8_t c = g[j];
        x |= (c == 'X' || (do_upper && c == 'x'));
    }
    if (__ballot(x) && lane_id() == 0) atomicOr(has_x, 1);
    if (!do_upper) return;
    if (i + 16 <= n && ((uintptr_t)(g + i) & 15) == 0) {
        uint4 v = *reinterpret_cast<uint4 *>(g + i);
        u32 *w = reinterpret_cast<u32 *>(&v);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            u32 x = w[k], r = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                u32 c = (x >> (8 * b)) & 0xff;
                if (c >= 'a' && c <= 'z') c -= 32;
                r |= c << (8 * b);
            }
            w[k] = r;
        }
        *reinterpret_cast<uint4 *>(g + i) = v;
    } else {
        for (int64_t j = i; j < n && j < i + 16; j++) {
            uint8_t c = g[j];
            if (c >= 'a' && c <= 'z') g[j] = c - 32;
        }
    }
}

// K0f: the sequence lines of one FASTA record, as they are in the file, -> its bases.  With the .fai's geometry (line_blen
// bases per line, line_len bytes per line) base i sits at byte (i / line_blen) * line_len + i % line_blen; every base must be
// a graphic character and every line terminator byte not one -- the test faidx's loader implies (deps/htslib-1.3/faidx.c
// reads with isgraph).  Anything else raises `bad` and the host falls back to filtering the characters itself.
__global__ __launch_bounds__(256) void k0_fasta(const uint8_t *raw, int64_t raw_bytes, int64_t n, int32_t line_blen, int32_t line_len,
                                                 uint8_t *out, int *bad) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i0 >= n) return;
    int64_t line = i0 / line_blen;
    int32_t col = (int32_t)(i0 - line * line_blen);
    int64_t src = line * line_len + col;
    bool wrong = false;
    const int64_t i1 = i0 + 16 < n ? i0 + 16 : n;
    for (int64_t i = i0; i < i1; i++) {
        uint8_t ch = 0;
        if (src < raw_bytes) ch = raw[src];
        else wrong = true;
        wrong |= ch <= 32 || ch >= 127;
        out[i] = ch;
        src++;
        if (++col == line_blen) { // end of a full line: its terminator bytes follow (if another base does)
            if (i + 1 < n)
                for (int32_t k = 0; k < line_len - line_blen; k++) {
                    const uint8_t t = src + k < raw_bytes ? raw[src + k] : (uint8_t)'?';
                    wrong |= t > 32 && t < 127;
                }
            src += line_len - line_blen;
            col = 0;
        }
    }
    if (__ballot(wrong) && lane_id() == 0) atomicOr(bad, 1);
}

// K0b: contig bases -> 4-bit nt16 codes, two per byte, LOW nibble first (base i at bits 4*(i&7) of
// word i>>3).  A byte outside the 16-letter alphabet "=ACMGRSVTWYHKDBN" has no code: the contig is
// flagged "exotic" and k4 then uses its byte-wise path, so equality semantics stay exact.
__device__ __forceinline__ u32 nt16_code(u32 c, bool &exotic) {
    switch (c) {
    case '=': return 0;
    case 'A': return 1;
    case 'C': return 2;
    case 'M': return 3;
    case 'G': return 4;
    case 'R': return 5;
    case 'S': return 6;
    case 'V': return 7;
    case 'T': return 8;
    case 'W': return 9;
    case 'Y': return 10;
    case 'H': return 11;
    case 'K': return 12;
    case 'D': return 13;
    case 'B': return 14;
    case 'N': return 15;
    default: exotic = true; return 0;
    }
}
__global__ __launch_bounds__(256) void k0_encode(const uint8_t *g, int64_t n, u32 *codes, int64_t n_words, int *exotic_flag) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool exotic = false;
    if (w < n_words) {
        u32 out = 0;
        const int64_t b0 = w * 8;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int64_t i = b0 + k;
            if (i < n) out |= nt16_code(g[i], exotic) << (4 * k);
        }
        codes[w] = out;
    }
    if (__ballot(exotic) && lane_id() == 0) atomicOr(exotic_flag, 1);
}

// K0c: the same bases in TWO bits (A 0, C 1, G 2, T 3; base i at bits 2 (i & 15) of word i >> 4; anything else is stored as 0) and
// the exceptions: bit i >> 6 of the bitmap is set when one of the bases 64 (i >> 6) .. 64 (i >> 6) + 63 is not A, C, G or T.  k1_emit
// compares a block of read bases in 2 bits only where the bitmap is clear under it (a read of pure ACGT against a stretch of pure
// ACGT: characters are equal exactly where the 2-bit codes are) and takes the 4-bit codes for every other block.  A thread owns one
// 64-base stretch: four words of codes (one 16-byte store), one bit; a wavefront's bits are one u64 of the bitmap.
//   Layout of the allocation: codes2[0 .. n2w) | K0_CODES2_PAD zero words | bitmap u32[(n + 2047) / 2048] | K0_GEXC_PAD zero words.
constexpr int K0_CODES2_PAD = 8, K0_GEXC_PAD = 4;
__host__ __device__ inline int64_t codes2_words(int64_t n) { return ((n + 63) / 64) * 4; }          // (whole stretches)
__host__ __device__ inline int64_t gexc_words(int64_t n) { return (((n + 63) / 64 + 63) / 64) * 2; } // (whole u64s)
__host__ __device__ inline int64_t codes2_alloc_words(int64_t n) { return codes2_words(n) + K0_CODES2_PAD + gexc_words(n) + K0_GEXC_PAD; }
__global__ __launch_bounds__(256) void k0_encode2(const uint8_t *g, int64_t n, u32 *codes2, u32 *gexc, int *any_exc) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; // stretch
    const int64_t n_str = (n + 63) / 64;
    bool exc = false;
    if (s < n_str) {
        u32 w[4] = {0, 0, 0, 0};
        const int64_t b0 = s * 64;
        if (b0 + 64 <= n && ((uintptr_t)(g + b0) & 15) == 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 v = *reinterpret_cast<const uint4 *>(g + b0 + 16 * q);
                const u32 x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const u32 c = (x[k >> 2] >> (8 * (k & 3))) & 0xffu;
                    const u32 code = c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 0u;
                    exc |= !(c == 'A' || c == 'C' || c == 'G' || c == 'T');
                    w[q] |= code << (2 * k);
                }
            }
        } else {
            for (int k = 0; k < 64; k++) {
                const int64_t i = b0 + k;
                if (i < n) {
                    const u32 c = g[i];
                    const u32 code = c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 0u;
                    exc |= !(c == 'A' || c == 'C' || c == 'G' || c == 'T');
                    w[k >> 4] |= code << (2 * (k & 15));
                }
            }
        }
        *reinterpret_cast<uint4 *>(codes2 + 4 * s) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    const u64 m = __ballot(exc);
    if (lane_id() == 0 && s < ((n_str + 63) / 64) * 64) reinterpret_cast<u64 *>(gexc)[s >> 6] = m;
    if (m && lane_id() == 0) atomicOr(any_exc, 1); // (a target without a single exception -- a telomere-to-telomere assembly, a bacterium -- is never asked)
}

// ---------------------------------------------------------------------------------------------
// K1a: per-read CIGAR walk, pass 1 (BamAlignment::init bam_alignment.cc:71-100, findJuncs length
// stats src/junction_builder.cc:333-343).  One thread per read; a tile is 1024 consecutive reads.
// ---------------------------------------------------------------------------------------------

// chk_ref_len > 0 (members of a group): a tile with an alignment that ends past the target reports max_end = INT32_MAX, so
// that k1_scan_tiles sees "weird coordinates" whatever the group's virtual length is (the host then finishes the
// members one by one).
// spl_rec: per spliced read of the tile's list, what this pass holds in registers anyway and k1_emit would have to gather again --
// {first operation's index, position, first word of the bases, operations (15 bits) | bases present (bit 15) | l_qseq (16 bits)};
// an operation count or l_qseq that does not fit is stored as all-ones and fetched by k1_emit.
__device__ __forceinline__ u32 spl_nlq(u32 n, bool seq_ok, int32_t lq) {
    return (n < 0x7fffu ? n : 0x7fffu) | (seq_ok ? 0x8000u : 0u) | ((u32)lq < 0xffffu ? (u32)lq << 16 : 0xffff0000u);
}
// A spliced read's span without its introns (TileStats::max_span): aligned length - sum of its N lengths.  An aligned length that left 31
// bits (nothing the walks' 32-bit coordinates can hold) or a sum that saturated gives all-ones: the chain's bound then excludes nothing.
__device__ __forceinline__ u32 read_span(int32_t aligned, u32 nsum) {
    return aligned < 0 || nsum > (u32)aligned ? 0xffffffffu : (u32)aligned - nsum;
}
#ifndef K1C_T
#define K1C_T 256 // threads of a k1_count block (a tile is K1_TILE reads: 4 per thread).  512 threads x 2 reads need 64 registers instead of
                  // 84 but took 88 against 63 us a launch beside the other chains' kernels: a block of 8 wavefronts waits for 8 free slots on ONE CU
#endif
#ifndef K1C_WAVES
#define K1C_WAVES 7 // waves per SIMD the register allocation aims at: 5 / 6 / 7 / 8 = 423 / 412 / 408 / 490 us a chain (8: 27 registers spilled)
#endif
// ONE launch per chain: block = one tile of the chain's tile space; its batch is the last one whose tile_base it has reached
// (the descriptors live in device memory, the index is uniform: scalar loads).  chk_members (groups): see chk_ref_len below.
__device__ __forceinline__ int batch_of_tile(const DevBatch *batches, int n_batches, u32 tile) {
    // lane k looks at batch base + k: one load and one ballot per 64 batches
    int found = 0;
    for (int base = 0; base < n_batches; base += 64) {
        const int k = base + lane_id();
        const u32 tb = k < n_batches ? gload(&batches[k].tile_base) : 0xffffffffu;
        const u64 m = __ballot(tb <= tile);
        if (m == 0) break;
        found = base + 63 - __clzll((long long)m);
    }
    return __builtin_amdgcn_readfirstlane(found);
}
// inclusive scan across the wave on the DPP path (row shifts, then the row totals carried up: no LDS traffic, ~14 instructions)
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ u32 dpp_shift0(u32 v) { // the source lane's value, 0 where there is none
    return (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, BANK_MASK, false);
}
__device__ __forceinline__ u32 wave_iscan_dpp(u32 v) {
    u32 o = v + dpp_shift0<0x111, 0xf, 0xf>(v) + dpp_shift0<0x112, 0xf, 0xf>(v) + dpp_shift0<0x113, 0xf, 0xf>(v); // row_shr:1..3
    o += dpp_shift0<0x114, 0xf, 0xe>(o); // row_shr:4
    o += dpp_shift0<0x118, 0xf, 0xc>(o); // row_shr:8
    o += dpp_shift0<0x142, 0xa, 0xf>(o); // row_bcast:15
    o += dpp_shift0<0x143, 0xc, 0xf>(o); // row_bcast:31
    return o;
}
#ifndef K1C_OPSW
#define K1C_OPSW 3072 // operations of a tile that the fast path of k1_count keeps in LDS (a tile of 1024 reads has ~1 700)
#endif
// The FAST path of a tile (all 1024 reads there, its operations fit in LDS): a thread owns four CONSECUTIVE reads, so every
// fixed-width field is one 16-byte load (the kernel was bound by VALU issue -- 83 % busy, round 5's SQ counters: 16 address
// computations and word loads for the operations, four 64-bit shuffle scans), the tile's operations come with coalesced loads
// straight to LDS and are read from there, and ONE scan per wavefront orders the spliced reads.
template <bool EXTRA>
__device__ __forceinline__ void k1_count_rows(const GBatch &b, const u32 tile_local, const u32 cA, const u32 n_ops, u32 *tile_cnt, TileStats *tile_stats, u32 *spl_idx,
                                              u32 *spl_poff, uint4 *spl_rec, u64 *err, const int32_t chk_ref_len, const XOut &X) {
    constexpr int NW = K1C_T / 64;
    static_assert(K1C_T * 4 == K1_TILE, "four reads a thread");
    __shared__ __attribute__((aligned(16))) u32 s_ops[K1C_OPSW + 8];
    __shared__ u32 s_scan[2][NW];
    __shared__ u64 r64[NW][2];
    __shared__ int32_t r32[NW][6];
    const int t = threadIdx.x, w = t >> 6;
    const int64_t r0 = (int64_t)tile_local * K1_TILE + 4 * t; // the thread's first read
    // ---- the tile's operations -> LDS (16 bytes a lane straight to LDS; the span starts at the 16-byte boundary below its first word)
    const uintptr_t a0 = (uintptr_t)(b.cigar + cA);
    const u32 shift = (u32)(a0 >> 2) & 3u;
    {
        const PJB_GLOBAL uint4 *p = (const PJB_GLOBAL uint4 *)(a0 - 4u * shift);
        const u32 total = n_ops + shift; // words from the aligned start; they all exist but for the last 16 bytes' tail: the array ends at cig_off[n]
        const u32 exist = b.cig_off[b.n] - cA + shift;
#pragma unroll
        for (int it = 0; it < (K1C_OPSW + 3 + K1C_T * 4 - 1) / (K1C_T * 4); it++) {
            if ((u32)it * (K1C_T * 4) < total) {
                const u32 i = (u32)it * (K1C_T * 4) + (u32)t * 4u;
                if (i + 4u <= exist) {
                    if (i < total) __builtin_amdgcn_global_load_lds(p + (i >> 2), (PJB_LDS void *)(s_ops + it * (K1C_T * 4) + w * 256), 16, 0, 0);
                } else if (i < exist) {
                    const PJB_GLOBAL u32 *q = (const PJB_GLOBAL u32 *)p + i;
                    s_ops[i] = q[0];
                    if (i + 1u < exist) s_ops[i + 1] = q[1];
                    if (i + 2u < exist) s_ops[i + 2] = q[2];
                }
            }
        }
    }
    // ---- the four reads' fields: one 16-byte load each
    const Words4 co = gload_as<Words4>(b.cig_off + r0);
    const u32 co4 = b.cig_off[r0 + 4];
    const Words4 po = gload_as<Words4>(b.pos + r0);
    const int32_t pprev = r0 > 0 ? b.pos[r0 - 1] : (b.prev_pos_ptr ? *b.prev_pos_ptr : b.prev_pos);
    const Words4 lqv = gload_as<Words4>(b.l_qseq + r0);
    const Words4 sov = gload_as<Words4>(b.seq_off + r0);
    const u32 so4 = b.seq_off[r0 + 4];
    const u32 xs4 = gload_as<u32>(b.xs + r0);
    u64 fl4 = 0;
    if (EXTRA) fl4 = gload_as<u64>(b.flag + r0);
    const u32 c[5] = {co.x, co.y, co.z, co.w, co4}, so[5] = {sov.x, sov.y, sov.z, sov.w, so4};
    const int32_t pos[4] = {(int32_t)po.x, (int32_t)po.y, (int32_t)po.z, (int32_t)po.w}, lq[4] = {(int32_t)lqv.x, (int32_t)lqv.y, (int32_t)lqv.z, (int32_t)lqv.w};
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (the LDS-DMA: hipcc does not wait for it before a ds_read of its own accord)
    __syncthreads();
    u32 cnt = 0, spl = 0, uns = 0;
    u64 sum = 0;
    int32_t mn = INT32_MAX, mx = 0, max_end = 0, max_nlen = 0, min_pos = INT32_MAX;
    u32 cN[4], nlq[4];
    u32 mspan = 0; // TileStats::max_span
    XLane xl; // (EXTRA; a chain of one member: offset 0, spans may leave it)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int64_t r = r0 + i;
        const int32_t p = pos[i], lenv = lq[i];
        const int32_t prv = i == 0 ? pprev : pos[i > 0 ? i - 1 : 0];
        if (p < prv) set_error(err, b.base + (u32)r, PJB_ERR_UNSORTED);
        if (((xs4 >> (8 * i)) & 0xffu) > 2u) set_error(err, b.base + (u32)r, PJB_ERR_BAD_XS);
        mn = lenv < mn ? lenv : mn;
        mx = lenv > mx ? lenv : mx;
        sum += (u64)(int64_t)lenv;
        const u32 n = c[i + 1] - c[i];
        nlq[i] = spl_nlq(n, (u64)(so[i + 1] - so[i]) * 8ull >= (u64)(int64_t)lenv, lenv);
        const u32 *ops = s_ops + (c[i] - cA + shift);
        u32 cc = 0, ngap = 0, gmax = 0, nsum = 0;
        int32_t al = 0;
        auto count_op = [&](u32 op) {
            const u32 ty = op & 15u;
            const int32_t ln = (int32_t)(op >> 4);
            if (op_consumes_ref(ty)) al += ln;
            if (ty == OP_N) {
                cc++;
                max_nlen = ln > max_nlen ? ln : max_nlen;
                nsum = __builtin_elementwise_add_sat(nsum, (u32)ln);
            }
            if (EXTRA && ty == OP_D && ln) { // inside the span, no depth
                ngap++;
                gmax = max(gmax, (u32)ln);
            }
        };
        const u32 o0 = ops[0], o1 = ops[1], o2 = ops[2], o3 = ops[3]; // (what lies behind the read's last operation is masked: 0M has no effect)
        count_op(0u < n ? o0 : 0u);
        count_op(1u < n ? o1 : 0u);
        count_op(2u < n ? o2 : 0u);
        count_op(3u < n ? o3 : 0u);
        for (u32 k = 4; k < n; k++) count_op(ops[k]);
        cnt += cc;
        if (cc) {
            spl++;
            const int32_t e = p + al;
            max_end = e > max_end ? e : max_end;
            min_pos = p < min_pos ? p : min_pos;
            mspan = max(mspan, read_span(al, nsum));
        } else
            uns++;
        cN[i] = cc;
        if (EXTRA) x_classify(X, b.base + (u32)r, p, al, ngap, gmax, cc != 0, (u32)(fl4 >> (16 * i)) & 0xffffu, 0, 0, (u32)b.member, false, xl);
    }
    if (EXTRA) x_counters(X.cnt, xl);
    // ---- ordered compaction of the tile's spliced reads: slot k holds the k-th of them (batch-local index) and the tile-local offset
    // of its first pair.  Thread order is read order: one scan of the threads' counts.
    {
        const u32 inc_s = wave_iscan_dpp(spl), inc_p = wave_iscan_dpp(cnt);
        if (lane_id() == 63) {
            s_scan[0][w] = inc_s;
            s_scan[1][w] = inc_p;
        }
        __syncthreads();
        u32 ex_s = inc_s - spl, ex_p = inc_p - cnt;
#pragma unroll
        for (int k = 0; k < NW; k++)
            if (k < w) {
                ex_s += s_scan[0][k];
                ex_p += s_scan[1][k];
            }
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (cN[i]) {
                const size_t slot = (size_t)blockIdx.x * K1_TILE + ex_s;
                spl_idx[slot] = (u32)(r0 + i);
                spl_poff[slot] = ex_p;
                spl_rec[slot] = make_uint4(c[i], (u32)pos[i], so[i], nlq[i]);
                ex_s++;
                ex_p += cN[i];
            }
    }
    // ---- the tile's statistics (whole-wave reductions on the DPP path; the length sum in 16-bit halves: nothing overflows 32 bits)
    const u32 w_cnt = wave_total<DppAdd>(cnt), w_su = wave_total<DppAdd>((spl << 16) | uns);
    sum = (u64)wave_total<DppAdd>((u32)(sum & 0xffffu)) + ((u64)wave_total<DppAdd>((u32)((sum >> 16) & 0xffffu)) << 16) +
          ((u64)wave_total<DppAdd>((u32)(sum >> 32)) << 32);
    auto smin = [](int32_t v) { return (int32_t)(wave_total<DppMin>((u32)v ^ 0x80000000u) ^ 0x80000000u); };
    auto smax = [](int32_t v) { return (int32_t)(wave_total<DppMax>((u32)v ^ 0x80000000u) ^ 0x80000000u); };
    mn = smin(mn);
    mx = smax(mx);
    max_end = smax(max_end);
    max_nlen = smax(max_nlen);
    min_pos = smin(min_pos);
    mspan = wave_total<DppMax>(mspan);
    if (lane_id() == 0) {
        r32[w][5] = (int32_t)mspan;
        r64[w][0] = ((u64)w_cnt << 32) | w_su;
        r64[w][1] = sum;
        r32[w][0] = mn;
        r32[w][1] = mx;
        r32[w][2] = max_end;
        r32[w][3] = max_nlen;
        r32[w][4] = min_pos;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 pk = 0;
        TileStats ts;
        ts.sum_len = 0;
        ts.min_len = INT32_MAX, ts.max_len = 0, ts.max_end = 0, ts.max_nlen = 0, ts.min_pos = INT32_MAX, ts.max_span = 0;
        for (int i = 0; i < NW; i++) {
            ts.max_span = max(ts.max_span, (u32)r32[i][5]);
            pk += r64[i][0];
            ts.sum_len += r64[i][1];
            ts.min_len = min(ts.min_len, r32[i][0]);
            ts.max_len = max(ts.max_len, r32[i][1]);
            ts.max_end = max(ts.max_end, r32[i][2]);
            ts.max_nlen = max(ts.max_nlen, r32[i][3]);
            ts.min_pos = min(ts.min_pos, r32[i][4]);
        }
        ts.spliced = (u32)((pk >> 16) & 0xffff);
        ts.unspliced = (u32)(pk & 0xffff);
        if (chk_ref_len > 0 && ts.max_end > chk_ref_len) ts.max_end = INT32_MAX;
        tile_stats[blockIdx.x] = ts;
        tile_cnt[blockIdx.x] = (u32)(pk >> 32);
    }
}
template <bool EXTRA>
__global__ __launch_bounds__(K1C_T) __attribute__((amdgpu_waves_per_eu(K1C_WAVES, K1C_WAVES))) void k1_count(const DevBatch *batches, int n_batches, u32 *tile_cnt, TileStats *tile_stats, u32 *spl_idx,
                                                 u32 *spl_poff, uint4 *spl_rec, u64 *err, GroupTab G, int chk_members, XOut X) {
    constexpr int NW = K1C_T / 64, RPT = K1_TILE / K1C_T; // wavefronts of the block; reads per thread
    __shared__ u64 sm64[NW];
    __shared__ u64 sm_scan4[RPT][NW];
    __shared__ int32_t smi[NW][6];
    const GBatch b = load_batch(batches + batch_of_tile(batches, n_batches, blockIdx.x));
    const u32 tile_local = blockIdx.x - b.tile_base;
    const int32_t chk_ref_len = chk_members ? max(G.len[b.member], 1) : 0;
    int64_t base = (int64_t)tile_local * K1_TILE;
    if (base + K1_TILE <= b.n) { // (a whole tile whose operations fit in LDS: the fast path; else the rounds below)
        const u32 cA = b.cig_off[base], cB = b.cig_off[base + K1_TILE];
        if (cB - cA + 3u <= (u32)K1C_OPSW) {
            k1_count_rows<EXTRA>(b, tile_local, cA, cB - cA, tile_cnt, tile_stats, spl_idx, spl_poff, spl_rec, err, chk_ref_len, X);
            return;
        }
    }
    u32 cnt = 0, spl = 0, uns = 0;
    u64 sum = 0;
    int32_t mn = INT32_MAX, mx = 0, max_end = 0, max_nlen = 0, min_pos = INT32_MAX;
    u32 mspan = 0; // TileStats::max_span
    // all loads of the thread's 4 reads are issued before anything is consumed: offsets, then the first
    // K1_OPS ops of every CIGAR (longer CIGARs continue from global memory), then the per-read scalars
    constexpr int K1_OPS = 4;
    u32 c0[RPT], nop[RPT], ops[RPT][K1_OPS];
    int32_t pos4[RPT];
    u32 c4[RPT], so4[RPT], nlq4[RPT]; // (nlq4: spl_nlq -- what the spliced list keeps of operations count, l_qseq and the presence of bases)
    u32 bad = 0;                // bit it: read `it` lies before its predecessor; bit 4 + it: its XS code is not one
    u32 xflag4[RPT] = {}; // (EXTRA)
    XLane xl;             // (EXTRA; a chain of one member: offset 0, spans may leave it)
    // (Every load below is UNCONDITIONAL -- a lane past the batch's end reads the last record, an operation past a CIGAR's end
    // reads a word that is always there -- and the value is masked afterwards.  Written as `cond ? load : 0` the compiler
    // may not speculate the load, turns it into a branch and waits for each one before issuing the next: the 16 CIGAR loads
    // of a thread were 16 round trips in a row.)
#pragma unroll
    for (int it = 0; it < RPT; it++) {
        const int64_t r = base + it * K1C_T + threadIdx.x;
        const bool on = r < b.n;
        const int64_t rr = on ? r : b.n - 1, rp = rr > 0 ? rr - 1 : 0;
        const u32 c0v = b.cig_off[rr], c1v = b.cig_off[rr + 1];
        const int32_t posv = b.pos[rr], prevv = b.pos[rp], lenv = b.l_qseq[rr];
        const u32 xsv = (u32)b.xs[rr], sov = b.seq_off[rr], so1v = b.seq_off[rr + 1];
        // (the scalars are folded as they arrive -- the operations' loads below need the offsets of this same batch of loads anyway --
        // so that only what the list and the walk need stays in registers: 58 of them, eight tiles a CU)
        so4[it] = sov;
        c0[it] = on ? c0v : 0u;
        nop[it] = on ? c1v - c0v : 0u;
        pos4[it] = on ? posv : 0;
        const int32_t prv = r > 0 ? prevv : (b.prev_pos_ptr ? *b.prev_pos_ptr : b.prev_pos);
        if (on && posv < prv) bad |= 1u << it;
        if (on && xsv > 2) bad |= 16u << it;
        if (on) {
            mn = lenv < mn ? lenv : mn;
            mx = lenv > mx ? lenv : mx;
            sum += (u64)(int64_t)lenv;
        }
        nlq4[it] = spl_nlq(c1v - c0v, (u64)(so1v - sov) * 8ull >= (u64)(int64_t)lenv, lenv);
        if (EXTRA) {
            const u32 fv = (u32)b.flag[rr];
            xflag4[it] = on ? fv : 0u;
        }
    }
    // (one 16-byte load per read instead of four words was measured: 55 against 52 us a launch -- consecutive reads' operations
    // are neighbours, the word loads coalesce)
#pragma unroll
    for (int it = 0; it < RPT; it++)
#pragma unroll
        for (int k = 0; k < K1_OPS; k++) {
            const bool has = (u32)k < nop[it];
            const u32 v = *(has ? b.cigar + c0[it] + k : b.cig_off);
            ops[it][k] = has ? v : 0u;
        }
#pragma unroll
    for (int it = 0; it < RPT; it++) {
        const int64_t r = base + it * K1C_T + threadIdx.x;
        u32 cthis = 0;
        if (r < b.n) {
            const int32_t p = pos4[it];
            if (bad & (1u << it)) set_error(err, b.base + (u32)r, PJB_ERR_UNSORTED);
            if (bad & (16u << it)) set_error(err, b.base + (u32)r, PJB_ERR_BAD_XS);
            u32 c = 0, ngap = 0, gmax = 0, nsum = 0;
            int32_t al = 0;
            auto count_op = [&](u32 op) {
                const u32 ty = op & 15u;
                const int32_t ln = (int32_t)(op >> 4);
                if (op_consumes_ref(ty)) al += ln;
                if (ty == OP_N) {
                    c++;
                    max_nlen = ln > max_nlen ? ln : max_nlen;
                    nsum = __builtin_elementwise_add_sat(nsum, (u32)ln);
                }
                if (EXTRA && ty == OP_D && ln) { // inside the span, no depth
                    ngap++;
                    gmax = max(gmax, (u32)ln);
                }
            };
#pragma unroll
            for (int k = 0; k < K1_OPS; k++) count_op(ops[it][k]); // padding ops are 0M: no effect
            for (u32 k = K1_OPS; k < nop[it]; k++) count_op(b.cigar[c0[it] + k]);
            cnt += c;
            if (c) {
                spl++;
                int32_t e = p + al;
                max_end = e > max_end ? e : max_end;
                min_pos = p < min_pos ? p : min_pos;
                mspan = max(mspan, read_span(al, nsum));
            } else
                uns++;
            cthis = c;
            if (EXTRA) x_classify(X, b.base + (u32)r, p, al, ngap, gmax, c != 0, xflag4[it], 0, 0, (u32)b.member, false, xl);
        }
        c4[it] = cthis;
    }
    if (EXTRA) x_counters(X.cnt, xl);
    // ordered compaction of the spliced reads of this tile: slot k holds the k-th spliced read
    // (batch-local index) and the tile-local offset of its first pair.  Read order is round-major
    // (r = base + it * 256 + thread): one wave scan per round, one barrier for all four.
    {
        u64 inc[RPT];
        const int w = threadIdx.x >> 6;
#pragma unroll
        for (int it = 0; it < RPT; it++) {
            inc[it] = wave_iscan<u64>(((u64)c4[it] << 16) | (u64)(c4[it] ? 1u : 0u));
            if (lane_id() == 63) sm_scan4[it][w] = inc[it];
        }
        __syncthreads();
        u64 run = 0; // (pairs << 16 | spliced reads) of everything before, in read order
#pragma unroll
        for (int it = 0; it < RPT; it++) {
            u64 before = run;
#pragma unroll
            for (int i = 0; i < NW; i++) {
                const u64 t = sm_scan4[it][i];
                if (i < w) before += t;
                run += t;
            }
            if (c4[it]) {
                const u64 ex = before + inc[it] - (((u64)c4[it] << 16) | 1u);
                const size_t slot = (size_t)blockIdx.x * K1_TILE + (u32)(ex & 0xffffu);
                spl_idx[slot] = (u32)(base + it * K1C_T + threadIdx.x);
                spl_poff[slot] = (u32)(ex >> 16);
                spl_rec[slot] = make_uint4(c0[it], (u32)pos4[it], so4[it], nlq4[it]);
            }
        }
    }
    // block reduce
    // whole-wave reductions on the DPP path (every lane gets the result); per wave: spl, uns <= 256, cnt <= 256 * 65535,
    // and the length sum goes in two 16-bit halves so that nothing can overflow 32 bits
    u64 packed = ((u64)wave_total<DppAdd>(cnt) << 32) | (u64)wave_total<DppAdd>((spl << 16) | uns);
    sum = (u64)wave_total<DppAdd>((u32)(sum & 0xffffu)) + ((u64)wave_total<DppAdd>((u32)((sum >> 16) & 0xffffu)) << 16) +
          ((u64)wave_total<DppAdd>((u32)(sum >> 32)) << 32);
    auto smin = [](int32_t v) { return (int32_t)(wave_total<DppMin>((u32)v ^ 0x80000000u) ^ 0x80000000u); };
    auto smax = [](int32_t v) { return (int32_t)(wave_total<DppMax>((u32)v ^ 0x80000000u) ^ 0x80000000u); };
    mn = smin(mn);
    mx = smax(mx);
    max_end = smax(max_end);
    max_nlen = smax(max_nlen);
    min_pos = smin(min_pos);
    mspan = wave_total<DppMax>(mspan);
    int w = threadIdx.x >> 6;
    __shared__ u64 smp[NW];
    if (lane_id() == 0) {
        smp[w] = packed;
        sm64[w] = sum;
        smi[w][0] = mn;
        smi[w][1] = mx;
        smi[w][2] = max_end;
        smi[w][3] = max_nlen;
        smi[w][4] = min_pos;
        smi[w][5] = (int32_t)mspan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 p = 0;
        TileStats t;
        t.sum_len = 0;
        t.min_len = INT32_MAX, t.max_len = 0, t.max_end = 0, t.max_nlen = 0, t.min_pos = INT32_MAX, t.max_span = 0;
        for (int i = 0; i < NW; i++) {
            t.max_span = max(t.max_span, (u32)smi[i][5]);
            p += smp[i];
            t.sum_len += sm64[i];
            t.min_len = min(t.min_len, smi[i][0]);
            t.max_len = max(t.max_len, smi[i][1]);
            t.max_end = max(t.max_end, smi[i][2]);
            t.max_nlen = max(t.max_nlen, smi[i][3]);
            t.min_pos = min(t.min_pos, smi[i][4]);
        }
        t.spliced = (u32)((p >> 16) & 0xffff);
        t.unspliced = (u32)(p & 0xffff);
        if (chk_ref_len > 0 && t.max_end > chk_ref_len) t.max_end = INT32_MAX;
        tile_stats[blockIdx.x] = t;
        tile_cnt[blockIdx.x] = (u32)(p >> 32);
    }
}

// exclusive scan of per-tile pair counts (in place) + reduction of tile stats
// (tile_desc != nullptr: the tiles of k1_walk placed their pairs themselves -- only the total is taken, from their
// descriptors, and nothing is written back)
// tile_soff / chunk_tile (both may be nullptr): the tiles' spliced reads seen as ONE dense list -- tile_soff[t] = spliced reads
// before tile t (n_tiles + 1 entries), chunk_tile[c] = the tile that holds list entry 256 c -- for k1_emit's dense mapping.
// A FEW blocks of 256 threads (at most K1S_BLOCKS), each over a contiguous range of tiles: a block first sums its range and
// publishes the sums (ScanPart, flag = this launch's epoch: nothing to reset between launches), then adds up what the blocks
// before it published -- one lane per predecessor, all of them produced at the same time: no chain -- and scans its range
// from there; the last block reduces the statistics and writes the ContigStats.  (Workgroups start in the order of their
// index: a block only ever waits for blocks that started before it.)  It was ONE block: 28 k tiles of a chain of configs[2] in
// seven rounds of dependent loads, 100 us alone and 310 us beside the other chains' kernels, on every chain's critical path.
// (And one block of 1024 before that: a workgroup of 16 wavefronts needs 16 free wave slots on ONE CU at once, and beside
// the inflate and other chains' kernels in the end-to-end run it waited for them -- 4 ms per target instead of 60 us.)
constexpr int K1S_THREADS = 256, K1S_PER = 16, K1S_BLOCKS = 64;
struct ScanPart { // what one block of k1_scan_tiles found in its range of tiles
    u64 pairs, spl, uns, sum;
    int32_t mn, mx, max_end, max_nlen, min_pos;
    u32 flag; // == the launch's epoch: the part is complete
    u32 max_span, _pad;
};
static_assert(sizeof(ScanPart) == 64, "ScanPart layout");
__host__ __device__ inline u32 k1s_blocks(u32 n_tiles) { // ~1024 tiles a block
    const u32 g = (n_tiles + 1023u) / 1024u;
    return g < 1u ? 1u : (g > (u32)K1S_BLOCKS ? (u32)K1S_BLOCKS : g);
}
__global__ __launch_bounds__(K1S_THREADS) void k1_scan_tiles(u32 *tile_cnt, const TileStats *ts, u32 n_tiles, ContigStats *out, u32 pair_limit,
                                                              KeyFmt kf, int32_t ref_len, const u64 *tile_desc, u32 *tile_soff, u32 *chunk_tile,
                                                              ScanPart *parts, u32 epoch, u32 window_skip) {
    constexpr int NW = K1S_THREADS / 64;
    __shared__ u64 wsum[NW];
    __shared__ u32 wsum2[NW];
    __shared__ u32 carry2_s;
    __shared__ u64 carry_s;
    __shared__ u64 r_pairs[NW], r_spl[NW], r_uns[NW], r_sum[NW];
    __shared__ int32_t r_i[NW][6];
    __shared__ ScanPart total_s; // (last block: everything before it)
    const u32 nblk = gridDim.x, blk = blockIdx.x;
    // the block's range: whole rounds of 16 tiles per thread so that ranges start at multiples of 16
    const u32 per_blk = ((n_tiles + nblk - 1) / nblk + (u32)K1S_PER - 1) / (u32)K1S_PER * (u32)K1S_PER;
    const u32 lo = min(n_tiles, blk * per_blk), hi = min(n_tiles, lo + per_blk);
    const int w = threadIdx.x >> 6;
    // ---- pass A: the range's sums
    u64 pairs = 0, spl = 0, uns = 0, sum = 0;
    int32_t mn = INT32_MAX, mx = 0, max_end = 0, max_nlen = 0, min_pos = INT32_MAX;
    u32 max_span = 0;
    for (u32 base = lo; base < hi; base += K1S_THREADS * K1S_PER) {
        const u32 i0 = base + K1S_PER * threadIdx.x;
#pragma unroll 4
        for (int q = 0; q < K1S_PER; q++) { // (loads from a clamped index, masked after: they travel together, see k1_count)
            const u32 i = i0 + q, ic = i < hi ? i : hi - 1;
            const u64 cnt = tile_desc ? (tile_desc[ic] & ((1ull << 40) - 1)) : (u64)tile_cnt[ic];
            const TileStats t = ts[ic];
            if (i < hi) {
                pairs += cnt;
                spl += t.spliced;
                uns += t.unspliced;
                sum += t.sum_len;
                mn = min(mn, t.min_len);
                mx = max(mx, t.max_len);
                max_end = max(max_end, t.max_end);
                max_nlen = max(max_nlen, t.max_nlen);
                min_pos = min(min_pos, t.min_pos);
                max_span = max(max_span, t.max_span);
            }
        }
    }
    pairs = wave_sum(pairs);
    spl = wave_sum(spl);
    uns = wave_sum(uns);
    sum = wave_sum(sum);
    mn = wave_min(mn);
    mx = wave_max(mx);
    max_end = wave_max(max_end);
    max_nlen = wave_max(max_nlen);
    min_pos = wave_min(min_pos);
    max_span = wave_max(max_span);
    if (lane_id() == 0) {
        r_i[w][5] = (int32_t)max_span;
        r_pairs[w] = pairs;
        r_spl[w] = spl;
        r_uns[w] = uns;
        r_sum[w] = sum;
        r_i[w][0] = mn;
        r_i[w][1] = mx;
        r_i[w][2] = max_end;
        r_i[w][3] = max_nlen;
        r_i[w][4] = min_pos;
    }
    __syncthreads();
    ScanPart mine;
    mine.pairs = mine.spl = mine.uns = mine.sum = 0;
    mine.mn = INT32_MAX, mine.mx = 0, mine.max_end = 0, mine.max_nlen = 0, mine.min_pos = INT32_MAX, mine.max_span = 0;
    for (int k = 0; k < NW; k++) {
        mine.max_span = max(mine.max_span, (u32)r_i[k][5]);
        mine.pairs += r_pairs[k];
        mine.spl += r_spl[k];
        mine.uns += r_uns[k];
        mine.sum += r_sum[k];
        mine.mn = min(mine.mn, r_i[k][0]);
        mine.mx = max(mine.mx, r_i[k][1]);
        mine.max_end = max(mine.max_end, r_i[k][2]);
        mine.max_nlen = max(mine.max_nlen, r_i[k][3]);
        mine.min_pos = min(mine.min_pos, r_i[k][4]);
    }
    if (threadIdx.x == 0 && blk + 1 < nblk) { // (nobody reads the last block's part)
        ScanPart *o = parts + blk;
        o->pairs = mine.pairs;
        o->spl = mine.spl;
        o->uns = mine.uns;
        o->sum = mine.sum;
        o->mn = mine.mn;
        o->mx = mine.mx;
        o->max_end = mine.max_end;
        o->max_nlen = mine.max_nlen;
        o->min_pos = mine.min_pos;
        o->max_span = mine.max_span;
        __hip_atomic_store(&o->flag, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- what the blocks before this one hold: lane k of the first wavefront waits for block k
    if (w == 0) {
        const u32 l = lane_id();
        ScanPart b;
        b.pairs = b.spl = b.uns = b.sum = 0;
        b.mn = INT32_MAX, b.mx = 0, b.max_end = 0, b.max_nlen = 0, b.min_pos = INT32_MAX, b.max_span = 0;
        if (l < blk) {
            const ScanPart *o = parts + l;
            while (__hip_atomic_load(&o->flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != epoch) __builtin_amdgcn_s_sleep(1);
            b.pairs = __hip_atomic_load(&o->pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            b.spl = __hip_atomic_load(&o->spl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (blk + 1 == nblk) {
                b.uns = __hip_atomic_load(&o->uns, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                b.sum = __hip_atomic_load(&o->sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                b.mn = __hip_atomic_load(&o->mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                b.mx = __hip_atomic_load(&o->mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                b.max_end = __hip_atomic_load(&o->max_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                b.max_nlen = __hip_atomic_load(&o->max_nlen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                b.min_pos = __hip_atomic_load(&o->min_pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                b.max_span = __hip_atomic_load(&o->max_span, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        b.pairs = wave_sum(b.pairs);
        b.spl = wave_sum(b.spl);
        if (blk + 1 == nblk) {
            b.uns = wave_sum(b.uns);
            b.sum = wave_sum(b.sum);
            b.mn = wave_min(b.mn);
            b.mx = wave_max(b.mx);
            b.max_end = wave_max(b.max_end);
            b.max_nlen = wave_max(b.max_nlen);
            b.min_pos = wave_min(b.min_pos);
            b.max_span = wave_max(b.max_span);
        }
        if (l == 0) {
            carry_s = b.pairs;
            carry2_s = (u32)b.spl;
            total_s = b;
        }
    }
    __syncthreads();
    // ---- pass B: the scan of the range, from the sums before it (the tiles' counts once more: L2 hits)
    for (u32 base = lo; base < hi; base += K1S_THREADS * K1S_PER) {
        const u32 i0 = base + K1S_PER * threadIdx.x;
        u64 v[K1S_PER];
        u32 v2[K1S_PER];
        u64 vs = 0;
        u32 vs2 = 0;
#pragma unroll
        for (int q = 0; q < K1S_PER; q++) {
            const u32 i = i0 + q, ic = i < hi ? i : hi - 1;
            const u64 cnt = tile_desc ? (tile_desc[ic] & ((1ull << 40) - 1)) : (u64)tile_cnt[ic];
            const u32 sp = ts[ic].spliced;
            v[q] = i < hi ? cnt : 0;
            v2[q] = i < hi ? sp : 0u;
            vs += v[q];
            vs2 += v2[q];
        }
        const u64 inc = wave_iscan(vs);
        const u32 inc2 = wave_iscan(vs2);
        if (lane_id() == 63) {
            wsum[w] = inc;
            wsum2[w] = inc2;
        }
        __syncthreads();
        u64 wb = 0, tot = 0;
        u32 wb2 = 0, tot2 = 0;
        for (int k = 0; k < NW; k++) {
            const u64 s = wsum[k];
            const u32 s2 = wsum2[k];
            if (k < w) {
                wb += s;
                wb2 += s2;
            }
            tot += s;
            tot2 += s2;
        }
        const u64 carry = carry_s;
        const u32 carry2 = carry2_s;
        // NOTE: exclusive offsets are stored as 32-bit: a contig is limited to < 2^32 pairs
        u64 ex = carry + wb + inc - vs;
        u32 so = carry2 + wb2 + inc2 - vs2;
#pragma unroll
        for (int q = 0; q < K1S_PER; q++) {
            const u32 i = i0 + q;
            if (i < hi) {
                if (!tile_desc) tile_cnt[i] = (u32)ex;
                if (tile_soff) {
                    tile_soff[i] = so;
                    for (u32 c = (so + 255u) >> 8; (c << 8) < so + v2[q]; c++) chunk_tile[c] = i; // list entries 256 c that fall into this tile
                }
            }
            ex += v[q];
            so += v2[q];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            carry_s = carry + tot;
            carry2_s = carry2 + tot2;
        }
        __syncthreads();
    }
    if (blk + 1 != nblk) return;
    if (threadIdx.x == 0) {
        if (tile_soff) tile_soff[n_tiles] = carry2_s;
        const ScanPart b = total_s;
        const u64 n_pairs = carry_s;
        const int32_t m0 = min(b.mn, mine.mn), m1 = max(b.mx, mine.mx), m2 = max(b.max_end, mine.max_end), m3 = max(b.max_nlen, mine.max_nlen),
                      m4 = min(b.min_pos, mine.min_pos);
        out->spliced = b.spl + mine.spl;
        out->unspliced = b.uns + mine.uns;
        out->sum_len = b.sum + mine.sum;
        out->min_len = m0;
        out->max_len = m1;
        out->max_end = m2;
        out->max_nlen = m3;
        out->min_pos = m4;
        out->n_tiles = n_tiles;
        out->n_pairs = n_pairs;
        // limits the host assumed: pair capacity and key format (the keys of k1_emit must fit the digits it planned)
        u32 ovf = 0;
        if (n_pairs > (u64)pair_limit) ovf |= OVF_PAIRS;
        if (n_pairs > 0) {
            const bool weird = m4 < 0 || m2 > ref_len || m2 < 0;
            if (!kf.raw) {
                int need = 0;
                for (u32 v = (u32)m3; v; v >>= 1) need++;
                if (weird || need > kf.lbits) ovf |= OVF_KEYFMT;
            }
        }
        out->overflow = ovf;
        out->P = ovf ? 0u : (u32)n_pairs;
        out->J = out->R = out->n_slots = out->n_slices = 0;
        out->n_junc = out->n_runs = 0;
        out->list_need = 0;
        out->n_cand = 0;
        out->max_span = window_skip ? max(b.max_span, mine.max_span) : 0xffffffffu;
    }
}

// ---------------------------------------------------------------------------------------------
// K1b: per-read CIGAR walk, pass 2: emit one pair per N op in BAM order
// (JunctionSystem::addJunctions junction_system.cc:140-210 restated iteratively:
//  after an N op the next left anchor starts at the CLAMPED rStart; rEndExc is the UNCLAMPED
//  rStart plus the reference-consuming ops up to the next N, then clamped).
// Per-pair predicates of Junction::addJunctionAlignment (junction.cc:477-502) and
// calcAlignmentStats (junction.cc:755-814) are evaluated here, where the read's fixed-width
// fields are read coalesced, and packed into `meta`.  The same thread then compares the anchors
// of a read of the common [S] M N M [S] shape with the genome (AlignmentInfo::calcMatchStats,
// junction.cc:147-240): the pair's record leaves this kernel complete.
// ---------------------------------------------------------------------------------------------
// (profiles/r04e_compare_variants.txt: 32 bases a round with both anchors' words in flight together / 56 together / 32 one anchor
// after the other / 56 one after the other = 10.56 / 11.56 / 10.07 / 9.97 ms a step; since then an anchor is a block compared on
// its own, one after the other)
constexpr int SIMPLE_NW = 8; // two 16-byte loads per stream and round, 56 bases a round (5: one 16-byte load and a word, 32 bases)
// what the walks find comparing one anchor (a block of emitted positions): its length, mismatches, first and last mismatch
struct CmpBlock {
    int32_t len, mism, first, last;
};
// a pair's packed statistics from its left and right anchor (junction.cc:263-272: matches from the left anchor's end / the right
// anchor's start; mmes; mismatches)
__device__ __forceinline__ u64 cmp_blocks_res(const CmpBlock &L, const CmpBlock &R) {
    const u32 upM = L.last < 0 ? (u32)L.len : (u32)(L.len - 1 - L.last);
    const u32 downM = R.first < 0 ? (u32)R.len : (u32)R.first;
    const u32 tu = (u32)(L.len - L.mism), td = (u32)(R.len - R.mism);
    return pack_res(upM < downM ? upM : downM, tu < td ? tu : td, (u32)(L.mism + R.mism));
}
// One spliced read's pairs (JunctionSystem::addJunctions junction_system.cc:140-210) -- everything that follows from
// the read's fixed-width fields is in R, the CIGAR behind `cig`.  Shape test, walk with the two monotone cursors for
// the up/down junction counts (junction.cc:795-812), one 32-byte record per pair.
struct EmitRead {
    u32 n;        // CIGAR operations
    int32_t pos;
    u32 g;        // global read ordinal
    u32 meta;     // per-read predicates (category, XS, UM, BPP, PPP, REL, MULTI)
    u32 nN;       // N operations
    int32_t aend; // pos + aligned length - 1
    int32_t lq;   // l_qseq
    bool seq_ok;  // the record carries at least lq bases
    u32 off;      // index of the read's first pair
    // A read of the shape [S] M (N M)+ [S] (l_qseq matching, bases present, nothing clamped): the anchors of pair k are the M
    // blocks either side of its N operation -- UNLESS another read's alignment makes the junction's anchor window reach over
    // a neighbouring intron of this read (bam_alignment.cc:359: the walks only stop at an N operation that leaves the
    // window).  The window is known after K2d; the block compares are done here, where the read's operations and bases are
    // at hand (closed != nullptr), and k4b_generic checks the window for the reads on its second list.
    const u32 *closed_seqw; // the read's packed bases (nullptr: not of that shape -- the generic walks fill PairRec::aux in)
    int32_t q_limit;        // last word behind closed_seqw that may be read (cmp_words)
    const u32 *gcodes;      // the target's 4-bit codes
    int32_t glen, voff;     // the target's length and its offset in the group's virtual sequence
};
// Blocks with I / D operations are in closed form too: the walk list all but empties -- k4b_generic 224 -> 140 us a chain, k1_generic
// 122 -> 162 -- 8.82 -> 8.64 ms a step.  (While these reads were walked by a few lanes of k1_emit's blocks the same cost 60 us a k1_emit
// launch: 9.75 against 9.1 ms.)
// (reads of the simple shape never come here: k1_emit finishes them in closed form.)  on_pair(key, lStart, rEnd) is called
// for every pair once its record is complete; the match statistics (PairRec::aux) of a read that is not `closed` are
// k4b_generic's to fill in.
template <typename Ops, typename PairFn>
__device__ __forceinline__ void emit_read_pairs(const Ops cig, const EmitRead R, const Pairs P, const KeyFmt kf, const int32_t ref_len,
                                                u64 *err, PairFn &&on_pair) {
    const u32 n = R.n, g = R.g, nN = R.nN;
    const int32_t pos = R.pos, aend = R.aend;
    u32 meta = R.meta;
    // ---- walk: pairs (junction_system.cc:140-210) and, with two monotone cursors over the read's own
    // introns, the up/down junction counts (junction.cc:795-812)
    NCursor U = {0, pos, false, 0}, D = {0, pos, false, 0};
    ncursor_advance(U, cig, n);
    ncursor_advance(D, cig, n);
    u32 cntU = 0, cntD = 0;
    int32_t lStart = pos, lEndExc = pos, sumAfter = 0, prevRStartU = 0, prevIend = 0, prevIstart = 0;
    int32_t qAcc = 0, prevQ = 0; // query bases (soft clips included) before the operation / before the pending pair's N
    int64_t prev = -1;
    u64 prev_key = 0;
    const bool closed = R.closed_seqw != nullptr;
    PairRec pend;
    pend.aux = 0;
    pend.lstart = pend.rend = 0;
    pend.pos = pos;
    pend.aend = aend;
    pend.meta = closed ? meta | META_SIMPLE : meta;
    pend.updown = 0;
    // closed: the read is [S] B (N B)+ [S], every block B a run of M = X I D operations that starts and ends with bases on both
    // sides.  What the walks emit for a block -- compared bases for M = X, read letters against 'X' padding for I, 'X' padding
    // against genome bases for D (never equal: such targets hold no 'X') -- is accumulated ONCE per block as the operations go
    // by: a block is the right anchor of the pair before it and the left anchor of the pair behind it (bam_alignment.cc:341-462
    // with the whole block inside the window, which k4b_generic checks).
    typedef CmpBlock Block;
    Block blkL = {0, 0, -1, -1}, blk = {0, 0, -1, -1}; // the pending pair's left block; the block being walked
    auto closed_stats = [&]() { return cmp_blocks_res(blkL, blk); };
    (void)prevIstart;
    (void)prevQ;
    u32 k = 0;
    for (u32 i = 0; i < n; i++) {
        const u32 op = cig[i];
        const u32 ty = op & 15u;
        const int32_t ln = (int32_t)(op >> 4);
        if (ty == OP_N) {
            if (prev >= 0) {
                int32_t rEndExc = prevRStartU + sumAfter;
                if (rEndExc - 1 >= ref_len) rEndExc = ref_len; // junction_system.cc:172-174
                pend.rend = rEndExc - 1;
                if (closed) pend.aux = closed_stats();
                rec_store(P.rec + prev, pend);
                on_pair(prev_key, pend.lstart, pend.rend);
                if (rEndExc - 1 < prevIend) set_error(err, g, PJB_ERR_MIN_ANCHOR); // intron.cc:76
            }
            const int32_t istart = lEndExc;
            const int32_t rStartU = lEndExc + ln;
            int32_t rStart = rStartU;
            if (rStart - 1 >= ref_len) rStart = ref_len - 1; // junction_system.cc:169-171
            const int32_t iend = rStart - 1;
            while (U.has && U.peek < istart) {
                cntU++;
                ncursor_advance(U, cig, n);
            }
            while (D.has && D.peek <= iend + 1) {
                cntD++;
                ncursor_advance(D, cig, n);
            }
            const int64_t idx = (int64_t)R.off + k;
            const u64 key = make_key(kf, istart, iend);
            P.key[idx] = key;
            if (P.g) P.g[idx] = g;
            pend.lstart = lStart;
            pend.updown = cntU | ((nN - cntD) << 16);
            if (lStart > istart) set_error(err, g, PJB_ERR_MIN_ANCHOR); // intron.cc:68
            prev = idx;
            prev_key = key;
            blkL = blk; // (the block that ends here is this pair's left anchor)
            blk = Block{0, 0, -1, -1};
            prevIstart = istart;
            prevQ = qAcc;
            prevIend = iend;
            prevRStartU = rStartU;
            sumAfter = 0;
            lStart = rStart;
            lEndExc = rStart;
            k++;
        } else {
            if (closed && ty != OP_S) {
                const bool cq = op_consumes_query(ty), cr = op_consumes_ref(ty);
                if (cq && cr) // M = X: bases against bases
                    cmp_words<SIMPLE_NW, true>(R.closed_seqw, qAcc, R.q_limit, R.gcodes, lEndExc - R.voff, (R.glen + 7) / 8 + 1, ln, blk.len, blk.mism, blk.first, blk.last);
                else { // I / D: ln positions that never match
                    blk.mism += ln;
                    if (blk.first < 0) blk.first = blk.len;
                    blk.last = blk.len + ln - 1;
                }
                blk.len += ln;
            }
            if (op_consumes_ref(ty)) {
                lEndExc += ln;
                sumAfter += ln;
            }
        }
        if (op_consumes_query(ty)) qAcc += ln;
    }
    if (prev >= 0) {
        int32_t rEndExc = prevRStartU + sumAfter;
        if (rEndExc - 1 >= ref_len) rEndExc = ref_len;
        pend.rend = rEndExc - 1;
        if (closed) pend.aux = closed_stats();
        rec_store(P.rec + prev, pend);
        on_pair(prev_key, pend.lstart, pend.rend);
        if (rEndExc - 1 < prevIend) set_error(err, g, PJB_ERR_MIN_ANCHOR);
    }
}

// per-read predicates of a pair's `meta` word (Junction::addJunctionAlignment junction.cc:477-502, calcAlignmentStats
// junction.cc:755-814, BamAlignment::calcIfProperPair bam_alignment.cc:271-292); MULTI and SIMPLE are added by the caller
__device__ __forceinline__ u32 read_meta(u32 flag, u32 xs, u32 mapq, int32_t pos, int32_t mtid, int32_t mpos, int32_t tid, int orientation) {
    const bool pp_check = orientation == PJB_OR_FR || orientation == PJB_OR_RF || orientation == PJB_OR_FF;
    const bool first = flag & 0x40, rev = flag & 0x10;
    u32 meta = (first ? 0u : 2u) + (rev ? 1u : 0u);
    meta |= (xs & 3u) << META_XS_SHIFT;
    const bool um = mapq >= 30;
    if (um) meta |= META_UM;
    if (flag & 0x2) meta |= META_BPP;
    bool ppp = false;
    if (pp_check) {
        const bool paired = flag & 0x1, mate_mapped = !(flag & 0x8);
        if (paired && mate_mapped && tid == mtid) {
            const bool mrev = flag & 0x20;
            const bool diff = rev != mrev;
            const bool gap = !rev ? pos < mpos : pos > mpos;
            ppp = orientation == PJB_OR_FR ? (diff && gap) : orientation == PJB_OR_RF ? (diff && !gap) : (!diff && gap);
        }
    }
    if (ppp) meta |= META_PPP;
    if (um && (!pp_check || ppp)) meta |= META_REL;
    return meta;
}

// The common shapes [S] M N M [S] and [S] M N M N M [S] (coordinates of the read's own target): an anchor is one block of bases,
// read[q, q + len) against genome[g, g + len) (cmp_words); neither depends on the junction-level window -- the walk rules of
// bam_alignment.cc:341-462 reduce to exactly this for the shapes (for two introns: unless a window reaches over the other
// intron, which k4b_generic checks).
// Thread per spliced read of the batch, DENSE: the tiles' spliced lists (k1_count compacted them per tile) are walked as one
// list -- entry s lies in the tile t with tile_soff[t] <= s < tile_soff[t + 1], found from chunk_tile (the tile of entry
// 256 * chunk) and a short walk -- so every thread of every block has a read.  The read's CIGAR is fetched once (8
// independent loads into an LDS column, the walks then run at LDS latency).  The grid is fixed; blocks stride over the
// batch's chunks of 256 list entries.
//   voff: the target's offset in its group's virtual sequence (0 for a single target); every coordinate a pair carries is
// virtual, the per-read predicates and the base compare work on the record's own coordinates.
//   gcodes: the target's 4-bit codes; nullptr (exotic characters, an 'X' in the sequence): no read is "simple", every
// pair goes through k4b_generic's byte-wise walks.
// By-products, so that no later kernel has to stream over the pairs for them:
//   * K2d's candidate keys: the block keeps the keys it emits in a small hash set in LDS -- with the smallest lStart and the
//     largest rEnd of the pairs behind each key (junction.cc:477-529: the junction anchors' first level of reduction) -- and
//     appends the distinct ones to the candidate list when the set is a quarter full (and when the block leaves); a
//     junction appears once per residency;
//   * the list of reads that need the generic walks (k4b_generic), in GEN_SHARDS sub-lists (one returning atomic per
//     wavefront, spread over 256 addresses).
constexpr int K1E_LOOK = 16;
#ifndef K1E_WAVES
#define K1E_WAVES 4 // wavefronts per SIMD the register allocation aims at (tools/build_variants.sh builds the others for A/B runs)
#endif
constexpr int K1E_T = 256, K1E_SHIFT = 8; // threads of a block = list entries of one trip
constexpr int KC_SLOTS = K1E_T;               // the block's candidate set (LDS), flushed when a quarter full: a slot per thread (two: 8.82 against 8.75 ms a step)
// What k1_emit and k1_generic share: the block's candidate set (LDS) and the appends to k4b_generic's / k1_generic's lists.
struct EmitShared {
    u64 set[KC_SLOTS];
    int32_t lo[KC_SLOTS], hi[KC_SLOTS];
    u32 set_n, base, scan[4];
};
// (k1_emit keeps its rarely used arguments -- the candidate list's pointers, the error word, the control block -- in scalar registers and unrolls
// the probes below: fetching them from the kernel-argument segment where they are used made it 15 % slower, not unrolling changed nothing --
// profiles/r06_k1_experiments.txt section 6.)
struct EmitCtx {
    EmitShared &sh;
    const EmitLists &E;
    const KeyFmt kf;
    ContigStats *cs;
    const bool want_cand;
    __device__ __forceinline__ void init() {
        if (!want_cand) return;
#pragma unroll
        for (int i = 0; i < KC_SLOTS / K1E_T; i++) {
            sh.set[i * K1E_T + threadIdx.x] = KD_EMPTY;
            sh.lo[i * K1E_T + threadIdx.x] = INT32_MAX;
            sh.hi[i * K1E_T + threadIdx.x] = INT32_MIN;
        }
        if (threadIdx.x == 0) sh.set_n = 0;
    }
    __device__ __forceinline__ void cand_mark(const EmitLists &C, u64 k) const { // (what kd_mark did in a launch of its own)
        int32_t ms, me;
        unpack_key(kf, k, ms, me);
        const u32 w = (u32)ms >> 6;
        const u64 bit = 1ull << (ms & 63);
        const u64 old = atomicOr((unsigned long long *)(C.bitmap + w), (unsigned long long)bit);
        if (!(old & bit)) atomicAdd(&C.page_cnt[w >> KD_PAGE_SHIFT], 1u); // (the ranks below are scanned over the pages, not over the words)
    }
    __device__ __forceinline__ void cand_insert(u64 k, int32_t lstart, int32_t rend) const {
        if (!want_cand) return;
        u32 h = (u32)((k * 0x9E3779B97F4A7C15ull) >> 40) & (KC_SLOTS - 1);
        for (int probe = 0; probe < 24; probe++) { // look first: most keys are there already, and a read of one address by many lanes is a broadcast
            u64 old = sh.set[h];
            if (old == KD_EMPTY) {
                old = atomicCAS((unsigned long long *)&sh.set[h], (unsigned long long)KD_EMPTY, (unsigned long long)k);
                if (old == KD_EMPTY) {
                    atomicAdd(&sh.set_n, 1u);
                    old = k;
                }
            }
            if (old == k) {
                if (lstart < sh.lo[h]) atomicMin(&sh.lo[h], lstart);
                if (rend > sh.hi[h]) atomicMax(&sh.hi[h], rend);
                return;
            }
            h = (h + 1) & (KC_SLOTS - 1);
        }
        // a crowded set (reads with hundreds of introns): straight to the list, where duplicates do no harm
        const u32 at = atomicAdd(&cs->n_cand, 1u);
        E.cand[at] = k;
        E.cand_anc[at] = (u64)(u32)lstart | ((u64)(u32)rend << 32);
        cand_mark(E, k);
    }
    // appends the wavefront's entries to list `kind` (1: reads for k4b_generic's walks, 2: for its window check, 3: reads for
    // k1_generic): one returning atomic per wavefront; sub-list `shard` (callers deal 256-entry chunks round-robin: gen_list_cap)
    // the same in two halves: the returning atomic early (list_reserve), the stores once its answer is there (list_write) -- a wavefront
    // that appends and stores at once waits a memory round trip for the atomic
    // (`pairs`: the same for every entry of the call -- k1_emit's lists hold reads of two pairs, or count none)
    __device__ __forceinline__ u32 list_reserve(u32 kind, bool mine, u32 pairs, u32 shard) const {
        const u64 gm2 = __ballot(mine);
        if (!gm2) return 0u;
        const u32 pairs_w = pairs * (u32)__popcll(gm2);
        const int leader = __ffsll((long long)gm2) - 1;
        const u32 w0 = shard * GEN_CNT_STRIDE + (kind - 1) * 2;
        u32 base = 0;
        if (lane_id() == leader) {
            base = atomicAdd(&E.gen_cnt[w0], (u32)__popcll(gm2));
            if (pairs_w) atomicAdd(&E.gen_cnt[w0 + 1], pairs_w);
        }
        return base; // (in the leader's lane)
    }
    __device__ __forceinline__ void list_write(u32 kind, bool mine, u32 base, u64 entry, u32 shard) const {
        const u64 gm2 = __ballot(mine);
        if (!gm2) return;
        base = (u32)__builtin_amdgcn_readlane((int)base, __ffsll((long long)gm2) - 1);
        const u32 at = base + (u32)__popcll(gm2 & ((1ull << lane_id()) - 1));
        if (mine && at < E.gen_cap) E.gen_list[((size_t)(kind - 1) * GEN_SHARDS + shard) * E.gen_cap + at] = entry;
    }
    __device__ __forceinline__ void list_append(u32 kind, bool mine, u32 pairs, u64 entry, u32 shard) const {
        const u64 gm2 = __ballot(mine);
        if (!gm2) return;
        const u32 pairs_w = wave_total<DppAdd>(mine ? pairs : 0u);
        const int leader = __ffsll((long long)gm2) - 1;
        const u32 w0 = shard * GEN_CNT_STRIDE + (kind - 1) * 2;
        u32 base = 0;
        if (lane_id() == leader) {
            base = atomicAdd(&E.gen_cnt[w0], (u32)__popcll(gm2));
            atomicAdd(&E.gen_cnt[w0 + 1], pairs_w);
        }
        base = (u32)__builtin_amdgcn_readlane((int)base, leader);
        const u32 at = base + (u32)__popcll(gm2 & ((1ull << lane_id()) - 1));
        if (mine && at < E.gen_cap) E.gen_list[((size_t)(kind - 1) * GEN_SHARDS + shard) * E.gen_cap + at] = entry;
    }
    // candidate keys: the set is flushed when it fills up, and before the block leaves (every thread of the block calls)
    __device__ __forceinline__ void cand_flush(bool force) const {
        if (!want_cand) return;
        lds_barrier();
        if (sh.set_n > (u32)KC_SLOTS / 4 || force) {
            u64 mine[KC_SLOTS / K1E_T], anc[KC_SLOTS / K1E_T];
            u32 cnt = 0;
#pragma unroll
            for (int i = 0; i < KC_SLOTS / K1E_T; i++) {
                const int at = i * K1E_T + threadIdx.x;
                mine[i] = sh.set[at];
                anc[i] = (u64)(u32)sh.lo[at] | ((u64)(u32)sh.hi[at] << 32);
                cnt += mine[i] != KD_EMPTY;
                sh.set[at] = KD_EMPTY;
                sh.lo[at] = INT32_MAX;
                sh.hi[at] = INT32_MIN;
            }
            u32 total;
            const u32 excl = block_escan<K1E_T / 64, u32, true>(cnt, sh.scan, &total);
            if (threadIdx.x == 0) {
                sh.base = total ? atomicAdd(&cs->n_cand, total) : 0u;
                sh.set_n = 0;
            }
            lds_barrier();
            u32 o = sh.base + excl;
#pragma unroll
            for (int i = 0; i < KC_SLOTS / K1E_T; i++)
                if (mine[i] != KD_EMPTY) {
                    E.cand[o] = mine[i];
                    E.cand_anc[o++] = anc[i];
                    cand_mark(E, mine[i]);
                }
        }
    }
};

// ---- bases in TWO bits (pjb_batch.seq2 / GroupTab::codes2).  Round 5 took the compares apart (profiles/r05_k1_experiments.txt sections
// 9, 10, 13): they are bound twice -- by the texture addresser, which takes a 4-byte-aligned 16-byte gather one LANE a cycle (16 gathers a
// read), and by ~20 vector instructions per 8 bases.  In 2 bits a 16-byte gather holds 64 bases and a word 16: a round of two gathers per
// stream covers 112 bases where the 4-bit round covers 56, and a word costs 13 instructions.  A lane compares in 2 bits when its read
// is pure ACGT (seq_exc clear), lies inside its target, and the target's exception bitmap is clear under every block of its bases
// (checked behind the compare: the bitmap words are asked for before the first round and looked at after the last); every other lane
// takes the 4-bit rounds as before -- characters are equal exactly where 2-bit codes are when both sides are pure ACGT.
//   Read base i of a read whose seq4 words start at so: bit 16 (so & 1) + 2 i from word so >> 1 of seq2 (a 16-bit granule per seq4 word).
struct __attribute__((packed, aligned(4))) Words2 {
    u32 x, y;
};
constexpr int C2_NW = 8;                      // words per stream and round: two 16-byte gathers, 7 words = 112 bases compared
constexpr int32_t C2_ROUND = 16 * (C2_NW - 1);
constexpr int32_t C2_MAX_BLOCK = 1900;        // a longer block of bases (31 stretches of the bitmap: one 8-byte load) takes the 4-bit rounds
template <int NW>
__device__ __forceinline__ void chunk2_cmp_bits(const u32 (&qw)[NW], const u32 (&gw)[NW], u32 shq, u32 shg, int32_t l, int32_t t, u32 &mism, u32 &fbit,
                                                u32 &lbit1) {
    const int32_t rem = l - t; // bases left from the chunk's first
    u32 fw = 0xffffffffu, lw = 0;
#pragma unroll
    for (int c = 0; c < NW - 1; c++) {
        int32_t v = rem - 16 * c; // the word's valid bases, 0 .. 16
        v = v < 0 ? 0 : (v > 16 ? 16 : v);
        const u32 inval = (0xffffffffu << (u32)v) << (u32)v; // (two shifts: a shift by 32 would not move)
        const u32 x = __builtin_amdgcn_alignbit(qw[c + 1], qw[c], shq) ^ __builtin_amdgcn_alignbit(gw[c + 1], gw[c], shg);
        const u32 m = (x | (x >> 1)) & (0x55555555u & ~inval); // bit 2 j: base j differs
        mism += (u32)__popc(m);
        fw = min(fw, __builtin_elementwise_add_sat(ffbl_hw(m), 32u * (u32)c));
        lw = max(lw, __builtin_elementwise_sub_sat(32u * (u32)c + 32u, ffbh_hw(m)));
    }
    fbit = min(fbit, __builtin_elementwise_add_sat(fw, 2u * (u32)t));
    lbit1 = lw ? lw + 2u * (u32)t : lbit1; // (rounds ascend)
}

// ONE launch per chain (25 launches of 13 - 690 us became 3): a block takes a range of the chain's consecutive trips -- (batch, chunk
// of 256 list entries), a batch after the other; a chunk that two batches share is visited once for each, its lanes masked.  The
// batch descriptors and the members' table are read through uniform indices (scalar loads).
//   The kernel waits for memory, not for bandwidth (round 4's SQ counters: three quarters of the wave-cycles parked on s_waitcnt),
// and a trip is a chain of dependent round trips: tile offsets -> list record -> operations and per-read fields -> bases -> stores.
// So the trips are software-pipelined: while trip v is compared, the list records of trip v + 2 and the operations / fields of
// trip v + 1 are already on their way (in registers).
//   (Round 5 also built the version that stages the wavefront's bases and genome windows through LDS with coalesced loads: 2.4 x fewer
// vector-memory instructions, the same time -- profiles/r05_k1_experiments.txt section 1; it left the tree with round 6, git has it.)
#ifdef K1E_PROF // (debug builds: wave-cycles per section of k1_emit, summed over every wavefront; printed by pjb_destroy)
__device__ unsigned long long g_k1e_prof[16];
#define K1E_T0() unsigned long long prof_t = __builtin_amdgcn_s_memtime()
#define K1E_MARK(i)                                                                  \
    do {                                                                             \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();                \
        if (lane_id() == 0) atomicAdd(&g_k1e_prof[i], now_ - prof_t);                \
        prof_t = now_;                                                               \
    } while (0)
#else
#define K1E_T0() do {} while (0)
#define K1E_MARK(i) do {} while (0)
#endif
constexpr int K1E_MAXB = 64; // batches one launch takes (the host splits longer lists)
struct EmitRec { // a trip's list records (per lane)
    bool on;
    u32 slot, r, toff, poff;
    uint4 sr;
};
struct EmitOps { // and what the records lead to: the read's first operations and its fixed-width fields
    u32 op[OPS_LDS];
    u32 n, flag, xs, mapq;
    u32 excw; // the word of seq_exc that holds the read's bit (all ones: no 2-bit bases in the batch).  Kept as it was loaded: anything computed from
              // it here would make fetch_ops WAIT for its loads -- they are asked for a trip ahead so that nothing waits for them
    int32_t mtid, mpos, lq;
};
struct EmitTrip { // (uniform)
    int bi;
    u32 chunk, s_begin, s_end;
};
__global__ __launch_bounds__(K1E_T) __attribute__((amdgpu_waves_per_eu(K1E_WAVES, K1E_WAVES))) void k1_emit(const DevBatch *batches, int n_batches, u32 n_tiles_total, const u32 *tile_off, const u32 *tile_soff,
                                                const u32 *chunk_tile, const u32 *spl_idx, const u32 *spl_poff, const uint4 *spl_rec, Pairs P, EmitLists E, KeyFmt kf,
                                                GroupTab G, int use_codes, int orientation, u64 *err, ContigStats *cs) {
    __shared__ u32 s_soff[K1E_LOOK];
    __shared__ EmitShared sh;
    __shared__ u32 s_cfirst[K1E_MAXB + 1]; // trips before batch i
    __shared__ u32 s_sbegin[K1E_MAXB + 1]; // list entries before batch i (batches follow each other in the tiles' space)
    __shared__ u32 s_seqw[K1E_MAXB], s_cigw[K1E_MAXB], s_tbase[K1E_MAXB]; // words of packed bases / operations in batch i; its first tile
    __shared__ u32 s_wsum[4];
    if (cs->P == 0) return; // no pairs, or a limit was exceeded: the contig is repeated with larger buffers
    const u32 max_span = cs->max_span; // (uniform: a scalar load)
    K1E_T0();
    const bool want_g = P.g != nullptr; // (--extra contexts: the pairs' read ordinals)
    const bool want_cand = E.cand != nullptr;
    EmitCtx ctx{sh, E, kf, cs, want_cand};
    ctx.init();
    auto cand_insert = [&](u64 k, int32_t lstart, int32_t rend) { ctx.cand_insert(k, lstart, rend); };
    {
        u32 trips = 0;
        if ((int)threadIdx.x < n_batches) {
            const PJB_GLOBAL DevBatch *d = as_global(batches + threadIdx.x);
            const u32 tb = d->tile_base, nt = (u32)((d->n + K1_TILE - 1) / K1_TILE);
            const u32 sb = tile_soff[tb], se = tile_soff[tb + nt];
            trips = sb == se ? 0u : ((se + (u32)K1E_T - 1u) >> K1E_SHIFT) - (sb >> K1E_SHIFT);
            s_sbegin[threadIdx.x] = sb;
            if ((int)threadIdx.x == n_batches - 1) s_sbegin[n_batches] = se;
            s_seqw[threadIdx.x] = as_global(d->seq_off)[d->n];
            s_cigw[threadIdx.x] = as_global(d->cig_off)[d->n];
            s_tbase[threadIdx.x] = tb;
        }
        u32 total;
        const u32 ex = block_escan<K1E_T / 64>(trips, s_wsum, &total);
        if (threadIdx.x < (u32)K1E_MAXB) s_cfirst[threadIdx.x] = ex;
        if (threadIdx.x == K1E_T - 1) s_cfirst[K1E_MAXB] = total;
        __syncthreads();
    }
    const u32 n_trips = s_cfirst[K1E_MAXB];
    // a block's trips are consecutive: the window of tile offsets (s_soff: 16 tiles ~ 18 trips) is fetched once and serves the trips
    // behind it; consecutive trips share junctions, so the block's candidate set lists each of them once
    const u32 per_block = (n_trips + gridDim.x - 1) / gridDim.x;
    const u32 v_lo = min(n_trips, blockIdx.x * per_block), v_hi = min(n_trips, v_lo + per_block);
    if (v_lo >= v_hi) return;
    u32 win_t0 = 0xffffffffu; // the tile of s_soff[0] (none yet)
    int win_bi = -1;
    // ---- the trip's batch: the last one with s_cfirst <= v (uniform)
    auto locate = [&](u32 v) {
        static_assert(K1E_MAXB <= 64, "one ballot");
        const int k = lane_id();
        const u64 m = __ballot(k < n_batches && s_cfirst[k] <= v);
        EmitTrip T;
        T.bi = __builtin_amdgcn_readfirstlane(63 - __clzll((long long)m));
        T.s_begin = s_sbegin[T.bi];
        T.s_end = s_sbegin[T.bi + 1];
        T.chunk = (T.s_begin >> K1E_SHIFT) + (v - s_cfirst[T.bi]);
        return T;
    };
    // ---- a trip's list records (k1_count's by-product: no gathers of cig_off, pos, l_qseq, seq_off); every thread of the block calls
    auto fetch_rec = [&](const EmitTrip &T) {
        const u32 s_last = min((T.chunk + 1u) << K1E_SHIFT, T.s_end) - 1u;
        // (the window is only written between two barriers below: reading it here needs none)
        const bool reload = win_bi != T.bi || win_t0 == 0xffffffffu || s_last >= s_soff[K1E_LOOK - 1];
        if (reload) { // the window of tile offsets: from the tile of the trip's first entry (for a batch's first chunk: of the batch's first entry)
            win_t0 = (T.chunk << K1E_SHIFT) < T.s_begin ? s_tbase[T.bi] : chunk_tile[T.chunk >> (8 - K1E_SHIFT)]; // (chunk_tile: the tile of entry 256 c)
            win_bi = T.bi;
            const u32 mine = threadIdx.x < K1E_LOOK && win_t0 + threadIdx.x <= n_tiles_total ? tile_soff[win_t0 + threadIdx.x] : 0xffffffffu;
            lds_barrier(); // (everybody is done with the old window)
            if (threadIdx.x < K1E_LOOK) s_soff[threadIdx.x] = mine;
            lds_barrier();
        }
        const u32 s = (T.chunk << K1E_SHIFT) + threadIdx.x;
        EmitRec R;
        R.on = s >= T.s_begin && s < T.s_end;
        R.slot = R.r = R.toff = R.poff = 0;
        R.sr = make_uint4(0, 0, 0, 0);
        // The entry's tile = the number of the window's offsets it has reached (they ascend).  A wavefront's 64 entries are consecutive: they
        // lie in one tile, seldom in two or three -- so lane m holds offset m, two ballots say how many offsets the wavefront's first and last
        // entry have reached, and only the offsets in between (none, mostly) are compared lane by lane.  (It was fifteen LDS reads and
        // compares a lane: the kernel is bound by instruction issue -- round 6's SQ counters: its four wavefronts keep a SIMD's issue port
        // busy 104 % of the time between them --, so every instruction of a trip counts.)
        const u32 w_first = (T.chunk << K1E_SHIFT) + (threadIdx.x & ~63u);
        const u32 off_m = lane_id() < K1E_LOOK ? s_soff[lane_id() & (K1E_LOOK - 1)] : 0xffffffffu;
        const u32 m_lo = (u32)__popcll(__ballot(off_m <= w_first)), m_hi = (u32)__popcll(__ballot(off_m <= w_first + 63u));
        if (R.on) {
            u32 k = m_lo ? m_lo - 1u : 0u; // (m_lo >= 1: offset 0 belongs to the tile of the trip's first entry or an earlier one)
            for (u32 m = m_lo ? m_lo : 1u; m < m_hi; m++) k += s >= (u32)__builtin_amdgcn_readlane((int)off_m, (int)m) ? 1u : 0u;
            u32 tile = win_t0 + k, soff = s_soff[k];
            if (k + 1 == (u32)K1E_LOOK && s >= soff) { // (a run of tiles without spliced reads longer than the window: search)
                u32 lo = tile, hi = n_tiles_total; // tile_soff[lo] <= s < tile_soff[hi]
                while (hi - lo > 1) {
                    const u32 mid = (lo + hi) >> 1;
                    if (tile_soff[mid] <= s) lo = mid;
                    else hi = mid;
                }
                tile = lo;
                soff = tile_soff[lo];
            }
            R.slot = tile * (u32)K1_TILE + (s - soff);
            R.sr = spl_rec[R.slot];
            R.r = spl_idx[R.slot];
            R.toff = tile_off[tile];
            R.poff = spl_poff[R.slot];
        }
        return R;
    };
    // ---- and what they lead to: the read's first eight operations (two 16-byte loads; whatever lies behind its last one is masked
    // by the consumer), its five fields and its bit of the batch's exception bitmap
    auto fetch_ops = [&](const EmitTrip &T, const EmitRec &R) {
        EmitOps O;
#pragma unroll
        for (int q = 0; q < OPS_LDS; q++) O.op[q] = 0;
        O.n = O.flag = O.xs = O.mapq = 0;
        O.excw = 0xffffffffu;
        O.mtid = O.mpos = O.lq = 0;
        if (R.on) {
            const GBatch b = load_batch(batches + T.bi);
            const u32 c0 = R.sr.x, cig_words = s_cigw[T.bi];
            const int64_t r = R.r;
            u32 n = R.sr.w & 0x7fffu;
            if (n == 0x7fffu) n = b.cig_off[r + 1] - c0;
            O.n = n;
            O.flag = b.flag[r];
            O.xs = b.xs[r];
            O.mapq = b.mapq[r];
            O.mtid = b.mtid[r];
            O.mpos = b.mpos[r];
            if (b.seq2 != nullptr) O.excw = b.seq_exc[r >> 5]; // (uniform test: the batch either has 2-bit bases or not)
            O.lq = (int32_t)(R.sr.w >> 16);
            if (O.lq == 0xffff) O.lq = b.l_qseq[r];
            fetch_ops8(b.cigar, c0, cig_words, O.op);
        }
        return O;
    };
    K1E_MARK(0); // block start: tables
    EmitTrip T = locate(v_lo);
    EmitRec R = fetch_rec(T);
    EmitOps O = fetch_ops(T, R);
    // (the list records run TWO trips ahead, the operations and fields one: what a trip asks for has had a whole trip to arrive)
    EmitTrip T1 = T;
    EmitRec R1 = R;
    if (v_lo + 1 < v_hi) {
        T1 = locate(v_lo + 1);
        R1 = fetch_rec(T1);
    }
    K1E_MARK(1); // prologue: first trip's records and operations issued
    for (u32 v = v_lo; v < v_hi; v++) {
        const GBatch b = load_batch(batches + T.bi);
        const int mem = b.member;
        const int32_t voff = G.voff[mem], ref_len = G.len[mem], tid = G.tid[mem];
        const PJB_GLOBAL u32 *gcodes = use_codes ? as_global(G.codes[mem]) : (const PJB_GLOBAL u32 *)nullptr;
        const PJB_GLOBAL u32 *gcodes2 = use_codes && b.seq2 != nullptr ? as_global(G.codes2[mem]) : (const PJB_GLOBAL u32 *)nullptr;
        const int32_t vlen = voff + ref_len; // the target's end in the group's virtual sequence
        const u32 seq_words = s_seqw[T.bi];  // words of packed bases in the batch: nothing reads past them
        const int32_t g_words = (ref_len + 7) / 8 + 1;
        const u32 chunk = T.chunk;
        const bool on = R.on;
        const u32 so = R.sr.z;
        const int32_t pos = (int32_t)R.sr.y, lq = O.lq;
        // A read of the shape [S] M N M [S] or [S] M N M N M [S] (l_qseq matching, bases present) is finished here, in closed form
        // (junction_system.cc:140-210 for one or two N operations); any other read goes on k1_generic's list: a few lanes of every
        // wavefront walking their reads kept the whole block waiting (84 of 307 us a launch for one read in twenty).
        bool generic = false, simple = false, two = false, chk2 = false; // (chk2: a read of two introns whose window check cannot be ruled out)
        u32 dS = 0, a = 0, nl = 0, b2 = 0, nl2 = 0, b3 = 0, meta = 0, off = 0, g = 0;
        if (on) {
            const u32 n = O.n;
            // (what lies behind the read's last operation -- the next read's operations -- is never looked at: every use below is behind a
            // test of n)
            const u32 (&op)[OPS_LDS] = O.op;
            g = b.base + R.r;
            off = R.toff + R.poff;
            meta = read_meta(O.flag, O.xs, O.mapq, pos, O.mtid, O.mpos, tid, orientation);
            const bool seq_ok = (R.sr.w & 0x8000u) != 0;
            // ---- shape: [S] M N M [S], or -- two introns, nothing clamped -- [S] M N M N M [S]
            if (gcodes != nullptr && n >= 3 && n <= 7) {
                const bool clipF = (op[0] & 15u) == OP_S;
                const u32 i0 = clipF ? 1u : 0u;
                const u32 oa = clipF ? op[1] : op[0], on_ = clipF ? op[2] : op[1], ob = clipF ? op[3] : op[2];
                const u32 o3 = clipF ? op[4] : op[3], o4 = clipF ? op[5] : op[4], o5 = clipF ? op[6] : op[5]; // (0 past the last operation)
                two = n >= i0 + 5u && (o3 & 15u) == OP_N;
                const u32 body = i0 + (two ? 5u : 3u);
                const u32 oL = two ? o5 : o3;
                const bool clipL = n == body + 1u && (oL & 15u) == OP_S;
                if (n == body || clipL) {
                    dS = clipF ? op[0] >> 4 : 0u;
                    const u32 dE = clipL ? oL >> 4 : 0u;
                    a = oa >> 4;
                    nl = on_ >> 4;
                    b2 = ob >> 4;
                    nl2 = two ? o3 >> 4 : 0u;
                    b3 = two ? o4 >> 4 : 0u;
                    simple = (oa & 15u) == OP_M && (on_ & 15u) == OP_N && (ob & 15u) == OP_M && a > 0 && b2 > 0 && a <= RES_FIELD_MAX && b2 <= RES_FIELD_MAX &&
                             dS <= RES_FIELD_MAX && lq > 1 && (u64)lq == (u64)dS + a + b2 + b3 + dE && seq_ok;
                    if (two) // (the clamps of junction_system.cc:169-174 are written out for one intron only: an alignment that leaves its target walks)
                        simple = simple && (o4 & 15u) == OP_M && b3 > 0 && b3 <= RES_FIELD_MAX && nl > 0 && nl2 > 0 && pos >= 0 &&
                                 (int64_t)pos + a + nl + b2 + nl2 + b3 <= (int64_t)ref_len;
                }
            }
            two = two && simple;
            chk2 = two && window_reach(b2, nl, nl2, max_span);
            generic = !simple;
        }
        const u32 shard = (chunk >> (8 - K1E_SHIFT)) % GEN_SHARDS;
        const u32 base2 = ctx.list_reserve(2, chk2, 2u, shard), base3 = ctx.list_reserve(3, generic, 0u, shard);
        K1E_MARK(2); // shapes (waits for the operations)
        // ---- in 2 bits: the read is pure ACGT, lies inside its target (nothing clamped: block k of its bases starts at g2s[k]), no block
        // longer than the bitmap load covers.  The exception bitmap under the blocks -- bits g2s >> 6 .. (g2s + len - 1) >> 6, at most 31 of
        // them, in the two words from word g2s >> 11 -- is asked for here and looked at just before the rounds.
        bool use2 = simple && gcodes2 != nullptr && !((O.excw >> (R.r & 31u)) & 1u) && pos >= 0 && (int64_t)pos + a + nl + b2 + nl2 + b3 <= (int64_t)ref_len &&
                    a <= (u32)C2_MAX_BLOCK && b2 <= (u32)C2_MAX_BLOCK && b3 <= (u32)C2_MAX_BLOCK;
        const int64_t n2w = codes2_words(ref_len);
        const bool any_exc = (G.exc_members >> mem) & 1u; // (uniform)
        Words2 x0 = {0, 0}, x1 = {0, 0}, x2 = {0, 0};
        if (use2 && any_exc) {
            const PJB_GLOBAL u32 *gexc = gcodes2 + n2w + K0_CODES2_PAD;
            const u32 g1 = (u32)pos + a + nl;
            x0 = gload_as<Words2>(gexc + ((u32)pos >> 11));
            x1 = gload_as<Words2>(gexc + (g1 >> 11));
            if (two) x2 = gload_as<Words2>(gexc + ((g1 + b2 + nl2) >> 11));
        }
        // the next trips' loads go out before this trip's compares: its list records (two ahead), then the operations and fields (one
        // ahead) -- they are in flight while this trip is compared
        const bool more = v + 1 < v_hi, more2 = v + 2 < v_hi;
        EmitTrip T2 = T1;
        EmitRec R2 = R1;
        EmitOps On = O;
        if (more2) {
            T2 = locate(v + 2);
            R2 = fetch_rec(T2);
        }
        K1E_MARK(4); // records of the trip after the next issued
        if (more) On = fetch_ops(T1, R1);
        K1E_MARK(6); // next operations issued
        // One read's pairs in closed form (junction_system.cc:140-210 for one or two N operations): its blocks of bases compared with
        // gathers, in 2 bits where that is exact and on the 4-bit codes elsewhere.
        const u32 *seqw = (const u32 *)b.seq4 + so;
        const int32_t q_limit = (int32_t)min(seq_words - 1u - so, 0x7fffffffu);
        if (simple) {
            const int32_t vpos = pos + voff;
            const int32_t aend_all = vpos + (int32_t)(a + nl + b2 + nl2 + b3) - 1;
            // ---- the pairs' geometry (junction_system.cc:140-210 for one or two N operations)
            const u32 npairs = two ? 2u : 1u;
            int32_t ist_[2], lst_[2], rend_[2], iend_[2];
            u32 ud_[2];
            {
                int32_t lst = vpos; // the left block of the pair: where it starts, its length; intron; right block
                u32 la = a, ln_ = nl, lb = b2;
#pragma unroll
                for (u32 pr = 0; pr < 2; pr++) {
                    const int32_t istart = lst + (int32_t)la;
                    const int32_t rStartU = istart + (int32_t)ln_;
                    int32_t rStart = rStartU;
                    if (rStart - 1 >= vlen) rStart = vlen - 1; // junction_system.cc:169-171
                    const int32_t iend = rStart - 1;
                    int32_t rEndExc = rStartU + (int32_t)lb;
                    if (rEndExc - 1 >= vlen) rEndExc = vlen; // junction_system.cc:172-174
                    if (pr < npairs && rEndExc - 1 < iend) set_error(err, g, PJB_ERR_MIN_ANCHOR); // intron.cc:76
                    ist_[pr] = istart;
                    lst_[pr] = lst;
                    rend_[pr] = rEndExc - 1;
                    iend_[pr] = iend;
                    // junction.cc:795-812.  One N operation: nothing upstream; "downstream" counts the operation itself unless its end was
                    // clamped.  Two: the first has the second downstream, the second the first upstream.
                    ud_[pr] = two ? (pr == 0 ? (1u << 16) : 1u) : (rStartU <= iend + 1 ? 0u : (1u << 16));
                    lst = rStart;
                    la = lb;
                    ln_ = nl2;
                    lb = b3;
                }
            }
            // ---- the anchors' match statistics: every block of bases is compared once -- the block between two introns is the first
            // pair's right anchor and the second pair's left one.  Block k: read [bq, bq + bl) against the target's [bg, bg + bl).
            const int32_t bq[3] = {(int32_t)dS, (int32_t)(dS + a), (int32_t)(dS + a + b2)};
            const int32_t bg[3] = {lst_[0] - voff, iend_[0] + 1 - voff, iend_[1] + 1 - voff};
            const int32_t bl[3] = {(int32_t)a, rend_[0] - iend_[0], rend_[1] - iend_[1]};
            CmpBlock res[3] = {{bl[0], 0, -1, -1}, {bl[1], 0, -1, -1}, {bl[2], 0, -1, -1}};
            // The gathers, a ROUND at a time, every lane through its own blocks one after the other: a lane with a long left anchor
            // has a short right one, so the wavefront needs max (rounds of all blocks of a lane) iterations where block after block it
            // needed max (rounds of block 0) + max (rounds of block 1) + ...; each iteration is a memory round trip as well.
            const int nb = two ? 3 : 2;
            { // a stretch with a character outside ACGT under one of the blocks: the lane compares on the 4-bit codes
                auto hit = [&](const Words2 &w, int32_t gi, int32_t l) {
                    const u32 b0 = (u32)gi >> 6, cnt = (((u32)(gi + l - 1)) >> 6) - b0 + 1u; // 1 .. 31 stretches
                    const u64 bits = (((u64)1 << cnt) - 1u) << (b0 & 31u);
                    return (((u64)w.x | ((u64)w.y << 32)) & bits) != 0;
                };
                if (any_exc && use2 && (hit(x0, bg[0], bl[0]) || hit(x1, bg[1], bl[1]) || (two && hit(x2, bg[2], bl[2])))) use2 = false;
            }
            if (__ballot(use2)) {
                const u32 *seq2w = (const u32 *)b.seq2 + (so >> 1);
                const int32_t q2_last = (int32_t)min(((seq_words + 1u) >> 1) - 1u - (so >> 1), 0x7fffffffu); // the batch's last word of 2-bit bases, from the read's first
                const int32_t g2_last = (int32_t)(n2w + K0_CODES2_PAD - 1);
                const u32 qodd = (so & 1u) * 16u;
                int k = use2 ? 0 : nb;
                int32_t t = 0;
                u32 mism = 0, fbit = 0xffffffffu, lbit1 = 0;
                for (;;) {
                    const int32_t l = k == 0 ? bl[0] : k == 1 ? bl[1] : bl[2];
                    const bool act = k < nb && t < l;
                    if (act) {
                        const int32_t qi = k == 0 ? bq[0] : k == 1 ? bq[1] : bq[2], gi = k == 0 ? bg[0] : k == 1 ? bg[1] : bg[2];
                        const u32 qbit = qodd + 2u * (u32)(qi + t), gbit = 2u * (u32)(gi + t);
                        u32 qw[C2_NW], gw[C2_NW];
                        const int32_t qf = (int32_t)(qbit >> 5), gf = (int32_t)(gbit >> 5);
                        // a round whose block has 48 bases or fewer left asks for ONE 16-byte gather per stream (the addresser takes a gather a LANE a cycle: lanes
                        // that do not ask cost nothing); the else arm is the path for a batch's last words
                        if (qf + C2_NW - 1 <= q2_last) { // (the genome's words are always there: K0_CODES2_PAD)
                            const Words4 qa = gload(reinterpret_cast<const Words4 *>(seq2w + qf)), ga = gload_as<Words4>(gcodes2 + gf);
                            Words4 qb = {0, 0, 0, 0}, gb = {0, 0, 0, 0};
                            if (l - t > 48) { // (words 4 .. 7 feed the bases from the 49th on)
                                qb = gload(reinterpret_cast<const Words4 *>(seq2w + qf + 4));
                                gb = gload_as<Words4>(gcodes2 + gf + 4);
                            }
                            qw[0] = qa.x, qw[1] = qa.y, qw[2] = qa.z, qw[3] = qa.w, qw[4] = qb.x, qw[5] = qb.y, qw[6] = qb.z, qw[7] = qb.w;
                            gw[0] = ga.x, gw[1] = ga.y, gw[2] = ga.z, gw[3] = ga.w, gw[4] = gb.x, gw[5] = gb.y, gw[6] = gb.z, gw[7] = gb.w;
                        } else {
                            load_words<C2_NW>(qw, seq2w, qf, q2_last);
                            load_words<C2_NW>(gw, (const u32 *)gcodes2, gf, g2_last);
                        }
                        chunk2_cmp_bits<C2_NW>(qw, gw, qbit & 31u, gbit & 31u, l, t, mism, fbit, lbit1);
                        t += C2_ROUND;
                    }
                    if (k < nb && t >= l) { // the lane's block is finished: its results, the next block
                        const int32_t first = (int32_t)fbit >> 1, last = ((int32_t)lbit1 - 1) >> 1; // (-1: no mismatch)
                        if (k == 0) res[0].mism = (int32_t)mism, res[0].first = first, res[0].last = last;
                        if (k == 1) res[1].mism = (int32_t)mism, res[1].first = first, res[1].last = last;
                        if (k == 2) res[2].mism = (int32_t)mism, res[2].first = first, res[2].last = last;
                        k++;
                        t = 0, mism = 0, fbit = 0xffffffffu, lbit1 = 0;
                    }
                    if (!__ballot(k < nb)) break;
                }
            }
            if (__ballot(!use2)) { // ---- on the 4-bit codes (rounds of 56 bases)
                int k = use2 ? nb : 0;
                int32_t t = 0;
                u32 mism = 0, fbit = 0xffffffffu, lbit1 = 0;
                for (;;) {
                    // (blocks without bases -- a clamped end -- are stepped over)
                    const int32_t l = k == 0 ? bl[0] : k == 1 ? bl[1] : bl[2];
                    const bool act = k < nb && t < l;
                    if (act) {
                        const int32_t qi = k == 0 ? bq[0] : k == 1 ? bq[1] : bq[2], gi = k == 0 ? bg[0] : k == 1 ? bg[1] : bg[2];
                        CmpChunkT<SIMPLE_NW> C;
                        chunk_load<SIMPLE_NW, true>(C, seqw, qi, q_limit, (const u32 *)gcodes, gi, g_words, l, t);
                        chunk_cmp_bits<SIMPLE_NW>(C, qi, gi, l, t, mism, fbit, lbit1);
                        t += 8 * (SIMPLE_NW - 1);
                    }
                    if (k < nb && t >= l) { // the lane's block is finished (or empty): its results, the next block
                        const int32_t first = (int32_t)fbit >> 2, last = ((int32_t)lbit1 - 1) >> 2; // (-1: no mismatch)
                        if (k == 0) res[0].mism = (int32_t)mism, res[0].first = first, res[0].last = last;
                        if (k == 1) res[1].mism = (int32_t)mism, res[1].first = first, res[1].last = last;
                        if (k == 2) res[2].mism = (int32_t)mism, res[2].first = first, res[2].last = last;
                        k++;
                        t = 0, mism = 0, fbit = 0xffffffffu, lbit1 = 0;
                    }
                    if (!__ballot(k < nb)) break;
                }
            }
#pragma unroll
            for (u32 pr = 0; pr < 2; pr++) {
                if (pr >= npairs) break;
                PairRec Q;
                Q.lstart = lst_[pr];
                Q.rend = rend_[pr];
                Q.pos = vpos;
                Q.aend = aend_all;
                Q.meta = meta | META_SIMPLE | (two ? META_MULTI : 0u);
                Q.updown = ud_[pr];
                Q.aux = cmp_blocks_res(res[pr], res[pr + 1]);
                const u64 key = make_key(kf, ist_[pr], iend_[pr]);
                P.key[off + pr] = key;
                if (want_g) P.g[off + pr] = g;
                rec_store(P.rec + off + pr, Q);
                if (want_cand) cand_insert(key, Q.lstart, Q.rend);
            }
        }
        const u64 p1_entry = (u64)(E.pack_nn ? R.slot | (2u << 28) : R.slot) | ((u64)off << 32);
        K1E_MARK(7); // compares, records, candidates
        ctx.list_write(2, chk2, base2, p1_entry, shard);
        ctx.list_write(3, generic, base3, (u64)R.slot | ((u64)off << 32), shard); // (the read's place in the tiles' lists, its first pair)
        K1E_MARK(8); // list entries
        // (the candidate set is flushed when the block leaves: a set that fills up before that sends its keys straight to the list --
        // cand_insert -- and no barrier ties the block's wavefronts together trip by trip)
        if (!more) ctx.cand_flush(true);
        K1E_MARK(9); // candidate flush (barrier)
        T = T1;
        R = R1;
        O = On;
        T1 = T2;
        R1 = R2;
    }
}

// The reads k1_emit did not finish (three and more introns, indels, = X P H operations, clamped ends, exotic targets, SEQ '*'):
// a thread per read of the chain's third list, dense.  The read's operations are walked (emit_read_pairs): keys and records
// of its pairs, candidates, and -- for [S] B (N B)+ [S] -- the blocks' compares; then the read goes on one of k4b_generic's
// lists: the walks', or -- closed, and a window can reach over one of its introns (window_reach) -- the window check's; a closed
// read that no window can reach is finished here.  One launch per chain, behind the chain's k1_emit launches.
__global__ __launch_bounds__(K1E_T) void k1_generic(const DevBatch *batches, int n_batches, const u32 *spl_idx, const uint4 *spl_rec, Pairs P, EmitLists E, KeyFmt kf,
                                                    GroupTab G, int use_codes, int orientation, u64 *err, ContigStats *cs) {
    __shared__ EmitShared sh;
    __shared__ u32 s_ops[OPS_LDS][K1E_T];
    __shared__ u32 s_first[GEN_SHARDS + 1];
    __shared__ u32 s_wsum[4];
    __shared__ BatchTab s_bt;
    if (cs->P == 0) return;
    const u32 max_span = cs->max_span;
    const bool want_cand = E.cand != nullptr;
    EmitCtx ctx{sh, E, kf, cs, want_cand};
    ctx.init();
    static_assert(GEN_SHARDS == K1E_T, "a sub-list per thread");
    {
        const u32 c = E.gen_cnt[threadIdx.x * GEN_CNT_STRIDE + 4];
        s_bt.fill(batches, n_batches);
        u32 total;
        const u32 ex = block_escan<K1E_T / 64>(c < E.gen_cap ? c : E.gen_cap, s_wsum, &total);
        s_first[threadIdx.x] = ex;
        if (threadIdx.x == K1E_T - 1) s_first[GEN_SHARDS] = total;
        __syncthreads();
    }
    const u32 n_items = s_first[GEN_SHARDS];
    for (u32 item0 = blockIdx.x * K1E_T; item0 < n_items; item0 += gridDim.x * K1E_T) {
        const u32 item = item0 + threadIdx.x;
        u32 gen_pairs = 0, gen_kind = 0;
        u64 gen_entry = 0;
        if (item < n_items) {
            u32 sub = 0; // the last sub-list with s_first[sub] <= item
#pragma unroll
            for (u32 step = GEN_SHARDS / 2; step > 0; step >>= 1)
                if (sub + step < GEN_SHARDS && s_first[sub + step] <= item) sub += step;
            const u64 e3 = E.gen_list[((size_t)2 * GEN_SHARDS + sub) * E.gen_cap + (item - s_first[sub])];
            const u32 slot = (u32)e3;
            const int bi = s_bt.find(batches, n_batches, slot / (u32)K1_TILE);
            const DevBatch &b = batches[bi];
            const u32 r = spl_idx[slot];
            const uint4 sr = spl_rec[slot];
            const int m = b.member;
            const int32_t voff = G.voff[m], ref_len = G.len[m], vlen = voff + ref_len;
            const u32 *gcodes = use_codes ? G.codes[m] : (const u32 *)nullptr;
            EmitRead R;
            R.n = sr.w & 0x7fffu;
            if (R.n == 0x7fffu) R.n = gload(b.cig_off + r + 1) - sr.x;
            R.lq = (int32_t)(sr.w >> 16);
            if (R.lq == 0xffff) R.lq = gload(b.l_qseq + r);
            const int32_t pos = (int32_t)sr.y;
            R.pos = pos + voff;
            R.g = b.base + r;
            R.meta = read_meta(gload(b.flag + r), (u32)gload(b.xs + r), gload(b.mapq + r), pos, gload(b.mtid + r), gload(b.mpos + r), G.tid[m], orientation);
            R.seq_ok = (sr.w & 0x8000u) != 0;
            R.off = (u32)(e3 >> 32);
            OpsViewT<K1E_T, OPS_LDS> cig;
            cig.g = b.cigar + sr.x;
            cig.lds = &s_ops[0][threadIdx.x];
            {
                u32 w[OPS_LDS];
                fetch_ops8(as_global(b.cigar), sr.x, s_bt.cig_words(b, bi), w);
#pragma unroll
                for (int q = 0; q < OPS_LDS; q++) s_ops[q][threadIdx.x] = (u32)q < R.n ? w[q] : 0u;
            }
            // operations counted, and the shape [S] B (N B)+ [S] recognised, B = M = X I D operations that begin and end with bases on
            // both sides: state 0 at the first operation, 5 after a leading S, 1 after M = X, 6 after I or D, 2 after an N, 3 after the
            // closing S, 4 any other shape
            u32 nN = 0, shape = 0;
            int32_t aligned = 0;
            int64_t qsum = 0, bsum = 0; // query bases; positions the walks emit for the current block
            u32 bref = 0, nl_prev = 0;  // reference positions of the current block; the N operation before it
            bool reach = max_span == 0xffffffffu; // a window can reach over one of the read's introns from the next one (window_reach; no bound: every closed read)
            for (u32 q = 0; q < R.n; q++) {
                const u32 o = cig[q], ty = o & 15u, ln = o >> 4;
                if (ty == OP_N) {
                    if (nN > 0) reach = reach || window_reach(bref, nl_prev, ln, max_span);
                    nl_prev = ln;
                    bref = 0;
                } else if (op_consumes_ref(ty))
                    bref = __builtin_elementwise_add_sat(bref, ln);
                nN += (ty == OP_N);
                if (op_consumes_ref(ty)) aligned += (int32_t)ln;
                if (op_consumes_query(ty)) qsum += ln;
                const bool len_ok = ln > 0 && ln <= RES_FIELD_MAX;
                if (ty == OP_M || ty == OP_EQ || ty == OP_X) shape = (shape == 0 || shape == 5 || shape == 2 || shape == 1 || shape == 6) && len_ok ? 1u : 4u;
                else if (ty == OP_I || ty == OP_D) shape = shape == 1 && len_ok ? 6u : 4u;
                else if (ty == OP_N) shape = shape == 1 && ln > 0 ? 2u : 4u;
                else if (ty == OP_S) shape = shape == 0 && len_ok ? 5u : shape == 1 && q + 1 == R.n ? 3u : 4u;
                else shape = 4;
                bsum = ty == OP_N ? 0 : ty == OP_S ? bsum : bsum + ln;
                if (bsum > (int64_t)RES_FIELD_MAX) shape = 4;
            }
            if (nN > 1) R.meta |= META_MULTI;
            R.nN = nN;
            R.aend = R.pos + aligned - 1;
            // (nothing clamped: the alignment lies inside its target -- junction_system.cc:169-174)
            const bool closed = gcodes != nullptr && (shape == 1 || shape == 3) && nN > 0 && R.seq_ok && R.lq > 1 && qsum == (int64_t)R.lq &&
                                R.pos >= voff && R.aend < vlen;
            R.closed_seqw = closed ? reinterpret_cast<const u32 *>(b.seq4) + sr.z : nullptr;
            R.q_limit = (int32_t)min(s_bt.seq_words(b, bi) - 1u - sr.z, 0x7fffffffu);
            R.gcodes = gcodes;
            R.glen = ref_len;
            R.voff = voff;
            emit_read_pairs(cig, R, P, kf, vlen, err, [&](u64 key, int32_t lstart, int32_t rend) { ctx.cand_insert(key, lstart, rend); });
            gen_pairs = nN;
            gen_kind = !closed ? 1u : reach ? 2u : 0u; // (closed, no window can reach: its pairs are finished)
            gen_entry = (u64)(closed && E.pack_nn ? slot | ((nN < 15u ? nN : 15u) << 28) : slot) | ((u64)R.off << 32);
        }
        // the read goes on k4b_generic's first list (the walks) or on its second (closed form done, window to be checked)
        const u32 shard = (item0 >> K1E_SHIFT) % GEN_SHARDS;
        ctx.list_append(1, gen_kind == 1, gen_pairs, gen_entry, shard);
        ctx.list_append(2, gen_kind == 2, gen_pairs, gen_entry, shard);
        ctx.cand_flush(item0 + gridDim.x * K1E_T >= n_items);
    }
}

// per-member counters of a group, from the tile statistics of the member's tiles (before k1_scan_tiles turns the tile pair
// counts into offsets): one block per member
// (behind k1_scan_tiles and off the chain's K1 stage: a member's pairs are the difference of the scanned counts at its first tile and
// the next member's)
__global__ __launch_bounds__(256) void kg_member_stats(const u32 *tile_off, const TileStats *ts, const u32 *tile_lo, int n_members, MemberStats *out, u32 n_tiles,
                                                       const ContigStats *cs) {
    __shared__ u64 sm[4][4];
    __shared__ int32_t smi[4][2];
    const int m = blockIdx.x;
    if (m >= n_members) return;
    u64 spl = 0, uns = 0, sum = 0, pairs = 0;
    int32_t mn = INT32_MAX, mx = 0;
    for (u32 t = tile_lo[m] + threadIdx.x; t < tile_lo[m + 1]; t += 256) {
        const TileStats x = ts[t];
        spl += x.spliced;
        uns += x.unspliced;
        sum += x.sum_len;
        mn = min(mn, x.min_len);
        mx = max(mx, x.max_len);
    }
    spl = wave_sum(spl);
    uns = wave_sum(uns);
    sum = wave_sum(sum);
    {
        const u32 t0 = tile_lo[m], t1 = tile_lo[m + 1], total = (u32)cs->n_pairs;
        pairs = threadIdx.x == 0 ? (u64)((t1 < n_tiles ? tile_off[t1] : total) - (t0 < n_tiles ? tile_off[t0] : total)) : 0ull;
    }
    mn = wave_min(mn);
    mx = wave_max(mx);
    const int w = threadIdx.x >> 6;
    if (lane_id() == 0) {
        sm[w][0] = spl;
        sm[w][1] = uns;
        sm[w][2] = sum;
        sm[w][3] = pairs;
        smi[w][0] = mn;
        smi[w][1] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        MemberStats S;
        S.spliced = sm[0][0] + sm[1][0] + sm[2][0] + sm[3][0];
        S.unspliced = sm[0][1] + sm[1][1] + sm[2][1] + sm[3][1];
        S.sum_len = sm[0][2] + sm[1][2] + sm[2][2] + sm[3][2];
        S.n_pairs = sm[0][3] + sm[1][3] + sm[2][3] + sm[3][3];
        S.min_len = min(min(smi[0][0], smi[1][0]), min(smi[2][0], smi[3][0]));
        S.max_len = max(max(smi[0][1], smi[1][1]), max(smi[2][1], smi[3][1]));
        S.n_junc = 0; // (counted by k5_finalize)
        S._pad = 0;
        out[m] = S;
    }
}

} // namespace pjb

#include "pjb_k2d_ids.hip.h"  // K2d  kd_*
#include "pjb_k2_sort.hip.h"   // K2   rs_*
#include "pjb_k2s_runs.hip.h"  // K2s  k2_*, kf_*
#include "pjb_k4_pairs.hip.h"  // K4b, K4, K5a  k4b_generic, k4_pairs, k5_frag_reduce

namespace pjb {

// ---------------------------------------------------------------------------------------------
// K5b: one thread per junction: strand from reads, entropy over position runs, splice motif,
// hamming scores, suspicious flag -> output row.
// ---------------------------------------------------------------------------------------------

// Entropy terms, one thread per position run: p*log2(p) with the reference's grouping
// (junction.cc:730-749): with runs r_0..r_m of equal read position the flush rule yields the counts
// (r_0+1, r_1, ..., r_{m-1}, r_m-1); a zero count contributes nothing.  k5_finalize adds the terms
// of a junction sequentially, in run order, so the sum rounds like the reference's loop.
// Entropy of a junction (junction.cc:730-749) = |sum over its position runs of p log2 p|, p = run length / pairs of the junction
// with the reference's grouping (first run + 1, last run - 1 when there are several), added one after the other in run
// order so that the sum rounds like the reference's loop (:742-748).  Sixteen lanes per junction: 16 runs at a time -- each
// lane its run's term from two neighbouring run starts -- folded in lane order (the chain of dependent adds is the
// reference's, there is no chain of dependent loads).  (The terms had a kernel and an array of their own until
// round 4.)
__global__ __launch_bounds__(256) void k5_entropy_sum(const u32 *seg_off, const u32 *run_first, const u32 *run_start, const u32 *n_junc_p,
                                                       double *ent_sum) {
    // sixteen lanes per junction, four junctions per wavefront: most junctions have a handful of runs (a whole wavefront each spent
    // its time on 60 idle lanes), the deep ones a hundred or two (read positions within a read length of the intron)
    const int lane = lane_id(), sl = lane & 15;
    const u32 j = ((blockIdx.x * 4 + (threadIdx.x >> 6)) << 2) + (u32)(lane >> 4);
    const bool valid = j < *n_junc_p;
    const u32 rf = valid ? run_first[j] : 0u, rl = valid ? run_first[j + 1] : 0u;
    const u32 n = valid ? seg_off[j + 1] - seg_off[j] : 0u;
    double sum = 0.0;
    for (u32 r0 = rf; __any(r0 < rl); r0 += 16) {
        const u32 r = r0 + (u32)sl;
        double t = 0.0;
        if (r < rl) {
            u32 c = run_start[r + 1] - run_start[r];
            if (rl - rf > 1) {
                if (r == rf) c += 1;
                else if (r == rl - 1) c -= 1;
            }
            if (c != 0 && n > 1) {
                const double pI = (double)c / (double)n;
                t = __dmul_rn(pI, log2(pI));
            }
        }
        const u32 cnt = r0 < rl ? (rl - r0 < 16u ? rl - r0 : 16u) : 0u;
#pragma unroll
        for (u32 k = 0; k < 16; k++) { // (in run order: the sum rounds like the reference's loop)
            const double v = __shfl(t, (int)k, 16);
            if (k < cnt) sum = __dadd_rn(sum, v);
        }
    }
    if (valid && sl == 0) ent_sum[j] = sum;
}

__global__ __launch_bounds__(256) void k5_finalize(const u64 *jkey, const u32 *seg_off, const u32 *run_first,
                                                    const u32 *run_start, const u32 *acc, const int32_t *anc_l,
                                                    const int32_t *anc_r, KeyFmt kf, GroupTab G, const u32 *n_junc_p, const double *ent_sum,
                                                    pjb_junction_row *rows, u64 *err, u32 *member_junc) {
    const u32 n_junc = *n_junc_p;
    const u32 j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_junc) return;
    const u32 *a = acc + (size_t)j * F_WORDS;
    pjb_junction_row R;
    memset(&R, 0, sizeof R);
    int32_t istart, iend;
    unpack_key(kf, jkey[j], istart, iend);
    // the junction's target: rows carry the target's own coordinates
    const Member M = member_of(G, istart);
    const uint8_t *genome = M.d;
    const int32_t glen = M.len;
    istart -= M.voff;
    iend -= M.voff;
    if (G.n > 1) { // junctions per member: neighbouring junctions share their member, so one add per wavefront and member
        const int m0 = __builtin_amdgcn_readfirstlane(M.idx);
        const u64 same = __ballot(M.idx == m0);
        if (M.idx == m0) {
            if (lane_id() == __ffsll((long long)same) - 1) atomicAdd(&member_junc[m0], (u32)__popcll(same));
        } else
            atomicAdd(&member_junc[M.idx], 1u);
    }
    R.refid = M.tid;
    R.start = istart;
    R.end = iend;
    R.left = anc_l[j] - M.voff;
    R.right = anc_r[j] - M.voff;
    const u32 n = a[F_N];
    R.nb_raw = n;
    R.nb_dist = a[F_DIST];
    R.nb_ms = a[F_MS];
    R.nb_um = a[F_UM];
    R.nb_bpp = a[F_BPP];
    R.nb_ppp = a[F_PPP];
    R.nb_rel = a[F_REL];
    R.r1pos = a[F_R1P];
    R.r1neg = a[F_R1N];
    R.r2pos = a[F_R2P];
    R.r2neg = a[F_R2N];
    R.max_min_anc = a[F_MAXMINANC];
    R.maxmmes = a[F_MAXMMES];
    R.nb_up_juncs = a[F_UP];
    R.nb_down_juncs = a[F_DOWN];
    const u64 mism = (u64)a[F_MISM_LO] | ((u64)a[F_MISM_HI] << 32);
    R.sum_mismatches = mism;
    for (int k = 0; k < 20; k++) R.jad[k] = a[F_JAD0 + k];
    // suspicious, junction.cc:897-908.  (nbMismatches is a uint32 in the reference; the test is > 0)
    {
        const u32 first_mis = a[F_FIRSTMIS];
        if ((u32)mism > 0 && first_mis < 20 && !(a[F_MAXMINMATCH] > first_mis)) R.suspicious = 1;
    }
    // determineStrandFromReads, junction.cc:531-559
    {
        const u32 np = a[F_XSP], nn = a[F_XSN];
        const double tot = (double)n;
        if ((double)np / tot >= 0.95) R.read_strand = PJB_STRAND_POS;
        else if ((double)nn / tot >= 0.95) R.read_strand = PJB_STRAND_NEG;
        else R.read_strand = PJB_STRAND_UNK;
    }
    // calcEntropy, junction.cc:730-749: the per-run terms summed in run order (k5_entropy_sum), then fabs
    R.entropy = n > 1 ? fabs(ent_sum[j]) : 0.0;
    // processJunctionWindow, junction.cc:561-649
    {
        int32_t b = istart, e = istart + 1;
        fetch_clamp(glen, b, e);
        int32_t b2 = iend - 1, e2 = iend;
        fetch_clamp(glen, b2, e2);
        if (e - b + 1 != 2 || e2 - b2 + 1 != 2 || glen <= 0) {
            set_error(err, 0xffffff00u + 0, PJB_ERR_SPLICE_SITE_LEN);
            rows[j] = R;
            return;
        }
        uint8_t d0 = genome[b], d1 = genome[b + 1], a0 = genome[b2], a1 = genome[b2 + 1];
        const u32 m4 = ((u32)d0 << 24) | ((u32)d1 << 16) | ((u32)a0 << 8) | (u32)a1;
        const u32 GTAG = 0x47544147u, CTAC = 0x43544143u, ATAC = 0x41544143u, GTAT = 0x47544154u, GCAG = 0x47434147u,
                  CTGC = 0x43544743u;
        int css, ss;
        if (m4 == GTAG || m4 == CTAC) css = PJB_CSS_CANONICAL;
        else if (m4 == ATAC || m4 == GTAT || m4 == GCAG || m4 == CTGC) css = PJB_CSS_SEMI;
        else css = PJB_CSS_NO;
        if (m4 == GTAG || m4 == ATAC || m4 == GCAG) ss = PJB_STRAND_POS;
        else if (m4 == CTAC || m4 == GTAT || m4 == CTGC) ss = PJB_STRAND_NEG;
        else ss = PJB_STRAND_UNK;
        const int rs = R.read_strand;
        const int cons = rs == ss ? rs : rs == PJB_STRAND_UNK ? ss : ss == PJB_STRAND_UNK ? rs : PJB_STRAND_UNK;
        R.canonical = (uint8_t)css;
        R.ss_strand = (uint8_t)ss;
        R.cons_strand = (uint8_t)cons;
        if (cons == PJB_STRAND_NEG) {
            R.da1[0] = revcomp_char(a1);
            R.da1[1] = revcomp_char(a0);
            R.da2[0] = revcomp_char(d1);
            R.da2[1] = revcomp_char(d0);
        } else {
            R.da1[0] = d0;
            R.da1[1] = d1;
            R.da2[0] = a0;
            R.da2[1] = a1;
        }
        // anchors / intron flanks
        int32_t lb = R.left, le = istart - 1;
        fetch_clamp(glen, lb, le);
        int32_t rb = iend + 1, re = R.right;
        fetch_clamp(glen, rb, re);
        int32_t lib = istart, lie = istart + 9;
        fetch_clamp(glen, lib, lie);
        int32_t rib = iend - 9, rie = iend;
        fetch_clamp(glen, rib, rie);
        const int32_t leftAncLen = le - lb + 1, rightAncLen = re - rb + 1;
        const int32_t expL = istart - R.left, expR = R.right - iend;
        if ((leftAncLen != expL && expL > 0) || (rightAncLen != expR && expR > 0)) {
            set_error(err, 0xffffff00u + 1, PJB_ERR_ANCHOR_LEN);
            rows[j] = R;
            return;
        }
        if (lie - lib + 1 != 10 || rie - rib + 1 != 10) {
            set_error(err, 0xffffff00u + 2, PJB_ERR_INTRON_FLANK_LEN);
            rows[j] = R;
            return;
        }
        // calcHammingScores, junction.cc:823-857
        const int32_t nla = leftAncLen < 10 ? leftAncLen : 10;  // last <=10 of left anchor
        const int32_t la_b = leftAncLen < 10 ? lb : le - 9;
        const int32_t nra = rightAncLen < 10 ? rightAncLen : 10; // first <=10 of right anchor
        const int32_t ra_b = rb;
        const int32_t nli = 10, nri = 10;
        const int32_t leftDelta = nla - nri;
        const int32_t leftOffset = leftDelta <= 0 ? 0 : leftDelta;
        const int32_t leftLen = nla < nri ? nla : nri;
        const int32_t rightLen = nli < nra ? nli : nra;
        // la' = nla > leftLen ? la.substr(leftOffset,leftLen) : la   (nla <= 10 = nri so never longer)
        const int32_t zla = nla, la_o = 0;
        const int32_t zli = nli > rightLen ? rightLen : nli, li_o = 0;
        const int32_t zri = nri > leftLen ? leftLen : nri, ri_o = nri > leftLen ? leftOffset : 0;
        const int32_t zra = nra > rightLen ? rightLen : nra, ra_o = 0;
        (void)la_o; (void)li_o; (void)ra_o;
        u32 h5 = 0, h3 = 0;
        if (zla != zri || zra != zli) {
            set_error(err, 0xffffff00u + 3, PJB_ERR_HAMMING_LEN);
            rows[j] = R;
            return;
        }
        if (cons == PJB_STRAND_NEG) {
            // anchor5p = rc(ra), intron3p = rc(li): H over reversed+complemented strings
            for (int32_t t = 0; t < zra; t++) {
                const uint8_t x = revcomp_char(genome[ra_b + (zra - 1 - t)]);
                const uint8_t y = revcomp_char(genome[lib + (zli - 1 - t)]);
                h5 += x != y;
            }
            for (int32_t t = 0; t < zla; t++) {
                const uint8_t x = revcomp_char(genome[la_b + (zla - 1 - t)]);
                const uint8_t y = revcomp_char(genome[rib + ri_o + (zri - 1 - t)]);
                h3 += x != y;
            }
        } else {
            for (int32_t t = 0; t < zla; t++) h5 += genome[la_b + t] != genome[rib + ri_o + t];
            for (int32_t t = 0; t < zra; t++) h3 += genome[ra_b + t] != genome[lib + t];
        }
        R.hamming5p = h5;
        R.hamming3p = h3;
    }
    rows[j] = R;
}

// K6: the contig's rows leave the device inside the kernel chain -- the host does not know the row count when it
// queues the work, so it cannot size a copy: 8-byte units go straight into page-locked host memory (mapped into the
// device's address space; consecutive lanes write consecutive addresses, PCIe posted writes) and, if the caller set a
// row mirror, into its exchange slot; the control block follows as the last thing on the stream.
constexpr int ROW_U64 = (int)(sizeof(pjb_junction_row) / 8);
static_assert(sizeof(pjb_junction_row) % 8 == 0, "rows are copied in 8-byte units");
// Where a contig's rows go is known to the host only when the contigs before it have been collected.  With two contigs
// queued (pjb_finish_contig_begin) the second one's place follows from the first one's junction count, which lives on
// the device: a cursor (rows written so far: host table, exchange slot), read by k6_rows_out and advanced by
// publish_chain (the last block of k6_rows_out), on the rows stream and so in contig order.  base < 0: take the cursor.
struct RowCursor {
    u32 rows, mirror_rows;
    u32 blocks_done; // k6_rows_out: blocks of the running launch that have written their rows (0 at rest)
    u32 _pad;
};
__device__ __forceinline__ void publish_chain(const ContigStats *cs, u64 *err, u32 *gen_cnt, uint8_t *host, int64_t base, int64_t mirror_base,
                                              RowCursor *cur, const MemberStats *members, u32 *member_junc, int n_members);
// Rows -> the row table, then -- the block that finishes last -- the chain's control block -> page-locked host memory, rest
// states restored, the cursor advanced (publish_chain; a launch of its own until round 4).  The rows stream runs these
// launches one after the other, so one counter in the cursor serves every slot.
__global__ __launch_bounds__(256) void k6_rows_out(const u64 *rows, const ContigStats *cs, u64 *host_table, int64_t base, int64_t mirror_base,
                                                   RowCursor *cur, u64 *mirror_table, u32 mirror_room, u64 *err, u32 *gen_cnt, uint8_t *host_pub,
                                                   const MemberStats *members, u32 *member_junc, int n_members) {
    // a grid of a few dozen blocks walks the rows: the kernel runs beside the next contig's first kernels, its stores
    // wait on PCIe, and it should not sit on their wave slots meanwhile
    const u32 nj = cs->J;
    const u64 n = (u64)nj * ROW_U64;
    const u64 at = base >= 0 ? (u64)base : (u64)cur->rows;
    const u64 mat = mirror_base >= 0 ? (u64)mirror_base : (u64)cur->mirror_rows;
    const bool to_mirror = mirror_table && mat + nj <= (u64)mirror_room; // (the slot is left alone by a contig that does not fit: the host reports it)
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u64 v = rows[i];
        host_table[at * ROW_U64 + i] = v;
        if (to_mirror) mirror_table[mat * ROW_U64 + i] = v;
    }
    __shared__ u32 s_last;
    // (The rows -- host memory, and a mirror that may be a peer's -- must be out before the control block that announces them: a
    // system-scope fence in every block before it counts itself done, and once more in the last block before it publishes.  Today
    // every consumer waits for the stream's event; a consumer that polls the control block would see the rows too.  The one
    // blocks_done counter serves every slot because the rows stream runs these launches one after the other.)
    __threadfence_system();
    __syncthreads(); // (every thread of the block has read the cursor)
    if (threadIdx.x == 0) s_last = atomicAdd(&cur->blocks_done, 1u) + 1u == gridDim.x ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    __threadfence_system();
    if (threadIdx.x == 0) cur->blocks_done = 0;
    publish_chain(cs, err, gen_cnt, host_pub, base, mirror_base, cur, members, member_junc, n_members);
}

// The last kernel of a contig: control block, error word and list counters go to page-locked host memory in one go
// (three small copies otherwise), error word and counters return to their rest state for the contig that uses this
// control slot next, and the row cursor moves on.
__device__ __forceinline__ void publish_chain(const ContigStats *cs, u64 *err, u32 *gen_cnt, uint8_t *host, int64_t base, int64_t mirror_base,
                                              RowCursor *cur, const MemberStats *members, u32 *member_junc, int n_members) {
    const u32 t = threadIdx.x;
    if (n_members > 1 && t < (u32)n_members) { // a group: the members' own counters
        MemberStats S = members[t];
        S.n_junc = member_junc[t];
        reinterpret_cast<MemberStats *>(host + PUB_MEMBERS_AT)[t] = S;
    }
    static_assert(sizeof(ContigStats) % 8 == 0 && sizeof(ContigStats) <= PUB_BASE_AT, "control block layout");
    static_assert(PUB_GEN_AT + GEN_SHARDS * 4 <= PUB_MEMBERS_AT && PUB_MEMBERS_AT + GROUP_MAX * sizeof(MemberStats) <= PUB_GREADS_AT &&
                      PUB_GREADS_AT + GEN_SHARDS * 4 <= PUB_BYTES,
                  "control block layout");
    if (t < sizeof(ContigStats) / 8) reinterpret_cast<u64 *>(host)[t] = reinterpret_cast<const u64 *>(cs)[t];
    __shared__ u32 s_chk[4];
    {
        const u32 chk = wave_total<DppAdd>(t < GEN_SHARDS ? gen_cnt[t * GEN_CNT_STRIDE + 2] : 0u);
        if (lane_id() == 0) s_chk[t >> 6] = chk;
    }
    if (t < GEN_SHARDS) { // pairs that took the generic walks, per sub-list; both counters back to their rest state
        reinterpret_cast<u32 *>(host + PUB_GEN_AT)[t] = gen_cnt[t * GEN_CNT_STRIDE + 1];
        reinterpret_cast<u32 *>(host + PUB_GREADS_AT)[t] = gen_cnt[t * GEN_CNT_STRIDE];
        reinterpret_cast<uint4 *>(gen_cnt + t * GEN_CNT_STRIDE)[0] = make_uint4(0, 0, 0, 0);
        reinterpret_cast<uint4 *>(gen_cnt + t * GEN_CNT_STRIDE)[1] = make_uint4(0, 0, 0, 0); // (the third list's)
    }
    if (t == 0) {
        *reinterpret_cast<u64 *>(host + PUB_ERR_AT) = *err;
        *err = ~0ull;
        const u32 at = base >= 0 ? (u32)base : cur->rows, mat = mirror_base >= 0 ? (u32)mirror_base : cur->mirror_rows;
        reinterpret_cast<u32 *>(host + PUB_BASE_AT)[0] = at;
        reinterpret_cast<u32 *>(host + PUB_BASE_AT)[1] = mat;
        cur->rows = at + cs->J;
        cur->mirror_rows = mat + cs->J;
    }
    __syncthreads();
    if (t < (u32)GROUP_MAX) member_junc[t] = 0; // (k5_finalize counts into it; rest state for the chain that uses the slot next)
    if (t == 0) *reinterpret_cast<u32 *>(host + PUB_CHECKED_AT) = s_chk[0] + s_chk[1] + s_chk[2] + s_chk[3];
}

} // namespace pjb
