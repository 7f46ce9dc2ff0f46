// pjb_basecmp.hip.h -- shared by k1_emit, k1_generic and k4b_generic: packed read bases (4 bits, high nibble first) against packed genome
// codes (4 bits, low nibble first), a chunk of words at a time.  No kernel; whoever compares bases includes it.
#pragma once

#include "pjb_device.hip.h"

namespace pjb {

// ---------------------------------------------------------------------------------------------
// Packed-base compare helpers (used by k1_emit for the simple shape and by the generic walks of k4b_generic)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 nt16_ascii(u32 c) { // seq_nt16_str "=ACMGRSVTWYHKDBN"
    // bytes: '=' 3D, 'A' 41, 'C' 43, 'M' 4D, 'G' 47, 'R' 52, 'S' 53, 'V' 56 | 'T' 54,'W' 57,'Y' 59,'H' 48,'K' 4B,'D' 44,'B' 42,'N' 4E
    const u64 t0 = 0x565352474D43413DULL;
    const u64 t1 = 0x4E42444B48595754ULL;
    const u64 t = (c & 8u) ? t1 : t0;
    return (u32)(t >> ((c & 7u) * 8)) & 0xffu;
}

// Read nibbles [qi, qi+l) (BAM order: high nibble first) against genome codes [gi, gi+l) (low nibble first), 64 bases
// = 9 words of each per round; mismatch positions are reported relative to `out_base`.
//   A lane's words are consecutive but the next lane's are somewhere else, so every load instruction of the wave
// touches 64 cache lines whatever its width, and the number of load INSTRUCTIONS sets the pace (measured in
// k4a_simple: 19 per-word loads per read cost 80 us per contig, the compare itself nothing).  So the words come as two
// 16-byte loads and one 4-byte load per stream -- 4-byte aligned (reads start on word boundaries), which
// global_load_dwordx4 accepts -- guarded so that nothing is read past the read's last word / the contig's last code
// word; the short tail of a stream takes guarded word loads.
__device__ __forceinline__ u32 swap_nibbles(u32 x) { return ((x & 0x0F0F0F0Fu) << 4) | ((x >> 4) & 0x0F0F0F0Fu); }
// A chunk = NW consecutive words of each stream = (NW - 1) * 8 anchor bases per round (the extra word feeds the funnel
// shift of the last one): NW = 9 -> two 16-byte loads and one word per stream, NW = 5 -> one 16-byte load and one word.
template <int NW>
struct CmpChunkT {
    u32 qw[NW], gg[NW];
};
// d[k] = p[first + k] for 0 <= first + k <= last, else 0
template <int NW>
__device__ __forceinline__ void load_words(u32 (&d)[NW], const u32 *p, int32_t first, int32_t last) {
    static_assert(NW == 9 || NW == 8 || NW == 5, "chunk width");
    if (first >= 0 && first + NW - 1 <= last) {
        const Words4 a = gload(reinterpret_cast<const Words4 *>(p + first));
        d[0] = a.x, d[1] = a.y, d[2] = a.z, d[3] = a.w;
        if constexpr (NW >= 8) {
            const Words4 b = gload(reinterpret_cast<const Words4 *>(p + first + 4));
            d[4] = b.x, d[5] = b.y, d[6] = b.z, d[7] = b.w;
        }
        if constexpr (NW != 8) d[NW - 1] = gload(p + first + NW - 1); // (NW = 8: two 16-byte loads and nothing else -- 56 bases a round)
    } else {
#pragma unroll
        for (int k = 0; k < NW; k++) d[k] = (first + k >= 0 && first + k <= last) ? gload(p + first + k) : 0u;
    }
}
// anchor bases [t, t + 8 (NW - 1)) of an anchor of l bases: read bases from qi (words of the read up to word q_last may be
// touched: whatever lies past the anchor only feeds bits that the length mask removes), genome from gi
// TO_BUFFER_END: q_last is the last word of the batch's bases (relative to the read) and the genome may be read up to its last
// code word, not only to the anchor's: the last round of an anchor then takes the 16-byte loads too instead of one guarded
// load per word (what lies past the anchor is masked either way).
template <int NW, bool TO_BUFFER_END = false>
__device__ __forceinline__ void chunk_load(CmpChunkT<NW> &C, const u32 *seqw, int32_t qi, int32_t q_last, const u32 *gw, int32_t gi, int32_t g_words,
                                           int32_t l, int32_t t) {
    const int32_t lastg = (gi + l - 1) >> 3;
    load_words<NW>(C.qw, seqw, (qi + t) >> 3, q_last);
    // (genome words outside [0, g_words) and -- but for TO_BUFFER_END -- past the anchor's last word read as 0, as they always did)
    load_words<NW>(C.gg, gw, (gi + t) >> 3, !TO_BUFFER_END && lastg < g_words - 1 ? lastg : g_words - 1);
}
template <int NW>
__device__ __forceinline__ void chunk_cmp(CmpChunkT<NW> &C, int32_t qi, int32_t gi, int32_t l, int32_t t, int32_t out_base, int32_t &mism,
                                          int32_t &first_mis, int32_t &last_mis) {
    const u32 shq = (u32)(qi & 7) * 4u, shg = (u32)(gi & 7) * 4u; // (t is a multiple of 8: the shifts do not move)
#pragma unroll
    for (int k = 0; k < NW; k++) C.qw[k] = swap_nibbles(C.qw[k]);
#pragma unroll
    for (int c = 0; c < NW - 1; c++) {
        const int32_t rem = l - t - 8 * c;
        if (rem > 0) {
            const u32 q = __builtin_amdgcn_alignbit(C.qw[c + 1], C.qw[c], shq);
            const u32 g = __builtin_amdgcn_alignbit(C.gg[c + 1], C.gg[c], shg);
            const u32 x = q ^ g;
            u32 m = (((x & 0x77777777u) + 0x77777777u) | x) & 0x88888888u; // top bit of every nibble that differs
            if (rem < 8) m &= (1u << (4 * rem)) - 1u;
            if (m) {
                mism += __popc(m);
                if (first_mis < 0) first_mis = out_base + t + 8 * c + ((__ffs((int)m) - 1) >> 2);
                last_mis = out_base + t + 8 * c + ((31 - __clz((int)m)) >> 2);
            }
        }
    }
}
// v_ffbl_b32 / v_ffbh_u32 as the hardware defines them: 0xffffffff for 0 (the language's count-zeros builtins leave 0 undefined or
// cost a second instruction)
__device__ __forceinline__ u32 ffbl_hw(u32 x) {
    u32 r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ u32 ffbh_hw(u32 x) {
    u32 r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
// chunk_cmp without a branch: the words' flags (top bit of every nibble that differs) are cut to the anchor's length by a shift pair
// (no compare / select, nothing skipped), and the first / last mismatch are kept as BIT positions 4 * base + 3 from the anchor's
// start -- fbit: the lowest (0xffffffff: none), lbit1: the highest + 1 (0: none) -- folded with saturating adds and min / max, which
// make a word without mismatches neutral (v_ffbl / v_ffbh return 0xffffffff for it).  base = (int32_t)fbit >> 2 and
// ((int32_t)lbit1 - 1) >> 2, -1 for none.  20 vector instructions a word where chunk_cmp takes 26 and seven scalar ones.
template <int NW>
__device__ __forceinline__ void chunk_cmp_bits(CmpChunkT<NW> &C, int32_t qi, int32_t gi, int32_t l, int32_t t, u32 &mism, u32 &fbit, u32 &lbit1) {
    const u32 shq = (u32)(qi & 7) * 4u, shg = (u32)(gi & 7) * 4u;
#pragma unroll
    for (int k = 0; k < NW; k++) C.qw[k] = swap_nibbles(C.qw[k]);
    const int32_t rem2 = 2 * (l - t); // twice the bases left from the chunk's first
    u32 fw = 0xffffffffu, lw = 0;
#pragma unroll
    for (int c = 0; c < NW - 1; c++) {
        int32_t w2 = rem2 - 16 * c; // twice the word's valid bases, 0 .. 16
        w2 = w2 < 0 ? 0 : (w2 > 16 ? 16 : w2);
        const u32 inval = (0xffffffffu << (u32)w2) << (u32)w2; // (two shifts: a shift by 32 would not move)
        const u32 q = __builtin_amdgcn_alignbit(C.qw[c + 1], C.qw[c], shq);
        const u32 g = __builtin_amdgcn_alignbit(C.gg[c + 1], C.gg[c], shg);
        const u32 x = q ^ g;
        const u32 m = (((x & 0x77777777u) + 0x77777777u) | x) & (0x88888888u & ~inval);
        mism += (u32)__popc(m);
        fw = min(fw, __builtin_elementwise_add_sat(ffbl_hw(m), 32u * (u32)c));
        lw = max(lw, __builtin_elementwise_sub_sat(32u * (u32)c + 32u, ffbh_hw(m)));
    }
    fbit = min(fbit, __builtin_elementwise_add_sat(fw, 4u * (u32)t));
    lbit1 = lw ? lw + 4u * (u32)t : lbit1; // (rounds ascend)
}
// one stretch of l bases
template <int NW, bool TO_BUFFER_END = false>
__device__ __forceinline__ void cmp_words(const u32 *seqw, int32_t qi, int32_t q_last, const u32 *gw, int32_t gi, int32_t g_words, int32_t l,
                                          int32_t out_base, int32_t &mism, int32_t &first_mis, int32_t &last_mis) {
    for (int32_t t = 0; t < l; t += 8 * (NW - 1)) {
        CmpChunkT<NW> C;
        chunk_load<NW, TO_BUFFER_END>(C, seqw, qi, q_last, gw, gi, g_words, l, t);
        chunk_cmp<NW>(C, qi, gi, l, t, out_base, mism, first_mis, last_mis);
    }
}

} // namespace pjb
