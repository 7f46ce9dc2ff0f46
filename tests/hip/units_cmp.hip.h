// groups cmp4 and cmp2 of device_units.hip: the packed base compares over an exhaustive lattice of (read phase, genome phase, length), one
// lane per variant, against a byte-by-byte compare of the unpacked bases.  A lattice point's variants: no mismatch; one mismatch at every
// position in turn; mismatches at both ends; all mismatching.  The bases just past the anchor differ between read and genome, so a length
// mask that is one base too long is seen; everything else in a lane's words is random (non-zero words around the guarded ranges).
#pragma once

struct LCase { // one lane's arguments (its words: slot i of both streams)
    int32_t qi, gi, l, q_last, g_words, place;
};
constexpr int CMP_SLOT = 32;              // words per stream and lane
constexpr int32_t CMP_OUT_BASE = 1000;    // cmp_words reports positions relative to this
constexpr size_t CMP_BATCH = 1200000;     // lanes a launch

template <int NW, bool TBE>
__global__ __launch_bounds__(K1E_T) void wk_cmp_words(const u32 *q, const u32 *g, const LCase *cs, u32 n, int32_t *res) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LCase c = cs[i];
    int32_t mism = 0, first = -1, last = -1;
    cmp_words<NW, TBE>(q + (size_t)i * CMP_SLOT, c.qi, c.q_last, g + (size_t)i * CMP_SLOT, c.gi, c.g_words, c.l, CMP_OUT_BASE, mism, first, last);
    res[3 * (size_t)i] = mism, res[3 * (size_t)i + 1] = first, res[3 * (size_t)i + 2] = last;
}
template <int NW, bool TBE>
__global__ __launch_bounds__(K1E_T) void wk_cmp_bits(const u32 *q, const u32 *g, const LCase *cs, u32 n, int32_t *res) { // the rounds as k1_emit walks them
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LCase c = cs[i];
    u32 mism = 0, fbit = 0xffffffffu, lbit1 = 0;
    for (int32_t t = 0; t < c.l; t += 8 * (NW - 1)) {
        CmpChunkT<NW> C;
        chunk_load<NW, TBE>(C, q + (size_t)i * CMP_SLOT, c.qi, c.q_last, g + (size_t)i * CMP_SLOT, c.gi, c.g_words, c.l, t);
        chunk_cmp_bits<NW>(C, c.qi, c.gi, c.l, t, mism, fbit, lbit1);
    }
    // bit positions to bases, as the header's comment gives them (-1: none)
    res[3 * (size_t)i] = (int32_t)mism, res[3 * (size_t)i + 1] = (int32_t)fbit >> 2, res[3 * (size_t)i + 2] = ((int32_t)lbit1 - 1) >> 2;
}

// read bases: high nibble first; genome codes: low nibble first
static inline u32 q4_get(const u32 *w, int32_t b) { return (((const uint8_t *)w)[b >> 1] >> ((b & 1) ? 0 : 4)) & 15u; }
static inline void q4_set(u32 *w, int32_t b, u32 v) {
    uint8_t &x = ((uint8_t *)w)[b >> 1];
    x = (b & 1) ? (uint8_t)((x & 0xf0u) | v) : (uint8_t)((x & 0x0fu) | (v << 4));
}
static inline u32 g4_get(const u32 *w, int32_t p) { return (w[p >> 3] >> (4 * (p & 7))) & 15u; }
static inline void g4_set(u32 *w, int32_t p, u32 v) { w[p >> 3] = (w[p >> 3] & ~(15u << (4 * (p & 7)))) | (v << (4 * (p & 7))); }

struct Tally {
    std::string name;
    long points = 0, variants = 0;
    bool bad = false;
    std::string first_miss;
};
static void tally_report(std::vector<Tally> &ts) {
    for (Tally &t : ts) {
        g_cases++;
        if (t.bad) g_failed++, printf("FAIL %s %s\n", t.name.c_str(), t.first_miss.c_str());
        else printf("ok %s: %ld lattice points, %ld variants\n", t.name.c_str(), t.points, t.variants);
    }
}

static const char *const place4_names[3] = {"anchor-begins-before-the-genome's-first-word", "anchor-ends-on-the-last-code-word", "anchor-ends-on-q_last"};

static void group_cmp4() {
    const int NWS[3] = {5, 8, 9};
    std::vector<Tally> tallies(2 * 3 * 2 * 3);
    auto tally_at = [&](int kind, int nwi, int tbe, int place) -> Tally & { return tallies[((kind * 3 + nwi) * 2 + tbe) * 3 + place]; };
    for (int kind = 0; kind < 2; kind++)
        for (int nwi = 0; nwi < 3; nwi++)
            for (int tbe = 0; tbe < 2; tbe++)
                for (int pl = 0; pl < 3; pl++)
                    tally_at(kind, nwi, tbe, pl).name = std::string("cmp4 ") + (kind ? "chunk_load+chunk_cmp_bits<" : "cmp_words<") + S(NWS[nwi]) + "," +
                                                        (tbe ? "TO_BUFFER_END" : "to-the-anchor's-end") + "> " + place4_names[pl];
    std::vector<u32> hq(CMP_BATCH * CMP_SLOT), hg(CMP_BATCH * CMP_SLOT);
    std::vector<LCase> hc(CMP_BATCH);
    std::vector<int32_t> want(CMP_BATCH * 3), got(CMP_BATCH * 3);
    std::vector<char> point_head(CMP_BATCH);
    Guarded dq(CMP_BATCH * CMP_SLOT * 4), dg(CMP_BATCH * CMP_SLOT * 4), dc(CMP_BATCH * sizeof(LCase)), dres(CMP_BATCH * 12);
    Rng r(4004);
    size_t nv = 0;
    auto flush = [&]() {
        if (!nv) return;
        // the reference: both streams unpacked to bytes (what the guards leave out reads as 0), compared one by one
        for (size_t i = 0; i < nv; i++) {
            const LCase &c = hc[i];
            const u32 *q = &hq[i * CMP_SLOT], *g = &hg[i * CMP_SLOT];
            uint8_t qb[160], gb[160];
            for (int32_t j = 0; j < c.l; j++) {
                const int32_t b = c.qi + j, p = c.gi + j;
                qb[j] = (b >> 3) > c.q_last ? 0 : (uint8_t)q4_get(q, b);
                gb[j] = (p < 0 || (p >> 3) >= c.g_words) ? 0 : (uint8_t)g4_get(g, p);
            }
            int32_t mism = 0, first = -1, last = -1;
            for (int32_t j = 0; j < c.l; j++)
                if (qb[j] != gb[j]) {
                    mism++;
                    if (first < 0) first = j;
                    last = j;
                }
            want[3 * i] = mism, want[3 * i + 1] = first, want[3 * i + 2] = last;
        }
        dq.up(hq.data(), nv * CMP_SLOT * 4), dg.up(hg.data(), nv * CMP_SLOT * 4), dc.up(hc.data(), nv * sizeof(LCase));
        const dim3 grid((unsigned)((nv + K1E_T - 1) / K1E_T)), block(K1E_T);
        for (int kind = 0; kind < 2; kind++)
            for (int nwi = 0; nwi < 3; nwi++)
                for (int tbe = 0; tbe < 2; tbe++) {
                    dres.fill(0xEE);
#define DU_CMP(KERN, NW, TBE) hipLaunchKernelGGL((KERN<NW, TBE>), grid, block, 0, 0, dq.p<u32>(), dg.p<u32>(), dc.p<LCase>(), (u32)nv, dres.p<int32_t>())
                    const int sel = (kind * 3 + nwi) * 2 + tbe;
                    switch (sel) {
                    case 0: DU_CMP(wk_cmp_words, 5, false); break;
                    case 1: DU_CMP(wk_cmp_words, 5, true); break;
                    case 2: DU_CMP(wk_cmp_words, 8, false); break;
                    case 3: DU_CMP(wk_cmp_words, 8, true); break;
                    case 4: DU_CMP(wk_cmp_words, 9, false); break;
                    case 5: DU_CMP(wk_cmp_words, 9, true); break;
                    case 6: DU_CMP(wk_cmp_bits, 5, false); break;
                    case 7: DU_CMP(wk_cmp_bits, 5, true); break;
                    case 8: DU_CMP(wk_cmp_bits, 8, false); break;
                    case 9: DU_CMP(wk_cmp_bits, 8, true); break;
                    case 10: DU_CMP(wk_cmp_bits, 9, false); break;
                    default: DU_CMP(wk_cmp_bits, 9, true); break;
                    }
#undef DU_CMP
                    launched();
                    dres.down(got.data(), nv * 12);
                    const int32_t ob = kind == 0 ? CMP_OUT_BASE : 0; // (cmp_words adds out_base to the positions it reports)
                    for (size_t i = 0; i < nv; i++) {
                        Tally &t = tally_at(kind, nwi, tbe, hc[i].place);
                        t.variants++;
                        if (point_head[i]) t.points++;
                        if (t.bad) continue;
                        const int32_t w[3] = {want[3 * i], want[3 * i + 1] < 0 ? -1 : want[3 * i + 1] + ob, want[3 * i + 2] < 0 ? -1 : want[3 * i + 2] + ob};
                        for (int k = 0; k < 3; k++)
                            if (got[3 * i + k] != w[k]) {
                                t.bad = true;
                                t.first_miss = std::string(k == 0 ? "mismatches" : k == 1 ? "first mismatch" : "last mismatch") + " at qi=" + S(hc[i].qi) + " gi=" + S(hc[i].gi) +
                                               " l=" + S(hc[i].l) + " (reference: " + S(want[3 * i]) + " mismatches, first " + S(want[3 * i + 1]) + ", last " +
                                               S(want[3 * i + 2]) + ") index " + S((long long)i) + " got " + S(got[3 * i + k]) + " want " + S(w[k]);
                                break;
                            }
                    }
                }
        if (!(dq.intact() && dg.intact() && dc.intact() && dres.intact()))
            for (Tally &t : tallies)
                if (!t.bad) t.bad = true, t.first_miss = "canaries index -1 got 0 want 1";
        nv = 0;
    };
    for (int32_t l = 1; l <= 150; l++) {
        if (nv + (size_t)64 * 3 * (l + 3) > CMP_BATCH) flush();
        for (int qp = 0; qp < 8; qp++)
            for (int gp = 0; gp < 8; gp++)
                for (int pl = 0; pl < 3; pl++) {
                    LCase c;
                    c.l = l, c.place = pl;
                    if (pl == 0) c.qi = qp, c.gi = gp - 8, c.q_last = CMP_SLOT - 1, c.g_words = CMP_SLOT; // the chunk's first genome word would be word -1
                    if (pl == 1) c.qi = qp + 8, c.gi = gp + 8, c.q_last = CMP_SLOT - 1, c.g_words = ((c.gi + l - 1) >> 3) + 1;
                    if (pl == 2) c.qi = qp, c.gi = gp, c.q_last = (c.qi + l - 1) >> 3, c.g_words = CMP_SLOT;
                    // the point's words without a mismatch
                    u32 bq[CMP_SLOT], bg[CMP_SLOT];
                    for (int k = 0; k < CMP_SLOT; k++) bq[k] = (u32)r.next() | 0x01010101u, bg[k] = (u32)r.next() | 0x10101010u;
                    for (int32_t j = 0; j < l + 16; j++) {
                        const int32_t b = c.qi + j, p = c.gi + j;
                        const bool q_there = (b >> 3) <= c.q_last && (b >> 3) < CMP_SLOT, g_there = p >= 0 && (p >> 3) < c.g_words;
                        u32 code = r.u(16);
                        if (j >= l) { // past the anchor: the two differ
                            if (q_there) q4_set(bq, b, 1 + r.u(15));
                            if (g_there) g4_set(bg, p, q_there ? (q4_get(bq, b) ^ (1 + r.u(15))) : 1 + r.u(15));
                            continue;
                        }
                        if (!g_there) code = 0; // (a genome word that is not there reads as code 0)
                        q4_set(bq, b, code);
                        if (g_there) g4_set(bg, p, code);
                    }
                    for (int32_t v = 0; v < l + 3; v++) {
                        u32 *q = &hq[nv * CMP_SLOT];
                        memcpy(q, bq, sizeof(bq)), memcpy(&hg[nv * CMP_SLOT], bg, sizeof(bg));
                        auto flip = [&](int32_t j) { q4_set(q, c.qi + j, q4_get(q, c.qi + j) ^ (1 + r.u(15))); };
                        if (v >= 1 && v <= l) flip(v - 1);
                        if (v == l + 1) {
                            flip(0);
                            if (l > 1) flip(l - 1);
                        }
                        if (v == l + 2)
                            for (int32_t j = 0; j < l; j++) flip(j);
                        hc[nv] = c, point_head[nv] = v == 0;
                        nv++;
                    }
                }
    }
    flush();
    tally_report(tallies);
}

// ---------------------------------------------------------------------------------------------
// cmp2: bases in two bits.  Read base i of a read whose seq4 words start at so: bit 16 (so & 1) + 2 i from word so >> 1 of seq2; genome base
// p at bits 2 (p & 15) of word p >> 4 (A 0, C 1, G 2, T 3).
// ---------------------------------------------------------------------------------------------
struct L2Case {
    int32_t qodd, qi, gi, l, q2_last, place;
};
constexpr int C2_SLOT = 24; // words per stream and lane (the genome's: its bases and what K0_CODES2_PAD stands for)
template <int UNUSED = 0>
__global__ __launch_bounds__(K1E_T) void wk_cmp2(const u32 *q, const u32 *g, const L2Case *cs, u32 n, int32_t *res) { // the rounds as k1_emit walks them
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const L2Case c = cs[i];
    const u32 *seq2w = q + (size_t)i * C2_SLOT, *gcodes2 = g + (size_t)i * C2_SLOT;
    const int32_t g2_last = C2_SLOT - 1;
    u32 mism = 0, fbit = 0xffffffffu, lbit1 = 0;
    for (int32_t t = 0; t < c.l; t += C2_ROUND) {
        const u32 qbit = (u32)c.qodd + 2u * (u32)(c.qi + t), gbit = 2u * (u32)(c.gi + t);
        u32 qw[C2_NW], gw[C2_NW];
        const int32_t qf = (int32_t)(qbit >> 5), gf = (int32_t)(gbit >> 5);
        if (qf + C2_NW - 1 <= c.q2_last) {
            const Words4 qa = gload(reinterpret_cast<const Words4 *>(seq2w + qf)), ga = gload(reinterpret_cast<const Words4 *>(gcodes2 + gf));
            Words4 qb = {0, 0, 0, 0}, gb = {0, 0, 0, 0};
            if (c.l - t > 48) { // (words 4 .. 7 feed the bases from the 49th on)
                qb = gload(reinterpret_cast<const Words4 *>(seq2w + qf + 4));
                gb = gload(reinterpret_cast<const Words4 *>(gcodes2 + gf + 4));
            }
            qw[0] = qa.x, qw[1] = qa.y, qw[2] = qa.z, qw[3] = qa.w, qw[4] = qb.x, qw[5] = qb.y, qw[6] = qb.z, qw[7] = qb.w;
            gw[0] = ga.x, gw[1] = ga.y, gw[2] = ga.z, gw[3] = ga.w, gw[4] = gb.x, gw[5] = gb.y, gw[6] = gb.z, gw[7] = gb.w;
        } else {
            load_words<C2_NW>(qw, seq2w, qf, c.q2_last);
            load_words<C2_NW>(gw, gcodes2, gf, g2_last);
        }
        chunk2_cmp_bits<C2_NW>(qw, gw, qbit & 31u, gbit & 31u, c.l, t, mism, fbit, lbit1);
    }
    res[3 * (size_t)i] = (int32_t)mism, res[3 * (size_t)i + 1] = (int32_t)fbit >> 1, res[3 * (size_t)i + 2] = ((int32_t)lbit1 - 1) >> 1;
}
static inline void b2_set(u32 *w, u32 bit, u32 v) { w[bit >> 5] = (w[bit >> 5] & ~(3u << (bit & 31))) | (v << (bit & 31)); }
static inline u32 acgt_code(char ch) { return ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 0u; }

static void group_cmp2() {
    const int32_t LMAX = 2 * C2_ROUND + 17;
    std::vector<Tally> tallies(2);
    tallies[0].name = "cmp2 chunk2_cmp_bits<C2_NW> read-words-to-spare (16-byte gathers)";
    tallies[1].name = "cmp2 chunk2_cmp_bits<C2_NW> anchor-ends-on-q2_last (guarded word loads)";
    std::vector<u32> hq(CMP_BATCH * C2_SLOT), hg(CMP_BATCH * C2_SLOT);
    std::vector<L2Case> hc(CMP_BATCH);
    std::vector<int32_t> want(CMP_BATCH * 3), got(CMP_BATCH * 3);
    std::vector<char> point_head(CMP_BATCH);
    Guarded dq(CMP_BATCH * C2_SLOT * 4), dg(CMP_BATCH * C2_SLOT * 4), dc(CMP_BATCH * sizeof(L2Case)), dres(CMP_BATCH * 12);
    Rng r(2002);
    size_t nv = 0;
    auto flush = [&]() {
        if (!nv) return;
        dq.up(hq.data(), nv * C2_SLOT * 4), dg.up(hg.data(), nv * C2_SLOT * 4), dc.up(hc.data(), nv * sizeof(L2Case));
        dres.fill(0xEE);
        hipLaunchKernelGGL(wk_cmp2<0>, dim3((unsigned)((nv + K1E_T - 1) / K1E_T)), dim3(K1E_T), 0, 0, dq.p<u32>(), dg.p<u32>(), dc.p<L2Case>(), (u32)nv, dres.p<int32_t>());
        launched();
        dres.down(got.data(), nv * 12);
        for (size_t i = 0; i < nv; i++) {
            Tally &t = tallies[hc[i].place];
            t.variants++;
            if (point_head[i]) t.points++;
            if (t.bad) continue;
            for (int k = 0; k < 3; k++)
                if (got[3 * i + k] != want[3 * i + k]) {
                    t.bad = true;
                    t.first_miss = std::string(k == 0 ? "mismatches" : k == 1 ? "first mismatch" : "last mismatch") + " at read phase " + S((hc[i].qodd >> 1) + hc[i].qi) +
                                   " genome phase " + S(hc[i].gi) + " l=" + S(hc[i].l) + " (reference: " + S(want[3 * i]) + " mismatches, first " + S(want[3 * i + 1]) +
                                   ", last " + S(want[3 * i + 2]) + ") index " + S((long long)i) + " got " + S(got[3 * i + k]) + " want " + S(want[3 * i + k]);
                    break;
                }
        }
        if (!(dq.intact() && dg.intact() && dc.intact() && dres.intact()))
            for (Tally &t : tallies)
                if (!t.bad) t.bad = true, t.first_miss = "canaries index -1 got 0 want 1";
        nv = 0;
    };
    static const char ACGT[5] = "ACGT";
    std::vector<char> sq(LMAX + 16), sg(LMAX + 16), vq(LMAX + 16);
    for (int32_t l = 1; l <= LMAX; l++) {
        if (nv + (size_t)256 * (l + 3 + 4) > CMP_BATCH) flush();
        for (int qp = 0; qp < 16; qp++)
            for (int gp = 0; gp < 16; gp++) {
                // the point's strings: equal along the anchor, different in the 16 bases past it
                for (int32_t j = 0; j < l + 16; j++) {
                    sq[j] = ACGT[r.u(4)];
                    sg[j] = j < l ? sq[j] : ACGT[(acgt_code(sq[j]) + 1 + r.u(3)) & 3];
                }
                u32 bg[C2_SLOT];
                for (int k = 0; k < C2_SLOT; k++) bg[k] = (u32)r.next() | 1u;
                for (int32_t j = 0; j < l + 16; j++) b2_set(bg, 2u * (u32)(gp + j), acgt_code(sg[j]));
                for (int pl = 0; pl < 2; pl++) {
                    L2Case c;
                    c.qodd = 16 * (qp >> 3), c.qi = qp & 7, c.gi = gp, c.l = l, c.place = pl;
                    const int32_t q_end_word = (int32_t)(((u32)c.qodd + 2u * (u32)(c.qi + l - 1)) >> 5);
                    c.q2_last = pl == 0 ? C2_SLOT - 1 : q_end_word;
                    // (the guarded placement: no mismatch, the last base, both ends, all -- the gathers' placement: every variant)
                    u32 bq[C2_SLOT]; // the read's words without a mismatch
                    for (int k = 0; k < C2_SLOT; k++) bq[k] = (u32)r.next() | 1u;
                    for (int32_t j = 0; j < l + 16; j++) {
                        const u32 bit = (u32)c.qodd + 2u * (u32)(c.qi + j);
                        if ((int32_t)(bit >> 5) <= c.q2_last) b2_set(bq, bit, acgt_code(sq[j]));
                    }
                    for (int32_t v = 0; v < l + 3; v++) {
                        if (pl == 1 && !(v == 0 || v == l || v >= l + 1)) continue;
                        u32 *q = &hq[nv * C2_SLOT];
                        memcpy(q, bq, sizeof(bq)), memcpy(&hg[nv * C2_SLOT], bg, sizeof(bg));
                        memcpy(vq.data(), sq.data(), (size_t)l);
                        auto flip = [&](int32_t j) { // another base in the string, and its two bits in the words
                            vq[j] = ACGT[(acgt_code(vq[j]) + 1 + r.u(3)) & 3];
                            b2_set(q, (u32)c.qodd + 2u * (u32)(c.qi + j), acgt_code(vq[j]));
                        };
                        if (v >= 1 && v <= l) flip(v - 1);
                        if (v == l + 1) {
                            flip(0);
                            if (l > 1) flip(l - 1);
                        }
                        if (v == l + 2)
                            for (int32_t j = 0; j < l; j++) flip(j);
                        // the reference: the two strings, byte by byte
                        int32_t mism = 0, first = -1, last = -1;
                        for (int32_t j = 0; j < l; j++)
                            if (vq[j] != sg[j]) {
                                mism++;
                                if (first < 0) first = j;
                                last = j;
                            }
                        want[3 * nv] = mism, want[3 * nv + 1] = first, want[3 * nv + 2] = last;
                        hc[nv] = c, point_head[nv] = v == 0;
                        nv++;
                    }
                }
            }
    }
    flush();
    tally_report(tallies);
}
