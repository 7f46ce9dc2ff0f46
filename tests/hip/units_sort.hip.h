// group sort of device_units.hip: one LSD pass (rs_hist -> rs_panel_sums -> rs_panel_scan -> rs_scatter), launched as sort_pass launches
// them (pjb_chain.hip.h), against a stable sort by that digit; a whole multi-pass sort; rs_place against the stable sort by id.
#pragma once

struct PassBufs { // the tables of a pass, sized as the chain sizes them: by the grid's tiles
    Guarded hist, psum, hscan, rtot;
    u32 tiles, nb;
    PassBufs(u32 tiles_, int bits) : tiles(tiles_), nb(1u << bits) {
        const u32 n_panels = (tiles + RSP_TILES - 1) / RSP_TILES;
        hist.alloc((size_t)tiles * nb * 4), psum.alloc((size_t)n_panels * nb * 4), hscan.alloc((size_t)tiles * nb * 4), rtot.alloc((size_t)nb * 4);
    }
    bool intact() const { return all_intact(hist, psum, hscan, rtot); }
};
static void sort_attributes() { // as pjb_api.hip sets them: 12-bit digits need more dynamic LDS than a kernel gets without asking
    CK(hipFuncSetAttribute((const void *)rs_scatter<0, u64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rs_scatter_lds_bytes(RS_MAX_BITS)));
    CK(hipFuncSetAttribute((const void *)rs_scatter<0, u32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rs_scatter_lds_bytes(RS_MAX_BITS, 4)));
}
// unrolled: widths 9, 10 and 11 through their own instantiation (what sort_pass does); else through rs_scatter<0, K>
template <typename K>
static void launch_pass(const K *kin, const u32 *vin, K *kout, u32 *vout, int shift, int bits, bool unrolled, const u32 *d_n, PassBufs &P) {
    const u32 tiles = P.tiles, nb = P.nb, n_panels = (tiles + RSP_TILES - 1) / RSP_TILES;
    u32 *hist = P.hist.p<u32>(), *psum = P.psum.p<u32>(), *hscan = P.hscan.p<u32>(), *rtot = P.rtot.p<u32>();
    hipLaunchKernelGGL(rs_hist<K>, dim3(tiles), dim3(256), 0, 0, kin, d_n, shift, bits, hist, tiles);
    hipLaunchKernelGGL(rs_panel_sums, dim3(n_panels, (nb + 255) / 256), dim3(256), 0, 0, (const u32 *)hist, tiles, nb, psum);
    hipLaunchKernelGGL(rs_panel_scan, dim3(n_panels, (nb + 255) / 256), dim3(256), 0, 0, (const u32 *)hist, (const u32 *)psum, tiles, nb, hscan, rtot);
#define DU_SCATTER(B)                                                                                                                          \
    hipLaunchKernelGGL((rs_scatter<B, K>), dim3(tiles), dim3(256), rs_scatter_lds_bytes(bits, sizeof(K)), 0, kin, vin, kout, vout, d_n, shift, \
                       bits, (const u32 *)hscan, (const u32 *)rtot, tiles)
    switch (unrolled ? bits : 0) {
    case 9: DU_SCATTER(9); break;
    case 10: DU_SCATTER(10); break;
    case 11: DU_SCATTER(11); break;
    default: DU_SCATTER(0); break;
    }
#undef DU_SCATTER
    launched();
}

static const char *const key_pat_names[7] = {"random", "all-equal", "two-alternating", "every-digit-then-repeated", "ascending", "descending",
                                             "tile-of-one-digit-beside-tile-of-distinct"};
template <typename K>
static std::vector<K> make_keys(u32 n, int shift, int bits, int pat, Rng &r) {
    const u32 nb = 1u << bits;
    const K field = (K)(nb - 1) << shift;
    std::vector<K> k(n);
    for (u32 i = 0; i < n; i++) {
        const K x = (K)r.next(); // (the bits outside the digit stay random, high bits set: they must come through unchanged)
        u32 d;
        switch (pat) {
        case 0: d = (u32)(r.next() >> 11) & (nb - 1); break;
        case 1: d = nb - 1; break;
        case 2: d = (i & 1) ? ((nb >> 1) | 1u) & (nb - 1) : 0u; break;
        case 3: d = i % nb; break;
        case 4: d = (u32)((u64)i * nb / n); break;
        case 5: d = nb - 1 - (u32)((u64)i * nb / n); break;
        default: d = i < (u32)RS_TILE ? 5u % nb : i % nb; break;
        }
        k[i] = (K)((x & ~field) | ((K)d << shift));
    }
    return k;
}
// stable sort by one digit, by counting
template <typename K>
static void ref_pass(const std::vector<K> &kin, const std::vector<u32> &vin, int shift, int bits, std::vector<K> &kout, std::vector<u32> &vout) {
    const u32 nb = 1u << bits, mask = nb - 1;
    std::vector<size_t> at(nb + 1, 0);
    for (const K k : kin) at[((u32)(k >> shift) & mask) + 1]++;
    for (u32 d = 0; d < nb; d++) at[d + 1] += at[d];
    kout.resize(kin.size()), vout.resize(kin.size());
    for (size_t i = 0; i < kin.size(); i++) {
        const size_t dst = at[(u32)(kin[i] >> shift) & mask]++;
        kout[dst] = kin[i], vout[dst] = vin[i];
    }
}

struct SortBufs {
    u32 n;
    Guarded kin, vin, kout, vout, np;
    SortBufs(u32 n_, size_t key_bytes) : n(n_) {
        // (one tile of slack behind the inputs: rs_scatter loads whole tiles unguarded)
        kin.alloc((size_t)n * key_bytes, (size_t)RS_TILE * key_bytes), vin.alloc((size_t)n * 4, (size_t)RS_TILE * 4);
        kout.alloc((size_t)n * key_bytes), vout.alloc((size_t)n * 4), np.alloc(4);
        np.up(&n, 4);
    }
};
template <typename K>
static void pass_case(SortBufs &B, PassBufs &P, int shift, int bits, bool unrolled, bool with_vin, int pat, const std::string &extra, Rng &r) {
    const u32 n = B.n;
    Case c(std::string("sort pass ") + (sizeof(K) == 8 ? "u64" : "u32") + " bits=" + S(bits) + (unrolled ? " rs_scatter<" + S(bits) + ">" : std::string(" rs_scatter<0>")) +
           " shift=" + S(shift) + (with_vin ? " vin=given" : " vin=null") + " n=" + S(n) + " keys=" + key_pat_names[pat] + extra);
    const std::vector<K> keys = make_keys<K>(n, shift, bits, pat, r);
    std::vector<u32> vals(n);
    for (u32 i = 0; i < n; i++) vals[i] = with_vin ? (u32)r.next() : i;
    B.kin.up(keys.data(), (size_t)n * sizeof(K));
    if (with_vin) B.vin.up(vals.data(), (size_t)n * 4);
    B.kout.fill(0xEE), B.vout.fill(0xEE);
    launch_pass<K>(B.kin.p<K>(), with_vin ? B.vin.p<u32>() : nullptr, B.kout.p<K>(), B.vout.p<u32>(), shift, bits, unrolled, B.np.p<u32>(), P);
    std::vector<K> wk;
    std::vector<u32> wv;
    ref_pass(keys, vals, shift, bits, wk, wv);
    c.eq("keys", B.kout.get<K>(n), wk);
    c.eq("values", B.vout.get<u32>(n), wv);
    c.flag("canaries", all_intact(B.kin, B.vin, B.kout, B.vout, P.hist, P.psum, P.hscan, P.rtot));
}
template <typename K>
static void pass_cases() {
    const int W = (int)sizeof(K) * 8;
    struct Width {
        int bits;
        bool unrolled;
    };
    const Width widths[] = {{1, false}, {4, false}, {8, false}, {9, true}, {9, false}, {10, true}, {10, false}, {11, true}, {11, false}, {12, false}};
    const u32 sizes[] = {1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17, 64 * 4096, 64 * 4096 + 1};
    Rng r(sizeof(K) * 31);
    for (u32 n : sizes) {
        SortBufs B(n, sizeof(K));
        const u32 tiles = (n + RS_TILE - 1) / RS_TILE;
        const bool big = n >= 64u * 4096u; // (the two sizes on a panel edge: a reduced set, see below)
        for (const Width &w : widths) {
            PassBufs P(tiles, w.bits);
            const int shifts[3] = {0, W == 64 ? 29 : 13, W - w.bits};
            if (!big) {
                for (int shift : shifts)
                    for (int with_vin = 0; with_vin < 2; with_vin++)
                        for (int pat = 0; pat < 7; pat++) {
                            if (pat == 6 && n <= (u32)RS_TILE) continue;
                            pass_case<K>(B, P, shift, w.bits, w.unrolled, with_vin != 0, pat, "", r);
                        }
            } else { // 64 and 65 tiles: every width and instantiation, the lowest digit without vin and the top digit with it, two key families
                for (int shift : {shifts[0], shifts[2]})
                    for (int pat : {0, 6}) pass_case<K>(B, P, shift, w.bits, w.unrolled, shift != 0, pat, "", r);
            }
        }
    }
    // *np below the grid's cover: the grid and the tables are sized for a larger limit, tiles past the data write nothing
    for (u32 n : {1u, 4097u, 3u * 4096u + 17u}) {
        SortBufs B(n, sizeof(K));
        const u32 limit = n + 2 * RS_TILE + 5, tiles = (limit + RS_TILE - 1) / RS_TILE;
        for (const Width &w : {Width{8, false}, Width{10, true}, Width{12, false}}) {
            PassBufs P(tiles, w.bits);
            pass_case<K>(B, P, W == 64 ? 29 : 13, w.bits, w.unrolled, true, 0, " grid=" + S(tiles) + "-tiles", r);
            pass_case<K>(B, P, 0, w.bits, w.unrolled, false, 3, " grid=" + S(tiles) + "-tiles", r);
        }
    }
}

static void full_sort_case(const std::vector<int> &widths, int key_bits) {
    std::string wn;
    for (int b : widths) wn += (wn.empty() ? "" : "/") + S(b);
    const u32 n = 5 * RS_TILE + 123, tiles = (n + RS_TILE - 1) / RS_TILE;
    Case c("sort full u64 keys of " + S(key_bits) + " bits, passes " + wn + " n=" + S(n));
    Rng r(4242 + key_bits);
    std::vector<u64> keys(n);
    for (u32 i = 0; i < n; i++) keys[i] = key_bits == 64 ? r.next() : r.next() >> (64 - key_bits);
    for (u32 i = 0; i + 7 < n; i += 97) keys[i + 7] = keys[i]; // (equal keys: their order must hold)
    Guarded kb[2], vb[2], np(4);
    for (int k = 0; k < 2; k++) kb[k].alloc((size_t)n * 8, (size_t)RS_TILE * 8), vb[k].alloc((size_t)n * 4, (size_t)RS_TILE * 4);
    np.up(&n, 4);
    kb[0].up(keys.data(), (size_t)n * 8);
    int cur = 0, shift = 0;
    bool tables = true;
    for (size_t p = 0; p < widths.size(); p++) {
        PassBufs P(tiles, widths[p]);
        launch_pass<u64>(kb[cur].p<u64>(), p == 0 ? nullptr : vb[cur].p<u32>(), kb[cur ^ 1].p<u64>(), vb[cur ^ 1].p<u32>(), shift, widths[p], true, np.p<u32>(), P);
        tables = tables && P.intact();
        cur ^= 1, shift += widths[p];
    }
    std::vector<u32> idx(n);
    for (u32 i = 0; i < n; i++) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](u32 a, u32 b) { return keys[a] < keys[b]; });
    std::vector<u64> wk(n);
    for (u32 i = 0; i < n; i++) wk[i] = keys[idx[i]];
    c.eq("keys", kb[cur].get<u64>(n), wk);
    c.eq("values", vb[cur].get<u32>(n), idx);
    c.flag("canaries", tables && kb[0].intact() && kb[1].intact() && vb[0].intact() && vb[1].intact());
}

// rs_place.  The run list is built here by the rule in pjb_device.hip.h ("The id runs of the tiles"): one entry per (tile, id), a tile's
// entries consecutive and ascending by id, key = id << tile_bits | tile; the place of a run's first pair is the exclusive prefix sum of the
// counts in key order.  Precondition the callers guarantee (kd_assign takes the radix route otherwise): a tile's ids span less than RUN_W.
static void place_case(const std::string &name, const std::vector<u32> &ids) {
    const u32 n = (u32)ids.size(), tiles = (n + RS_TILE - 1) / RS_TILE;
    const int tile_bits = 8;
    Case c("sort rs_place " + name + " n=" + S(n));
    std::vector<u64> run_key;
    std::vector<u32> cnt, tile_first(tiles), tile_n(tiles);
    for (u32 t = 0; t < tiles; t++) {
        std::vector<u32> s(ids.begin() + (size_t)t * RS_TILE, ids.begin() + std::min<size_t>(n, (size_t)(t + 1) * RS_TILE));
        std::sort(s.begin(), s.end());
        if (s.back() - s.front() >= RUN_W) {
            c.miss("the case breaks rs_place's precondition", t, s.back() - s.front(), RUN_W - 1);
            return;
        }
        tile_first[t] = (u32)run_key.size();
        for (size_t i = 0; i < s.size();) {
            size_t j = i;
            while (j < s.size() && s[j] == s[i]) j++;
            run_key.push_back(((u64)s[i] << tile_bits) | t), cnt.push_back((u32)(j - i));
            i = j;
        }
        tile_n[t] = (u32)run_key.size() - tile_first[t];
    }
    const u32 runs = (u32)run_key.size();
    std::vector<u32> order(runs), dest(runs);
    for (u32 e = 0; e < runs; e++) order[e] = e;
    std::stable_sort(order.begin(), order.end(), [&](u32 a, u32 b) { return run_key[a] < run_key[b]; });
    u32 at = 0;
    for (u32 e : order) dest[e] = at, at += cnt[e];
    Guarded jid((size_t)n * 4, (size_t)RS_TILE * 4), np(4), dkey((size_t)runs * 8), ddest((size_t)runs * 4), dfirst((size_t)tiles * 4), dn((size_t)tiles * 4);
    Guarded kout((size_t)n * 4), vout((size_t)n * 4);
    jid.up(ids.data(), (size_t)n * 4), np.up(&n, 4), dkey.up(run_key.data(), (size_t)runs * 8), ddest.up(dest.data(), (size_t)runs * 4);
    dfirst.up(tile_first.data(), (size_t)tiles * 4), dn.up(tile_n.data(), (size_t)tiles * 4);
    kout.fill(0xEE), vout.fill(0xEE);
    hipLaunchKernelGGL(rs_place, dim3(tiles), dim3(256), 0, 0, (const u32 *)jid.p<u32>(), (const u32 *)np.p<u32>(), (const u64 *)dkey.p<u64>(), (const u32 *)ddest.p<u32>(),
                       (const u32 *)dfirst.p<u32>(), (const u32 *)dn.p<u32>(), runs, tile_bits, kout.p<u32>(), vout.p<u32>());
    launched();
    std::vector<u32> idx(n), wk(n);
    for (u32 i = 0; i < n; i++) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](u32 a, u32 b) { return ids[a] < ids[b]; });
    for (u32 i = 0; i < n; i++) wk[i] = ids[idx[i]];
    c.eq("ids", kout.get<u32>(n), wk);
    c.eq("pair indices", vout.get<u32>(n), idx);
    c.flag("canaries", jid.intact() && kout.intact() && vout.intact() && dkey.intact() && ddest.intact());
}

static void group_sort() {
    sort_attributes();
    pass_cases<u32>();
    pass_cases<u64>();
    full_sort_case({12, 12, 12, 12, 12, 4}, 64);
    full_sort_case({11, 11, 10}, 32);
    Rng r(606);
    auto ids_of = [&](u32 n, auto f) {
        std::vector<u32> v(n);
        for (u32 i = 0; i < n; i++) v[i] = f(i);
        return v;
    };
    place_case("one id over three tiles", ids_of(3 * RS_TILE, [](u32) { return 7u; }));
    place_case("64 distinct ids in every slice", ids_of(RS_TILE + 100, [](u32 i) { return 1000u + ((i * 29u) & 63u); }));
    place_case("ids in all four waves of a tile", ids_of(RS_TILE, [](u32 i) { return 50u + (i % 1024u) / 400u; }));
    place_case("ids straddling a multiple of RUN_W", ids_of(2 * RS_TILE + 33, [&](u32) { return 3u * RUN_W - 20u + r.u(40); }));
    place_case("ids ascending over a window wrap", ids_of(3 * RS_TILE + 5, [&](u32 i) { return RUN_W - 30u + i / 200u + r.u(3); }));
    for (u32 n : {4095u, 4096u, 4097u}) place_case("nearly sorted ids", ids_of(n, [&](u32 i) { return 500u + i / 200u + r.u(3); }));
}
