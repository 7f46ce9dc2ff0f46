// group scan of device_units.hip: the generic multi-block scan of pjb_device.hip.h on both of run_scan's routes, launched as run_scan
// launches them (pjb_host.hip.h), whatever route run_scan would choose for the size; scan_tiles_kernel on tile-sum arrays of its own.
#pragma once

template <typename F>
static F scan_fn(const void *p) {
    F f;
    f.a = (decltype(f.a))p;
    return f;
}
template <typename F> struct ScanTerm;
template <> struct ScanTerm<ArrU32Fn> {
    static constexpr const char *name = "ArrU32Fn";
    static constexpr bool bytes = false;
    static u64 term(u32 w, uint8_t) { return w; }
};
template <> struct ScanTerm<ArrU8Fn> {
    static constexpr const char *name = "ArrU8Fn";
    static constexpr bool bytes = true;
    static u64 term(u32, uint8_t b) { return b; }
};
template <> struct ScanTerm<ArrU8Bit0Fn> {
    static constexpr const char *name = "ArrU8Bit0Fn";
    static constexpr bool bytes = true;
    static u64 term(u32, uint8_t b) { return b & 1u; }
};
template <> struct ScanTerm<ArrI32Fn> { // negative terms: the sum is taken modulo 2^64
    static constexpr const char *name = "ArrI32Fn";
    static constexpr bool bytes = false;
    static u64 term(u32 w, uint8_t) { return (u64)(int64_t)(int32_t)w; }
};

struct ScanBufs {
    u64 n = 0;
    u32 nt = 0;
    std::vector<u32> h32;
    std::vector<uint8_t> h8;
    Guarded in32, in8, out, tiles, total, np;
    explicit ScanBufs(u64 n_) : n(n_) {
        nt = std::max<u32>(1, (u32)((n + SCAN_TILE - 1) / SCAN_TILE));
        Rng r(1000 + n);
        h32.resize(n), h8.resize(n);
        for (u64 i = 0; i < n; i++) { // values near 2^32 - 1 among them: a few terms pass 2^32
            const u64 x = r.next();
            h32[i] = (x >> 60) == 0 ? 0xffffffffu - (u32)(x & 7) : (u32)x;
            h8[i] = (uint8_t)(x >> 32);
        }
        in32.alloc(n * 4), in8.alloc(n), out.alloc(n * 4), tiles.alloc((size_t)nt * 8), total.alloc(8), np.alloc(4);
        in32.up(h32.data(), n * 4), in8.up(h8.data(), n);
    }
};
static const u32 SCAN_UNTOUCHED = 0xEEEEEEEEu;
static const char *const scan_np_names[5] = {"null", "n", "n-1", "n-tile", "n+5"};

// np_mode: see scan_np_names.  route 1: reduce + apply2; route 2: reduce + tiles + apply.  alias: the sink writes over the functor's input
template <typename F, typename G, bool INCLUSIVE>
static void scan_case(ScanBufs &b, int np_mode, int route, bool alias) {
    typedef ScanTerm<F> TR;
    const u64 n = b.n;
    Case c(std::string("scan ") + TR::name + "/" + (INCLUSIVE ? "InclusiveU32Sink" : "ExclusiveU32Sink") + (alias ? " in-place" : "") + " n=" + S((long long)n) +
           " np=" + scan_np_names[np_mode] + (route == 1 ? " route=reduce+apply2" : " route=reduce+tiles+apply"));
    const u64 npv = np_mode == 1 ? n : np_mode == 2 ? n - 1 : np_mode == 3 ? n - SCAN_TILE : n + 5;
    const u64 n_eff = np_mode == 0 ? n : std::min(npv, n); // (a count beyond the host's n is clamped to it)
    const u32 *d_np = nullptr;
    if (np_mode) {
        const u32 v = (u32)npv;
        b.np.up(&v, 4);
        d_np = b.np.p<u32>();
    }
    if (alias && n) CK(hipMemcpy(b.out.p(), b.in32.p(), n * 4, hipMemcpyDeviceToDevice));
    else b.out.fill(0xEE);
    b.tiles.fill(0x77), b.total.fill(0x77);
    const F f = scan_fn<F>(alias ? b.out.p() : TR::bytes ? b.in8.p() : b.in32.p());
    G g;
    g.out = b.out.p<u32>();
    u64 *ts = b.tiles.p<u64>(), *d_total = b.total.p<u64>();
    const u32 nt = b.nt;
    hipLaunchKernelGGL((scan_reduce_kernel<F>), dim3(nt), dim3(256), 0, 0, f, n, ts, d_np);
    if (route == 1) {
        hipLaunchKernelGGL((scan_apply2_kernel<F, G>), dim3(nt), dim3(256), 0, 0, f, g, n, (const u64 *)ts, d_np, d_total);
    } else {
        hipLaunchKernelGGL(scan_tiles_kernel<0>, dim3(1), dim3(1024), 0, 0, ts, nt, d_total);
        hipLaunchKernelGGL((scan_apply_kernel<F, G>), dim3(nt), dim3(256), 0, 0, f, g, n, (const u64 *)ts, d_np);
    }
    launched();
    const auto got = b.out.get<u32>(n);
    u64 run = 0;
    for (u64 i = 0; i < n && !c.bad; i++) {
        u32 want;
        if (i < n_eff) {
            const u64 v = TR::term(b.h32[i], b.h8[i]);
            want = INCLUSIVE ? (u32)(run + v) : (u32)run; // (the sinks truncate)
            run += v;
        } else {
            want = alias ? b.h32[i] : SCAN_UNTOUCHED; // past the device's length nothing is written
        }
        if (got[i] != want) c.miss(i < n_eff ? "out" : "out past the length", (long)i, got[i], want);
    }
    if (!c.bad) {
        u64 total = 0;
        b.total.down(&total, 8);
        if (total != run) c.miss("grand total", 0, total, run);
    }
    c.flag("canaries", b.out.intact() && b.tiles.intact() && b.total.intact() && b.in32.intact() && b.in8.intact());
}
template <typename F>
static void scan_both_sinks(ScanBufs &b, int np_mode, int route, bool alias) {
    scan_case<F, ExclusiveU32Sink, false>(b, np_mode, route, alias);
    scan_case<F, InclusiveU32Sink, true>(b, np_mode, route, alias);
}

static void group_scan() {
    const u64 T1 = (u64)SCAN_TILE * 1024, T2 = (u64)SCAN_TILE * SCAN2_MAX_TILES;
    const u64 sizes[] = {0, 1, 255, 256, 257, 2047, 2048, 2049, T1, T1 + 1, T2, T2 + 1};
    for (u64 n : sizes) {
        ScanBufs b(n);
        const bool big = n >= T1;
        for (int route = 1; route <= 2; route++) {
            if (route == 1 && b.nt > SCAN2_MAX_TILES) continue; // the two-kernel route stops at SCAN2_MAX_TILES tiles
            for (int np_mode = 0; np_mode < 5; np_mode++) {
                if ((np_mode == 2 && n < 1) || (np_mode == 3 && n < (u64)SCAN_TILE)) continue;
                if (!big) { // every functor, both sinks, every np
                    scan_both_sinks<ArrU32Fn>(b, np_mode, route, false);
                    scan_both_sinks<ArrU8Fn>(b, np_mode, route, false);
                    scan_both_sinks<ArrU8Bit0Fn>(b, np_mode, route, false);
                    scan_both_sinks<ArrI32Fn>(b, np_mode, route, false);
                    if (np_mode == 0 || np_mode == 2) scan_both_sinks<ArrU32Fn>(b, np_mode, route, true), scan_both_sinks<ArrI32Fn>(b, np_mode, route, true);
                } else { // 2 M and 8 M elements: every functor and sink once, every np once, the two in-place pairs of kx_ends and kx_depth
                    scan_case<ArrU32Fn, ExclusiveU32Sink, false>(b, np_mode, route, false);
                    if (np_mode) continue;
                    scan_case<ArrU8Fn, InclusiveU32Sink, true>(b, 0, route, false);
                    scan_case<ArrU8Bit0Fn, ExclusiveU32Sink, false>(b, 0, route, false);
                    scan_case<ArrI32Fn, InclusiveU32Sink, true>(b, 0, route, false);
                    scan_case<ArrU32Fn, ExclusiveU32Sink, false>(b, 0, route, true);
                    scan_case<ArrI32Fn, InclusiveU32Sink, true>(b, 0, route, true);
                }
            }
        }
    }
    for (u32 nt : {1u, 1023u, 1024u, 1025u, 2048u, 2049u, 5000u}) { // scan_tiles_kernel on its own: the carry across rounds of 1024
        Case c("scan scan_tiles_kernel tiles=" + S(nt));
        Rng r(77 + nt);
        std::vector<u64> v(nt), want(nt);
        u64 run = 0;
        for (u32 i = 0; i < nt; i++) v[i] = r.next() >> (i % 3 == 0 ? 0 : 20), want[i] = run, run += v[i]; // (sums modulo 2^64)
        Guarded ts((size_t)nt * 8), total(8);
        ts.up(v.data(), (size_t)nt * 8);
        hipLaunchKernelGGL(scan_tiles_kernel<0>, dim3(1), dim3(1024), 0, 0, ts.p<u64>(), nt, total.p<u64>());
        launched();
        c.eq("exclusive tile sums", ts.get<u64>(nt), want);
        u64 t = 0;
        total.down(&t, 8);
        if (t != run) c.miss("total", 0, t, run);
        c.flag("canaries", ts.intact() && total.intact());
    }
}
