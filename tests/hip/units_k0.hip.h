// group k0 of device_units.hip: k0_upper, k0_encode, k0_encode2 and k0_fasta, launched as pjb_api.hip launches them, with base pointers
// that hipMalloc never returns (offset by 1 .. 15 bytes: the byte-wise fallbacks) as well as aligned ones.
#pragma once

static std::vector<uint8_t> every_byte(size_t n, Rng &r) { // all 256 values, the first 256 positions a permutation of them
    std::vector<uint8_t> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (uint8_t)((i * 167u + 13u) & 255u);
    for (size_t i = 256; i < n; i++)
        if (r.u(4) == 0) v[i] = "acgtxXnN"[r.u(8)];
    return v;
}
static std::vector<uint8_t> no_x(std::vector<uint8_t> v) {
    for (uint8_t &c : v)
        if (c == 'X' || c == 'x') c = 'Q';
    return v;
}

static void k0_upper_cases() {
    Rng r(909);
    for (int64_t n : {0, 1, 15, 16, 17, 4095, 4096, 4097})
        for (int off : {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15})
            for (int do_upper = 0; do_upper < 2; do_upper++)
                for (int xcase = 0; xcase < 4; xcase++) { // no X at all; an 'X'; an 'x' only; whatever the bytes hold
                    if (n == 0 && xcase) continue;
                    if ((off % 5) && xcase && xcase < 3 && n > 17) continue; // (the planted cases at every fifth offset of the long inputs)
                    Case c("k0 k0_upper do_upper=" + S(do_upper) + " n=" + S(n) + " offset=" + S(off) + (xcase == 0 ? " no-X" : xcase == 1 ? " X" : xcase == 2 ? " x-only" : " every-byte"));
                    std::vector<uint8_t> in = every_byte((size_t)n, r);
                    if (xcase < 3) in = no_x(in);
                    if (xcase == 1) in[r.u((u32)n)] = 'X';
                    if (xcase == 2) in[r.u((u32)n)] = 'x';
                    const size_t room = (size_t)n + 48; // the bytes around the sequence must come back as they were
                    std::vector<uint8_t> host(room, 'z');
                    std::copy(in.begin(), in.end(), host.begin() + off);
                    Guarded g(room), flag(4);
                    g.up(host.data(), room), flag.fill(0);
                    const int64_t nthreads = (n + 15) / 16;
                    const unsigned nblk = (unsigned)std::max<int64_t>(1, (nthreads + 255) / 256);
                    hipLaunchKernelGGL(k0_upper, dim3(nblk), dim3(256), 0, 0, g.p() + off, n, do_upper, flag.p<int>());
                    launched();
                    std::vector<uint8_t> want = host;
                    int has_x = 0;
                    for (int64_t i = 0; i < n; i++) {
                        uint8_t &ch = want[off + i];
                        if (ch == 'X' || (do_upper && ch == 'x')) has_x = 1;
                        if (do_upper && ch >= 'a' && ch <= 'z') ch = (uint8_t)(ch - 32);
                    }
                    c.eq("bases", g.get<uint8_t>(room), want);
                    const int got_x = flag.get<int>(1)[0];
                    if (got_x != has_x) c.miss("has_x", 0, got_x, has_x);
                    c.flag("canaries", g.intact() && flag.intact());
                }
}

static u32 nt16_of(uint8_t ch, bool &exotic) {
    static const char tab[17] = "=ACMGRSVTWYHKDBN";
    for (u32 k = 0; k < 16; k++)
        if ((uint8_t)tab[k] == ch) return k;
    exotic = true;
    return 0;
}
static void k0_encode_cases() {
    Rng r(910);
    for (int64_t n : {1, 7, 8, 9, 256, 4097})
        for (int off : {0, 3})
            for (int alphabet_only = 0; alphabet_only < 2; alphabet_only++) {
                Case c("k0 k0_encode n=" + S(n) + " offset=" + S(off) + (alphabet_only ? " alphabet-only" : " every-byte"));
                std::vector<uint8_t> in = every_byte((size_t)n, r);
                if (alphabet_only)
                    for (uint8_t &ch : in) ch = (uint8_t)"=ACMGRSVTWYHKDBN"[ch & 15];
                const int64_t n_words = (n + 7) / 8;
                Guarded g((size_t)n + off), codes((size_t)n_words * 4), flag(4);
                g.up(in.data(), (size_t)n, off), flag.fill(0);
                hipLaunchKernelGGL(k0_encode, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, 0, (const uint8_t *)g.p() + off, n, codes.p<u32>(), n_words, flag.p<int>());
                launched();
                std::vector<u32> want((size_t)n_words, 0);
                bool exotic = false;
                for (int64_t i = 0; i < n; i++) want[i >> 3] |= nt16_of(in[i], exotic) << (4 * (i & 7));
                c.eq("codes", codes.get<u32>((size_t)n_words), want);
                const int got = flag.get<int>(1)[0];
                if (got != (exotic ? 1 : 0)) c.miss("exotic_flag", 0, got, exotic ? 1 : 0);
                c.flag("canaries", g.intact() && codes.intact() && flag.intact());
            }
}

static void k0_encode2_cases() {
    Rng r(911);
    for (int64_t n : {1, 63, 64, 65, 4095, 4096, 4097, 64 * 64 * 3 + 5})
        for (int off : {0, 1, 8, 15})
            for (int plant = 0; plant < 7; plant++) { // none; a non-ACGT base at 0, 63, 64, n - 1; a lower-case base; every byte value
                const int64_t at = plant == 1 ? 0 : plant == 2 ? 63 : plant == 3 ? 64 : plant == 4 ? n - 1 : n / 2;
                if (plant && plant < 5 && at >= n) continue;
                Case c("k0 k0_encode2 n=" + S(n) + " offset=" + S(off) +
                       (plant == 0 ? " pure-ACGT" : plant < 4 ? " N-at-" + S(at) : plant == 4 ? " N-at-the-last-base-" + S(at) : plant == 5 ? " lower-case-at-" + S(at) : std::string(" every-byte")));
                std::vector<uint8_t> in((size_t)n);
                for (uint8_t &ch : in) ch = (uint8_t)"ACGT"[r.u(4)];
                if (plant >= 1 && plant <= 4) in[(size_t)at] = 'N';
                if (plant == 5) in[(size_t)at] = (uint8_t)"acgt"[r.u(4)];
                if (plant == 6) {
                    const std::vector<uint8_t> e = every_byte((size_t)n, r);
                    for (int64_t i = 0; i < n; i++)
                        if ((i >> 6) % 3 != 1) in[(size_t)i] = e[(size_t)i]; // (every third stretch stays pure)
                }
                const int64_t n2w = codes2_words(n), nxw = gexc_words(n), all = codes2_alloc_words(n);
                // codes2[0 .. n2w) | K0_CODES2_PAD zero words | bitmap | K0_GEXC_PAD zero words; the pads are zeroed beforehand, as pjb_api.hip does
                std::vector<u32> host((size_t)all, 0xEEEEEEEEu);
                for (int k = 0; k < K0_CODES2_PAD; k++) host[(size_t)n2w + k] = 0;
                for (int k = 0; k < K0_GEXC_PAD; k++) host[(size_t)(n2w + K0_CODES2_PAD + nxw) + k] = 0;
                Guarded g((size_t)n + off), codes2((size_t)all * 4), flag(4);
                g.up(in.data(), (size_t)n, off), codes2.up(host.data(), (size_t)all * 4), flag.fill(0);
                hipLaunchKernelGGL(k0_encode2, dim3((unsigned)(((n + 63) / 64 + 255) / 256)), dim3(256), 0, 0, (const uint8_t *)g.p() + off, n, codes2.p<u32>(),
                                   codes2.p<u32>() + n2w + K0_CODES2_PAD, flag.p<int>());
                launched();
                std::vector<u32> want((size_t)all, 0);
                int any = 0;
                for (int64_t i = 0; i < n; i++) {
                    const uint8_t ch = in[(size_t)i];
                    const u32 code = ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 0u;
                    want[(size_t)(i >> 4)] |= code << (2 * (i & 15));
                    if (!(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T')) {
                        const int64_t s = i >> 6;
                        want[(size_t)(n2w + K0_CODES2_PAD + (s >> 5))] |= 1u << (s & 31);
                        any = 1;
                    }
                }
                c.eq("codes, pads and bitmap", codes2.get<u32>((size_t)all), want);
                const int got = flag.get<int>(1)[0];
                if (got != any) c.miss("any_exc", 0, got, any);
                c.flag("canaries", g.intact() && codes2.intact() && flag.intact());
            }
}

// tests/test_host_fasta_raw.py::delinearize, as a plain loop: base i is byte (i / line_blen) * line_len + i % line_blen; every base a graphic
// character, every terminator byte behind a full line that another base follows not one (a byte past the end counts as '?')
static bool delinearize(const std::vector<uint8_t> &raw, int64_t raw_bytes, int64_t n, int32_t lb, int32_t lw, std::vector<uint8_t> &bases) {
    bases.assign((size_t)n, 0);
    bool fine = true;
    for (int64_t i = 0; i < n; i++) {
        const int64_t src = i / lb * lw + i % lb;
        const uint8_t ch = src < raw_bytes ? raw[(size_t)src] : 0;
        if (src >= raw_bytes || ch <= 32 || ch >= 127) fine = false;
        bases[(size_t)i] = ch;
        if (i % lb == lb - 1 && i + 1 < n)
            for (int32_t k = 0; k < lw - lb; k++) {
                const int64_t t = i / lb * lw + lb + k;
                const uint8_t tb = t < raw_bytes ? raw[(size_t)t] : (uint8_t)'?';
                if (tb > 32 && tb < 127) fine = false;
            }
    }
    return fine;
}
static void fasta_case(const std::string &name, int64_t n, int32_t width, const char *term, int damage) {
    // damage: 0 none; 1 a graphic byte in a terminator; 2 a blank inside a line; 3 raw_bytes one short
    Case c("k0 k0_fasta " + name + " n=" + S(n) + " line=" + S(width) + (strlen(term) == 2 ? " CRLF" : " LF") +
           (damage == 0 ? "" : damage == 1 ? " bad: graphic byte in a terminator" : damage == 2 ? " bad: blank inside a line" : " bad: raw_bytes one short"));
    Rng r(912 + n * 7 + width);
    std::vector<uint8_t> raw;
    for (int64_t i = 0; i < n; i++) {
        raw.push_back((uint8_t)"ACGTacgtNnRYKM"[r.u(14)]);
        if ((i + 1) % width == 0 && i + 1 < n)
            for (const char *t = term; *t; t++) raw.push_back((uint8_t)*t);
    }
    const int32_t lb = (int32_t)std::min<int64_t>(width, n), lw = lb + (int32_t)strlen(term); // (the .fai's line of a record: its first line)
    int64_t raw_bytes = (int64_t)raw.size();
    if (damage == 1) raw[(size_t)lb] = 'A';
    if (damage == 2) raw[(size_t)(lw + lb / 2)] = ' ';
    if (damage == 3) raw_bytes--;
    Guarded draw(raw.size()), out((size_t)n), flag(4);
    draw.up(raw.data(), raw.size()), flag.fill(0), out.fill(0xEE);
    const int64_t nthreads = (n + 15) / 16;
    hipLaunchKernelGGL(k0_fasta, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, 0, (const uint8_t *)draw.p(), raw_bytes, n, lb, lw, out.p(), flag.p<int>());
    launched();
    std::vector<uint8_t> want;
    const bool fine = delinearize(raw, raw_bytes, n, lb, lw, want);
    if (fine != (damage == 0)) c.miss("the case is not what its name says", -1, fine, damage == 0);
    const int got = flag.get<int>(1)[0];
    if (got != (fine ? 0 : 1)) c.miss("bad", 0, got, fine ? 0 : 1);
    if (fine) c.eq("bases", out.get<uint8_t>((size_t)n), want); // (a record that is refused is parsed by the host: its bases here are nobody's)
    c.flag("canaries", draw.intact() && out.intact() && flag.intact());
}

static void group_k0() {
    k0_upper_cases();
    k0_encode_cases();
    k0_encode2_cases();
    fasta_case("short last line", 1234, 60, "\n", 0);
    fasta_case("CRLF", 700, 70, "\r\n", 0);
    fasta_case("whole lines", 50 * 9, 50, "\n", 0);
    fasta_case("one line", 333, 333, "\n", 0);
    fasta_case("one base", 1, 80, "\n", 0);
    fasta_case("many blocks", 256 * 16 * 2 + 77, 61, "\n", 0);
    for (int64_t n : {15, 16, 17, 31, 32, 33, 47, 48, 49}) { // a 16-base thread boundary on a line end, n on either side of it
        fasta_case("thread boundary on a line end", n, 16, "\n", 0);
        fasta_case("thread boundary on a line end", n, 16, "\r\n", 0);
        fasta_case("thread boundary on a line end", n, 32, "\n", 0);
    }
    for (int damage = 1; damage <= 3; damage++) {
        fasta_case("refused", 1234, 60, "\n", damage);
        fasta_case("refused", 700, 70, "\r\n", damage);
        fasta_case("refused", 33, 16, "\n", damage);
    }
}
