// The limit policy of a `junc` chain (pjb_limits.hip.h) on a machine without a GPU: first_limits, relimit, attempt_budget, group_span.
// Every expected value is written out by hand from the expressions of pjb_api.hip at commit e9bda34 (the line is given with each group);
// nothing here is computed by calling the function under test.  Stand-alone host program: tests/test_host_chain_limits.py builds it with
// the address and undefined-behaviour sanitizers linked in and runs it.
#include "pjb_host.hip.h"
#include "pjb_limits.hip.h"

static int g_checks = 0, g_failed = 0;
#define CHECK_EQ(got, want)                                                                                                      \
    do {                                                                                                                         \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                                           \
        g_checks++;                                                                                                              \
        if (g_ != w_) {                                                                                                          \
            g_failed++;                                                                                                          \
            fprintf(stderr, "%s:%d: %s is %lld, expected %lld (%s)\n", __FILE__, __LINE__, #got, g_, w_, #want);                 \
        }                                                                                                                        \
    } while (0)

// a lone target of 1 000 reads in a fresh context (junc_seen 0, lbits_seen 18, junc_per_read 0, sort_floor 2^16, dense ids, run sort)
static LimitInputs fresh(int64_t n_reads) { return LimitInputs{n_reads, 1, 200000, true, 0, 18, 0.0, 1u << 16, true, true}; }

// what such a chain is queued with: pair_limit 4 721, junc_limit 4 096, list_cap 0 (gen_list_cap), sort_limit 0, key 18 + 18 bits
static ContigLimits base_limits() {
    ContigLimits lim;
    lim.pair_limit = 4721;
    lim.junc_limit = 4096;
    lim.kf.raw = 0;
    lim.kf.lbits = 18;
    lim.kf.total_bits = 36;
    lim.dense = true;
    lim.run_sort = true;
    return lim;
}
static ContigStats stats(u32 overflow) { // a control block whose coordinates lie inside a target of 200 000 bases
    ContigStats cs;
    memset(&cs, 0, sizeof cs);
    cs.overflow = overflow;
    cs.max_end = 150000;
    cs.max_nlen = 1000;
    return cs;
}
static const int32_t REF = 200000; // bits_of: 18 (2^17 = 131 072 < 200 000 < 2^18)

#define CHECK_LIMITS(lim, pl, jl, lc, sl, raw_, lbits_, total_, dense_, run_) \
    do {                                                                      \
        CHECK_EQ((lim).pair_limit, pl);                                       \
        CHECK_EQ((lim).junc_limit, jl);                                       \
        CHECK_EQ((lim).list_cap, lc);                                         \
        CHECK_EQ((lim).sort_limit, sl);                                       \
        CHECK_EQ((lim).kf.raw, raw_);                                         \
        CHECK_EQ((lim).kf.lbits, lbits_);                                     \
        CHECK_EQ((lim).kf.total_bits, total_);                                \
        CHECK_EQ((lim).dense, dense_);                                        \
        CHECK_EQ((lim).run_sort, run_);                                       \
    } while (0)

// ---- first limits: e9bda34 pjb_api.hip lines 651-662
static void test_first_limits() {
    // 651-652: guess = min(0xffffff00, n * 5 / 8 + 4096), pair_limit = max(guess, 4096); 653: junc_limit = max(pair_limit / 32, 4096, ...)
    ContigLimits a = first_limits(fresh(0));
    CHECK_LIMITS(a, 4096, 4096, 0, 0, 0, 18, 36, 1, 1);
    a = first_limits(fresh(1000)); // 625 + 4096
    CHECK_LIMITS(a, 4721, 4096, 0, 0, 0, 18, 36, 1, 1);
    a = first_limits(fresh(10000000000ll)); // 6.25e9 + 4096 is over the cap; 0xffffff00 / 32 = 134 217 720
    CHECK_LIMITS(a, 0xffffff00u, 134217720u, 0, 0, 0, 18, 36, 1, 1);
    a = first_limits(fresh(1000000)); // 625 000 + 4 096 = 629 096; / 32 = 19 659
    CHECK_EQ(a.pair_limit, 629096);
    CHECK_EQ(a.junc_limit, 19659);
    // 653: 2 * junc_seen, * 2 again for a group
    LimitInputs in = fresh(1000);
    in.junc_seen = 100000;
    CHECK_EQ(first_limits(in).junc_limit, 200000);
    in.n_members = 3;
    CHECK_EQ(first_limits(in).junc_limit, 400000);
    in.junc_seen = 1000; // 4 000 < 4 096: the floor
    CHECK_EQ(first_limits(in).junc_limit, 4096);
    // 654: without a genome no pair may be worked on; the junction limit is what the pair limit would have given
    in = fresh(1000000);
    in.genomes_ok = false;
    a = first_limits(in);
    CHECK_EQ(a.pair_limit, 0);
    CHECK_EQ(a.junc_limit, 19659);
    // 662: sort_limit 0 while junc_per_read == 0, then min(junc_limit, max(sort_floor, min(4e9, 2 * jpr * n + 64)))
    in = fresh(1000000);
    in.junc_per_read = 0.0078125; // 2^-7: 2 * jpr * 1e6 + 64 = 15 689 exactly
    CHECK_EQ(first_limits(in).sort_limit, 19659); // max(65 536, 15 689) capped by junc_limit 19 659
    in.junc_seen = 50000;                         // junc_limit 100 000
    CHECK_EQ(first_limits(in).junc_limit, 100000);
    CHECK_EQ(first_limits(in).sort_limit, 65536); // the floor
    in.sort_floor = 1;
    CHECK_EQ(first_limits(in).sort_limit, 15689);
    in = fresh(10000000000ll);
    in.junc_per_read = 1.0; // 2e10 + 64 -> 4e9, capped by junc_limit 134 217 720
    CHECK_EQ(first_limits(in).sort_limit, 134217720u);
    // 655-657: lbits = max(1, lbits_seen), total_bits = lbits + max(1, bits_of(max(vlen, 1)))
    in = fresh(1000);
    in.vlen = 1;
    CHECK_EQ(first_limits(in).kf.total_bits, 18 + 1);
    in.vlen = 0;
    CHECK_EQ(first_limits(in).kf.total_bits, 18 + 1);
    in.vlen = 1ll << 18; // bits_of(2^18) = 19
    CHECK_EQ(first_limits(in).kf.total_bits, 18 + 19);
    in.vlen = (1ll << 31) - (1ll << 20); // 2 146 435 072 < 2^31: 31 bits
    CHECK_EQ(first_limits(in).kf.total_bits, 18 + 31);
    in.lbits_seen = 0;
    CHECK_EQ(first_limits(in).kf.lbits, 1);
    CHECK_EQ(first_limits(in).kf.total_bits, 1 + 31);
    in.lbits_seen = 25;
    CHECK_EQ(first_limits(in).kf.lbits, 25);
    CHECK_EQ(first_limits(in).kf.raw, 0);
    // 658-659: the context's switches
    in = fresh(1000);
    in.dense_ids = false;
    CHECK_EQ(first_limits(in).dense, 0);
    CHECK_EQ(first_limits(in).run_sort, 1);
    in.run_sort = false;
    CHECK_EQ(first_limits(in).run_sort, 0);
}

// ---- relimit, one bit at a time: e9bda34 pjb_api.hip lines 804-836
static void test_relimit() {
    ContigLimits lim;
    ContigStats cs;
    Relimit v;
    // 804-810 OVF_PAIRS: pair_limit = n_pairs + 64, junc_limit = max(junc_limit, pair_limit / 8)
    lim = base_limits();
    cs = stats(OVF_PAIRS);
    cs.n_pairs = 1000000;
    v = relimit(lim, cs, REF, false);
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_EQ(v.run_sort_off, 0);
    CHECK_LIMITS(lim, 1000064, 125008, 0, 0, 0, 18, 36, 1, 1); // 1 000 064 / 8 = 125 008
    lim = base_limits();
    lim.junc_limit = 200000; // already above an eighth of the pairs: stays
    relimit(lim, cs, REF, false);
    CHECK_LIMITS(lim, 1000064, 200000, 0, 0, 0, 18, 36, 1, 1);
    // 805-807: the error, and its two texts
    for (int group = 0; group < 2; group++) {
        lim = base_limits();
        cs = stats(OVF_PAIRS);
        cs.n_pairs = 0xfffffff0ull;
        v = relimit(lim, cs, REF, group != 0);
        CHECK_EQ(v.what, Relimit::TOO_MANY_PAIRS);
        CHECK_EQ(v.run_sort_off, 0);
        CHECK_LIMITS(lim, 4721, 4096, 0, 0, 0, 18, 36, 1, 1);
    }
    CHECK_EQ(strcmp(too_many_pairs_text(false), "finish: more than 2^32 spliced pairs on one target are not supported"), 0);
    CHECK_EQ(strcmp(too_many_pairs_text(true), "finish_group: more than 2^32 spliced pairs in one group: finish its targets in smaller groups"), 0);
    // (808 as the parent has it: `(u32)cs.n_pairs + 64` is a 32-bit sum, and 0xffffffc0 .. 0xffffffef pairs pass the test of line 805 and
    // wrap -- 0xffffffef + 64 = 2^32 + 47.  A finding of this test, kept as it is: profiles/chain_collector_checks.txt.)
    lim = base_limits();
    cs.n_pairs = 0xffffffefull;
    v = relimit(lim, cs, REF, false);
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_EQ(lim.pair_limit, 47);
    cs.n_pairs = 0xffffffbfull; // the last count that does not wrap: 0xffffffff
    lim = base_limits();
    relimit(lim, cs, REF, false);
    CHECK_EQ(lim.pair_limit, 0xffffffffu);
    CHECK_EQ(lim.junc_limit, 0x1fffffffu);
    // 811-826 OVF_KEYFMT, coordinates inside the sequence: lbits = max(1, bits_of(max_nlen)), total_bits = lbits + max(1, bits_of(max(ref_len, 1)))
    lim = base_limits();
    cs = stats(OVF_KEYFMT);
    cs.max_nlen = 1 << 18; // 19 bits
    v = relimit(lim, cs, REF, false);
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_LIMITS(lim, 4721, 4096, 0, 0, 0, 19, 19 + 18, 1, 1);
    lim = base_limits();
    v = relimit(lim, cs, REF, true); // (a group whose coordinates are in order is repeated like a lone target)
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_LIMITS(lim, 4721, 4096, 0, 0, 0, 19, 19 + 18, 1, 1);
    lim = base_limits();
    cs.max_end = REF; // (max_end == ref_len is inside)
    cs.max_nlen = 0;  // max(1, bits_of(0))
    relimit(lim, cs, REF, false);
    CHECK_LIMITS(lim, 4721, 4096, 0, 0, 0, 1, 1 + 18, 1, 1);
    // 812, 817-821: weird on a lone target, three ways: raw keys of 32 + 32 bits, dense ids off
    for (int way = 0; way < 3; way++) {
        lim = base_limits();
        cs = stats(OVF_KEYFMT);
        if (way == 0) cs.min_pos = -1;
        if (way == 1) cs.max_end = REF + 1;
        if (way == 2) cs.max_end = -5;
        v = relimit(lim, cs, REF, false);
        CHECK_EQ(v.what, Relimit::REPEAT);
        CHECK_EQ(v.run_sort_off, 0);
        CHECK_LIMITS(lim, 4721, 4096, 0, 0, 1, 32, 64, 0, 1);
        // 813-816: in a group: taken apart, limits untouched
        lim = base_limits();
        v = relimit(lim, cs, REF, true);
        CHECK_EQ(v.what, Relimit::APART);
        CHECK_EQ(v.run_sort_off, 0);
        CHECK_LIMITS(lim, 4721, 4096, 0, 0, 0, 18, 36, 1, 1);
    }
    // 827-829 OVF_JUNC with the sort's digits planned for fewer ids than the buffers hold, and the junctions within the buffers: sort_limit only
    lim = base_limits();
    lim.sort_limit = 1000;
    cs = stats(OVF_JUNC);
    cs.n_junc = 3000;
    v = relimit(lim, cs, REF, false);
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_LIMITS(lim, 4721, 4096, 0, 0, 0, 18, 36, 1, 1);
    lim = base_limits();
    lim.sort_limit = 1000;
    cs.n_junc = 4096; // (n_junc == junc_limit: still within)
    relimit(lim, cs, REF, false);
    CHECK_LIMITS(lim, 4721, 4096, 0, 0, 0, 18, 36, 1, 1);
    // 829 beyond junc_limit, under dense ids: max(n_junc + 64, 4 * junc_limit)
    lim = base_limits();
    cs.n_junc = 10000;
    relimit(lim, cs, REF, false);
    CHECK_LIMITS(lim, 4721, 16384, 0, 0, 0, 18, 36, 1, 1);
    lim = base_limits();
    lim.sort_limit = 1000; // (set, but the buffers were too small as well)
    cs.n_junc = 100000;
    relimit(lim, cs, REF, false);
    CHECK_LIMITS(lim, 4721, 100064, 0, 0, 0, 18, 36, 1, 1);
    // 829 without dense ids: n_junc + 64
    lim = base_limits();
    lim.dense = false;
    cs.n_junc = 10000;
    relimit(lim, cs, REF, false);
    CHECK_LIMITS(lim, 4721, 10064, 0, 0, 0, 18, 36, 0, 1);
    // 829, 835 OVF_JUNC | OVF_DENSE: no * 4 (the repeat sorts full keys), dense ids off
    lim = base_limits();
    cs = stats(OVF_JUNC | OVF_DENSE);
    cs.n_junc = 10000;
    v = relimit(lim, cs, REF, false);
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_LIMITS(lim, 4721, 10064, 0, 0, 0, 18, 36, 0, 1);
    lim = base_limits();
    lim.sort_limit = 1000;
    cs.n_junc = 3000; // sort_only with OVF_DENSE
    relimit(lim, cs, REF, false);
    CHECK_LIMITS(lim, 4721, 4096, 0, 0, 0, 18, 36, 0, 1);
    // 835 OVF_DENSE alone
    lim = base_limits();
    lim.sort_limit = 1000;
    cs = stats(OVF_DENSE);
    v = relimit(lim, cs, REF, false);
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_EQ(v.run_sort_off, 0);
    CHECK_LIMITS(lim, 4721, 4096, 0, 1000, 0, 18, 36, 0, 1);
    // 830-834 OVF_RUNS: the verdict only (run_sort of the context and of every flight is the caller's)
    lim = base_limits();
    cs = stats(OVF_RUNS);
    v = relimit(lim, cs, REF, false);
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_EQ(v.run_sort_off, 1);
    CHECK_LIMITS(lim, 4721, 4096, 0, 0, 0, 18, 36, 1, 1);
    // 836 OVF_LISTS: max(gen_list_cap(pair_limit), (need + need / 4 + 511) & ~255); gen_list_cap(p) = ceil((p / 256 + 2) / 256) * 256
    lim = base_limits(); // gen_list_cap(4 721) = ceil(20 / 256) * 256 = 256
    cs = stats(OVF_LISTS);
    cs.list_need = 100; // (100 + 25 + 511) & ~255 = 512
    v = relimit(lim, cs, REF, false);
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_LIMITS(lim, 4721, 4096, 512, 0, 0, 18, 36, 1, 1);
    lim = base_limits();
    cs.list_need = 5000; // (5000 + 1250 + 511) & ~255 = 6 656
    relimit(lim, cs, REF, false);
    CHECK_LIMITS(lim, 4721, 4096, 6656, 0, 0, 18, 36, 1, 1);
    lim = base_limits();
    lim.pair_limit = 1000000; // gen_list_cap: 3 906 + 2 = 3 908 chunks, ceil(3 908 / 256) = 16, * 256 = 4 096: the other arm
    cs.list_need = 100;
    relimit(lim, cs, REF, false);
    CHECK_LIMITS(lim, 1000000, 4096, 4096, 0, 0, 18, 36, 1, 1);
    // several bits: pairs, key format and lists -- the lists' room follows the NEW pair limit (1 000 064 / 256 + 2 = 3 908 chunks: 4 096)
    lim = base_limits();
    cs = stats(OVF_PAIRS | OVF_KEYFMT | OVF_LISTS);
    cs.n_pairs = 1000000;
    cs.max_nlen = 1 << 18;
    cs.list_need = 100;
    v = relimit(lim, cs, REF, false);
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_EQ(v.run_sort_off, 0);
    CHECK_LIMITS(lim, 1000064, 125008, 4096, 0, 0, 19, 37, 1, 1);
    // several bits: junctions, dense, runs and lists
    lim = base_limits();
    lim.sort_limit = 1000;
    cs = stats(OVF_JUNC | OVF_DENSE | OVF_RUNS | OVF_LISTS);
    cs.n_junc = 10000;
    cs.list_need = 5000;
    v = relimit(lim, cs, REF, false);
    CHECK_EQ(v.what, Relimit::REPEAT);
    CHECK_EQ(v.run_sort_off, 1);
    CHECK_LIMITS(lim, 4721, 10064, 6656, 0, 0, 18, 36, 0, 1);
}

// ---- budget: e9bda34 pjb_api.hip lines 776, 792-796.  `for (;; f.attempt++)`, and a repeat whose overflow word is exactly OVF_LISTS takes the
// increment back while list_attempt < 3; any other one fails at attempt >= 3
static bool run_budget(const char *seq, int &attempt, int &list_attempt) { // L: lists only, O: another overflow, M: lists and junctions
    bool ok = true;
    for (const char *p = seq; *p; p++) ok = attempt_budget(*p == 'L' ? (u32)OVF_LISTS : *p == 'O' ? (u32)OVF_JUNC : (u32)(OVF_LISTS | OVF_JUNC), attempt, list_attempt);
    return ok; // (of the last one)
}
static void test_budget() {
    const char *pass[] = {"LLLOOO", "OOOLLL", "OLOLOL", "LOLOLO", "LLLL", "LLLLOO", "MMM", "LLLMMM"};
    const int attempt_after[] = {3, 3, 3, 3, 1, 3, 3, 3}, list_after[] = {3, 3, 3, 3, 3, 3, 0, 3};
    for (size_t k = 0; k < sizeof pass / sizeof pass[0]; k++) {
        int attempt = 0, list_attempt = 0;
        bool all = true;
        for (size_t n = 1; n <= strlen(pass[k]); n++) { // every prefix passes
            attempt = list_attempt = 0;
            all = all && run_budget(std::string(pass[k], n).c_str(), attempt, list_attempt);
        }
        CHECK_EQ(all, 1);
        CHECK_EQ(attempt, attempt_after[k]);
        CHECK_EQ(list_attempt, list_after[k]);
    }
    // the fourth overflow that is not the lists' alone fails -- whatever the lists have drawn; the fourth for the lists alone draws on `attempt`
    const char *fails[] = {"OOOO", "LLLOOOO", "OLOLOLO", "OOOLLLL", "LLLLOOO", "MMMM", "OMOM"};
    for (size_t k = 0; k < sizeof fails / sizeof fails[0]; k++) {
        int attempt = 0, list_attempt = 0;
        const size_t n = strlen(fails[k]);
        CHECK_EQ(run_budget(std::string(fails[k], n - 1).c_str(), attempt, list_attempt), 1);
        attempt = list_attempt = 0;
        CHECK_EQ(run_budget(fails[k], attempt, list_attempt), 0);
        CHECK_EQ(attempt, 3); // (a refused repeat draws on nothing)
    }
}

// ---- progress: where a bit is set, the limit it names covers the need the control block reports -- a repeat never queues the same
// too-small chain twice.  Counts stay below the 32-bit wraps of the parent's expressions (see the finding above: pairs from 0xffffffc0;
// likewise junctions near 2^32 and a list_need above 3.4e9, which no chain of fewer than 2^32 alignments reports).
static u64 g_rng = 0x9e3779b97f4a7c15ull;
static u64 rnd() { // xorshift64*, fixed seed
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545f4914f6cdd1dull;
}
static u64 rnd_scale(u64 below) { return rnd() % (1 + (below >> (rnd() % 32))); } // every order of magnitude below `below`
static void test_progress() {
    const u32 bits[] = {OVF_PAIRS, OVF_KEYFMT, OVF_JUNC, OVF_DENSE, OVF_LISTS, OVF_RUNS};
    int repeats = 0;
    for (int it = 0; it < 6000; it++) {
        LimitInputs in = fresh((int64_t)rnd_scale(0xffffff00ull));
        in.n_members = 1 + (int)(rnd() % 3);
        in.junc_seen = (u32)rnd_scale(1u << 28);
        in.junc_per_read = rnd() % 2 ? 0.0 : (double)(rnd() % 1000) / 4096.0;
        in.sort_floor = 1u << (rnd() % 20);
        in.dense_ids = rnd() % 4 != 0;
        ContigLimits lim = first_limits(in);
        ContigStats cs = stats(0);
        for (u32 b : bits)
            if (rnd() % 3 == 0) cs.overflow |= b;
        if (!cs.overflow) cs.overflow = bits[rnd() % 6];
        cs.n_pairs = rnd_scale(0xffffffbfull);
        cs.n_junc = (u32)rnd_scale(1u << 31);
        cs.list_need = (u32)rnd_scale(1u << 31);
        cs.max_nlen = (int32_t)rnd_scale(0x7fffffffu);
        cs.min_pos = rnd() % 8 ? 0 : -1;
        cs.max_end = rnd() % 8 ? 150000 : REF + 7;
        const bool group = in.n_members > 1;
        u32 jl = lim.junc_limit; // (line 827 reads the junction limit behind line 809)
        if ((cs.overflow & OVF_PAIRS) && jl < ((u32)cs.n_pairs + 64) / 8) jl = ((u32)cs.n_pairs + 64) / 8;
        const bool sort_only = (cs.overflow & OVF_JUNC) && lim.sort_limit && cs.n_junc <= jl;
        const Relimit v = relimit(lim, cs, REF, group);
        if (v.what != Relimit::REPEAT) continue;
        repeats++;
        int need_bits = 0; // bits of max_nlen, by hand
        for (u64 x = (u64)cs.max_nlen; x; x >>= 1) need_bits++;
        if (cs.overflow & OVF_PAIRS) CHECK_EQ((u64)lim.pair_limit > cs.n_pairs, 1);
        if (cs.overflow & OVF_JUNC) CHECK_EQ(lim.junc_limit > cs.n_junc || sort_only, 1);
        if (cs.overflow & OVF_JUNC) CHECK_EQ(lim.sort_limit, 0);
        if (cs.overflow & OVF_LISTS) CHECK_EQ(lim.list_cap >= cs.list_need, 1);
        if (cs.overflow & OVF_KEYFMT) CHECK_EQ(lim.kf.raw || lim.kf.lbits >= need_bits, 1);
        if (cs.overflow & OVF_DENSE) CHECK_EQ(lim.dense, 0);
        CHECK_EQ(v.run_sort_off, (cs.overflow & OVF_RUNS) != 0);
    }
    CHECK_EQ(repeats > 4000, 1); // (the sweep is not mostly errors and groups taken apart)
}

// ---- group_span: e9bda34 pjb_api.hip lines 615, 715, 1075: ((max(ref_len, 1) + GROUP_GAP) + 63) & ~63, GROUP_GAP 4 096
static void test_group_span() {
    CHECK_EQ(group_span(0), 4160); // 1 + 4096 + 63 = 4160 = 65 * 64
    CHECK_EQ(group_span(1), 4160);
    CHECK_EQ(group_span(63), 4160); // 4222
    CHECK_EQ(group_span(64), 4160); // 4223
    CHECK_EQ(group_span(65), 4224);
    CHECK_EQ(group_span(-7), 4160);
    CHECK_EQ(group_span(INT32_MAX - 8192), 2147479552ll); // 2 147 475 455 + 4 159 = 2 147 479 614 -> 2^31 - 4096: the sum is a 64-bit one
}

int main() {
    test_first_limits();
    test_relimit();
    test_budget();
    test_progress();
    test_group_span();
    printf("chain_limits: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
