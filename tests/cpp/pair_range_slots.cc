// The fragment rule of k4_pairs / k5_frag_reduce (frag_slot, frag_slots, frag_unused_*, frag_slots_limit in pjb_device.hip.h) on a machine
// without a GPU.  The model below walks a sorted id array the way the rule is stated -- a fragment is a maximal run of one id inside one
// range of 64 R pairs -- and checks what every user of the rule relies on: the used slots strictly increase along the array, all lie
// below frag_slots(J, P), the slots left unused are exactly the ones the rule marks, R = 1 gives jid + (i >> 6), and the limit bounds
// the slots of every chain within its limits.  Stand-alone host program: tests/test_host_pair_range.py builds it with the address and
// undefined-behaviour sanitizers linked in and runs it.
#include <random>
#include <vector>

#include "pjb_host.hip.h"

using namespace pjb;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        g_checks++;                                           \
        if (!(cond)) {                                        \
            if (g_failed++ < 20) {                            \
                fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
                fprintf(stderr, __VA_ARGS__);                 \
                fprintf(stderr, "\n");                        \
            }                                                 \
        }                                                     \
    } while (0)

// ascending ids in steps of 0 or 1 that begin at 0: every id below J = last + 1 occurs
static std::vector<u32> random_ids(std::mt19937 &rng, u32 P, double p_step) {
    std::vector<u32> id(P);
    std::bernoulli_distribution step(p_step);
    u32 j = 0;
    for (u32 i = 0; i < P; i++) {
        if (i && step(rng)) j++;
        id[i] = j;
    }
    return id;
}

static void check_array(const std::vector<u32> &id, int shift, const char *what) {
    const u32 P = (u32)id.size(), J = id.back() + 1, n_slots = frag_slots(J, P, shift);
    const u32 range_pairs = 64u << shift;
    std::vector<int> state(n_slots, 0); // 0 untouched, 1 used by a fragment, 2 marked unused
    int64_t before = -1;
    u32 fragments = 0;
    for (u32 i = 0; i < P; i++) {
        const bool junction_head = i == 0 || id[i] != id[i - 1];
        const bool fragment_head = junction_head || i % range_pairs == 0;
        const u32 slot = frag_slot(id[i], i, shift);
        if (shift == 0) CHECK(slot == id[i] + (i >> 6), "%s: pair %u", what, i);
        CHECK(slot < n_slots, "%s: pair %u slot %u of %u", what, i, slot, n_slots);
        if (slot >= n_slots) return;
        if (fragment_head) {
            CHECK((int64_t)slot > before, "%s: pair %u slot %u after %lld", what, i, slot, (long long)before);
            CHECK(state[slot] == 0, "%s: pair %u slot %u taken", what, i, slot);
            state[slot] = 1;
            before = slot;
            fragments++;
        } else {
            CHECK((int64_t)slot == before, "%s: pair %u leaves its fragment's slot", what, i);
        }
        for (int64_t u : {frag_unused_before(id[i], i, junction_head, shift), frag_unused_behind(id[i], i, P, shift)}) {
            if (u < 0) continue;
            CHECK(u < (int64_t)n_slots, "%s: pair %u marks slot %lld of %u", what, i, (long long)u, n_slots);
            if (u >= (int64_t)n_slots) return;
            CHECK(state[(size_t)u] == 0, "%s: pair %u marks slot %lld twice or over a fragment", what, i, (long long)u);
            state[(size_t)u] = 2;
        }
    }
    u32 untouched = 0, marked = 0;
    for (u32 s = 0; s < n_slots; s++) {
        untouched += state[s] == 0;
        marked += state[s] == 2;
    }
    // (a slot that is neither written nor marked would hand k5_frag_reduce whatever the buffer held)
    CHECK(untouched == 0, "%s: %u slots neither used nor marked", what, untouched);
    CHECK(fragments + marked == n_slots, "%s: %u fragments + %u marked != %u", what, fragments, marked, n_slots);
    CHECK(state[n_slots - 1] == 2, "%s: the last slot is not marked", what);
}

static void test_random_arrays() {
    std::mt19937 rng(20240917);
    const u32 sizes[] = {1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 4097};
    const double steps[] = {0.0, 0.004, 0.05, 0.5, 1.0}; // one junction ... every pair a junction
    char what[96];
    for (int shift : {0, 1, 2, 4})
        for (u32 P : sizes)
            for (double p : steps) {
                snprintf(what, sizeof what, "R %d P %u step %.3f", 1 << shift, P, p);
                check_array(random_ids(rng, P, p), shift, what);
            }
    std::uniform_int_distribution<u32> any(1, 5000);
    for (int k = 0; k < 200; k++) {
        const u32 P = any(rng);
        static const int shifts[4] = {0, 1, 2, 4};
        const int shift = shifts[k % 4];
        snprintf(what, sizeof what, "random %d: R %d P %u", k, 1 << shift, P);
        check_array(random_ids(rng, P, k % 3 == 0 ? 0.3 : 0.01), shift, what);
    }
}

// junctions that begin exactly with a range, all of them: the most slots a chain can skip
static void test_heads_on_every_range() {
    for (int shift : {0, 1, 2, 4}) {
        const u32 range_pairs = 64u << shift, P = 5 * range_pairs + 1;
        std::vector<u32> id(P);
        for (u32 i = 0; i < P; i++) id[i] = i / range_pairs;
        check_array(id, shift, "a junction a range");
    }
}

static void test_limit() {
    // frag_slots is monotone in both counts, so the limit at (JL, PL) bounds every chain with J <= JL, P <= PL: checked on a grid, and at
    // the largest limits a chain can have (pair_limit <= 0xffffff00: first_limits)
    for (int shift = 0; shift <= PAIR_RANGE_SHIFT_MAX; shift++) {
        for (u32 PL : {0u, 1u, 63u, 64u, 65u, 4096u, 4721u, 100000u})
            for (u32 JL : {0u, 1u, 4096u, 5000u}) {
                const u32 lim = frag_slots_limit(JL, PL, shift);
                for (u32 P = 0; P <= PL; P += (P < 200 ? 1 : 997))
                    for (u32 J : {0u, JL / 3, JL / 2, JL}) CHECK(frag_slots(J, P, shift) < lim, "R %d: (%u, %u) within (%u, %u)", 1 << shift, J, P, JL, PL);
                CHECK(frag_slots(JL, PL, shift) + 1 == lim, "R %d: limit of (%u, %u)", 1 << shift, JL, PL);
            }
        CHECK(frag_ranges(0xffffff00u, shift) == (u32)((0xffffff00ull + (64ull << shift) - 1) / (64ull << shift)), "R %d: ranges of the largest pair limit", 1 << shift);
        CHECK(frag_slots(5u, 64u << shift, shift) == 6u && frag_slots(5u, (64u << shift) + 1, shift) == 7u, "R %d: a range's edge", 1 << shift);
    }
    CHECK(frag_slots_limit(4096, 4721, 0) == 4096 + 74 + 1, "the limit of a fragment a slice is what it was");
}

int main() {
    test_random_arrays();
    test_heads_on_every_range();
    test_limit();
    printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
