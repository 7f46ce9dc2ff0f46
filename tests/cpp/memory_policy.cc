// The device-memory policy of a context (pjb_memory.hip.h) on a machine without a GPU: fits_limit, plan_room, slab_sizes.  Every
// expected value is written out by hand from the rule as include/portcullis_amd.h states it (pjb_memory_info); nothing here is
// computed by calling the function under test.  Stand-alone host program: tests/test_host_device_mem.py builds it with the address
// and undefined-behaviour sanitizers linked in and runs it.
#include "pjb_memory.hip.h"

#include <cstdint>
#include <cstdio>

static int g_checks = 0, g_failed = 0;
#define CHECK_EQ(got, want)                                                                                      \
    do {                                                                                                         \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                           \
        g_checks++;                                                                                              \
        if (g_ != w_) {                                                                                          \
            g_failed++;                                                                                          \
            fprintf(stderr, "%s:%d: %s is %lld, expected %lld (%s)\n", __FILE__, __LINE__, #got, g_, w_, #want); \
        }                                                                                                        \
    } while (0)
#define CHECK_PLAN(p, parked_, slabs_, stage_, retry_) \
    do {                                               \
        CHECK_EQ((p).parked, parked_);                 \
        CHECK_EQ((p).slabs, slabs_);                   \
        CHECK_EQ((p).stage, stage_);                   \
        CHECK_EQ((p).retry, retry_);                   \
    } while (0)

static const size_t MB = (size_t)1 << 20;

static void test_fits_limit() {
    CHECK_EQ(fits_limit(1, 0, 0), 1);                 // no limit
    CHECK_EQ(fits_limit(SIZE_MAX, SIZE_MAX, 0), 1);   // no limit: nothing is added up
    CHECK_EQ(fits_limit(100, 900, 1000), 1);          // exactly at the limit
    CHECK_EQ(fits_limit(101, 900, 1000), 0);          // one byte beyond
    CHECK_EQ(fits_limit(1001, 0, 1000), 0);           // larger than the limit itself
    CHECK_EQ(fits_limit(0, 1000, 1000), 1);
    CHECK_EQ(fits_limit(1, 2000, 1000), 0);           // held beyond a limit that was lowered meanwhile
    CHECK_EQ(fits_limit(SIZE_MAX, 16, SIZE_MAX - 8), 0); // (want + held would wrap)
}

static void test_plan_room_by_limit() {
    // limit 1000, held 900, want 200: 100 bytes must go
    RoomState s = {200, 900, 1000, true, 0, 0, 0};
    CHECK_PLAN(plan_room(s), 0, 0, 0, 0); // nothing to give back: give up
    s.parked = 100;
    CHECK_PLAN(plan_room(s), 1, 0, 0, 1); // the parked buffers suffice: the pools stay
    s.parked = 50;
    s.pooled_slabs = 40;
    CHECK_PLAN(plan_room(s), 0, 0, 0, 0); // 90 < 100: give up at once, and nothing is released
    s.pooled_stage = 10;
    CHECK_PLAN(plan_room(s), 1, 1, 1, 1); // 50 + 40 + 10: all three kinds, in that order
    s.pooled_slabs = 60;
    CHECK_PLAN(plan_room(s), 1, 1, 0, 1); // 50 + 60 suffice: the stage buffers stay
    s.parked = 0;
    s.pooled_slabs = 128 * MB;
    CHECK_PLAN(plan_room(s), 0, 1, 0, 1); // nothing parked: the slabs alone
    s.pooled_slabs = 0;
    s.pooled_stage = 100;
    CHECK_PLAN(plan_room(s), 0, 0, 1, 1); // the stage buffers alone
    // a request larger than the limit never fits, whatever is released
    RoomState big = {2000, 900, 1000, true, 500, 500, 500};
    CHECK_PLAN(plan_room(big), 0, 0, 0, 0);
    // the figures moved on between the refusal and the plan (another thread freed): ask again, release nothing
    RoomState stale = {100, 900, 1000, true, 50, 50, 50};
    CHECK_PLAN(plan_room(stale), 0, 0, 0, 1);
    // held beyond a limit that was lowered: want 10, limit 1000, held 1200 -> 210 must go
    RoomState low = {10, 1200, 1000, true, 100, 100, 9};
    CHECK_PLAN(plan_room(low), 0, 0, 0, 0); // 209 < 210
    low.pooled_stage = 10;
    CHECK_PLAN(plan_room(low), 1, 1, 1, 1);
}

static void test_plan_room_by_runtime() {
    // the runtime refused: the room it takes is not known, everything that is held without need goes
    RoomState s = {200, 900, 0, false, 0, 0, 0};
    CHECK_PLAN(plan_room(s), 0, 0, 0, 0); // nothing to give back: give up
    s.parked = 1;
    CHECK_PLAN(plan_room(s), 1, 0, 0, 1);
    s.pooled_slabs = 1;
    s.pooled_stage = 1;
    CHECK_PLAN(plan_room(s), 1, 1, 1, 1);
    s.parked = 0;
    s.pooled_slabs = 0;
    CHECK_PLAN(plan_room(s), 0, 0, 1, 1);
    s.limit = 1000; // (a limit that did not bite changes nothing)
    CHECK_PLAN(plan_room(s), 0, 0, 1, 1);
}

static void test_slab_sizes() {
    size_t out[2] = {0, 0};
    // a small request: 128 MB first, then the exact size
    CHECK_EQ(slab_sizes(4096, 0, true, out), 2);
    CHECK_EQ(out[0], 128 * MB);
    CHECK_EQ(out[1], 4096);
    // a target's first slab takes the hint where it is larger
    CHECK_EQ(slab_sizes(4096, 300 * MB, true, out), 2);
    CHECK_EQ(out[0], 300 * MB);
    CHECK_EQ(out[1], 4096);
    // ... a later slab does not
    CHECK_EQ(slab_sizes(4096, 300 * MB, false, out), 2);
    CHECK_EQ(out[0], 128 * MB);
    // a hint below 128 MB changes nothing
    CHECK_EQ(slab_sizes(4096, 1 * MB, true, out), 2);
    CHECK_EQ(out[0], 128 * MB);
    // a request of 128 MB and more is asked for once, as it is
    CHECK_EQ(slab_sizes(128 * MB, 0, true, out), 1);
    CHECK_EQ(out[0], 128 * MB);
    CHECK_EQ(slab_sizes(200 * MB, 100 * MB, true, out), 1);
    CHECK_EQ(out[0], 200 * MB);
    CHECK_EQ(out[1], 200 * MB);
}

static void test_slab_exact_now() {
    CHECK_EQ(slab_exact_now(false, false), 1); // nobody else holds slabs: the exact size at once
    CHECK_EQ(slab_exact_now(true, false), 0);  // a chain to collect, another open target: refused first
    CHECK_EQ(slab_exact_now(true, true), 1);   // the repeat of a refused call, nothing freed in between
    CHECK_EQ(slab_exact_now(false, true), 1);
}

int main() {
    test_slab_exact_now();
    test_fits_limit();
    test_plan_room_by_limit();
    test_plan_room_by_runtime();
    test_slab_sizes();
    printf("memory_policy: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
