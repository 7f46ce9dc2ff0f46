// pjb_memory.hip.h -- what a context does when a device allocation does not fit, as pure functions: whether a request passes the context's
// own limit (fits_limit), what the context gives back before it tries again (plan_room), and the sizes a target's slab is asked for, in
// order (slab_sizes).  Host code with no context, no HIP call and no globals -- values in, values out --: tests/cpp/memory_policy.cc runs
// it on a machine without a GPU.  Included by pjb_host.hip.h, whose counted allocator (dev_alloc) applies the results.
#pragma once
#include <algorithm>
#include <cstddef>

// the categories pjb_memory reports (include/portcullis_amd.h), in its order
enum MemCat { MEM_GENOMES = 0, MEM_SLABS_OPEN, MEM_SLABS_POOLED, MEM_STAGING, MEM_SCRATCH, MEM_ROWS, MEM_OTHER, MEM_NCAT };

// pjb_set_option("mem_limit", n): n == 0 is "no limit of the context's own".  (want + held cannot wrap: both are sizes of device memory.)
inline bool fits_limit(size_t want, size_t held, size_t limit) { return limit == 0 || (want <= limit && held <= limit - want); }

// what a context holds without needing it when an allocation of `want` bytes has failed
struct RoomState {
    size_t want, held, limit;
    bool by_limit;       // the context's own limit refused the request (else: the runtime did, and nobody knows by how much)
    size_t parked;       // buffers that were replaced by larger ones and wait for their hipFree (the graveyard)
    size_t pooled_slabs; // slabs of collected targets
    size_t pooled_stage; // stage buffers no target is using
};
// Give back, in this order: the parked buffers (nothing will ever use them), the pooled slabs, the pooled stage buffers (both are only there
// to save the next target an allocation) -- each kind whole, and no more kinds than the request needs.  A request the limit refused
// and that all of it together would not make fit gives up at once and keeps the pools: the caller frees what it is using (collects a
// chain) and comes back.  After a refusal by the runtime everything goes: the room it takes is not known.
struct RoomPlan {
    bool parked, slabs, stage; // release these
    bool retry;                // then ask once more (false: report PJB_ERR_NOMEM)
};
inline RoomPlan plan_room(const RoomState &s) {
    RoomPlan p = {false, false, false, false};
    if (!s.by_limit) {
        p.parked = s.parked > 0;
        p.slabs = s.pooled_slabs > 0;
        p.stage = s.pooled_stage > 0;
        p.retry = p.parked || p.slabs || p.stage;
        return p;
    }
    if (s.want > s.limit) return p; // (never fits)
    const size_t over = s.held > s.limit - s.want ? s.held - (s.limit - s.want) : 0; // bytes that must go
    if (over == 0) { // (it fits already: the caller's figures were stale)
        p.retry = true;
        return p;
    }
    // (sums of parts of `held`, which is a size of device memory: no wrap)
    if (s.parked + s.pooled_slabs + s.pooled_stage < over) return p;
    size_t got = 0;
    if (s.parked) p.parked = true, got += s.parked;
    if (got < over && s.pooled_slabs) p.slabs = true, got += s.pooled_slabs;
    if (got < over && s.pooled_stage) p.stage = true, got += s.pooled_stage;
    p.retry = true;
    return p;
}

// The exact size is a slab's last resort: it leaves a target's records in one small allocation per array.  While the context holds slabs
// its caller can get back -- a queued chain's, another open target's: collecting returns them to the pool -- a request that only the exact
// size would meet is refused first (PJB_ERR_NOMEM, retryable); the repeat of a refused call with nothing freed in between gets it.
inline bool slab_exact_now(bool others_hold_slabs, bool repeat_nothing_freed) { return !others_hold_slabs || repeat_nothing_freed; }

// The sizes a new slab is asked for, in order (n of them, 1 or 2): 128 MB or what the target is expected to take in all (its first slab),
// then exactly what the request needs.  Each is asked for once; the release above comes between a failure of the first and its repeat.
constexpr size_t SLAB_BYTES = (size_t)128 << 20;
inline int slab_sizes(size_t bytes, size_t hint, bool first_of_target, size_t out[2]) {
    out[0] = std::max(bytes, std::max(SLAB_BYTES, first_of_target ? hint : (size_t)0));
    out[1] = bytes;
    return out[0] > bytes ? 2 : 1;
}
