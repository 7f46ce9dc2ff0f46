// PinnedPool: page-locked buffers for file bytes on their way to the device, and the gate that decides whose bytes cross.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

#include "../../../include/portcullis_amd.h"

namespace portcullis {

// A few page-locked buffers for the file bytes of large inputs (device ingest): a worker preads straight into one,
// the device thread DMAs from it without the staging copy and hands it back.  Allocated on first use and kept.
class PinnedPool {
    struct Buf {
        uint8_t* p = nullptr;
        size_t cap = 0;
        bool busy = false;
    };
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Buf> bufs;

    size_t pieceBytes = 0;  // > 0: every buffer has exactly this size (the ring of pieces of the streaming ingest)

    // Targets stream their pieces a few at a time, in the order they asked: with every worker's target on its way at once
    // all of them arrive at about the same time -- late -- and the device has nothing to inflate until then (measured:
    // first bgzf_inflate 1.0 s after the contexts were ready, PCIe idle before and after a burst).  A target that has the
    // ring to itself and three others is complete after a few hundred milliseconds and inflates while the next ones cross.
    // (One gate per device thread: a target's pieces, its genome and its kernels all go through the context of the worker
    // that took it, so the targets in transfer must be spread over the contexts.)
    struct Gate {
        std::mutex mu;
        std::condition_variable cv;
        std::vector<int> waiting;  // ranks of the targets that wait (the best rank = the smallest goes first)
        int active = 0;
        uint64_t used = 0;  // slots in use (bit k)
    };
    Gate gates[16];
    int gatePermits = 1 << 30;

public:
    explicit PinnedPool(size_t n, size_t piece = 0) : bufs(n), pieceBytes(piece) {}
    size_t piece() const { return pieceBytes; }
    int readThreads = 1;  // threads a target in transfer reads its pieces with
    void setTransferSlots(int perLane) { gatePermits = std::max(1, perLane); }
    // `rank`: the target's place in the order the run wants its targets to cross (the workers all arrive here in the same
    // instant, when the context is ready: who gets the lock first must not decide that chr1 crosses sixth)
    // returns the slot taken (0 .. slots - 1): the slots differ in how their target's bytes travel
    int enterTransfer(int lane, int rank) {
        Gate& g = gates[lane & 15];
        std::unique_lock<std::mutex> lk(g.mu);
        g.waiting.push_back(rank);
        g.cv.wait(lk, [&] { return g.active < gatePermits && *std::min_element(g.waiting.begin(), g.waiting.end()) == rank; });
        g.waiting.erase(std::find(g.waiting.begin(), g.waiting.end(), rank));
        g.active++;
        int slot = 0;
        while (slot < 63 && (g.used >> slot) & 1) slot++;
        g.used |= 1ull << slot;
        g.cv.notify_all();
        return slot;
    }
    void leaveTransfer(int lane, int slot) {
        Gate& g = gates[lane & 15];
        std::lock_guard<std::mutex> lk(g.mu);
        g.active--;
        g.used &= ~(1ull << slot);
        g.cv.notify_all();
    }
    // PORTCULLIS_REGISTER_SLOT=k: the target in slot k sends pieces of the file's own mapping (page-locked for the copy)
    int registerSlot = -1;
    ~PinnedPool() {
        for (auto& b : bufs) pjb_host_free(b.p);
    }
    // a free buffer of the ring, or nullptr at once (ring pieces only: every buffer has the ring's size once allocated)
    uint8_t* tryAcquire(size_t bytes) { return take(bytes, false); }
    uint8_t* acquire(size_t bytes) { return take(bytes, true); }

private:
    // The buffer is picked and marked busy under one lock (a second caller can never be sent to sleep for a buffer the
    // first one saw); a first-use or growing allocation happens with the slot marked busy and its pointer and size are
    // published under the lock again (release() compares pointers of every slot).
    uint8_t* take(size_t bytes, bool wait) {
        Buf* mine = nullptr;
        {
            std::unique_lock<std::mutex> lk(mu);
            auto anyFree = [&] {
                for (auto& b : bufs)
                    if (!b.busy) return true;
                return false;
            };
            if (!anyFree()) {
                if (!wait) return nullptr;
                cv.wait(lk, anyFree);
            }
            for (auto& b : bufs)  // prefer one that is large enough already
                if (!b.busy && b.cap >= bytes) mine = &b;
            if (!mine)
                for (auto& b : bufs)
                    if (!b.busy) mine = &b;
            mine->busy = true;
            if (mine->cap >= bytes) return mine->p;
        }
        uint8_t* old = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu);
            old = mine->p;
            mine->p = nullptr;
            mine->cap = 0;
        }
        pjb_host_free(old);
        const size_t cap = pieceBytes ? bytes : bytes + bytes / 8;  // (the ring's pieces never grow; page-locking costs ~0.1 s per GB, twice: to get and to give back)
        uint8_t* np = (uint8_t*)pjb_host_alloc(cap);
        std::lock_guard<std::mutex> lk(mu);
        if (!np) {
            mine->busy = false;
            cv.notify_all();
            return nullptr;
        }
        mine->p = np;
        mine->cap = cap;
        return np;
    }

public:
    void release(uint8_t* p) {
        std::lock_guard<std::mutex> lk(mu);
        for (auto& b : bufs)
            if (p && b.p == p) b.busy = false;
        cv.notify_all();
    }
};

}  // namespace portcullis
