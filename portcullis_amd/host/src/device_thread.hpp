// ---------------------------------------------------------------------------------------------
// DeviceThread: the one thread that talks to a GPU.  It owns the pjb context (created here, so HIP
// start-up overlaps the first BGZF blocks) and executes commands from the decode workers in order:
// genome uploads, batches (of several contigs at once, interleaved) and contig finishes.  Keeping a
// single context per GPU avoids the runtime-lock contention of one context per worker.
// ---------------------------------------------------------------------------------------------
#pragma once

#include <condition_variable>
#include <deque>
#include <future>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include <portcullis/bam/bam_reader.hpp>

#include "../../../include/portcullis_amd.h"
#include "pinned_pool.hpp"

namespace portcullis {

struct ContigDone {
    pjb_region_result rr = {};
    std::vector<pjb_junction_row> rows;
    size_t rowBase = 0;  // --extra: index of rows[0] in the context's row table (pjb_extra_finish's order)
};

class DeviceThread {
public:
    struct Cmd {
        enum Kind { GENOME, BATCH, BAM, FINISH, EXTRA, STOP, BAMEND, FLUSH, ROOM } kind;
        int32_t tid;
        explicit Cmd(Kind k, int32_t t = -1) : kind(k), tid(t) {}
        std::string genome;
        // GENOME with the record's bytes as they are in the FASTA file (page-locked, from rawPool; the device takes the line
        // terminators out): rawBytes > 0
        uint8_t* raw = nullptr;
        size_t rawBytes = 0;
        int32_t lineBases = 0, lineWidth = 0;
        int64_t genomeLen = 0;
        PinnedPool* rawPool = nullptr;
        std::promise<bool>* rawDone = nullptr;  // false: the record is not laid out as its index says (the worker sends the filtered bases)
        bam::ReadBatch batch;
        std::vector<bam::ReadBatch>* spare = nullptr;  // where the batch storage goes back to
        std::mutex* spareMu = nullptr;
        std::promise<ContigDone>* done = nullptr;
        std::promise<void>* seen = nullptr;  // FINISH: fulfilled when the device thread takes the command (everything the worker queued before it -- batches that point at the worker's stack -- has been served)
        // BAM: the target's file bytes for the device-side ingest (bigAlloc'ed; freed by the device thread)
        uint8_t* bamBytes = nullptr;
        size_t bamSize = 0;
        uint32_t bamFirst = 0;
        std::promise<int64_t>* bamDone = nullptr;
        std::promise<std::vector<pjb_extra_row>>* extraDone = nullptr;  // EXTRA: calcExtraMetrics for every row so far
        std::promise<bool>* roomDone = nullptr;  // ROOM: a worker's pjb_bam_begin ran out of device memory -- true: a chain was collected, try again
    };

    // what every device thread of a run is made with
    struct Setup {
        bam::Orientation orientation;
        bam::Strandedness strandedness;
        std::vector<int32_t> lens;  // the targets' lengths (pjb_set_refs)
        std::shared_future<int> deviceCount;
        bool extra = false;
        bool shareGpu = false;   // PORTCULLIS_DEVICES_SHARE_GPU
        bool printPlan = false;  // PJB_PRINT_CHAIN_PLAN
        uint64_t memLimit = 0;   // --device_mem: this context's share (pjb_set_option "mem_limit"; 0: none)
        bool report = false;     // -v / PJB_PROFILE_HOST: the [memory] line when the thread stops
        std::vector<std::string> names;  // the targets' names (messages)
    };
    DeviceThread(int device, const Setup& setup, std::vector<std::vector<int32_t>> chainPlan = {});
    ~DeviceThread();  // STOP, then joins the thread (which destroys the context)

    // blocks until this thread's context exists (or failed): page-locking the file pieces and creating contexts at the same
    // time fight over the runtime's locks (contexts ready at 0.65 s instead of 0.4 s)
    void waitReady() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return ready; });
    }
    // the context, for the calls that may come from other threads (pjb_bam_begin / _piece / _pieces_done); nullptr if its
    // creation failed (the commands then report why)
    pjb_ctx* context() {
        waitReady();
        return sharedCtx;
    }
    bool grouped() const { return !plan.empty(); }
    // A worker's own pjb_bam_begin returned PJB_ERR_NOMEM (pjb_bam_piece never does: it allocates nothing the target needs): this thread
    // makes room as it does for its own calls (makeRoom).  true: something was collected, repeat the call.
    bool askForRoom() {
        std::promise<bool> p;
        std::future<bool> f = p.get_future();
        Cmd c(Cmd::ROOM);
        c.roomDone = &p;
        push(std::move(c));
        return f.get();
    }
    // what a run that ends for want of device memory tells the user: the target, the library's figures, the ways out
    std::string memoryAdvice(int32_t tid) const;
    int lane = 0;  // index among the device threads (the transfer gate of this context)
    void push(Cmd&& c) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return q.size() < cap; });
        q.emplace_back(std::move(c));
        cv.notify_all();
    }

private:
    // ---- the command queue (workers push, this thread takes)
    bool ready = false;
    pjb_ctx* sharedCtx = nullptr;
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Cmd> q;
    size_t cap = 6;  // (commands waiting for the device thread; workers block when it is full)

    // ---- this thread's own state (nobody else reads it)
    pjb_ctx* ctx = nullptr;
    std::map<int32_t, std::string> failed;  // contig -> first error
    std::string fatal;                      // context creation failed
    bool printPlan = false;
    // BAMEND commands whose inflate (started by the target's last piece) is still running: the thread serves other
    // targets meanwhile -- pieces, whose last one starts the next inflate beside this one -- instead of waiting
    std::deque<Cmd> deferred;
    std::set<int32_t> ended;  // targets whose records are complete (BAMEND / BAM taken from the queue)
    int profId = 0;
    double tKind[16] = {0}, tIdle = 0, tCollect = 0, tStart = 0;  // PJB_PROFILE_HOST: where this thread's time goes

    // ---- the chains
    // The chain plan (pjb_plan_groups over the targets this thread will be asked to finish, in index order): a FINISH of a target that
    // belongs to a group of several waits here until the group's last member has been asked for, then the group is queued as ONE
    // kernel chain (pjb_finish_group_begin) -- three chains for a human genome instead of twenty-five, which is what bench.py measures.
    // Empty: every target is a chain of its own (several contexts share the targets, --extra unless PORTCULLIS_CHAIN_PLAN=groups, PORTCULLIS_CHAIN_PLAN=targets).
    std::vector<std::vector<int32_t>> plan;
    std::map<int32_t, size_t> groupOf;  // target -> its group in `plan`
    struct Waiting {                    // the members of a group that have been asked for so far
        std::vector<std::pair<int32_t, std::promise<ContigDone>*>> got;
        bool single = false; // a member failed, the library said "not as a group", or device memory ran short: the members go one by one
        bool begun = false;  // the group has been queued as one chain
    };
    std::vector<Waiting> waiting;  // per group of `plan`
    // Targets are QUEUED on the device (pjb_finish_contig_begin) and collected later (_end): the kernel chains of up
    // to kQueued targets run side by side on the GPU, the device never waits for this thread between targets, and
    // the next target's upload / ingest overlaps the queued chains.  The rows of every target stay in the context's
    // table (rows arrive in queue order; rowsSoFar marks where the next target's begin).  --extra queues the same
    // way (a target's extra metrics are queued when its chain is collected).
    size_t kQueued = 3;  // (the library creates the streams of four control slots up front; deeper ones on a busy device cost seconds)
    struct Pending {
        int32_t tid;
        std::promise<ContigDone>* done; // (the worker thread that owns it waits on its future)
        std::vector<int32_t> tids;      // a group chain: its members, in the order they were named to pjb_finish_group_begin
        std::vector<std::promise<ContigDone>*> dones;
    };
    std::deque<Pending> pending;
    size_t rowsSoFar = 0;
    void beginSingle(int32_t tid, std::promise<ContigDone>* done);
    void beginGroup(Waiting& w);
    void collectOldest();
    void collectReady();  // every chain that has completed, without waiting for one that has not
    void flushChains();   // what still waits for the rest of its group is queued, every queued chain is collected

    // ---- device memory (--device_mem, or a device that is simply full)
    // A submit call (pjb_submit_batch, pjb_submit_bam, pjb_bam_end) that returns PJB_ERR_NOMEM has left its target as it was: makeRoom marks
    // every group that still waits for members as `single`, queues what is present of them as chains of their own, and collects the oldest
    // queued chain -- whose slabs go back to the pool --; withRoom repeats the call until it succeeds or nothing is left to collect, and
    // then once more.
    bool makeRoom();
    template <typename F>
    int withRoom(F call) {
        int rc;
        while ((rc = call()) == PJB_ERR_NOMEM && makeRoom()) {
        }
        if (rc == PJB_ERR_NOMEM) rc = call();  // (nothing is left to collect: the repeat gets the library's last resort, slabs of exactly the bytes needed)
        return rc;
    }
    std::string describe(const char* call, int rc, int32_t tid) const;  // "<call>: <the library's message>", with memoryAdvice after PJB_ERR_NOMEM
    uint64_t memLimit = 0;
    bool report = false;
    std::vector<std::string> names;
    size_t flushedEarly = 0;                 // groups that went target by target because memory ran short
    void reportMemory();

    void run(int device, const Setup& setup);
    void createContext(int device, const Setup& setup);
    int readyDeferred();
    Cmd next();
    void serve(Cmd& c);
    void serveGenome(Cmd& c, const std::string& err);
    void serveFinish(Cmd& c, const std::string& err);
};

}  // namespace portcullis
