// DeviceThread: the command loop of one device context and the book-keeping of its kernel chains.
#include "device_thread.hpp"

#include <atomic>
#include <chrono>
#include <cstring>

#include <portcullis/junction_builder.hpp>

#include "host_profile.hpp"

namespace portcullis {

using std::cerr;
using std::endl;

HostProfile g_prof;

static const char* const kTryHostIngest = " (--ingest host decodes the file on the host threads and streams batches instead)";

DeviceThread::DeviceThread(int device, const Setup& setup, std::vector<std::vector<int32_t>> chainPlan) {
    plan = std::move(chainPlan);
    for (size_t g = 0; g < plan.size(); g++)
        for (int32_t t : plan[g]) groupOf[t] = g;
    waiting.resize(plan.size());
    printPlan = setup.printPlan;
    memLimit = setup.memLimit;
    report = setup.report;
    names = setup.names;
    th = std::thread([this, device, setup] { run(device, setup); });
}

DeviceThread::~DeviceThread() {
    push(Cmd(Cmd::STOP));
    th.join();
}

void DeviceThread::createContext(int device, const Setup& setup) {
    try {
        if (setup.deviceCount.get() <= 0)
            throw JunctionBuilderException("No MI355X (HIP device) is visible: the junc hot path runs on the GPU and has no CPU fallback");
        pjb_config cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.abi_version = PJB_ABI_VERSION;
        // PORTCULLIS_DEVICES_SHARE_GPU=1: every device thread of a --devices N run uses GPU 0 (a one-GPU box walks through
        // the N-device code path: worker -> device thread assignment, N contexts, the host merge; never a measurement)
        cfg.device = setup.shareGpu ? 0 : device;
        cfg.orientation = (int32_t)setup.orientation;
        cfg.strandedness = (int32_t)setup.strandedness;
        if (setup.extra) cfg.flags |= PJB_FLAG_EXTRA;
        if (pjb_create(&ctx, &cfg) != PJB_OK) throw JunctionBuilderException(std::string("pjb_create: ") + pjb_last_error(nullptr));
        if (pjb_set_refs(ctx, (int32_t)setup.lens.size(), setup.lens.data()) != PJB_OK)
            throw JunctionBuilderException(std::string("pjb_set_refs: ") + pjb_last_error(ctx));
        if (memLimit && pjb_set_option(ctx, "mem_limit", (int64_t)memLimit) != PJB_OK)
            throw JunctionBuilderException(std::string("pjb_set_option: ") + pjb_last_error(ctx));
    } catch (const std::exception& e) {
        fatal = e.what();
    }
}

void DeviceThread::run(int device, const Setup& setup) {
    createContext(device, setup);
    if (printPlan && !plan.empty()) {
        std::string txt;
        for (auto& g : plan) {
            txt += txt.empty() ? "" : " | ";
            for (size_t k = 0; k < g.size(); k++) txt += (k ? "," : "") + std::to_string(g[k]);
        }
        cerr << "[chain plan] " << plan.size() << " chains: " << txt << endl;
    }
    g_prof.mark("device thread: context ready");
    sharedCtx = fatal.empty() ? ctx : nullptr;
    static std::atomic<int> profIds{0};
    profId = profIds++;
    {
        std::lock_guard<std::mutex> lk(mu);
        ready = true;
        cv.notify_all();
    }
    tStart = HostProfile::now();
    for (;;) {
        Cmd c = next();
        const double t0 = HostProfile::now();
        serve(c);
        const double t1 = HostProfile::now();
        tKind[(int)c.kind & 15] += t1 - t0;
        static const char* kinds[] = {"GENOME", "BATCH", "BAM", "FINISH", "EXTRA", "STOP", "BAMEND", "FLUSH", "ROOM"};
        if (g_prof.events_on) g_prof.event(t0, t1, "dev" + std::to_string(profId) + " " + kinds[c.kind] + " tid " + std::to_string(c.tid));
        if (c.kind == Cmd::STOP) break;
    }
    if (ctx) pjb_destroy(ctx);
}

// ---- the chains --------------------------------------------------------------------------------------------------------------

void DeviceThread::collectOldest() {
    Pending p = std::move(pending.front());
    pending.pop_front();
    std::string err;
    const pjb_junction_row* rows = nullptr;
    int64_t n = 0;
    if (!p.tids.empty()) { // a group: one result per member, the rows member after member in the order of `tids`
        std::vector<pjb_region_result> rr(p.tids.size());
        if (pjb_finish_group_end(ctx, p.tids.data(), (int32_t)p.tids.size(), rr.data()) != PJB_OK) err = std::string("pjb_finish_group: ") + pjb_last_error(ctx);
        else if (pjb_collect(ctx, &rows, &n) != PJB_OK) err = std::string("pjb_collect: ") + pjb_last_error(ctx);
        size_t at = rowsSoFar;
        for (size_t m = 0; m < p.tids.size(); m++) {
            (void)pjb_release_contig(ctx, p.tids[m]);
            if (!err.empty()) {
                p.dones[m]->set_exception(std::make_exception_ptr(JunctionBuilderException(err)));
                continue;
            }
            ContigDone d;
            d.rr = rr[m];
            size_t e = at;
            while (e < (size_t)n && rows[e].refid == p.tids[m]) e++;
            d.rows.assign(rows + at, rows + e);
            d.rowBase = at;
            at = e;
            p.dones[m]->set_value(std::move(d));
        }
        if (err.empty()) rowsSoFar = (size_t)n;
        g_prof.mark(("chain collected: group from target " + std::to_string(p.tids[0])).c_str());
        return;
    }
    ContigDone d;
    if (pjb_finish_contig_end(ctx, p.tid, &d.rr) != PJB_OK) err = std::string("pjb_finish_contig: ") + pjb_last_error(ctx);
    else if (pjb_collect(ctx, &rows, &n) != PJB_OK) err = std::string("pjb_collect: ") + pjb_last_error(ctx);
    else {
        d.rows.assign(rows + rowsSoFar, rows + n);
        d.rowBase = rowsSoFar;
        rowsSoFar = (size_t)n;
    }
    (void)pjb_release_contig(ctx, p.tid);
    if (err.empty()) p.done->set_value(std::move(d));
    else p.done->set_exception(std::make_exception_ptr(JunctionBuilderException(err)));
}

// chains that have completed are collected at once, without ever waiting for one that has not: a chain queued beside
// the inflates of the next targets can take 100 ms and more (their resident workgroups hold the CUs' LDS), and a
// thread that sat in pjb_finish_contig_end for that long held up every other target's commands -- and, through the
// bounded command queue, the workers that read the file (the input stood still whenever this thread waited)
void DeviceThread::collectReady() {
    while (!pending.empty() && ctx && pjb_finish_ready(ctx)) {
        const double t0 = HostProfile::now();
        const int ptid = pending.front().tid;
        collectOldest();
        tCollect += HostProfile::now() - t0;
        g_prof.event(t0, HostProfile::now(), "dev" + std::to_string(profId) + " collect tid " + std::to_string(ptid));
    }
}

void DeviceThread::flushChains() {
    for (auto& w : waiting) beginGroup(w);
    while (!pending.empty()) collectOldest();
}

// ---- device memory -----------------------------------------------------------------------------------------------------------

bool DeviceThread::makeRoom() {
    for (size_t g = 0; g < waiting.size(); g++) {
        Waiting& w = waiting[g];
        if (w.single || w.begun || plan[g].size() < 2) continue;
        w.single = true;
        flushedEarly++;
        if (printPlan) {
            std::string txt;
            for (auto& x : w.got) txt += (txt.empty() ? "" : ",") + std::to_string(x.first);
            cerr << "[chain] device memory ran short: group " << g << " of the plan goes target by target (present: " << (txt.empty() ? "none" : txt) << ")" << endl;
        }
        beginGroup(w);  // (what is present of it, as chains of their own)
    }
    if (pending.empty()) return false;
    collectOldest();
    return true;
}

std::string DeviceThread::memoryAdvice(int32_t tid) const {
    const std::string name = tid >= 0 && (size_t)tid < names.size() ? names[(size_t)tid] : std::to_string(tid);
    return " -- target " + name + " does not fit the device memory this run may hold (limit " + (memLimit ? std::to_string(memLimit) + " bytes" : std::string("none: the device is full")) +
           "): give the run more with a larger --device_mem, or spread its targets over more GPUs with --devices N";
}

std::string DeviceThread::describe(const char* call, int rc, int32_t tid) const {
    std::string msg = std::string(call) + ": " + pjb_last_error(ctx);
    if (rc == PJB_ERR_NOMEM) msg += memoryAdvice(tid);
    return msg;
}

// (one call, when the thread stops: the library keeps the peak, what the slabs held at that moment and the largest target itself)
void DeviceThread::reportMemory() {
    pjb_memory m;
    if (!report || !ctx || pjb_memory_info(ctx, &m) != PJB_OK) return;
    const int64_t big = m.largest_target;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    cerr << "[memory] peak held " << m.peak_held << " (records " << m.peak_records << ", other " << m.peak_held - m.peak_records << "); limit "
         << (m.limit ? std::to_string(m.limit) : std::string("none")) << "; groups flushed early: " << flushedEarly << "; largest target: "
         << (big < 0 ? std::string("none") : (size_t)big < names.size() ? names[(size_t)big] : std::to_string(big)) << " " << m.largest_target_bytes << endl;
}

void DeviceThread::beginSingle(int32_t tid, std::promise<ContigDone>* done) {
    while (pending.size() >= kQueued) collectOldest();
    if (const int rc = pjb_finish_contig_begin(ctx, tid)) {
        const std::string err = describe("pjb_finish_contig", rc, tid);
        (void)pjb_release_contig(ctx, tid);
        done->set_exception(std::make_exception_ptr(JunctionBuilderException(err)));
    } else {
        if (printPlan) cerr << "[chain] target " << tid << endl;
        g_prof.mark(("chain queued: target " + std::to_string(tid)).c_str());
        pending.push_back(Pending{tid, done, {}, {}});
    }
}

void DeviceThread::beginGroup(Waiting& w) {
    std::sort(w.got.begin(), w.got.end());
    std::vector<int32_t> tids;
    std::vector<std::promise<ContigDone>*> dones;
    for (auto& x : w.got) tids.push_back(x.first), dones.push_back(x.second);
    w.got.clear();
    if (tids.empty()) return;
    while (pending.size() >= kQueued) collectOldest();
    if (tids.size() > 1 && !w.single && pjb_finish_group_begin(ctx, tids.data(), (int32_t)tids.size()) == PJB_OK) {
        if (printPlan) {
            std::string txt;
            for (size_t k = 0; k < tids.size(); k++) txt += (k ? "," : "") + std::to_string(tids[k]);
            cerr << "[chain] group " << txt << endl;
        }
        g_prof.mark(("chain queued: group of " + std::to_string(tids.size()) + " from target " + std::to_string(tids[0])).c_str());
        w.begun = true;
        pending.push_back(Pending{tids[0], nullptr, tids, dones});
        return;
    }
    // (PJB_ERR_ARG: "not as a group" -- a target with characters outside the nucleotide alphabet, ...: one by one)
    for (size_t k = 0; k < tids.size(); k++) beginSingle(tids[k], dones[k]);
}

// ---- the next command --------------------------------------------------------------------------------------------------------

int DeviceThread::readyDeferred() {
    for (size_t k = 0; k < deferred.size(); k++)
        if (!ctx || pjb_bam_inflate_done(ctx, deferred[k].tid)) return (int)k;
    return -1;
}

// A deferred BAMEND whose inflate has completed goes first; otherwise the queue's next command, waited for while the chains that
// complete meanwhile are collected.
DeviceThread::Cmd DeviceThread::next() {
    for (;;) {
        const int k = readyDeferred();
        if (k >= 0) {
            Cmd c = std::move(deferred[(size_t)k]);
            deferred.erase(deferred.begin() + k);
            collectReady();
            return c;
        }
        collectReady();
        std::unique_lock<std::mutex> lk(mu);
        const double t0 = HostProfile::now();
        bool again = false;
        while (q.empty()) {
            if (deferred.empty() && pending.empty()) cv.wait(lk, [&] { return !q.empty(); });
            else {  // deferred inflates and queued chains complete: keep asking
                cv.wait_for(lk, std::chrono::microseconds(200), [&] { return !q.empty(); });
                lk.unlock();
                const bool ready = readyDeferred() >= 0 || (!pending.empty() && ctx && pjb_finish_ready(ctx));
                lk.lock();
                if (ready && q.empty()) {
                    again = true;
                    break;
                }
            }
        }
        tIdle += HostProfile::now() - t0;
        if (again) continue;
        // a genome is needed when its target is finished, the file pieces are needed now: uploads of genomes whose
        // target's records are not complete yet let every other command pass (each is 30-70 ms of allocations and
        // a synchronisation, and pieces stuck behind them left PCIe idle at the start of a run)
        size_t pick = 0;
        // (only the uploads a worker waits for before it asks for the finish: the others must keep their place)
        if (q.front().kind == Cmd::GENOME && q.front().rawDone && !ended.count(q.front().tid)) {
            size_t urgent = q.size(), other = q.size();
            for (size_t k = 0; k < q.size(); k++) {
                if (q[k].kind == Cmd::GENOME && q[k].rawDone) {
                    if (urgent == q.size() && ended.count(q[k].tid)) urgent = k;
                } else if (other == q.size())
                    other = k;
            }
            pick = urgent < q.size() ? urgent : other < q.size() ? other : 0;
        }
        Cmd c = std::move(q[pick]);
        q.erase(q.begin() + (long)pick);
        if (c.kind == Cmd::BAMEND || c.kind == Cmd::BAM) ended.insert(c.tid);
        cv.notify_all();
        if (c.kind == Cmd::BAMEND && ctx) {
            // (asked without the queue's lock: pjb_bam_inflate_done takes the context's staging lock, which a worker
            // holds for the length of a pjb_bam_piece -- push() must not wait for that)
            lk.unlock();
            const bool inflated = pjb_bam_inflate_done(ctx, c.tid) != 0;
            lk.lock();
            if (!inflated) {
                deferred.push_back(std::move(c));
                continue;
            }
        }
        if (c.kind == Cmd::STOP && !deferred.empty()) { // (cannot happen: a worker waits for its BAMEND; keep the order anyway)
            q.push_back(std::move(c));
            continue;
        }
        return c;
    }
}

// ---- serving a command -------------------------------------------------------------------------------------------------------

void DeviceThread::serve(Cmd& c) {
    std::string err = fatal;
    if (err.empty() && failed.count(c.tid)) err = failed[c.tid];
    switch (c.kind) {
    case Cmd::GENOME: serveGenome(c, err); break;
    case Cmd::BATCH:
        if (err.empty()) {
            pjb_batch pb;
            c.batch.view(pb);
            if (const int rc = withRoom([&] { return pjb_submit_batch(ctx, c.tid, &pb); })) failed[c.tid] = describe("pjb_submit_batch", rc, c.tid);
        }
        if (c.spare) {
            std::lock_guard<std::mutex> lk(*c.spareMu);
            if (c.spare->size() < 4) c.spare->emplace_back(std::move(c.batch));
        }
        break;
    case Cmd::BAM: {
        int64_t n = 0;
        if (err.empty()) {
            if (const int rc = withRoom([&] { return pjb_submit_bam(ctx, c.tid, c.bamBytes, (int64_t)c.bamSize, (int32_t)c.bamFirst, &n); }))
                failed[c.tid] = describe("pjb_submit_bam", rc, c.tid) + (rc == PJB_ERR_NOMEM ? "" : kTryHostIngest);
        }
        bam::bigFree(c.bamBytes);
        c.bamDone->set_value(n);
        break;
    }
    case Cmd::BAMEND: {
        int64_t n = 0;
        if (!err.empty() && ctx) (void)pjb_bam_end(ctx, c.tid, (int32_t)c.bamFirst, nullptr);  // (drops what was staged)
        if (err.empty()) {
            if (const int rc = withRoom([&] { return pjb_bam_end(ctx, c.tid, (int32_t)c.bamFirst, &n); }))
                failed[c.tid] = describe("pjb_bam_end", rc, c.tid) + (rc == PJB_ERR_NOMEM ? "" : kTryHostIngest);
        }
        c.bamDone->set_value(n);
        break;
    }
    case Cmd::FLUSH: flushChains(); break;  // (no more targets will come: what still waits for the rest of its group goes now)
    case Cmd::ROOM: c.roomDone->set_value(ctx != nullptr && makeRoom()); break;
    case Cmd::FINISH: serveFinish(c, err); break;
    case Cmd::EXTRA: {
        while (!pending.empty()) collectOldest();
        const pjb_extra_row* xr = nullptr;
        int64_t n = 0;
        if (err.empty() && pjb_extra_finish(ctx, &xr, &n) != PJB_OK) err = std::string("pjb_extra_finish: ") + pjb_last_error(ctx);
        if (err.empty()) c.extraDone->set_value(std::vector<pjb_extra_row>(xr, xr + n));
        else c.extraDone->set_exception(std::make_exception_ptr(JunctionBuilderException(err)));
        break;
    }
    case Cmd::STOP:
        flushChains();
        reportMemory();
        if (g_prof.on) {
            std::lock_guard<std::mutex> lk(g_prof.mu);
            cerr << "[host profile] device thread: alive " << (HostProfile::now() - tStart) << " s: idle " << tIdle << ", collect " << tCollect
                 << ", GENOME " << tKind[(int)Cmd::GENOME] << ", BATCH " << tKind[(int)Cmd::BATCH] << ", BAM " << tKind[(int)Cmd::BAM]
                 << ", BAMEND " << tKind[(int)Cmd::BAMEND] << ", FINISH " << tKind[(int)Cmd::FINISH] << ", EXTRA " << tKind[(int)Cmd::EXTRA] << endl;
        }
        break;
    }
}

void DeviceThread::serveGenome(Cmd& c, const std::string& err) {
    if (c.rawDone) {
        int ok = 0;
        int rc = PJB_OK;
        if (err.empty() && (rc = pjb_upload_contig_fasta(ctx, c.tid, c.raw, (int64_t)c.rawBytes, c.lineBases, c.lineWidth, c.genomeLen, &ok)) != PJB_OK) {
            failed[c.tid] = describe("pjb_upload_contig_fasta", rc, c.tid);
            ok = 1;  // (an error, not a malformed record: no second attempt)
        }
        if (c.rawPool) c.rawPool->release(c.raw);
        c.rawDone->set_value(ok != 0 || !err.empty());
    } else {
        int rc = PJB_OK;
        if (err.empty() && (rc = pjb_upload_contig(ctx, c.tid, (const uint8_t*)c.genome.data(), (int64_t)c.genome.size())) != PJB_OK)
            failed[c.tid] = describe("pjb_upload_contig", rc, c.tid);
    }
}

void DeviceThread::serveFinish(Cmd& c, const std::string& err) {
    if (c.seen) c.seen->set_value();
    auto git = groupOf.find(c.tid);
    if (err.empty() && git != groupOf.end() && plan[git->second].size() > 1 && !waiting[git->second].single) {
        Waiting& w = waiting[git->second];
        w.got.emplace_back(c.tid, c.done);
        if (w.got.size() == plan[git->second].size()) beginGroup(w);
    } else if (err.empty()) {
        beginSingle(c.tid, c.done);
    } else {
        if (git != groupOf.end()) { // the group is not complete any more: its members go one by one
            Waiting& w = waiting[git->second];
            w.single = true;
            beginGroup(w);
        }
        if (ctx) {
            while (!pending.empty()) collectOldest();
            pjb_region_result dummy;
            (void)pjb_finish_contig(ctx, c.tid, &dummy); // drop whatever was submitted
            const pjb_junction_row* rows = nullptr;
            int64_t n = 0;
            if (pjb_collect(ctx, &rows, &n) == PJB_OK) rowsSoFar = (size_t)n; // (rows of a dropped target are skipped)
            (void)pjb_release_contig(ctx, c.tid);
        }
        c.done->set_exception(std::make_exception_ptr(JunctionBuilderException(err)));
    }
    failed.erase(c.tid);
}

}  // namespace portcullis
