// JunctionBuilder: orchestration of the junc stage on top of the device path.
// Flow and console output follow src/junction_builder.cc:84-291 of the reference.
#include <portcullis/junction_builder.hpp>
#include <portcullis/bam/bam_writer.hpp>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <future>
#include <iomanip>
#include <iostream>
#include <malloc.h>
#include <memory>
#include <mutex>
#include <sys/stat.h>
#include <thread>

#include "device_thread.hpp"
#include "host_profile.hpp"

namespace portcullis {

using bam::BamReader;
using bam::GenomeMapper;
using std::cerr;
using std::cout;
using std::endl;

static bool pathExists(const std::string& p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}

static bool makeDirs(const std::string& p) {
    if (p.empty() || pathExists(p)) return true;
    const size_t slash = p.find_last_of('/');
    if (slash != std::string::npos && slash > 0 && !makeDirs(p.substr(0, slash))) return false;
    return mkdir(p.c_str(), 0777) == 0 || pathExists(p);
}

namespace {
struct WallTimer {  // prints like boost::timer::auto_cpu_timer(1, " = Wall time taken: %ws\n\n")
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double elapsed() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    ~WallTimer() {
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::ios::fmtflags f(cout.flags());
        cout << " = Wall time taken: " << std::fixed << std::setprecision(1) << s << "s" << endl << endl;
        cout.flags(f);
    }
};
}  // namespace

static int envInt(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}
static int envIs(const char* name, const char* value) {  // -1: not set
    const char* e = getenv(name);
    return e ? strcmp(e, value) == 0 : -1;
}

// Every environment variable the junc driver reads, in the order of INTEGRATION.md's table (PJB_PROFILE_HOST: host_profile.hpp).
// Read once, when the JunctionBuilder is made; the setters and the command line override the first two and PJB_TEST_BATCH.
struct JuncEnv {
    int gpus = envInt("PORTCULLIS_GPUS", 0);                                           // as --devices N (0: every visible GPU)
    int ingestDevice = envIs("PORTCULLIS_INGEST", "device");                           // as --ingest device|host
    int ctxPerGpu = envInt("PORTCULLIS_CTX_PER_GPU", -1);                              // (-1: 1 for file-piece ingest, else 2)
    int transferSlots = envInt("PORTCULLIS_TRANSFER_SLOTS", 2);                        // (0: no limit)
    int readThreads = envInt("PORTCULLIS_READ_THREADS", -1);                           // (-1: 2, fewer where the host threads do not reach)
    size_t pinnedBuffers = (size_t)std::max(2, envInt("PORTCULLIS_PINNED_BUFFERS", 12));
    size_t pieceMB = (size_t)std::max(1, envInt("PORTCULLIS_PIECE_MB", 64));
    int pieceBytes = envInt("PORTCULLIS_PIECE_BYTES", -1);                             // (tests; -1: not set) pieces of this size, at least 64, for files and targets of any size
    int registerSlot = envInt("PORTCULLIS_REGISTER_SLOT", -1);
    bool normalExit = getenv("PJB_NORMAL_EXIT") != nullptr;
    bool shareGpu = getenv("PORTCULLIS_DEVICES_SHARE_GPU") != nullptr;
    const char* testBatch = getenv("PJB_TEST_BATCH");                                  // (used by the constructor only)
    int chainGroups = envIs("PORTCULLIS_CHAIN_PLAN", "groups");                        // [groups for file-piece ingest with one context, else targets]
    int64_t groupBases = getenv("PORTCULLIS_GROUP_BASES") ? atoll(getenv("PORTCULLIS_GROUP_BASES")) : 0;  // (0: pjb_plan_groups' own 2^30)
    bool printPlan = getenv("PJB_PRINT_CHAIN_PLAN") != nullptr;
    const char* deviceMem = getenv("PORTCULLIS_DEVICE_MEM");                           // as --device_mem <size>
};

uint64_t JunctionBuilder::parseDeviceMem(const std::string& text) {
    const std::string why = "--device_mem takes a number of bytes, optionally followed by K, M or G (powers of 1024): '" + text + "'";
    size_t k = 0;
    uint64_t v = 0;
    for (; k < text.size() && text[k] >= '0' && text[k] <= '9'; k++) {
        if (v > (UINT64_MAX - 9) / 10) throw JunctionBuilderException(why);
        v = v * 10 + (uint64_t)(text[k] - '0');
    }
    if (k == 0 || text.size() > k + 1) throw JunctionBuilderException(why);
    int shift = 0;
    if (k < text.size()) {
        const char u = text[k];
        shift = u == 'K' || u == 'k' ? 10 : u == 'M' || u == 'm' ? 20 : u == 'G' || u == 'g' ? 30 : -1;
        if (shift < 0) throw JunctionBuilderException(why);
    }
    if (v > ((uint64_t)INT64_MAX >> shift)) throw JunctionBuilderException(why);  // (the library's option is an int64_t)
    return v << shift;
}

JunctionBuilder::JunctionBuilder(const std::string& prepDir, const std::string& output) : env(std::make_shared<const JuncEnv>()) {
    prepData = PreparedFiles(prepDir);
    if (output.empty()) {
        outputDir = ".";
        outputPrefix = "portcullis";
    } else {
        const size_t slash = output.find_last_of('/');
        outputDir = slash == std::string::npos ? "" : output.substr(0, slash);
        outputPrefix = slash == std::string::npos ? output : output.substr(slash + 1);
        if (slash == 0) outputDir = "/";
    }
    devices = env->gpus;
    if (env->testBatch) setBatchRecords((size_t)atol(env->testBatch));
    if (env->ingestDevice >= 0) setDeviceIngest(env->ingestDevice == 1);
    if (env->deviceMem) setDeviceMem(parseDeviceMem(env->deviceMem));
}

void JunctionBuilder::process() {
    const double t_p0 = HostProfile::now();
    // many decode threads allocate and free multi-megabyte arrays: keep them on the heap instead of
    // one mmap/munmap pair each (munmap broadcasts TLB shootdowns to every core running a thread)
    mallopt(M_MMAP_THRESHOLD, 1 << 30);
    mallopt(M_TRIM_THRESHOLD, -1);
    // the HIP runtime takes ~0.2 s to come up: start it now, beside the header / index reads
    deviceCount = std::async(std::launch::async, [] { return pjb_device_count(); }).share();
    const std::string outDir = outputDir.empty() ? "." : outputDir;
    if (!pathExists(outDir) && !makeDirs(outDir))
        throw JunctionBuilderException("Could not create output directory at: " + outDir);
    if (!pathExists(prepData.getSortedBamFilePath()))
        throw JunctionBuilderException("Could not find prepared BAM file at: " + prepData.getSortedBamFilePath());
    try {
        prepData.valid(useCsi);
    } catch (const PrepareException& e) {
        throw JunctionBuilderException(std::string("Prepared data is not complete: ") + prepData.getPrepDir() + " (" + e.what() + ")");
    }
    BamReader reader(prepData.getSortedBamFilePath());
    reader.open(useCsi);
    refs = reader.createRefList();
    refMap = reader.createRefMap(*refs);
    reader.close();
    junctionSystem = JunctionSystem();
    junctionSystem.setRefs(refs);
    if (hostThreads == 0) hostThreads = threads;  // total decode threads survive the per-target cap below
    if (refs->size() < threads) {
        cerr << "Warning: User requested " << threads << " threads but there are only " << refs->size()
             << " target sequences to process.  Setting number of threads to " << refs->size() << "." << endl << endl;
        threads = (uint16_t)refs->size();
    }
    // (the reference forces --separate when --extra is given because calcExtraMetrics re-reads the split files,
    // src/junction_builder.cc:113-117; here --extra works on the records in device memory and writes no files)
    cout << "Settings:" << endl
         << std::boolalpha << " - BAM Strandedness: " << bam::strandednessToString(strandSpecific) << endl
         << " - BAM Read Orientation: " << bam::orientationToString(orientation) << endl
         << " - BAM Indexing mode: " << (useCsi ? "CSI" : "BAI") << endl
         << " - Threads: " << threads << endl
         << " - Separate BAMs: " << separate << endl;
    if (deviceMem) cout << " - Device memory: " << deviceMem << " bytes per GPU" << endl;
    cout << endl;
    cout << reader.bamDetails() << endl;
    const double t_p1 = HostProfile::now();
    if (separate) separateBams();
    findJunctions();
    const double t_p2 = HostProfile::now();
    cout << "Saving junctions: " << endl;
    {
        WallTimer t;
        junctionSystem.saveAll(outDir + "/" + outputPrefix, source, false, outputExonGFF, outputIntronGFF);
    }
    g_prof.mark("outputs written");
    g_prof.dumpEvents();
    if (g_prof.on)
        cerr << "[host profile] process: header+index " << (t_p1 - t_p0) << " s, findJunctions " << (t_p2 - t_p1) << " s, saveAll "
             << (HostProfile::now() - t_p2) << " s" << endl;
    std::pair<bam::Orientation, bam::Strandedness> actual = junctionSystem.determineStrandedness(true);
    cout << "Determined sequence orientation to be: " << bam::orientationToLongString(actual.first) << endl;
    cout << "Determined RNAseq strandedness to be: " << bam::strandednessToLongString(actual.second) << endl << endl;
    if (strandSpecific != bam::Strandedness::UNKNOWN && strandSpecific != actual.second)
        cerr << "Warning!  User input and portcullis disagree about the strandedness of the dataset" << endl << endl;
}



// src/junction_builder.cc:152-226: one pass over the whole prepared BAM (unplaced records included); a record with an N
// operation goes to <prefix>.spliced.bam, another mapped one to <prefix>.unspliced.bam, the rest to <prefix>.unmapped.bam.
// The reference then shells out to `samtools index` for the first two; BamWriter writes the .bai itself.
void JunctionBuilder::separateBams() {
    WallTimer timer;
    uint64_t splicedCount = 0, unsplicedCount = 0, unmappedCount = 0;
    bam::BamReader reader(prepData.getSortedBamFilePath());
    reader.open(useCsi);
    const int wt = std::max(1, (int)threads);
    bam::BamWriter unsplicedWriter(getUnsplicedBamFile(), wt), splicedWriter(getSplicedBamFile(), wt), unmappedWriter(getUnmappedBamFile(), wt);
    unmappedWriter.setWriteIndex(false);
    cout << "Splitting BAM:" << endl;
    cout << " - Saving unspliced alignments to: " << getUnsplicedBamFile() << endl;
    unsplicedWriter.open(reader.getHeaderText(), reader.getTargets());
    cout << " - Saving spliced alignments to: " << getSplicedBamFile() << endl;
    splicedWriter.open(reader.getHeaderText(), reader.getTargets());
    cout << " - Saving unmapped reads to: " << getUnmappedBamFile() << endl;
    unmappedWriter.open(reader.getHeaderText(), reader.getTargets());
    cout << " - Processing BAM ...";
    cout.flush();
    std::vector<uint8_t> rec;
    reader.rewind();
    while (reader.nextRecord(rec)) {
        const uint8_t* r = rec.data();
        const uint32_t l_name = r[12], n_cig = (uint32_t)r[16] | ((uint32_t)r[17] << 8);
        const uint32_t flag = (uint32_t)r[18] | ((uint32_t)r[19] << 8);
        if (36ull + l_name + 4ull * n_cig > rec.size()) throw JunctionBuilderException("Invalid BAM record layout");
        bool spliced = false;  // BamAlignment::isSplicedRead, lib/src/bam_alignment.cc:294-301
        for (uint32_t k = 0; k < n_cig && !spliced; k++) spliced = (r[36 + l_name + 4 * k] & 15u) == 3u;
        if (spliced) {
            splicedWriter.write(r, rec.size());
            splicedCount++;
        } else if (!(flag & 0x4u)) {
            unsplicedWriter.write(r, rec.size());
            unsplicedCount++;
        } else {
            unmappedWriter.write(r, rec.size());
            unmappedCount++;
        }
    }
    cout << " done." << endl;
    cout << " - Found " << splicedCount << " spliced alignments." << endl;
    cout << " - Found " << unsplicedCount << " unspliced alignments." << endl;
    cout << " - Found " << unmappedCount << " unmapped reads." << endl;
    reader.close();
    cout << " - Indexing unspliced alignments ... ";
    unsplicedWriter.close();
    cout << "done." << endl << " - Indexing spliced alignments ... ";
    splicedWriter.close();
    unmappedWriter.close();
    cout << "done." << endl;
}

// a target between "a worker took it" and "its chain has been collected": what the steps of findJuncs hand to each other
struct DeferredTarget {
    std::promise<void> seen;
    std::promise<ContigDone> done;
    std::future<ContigDone> fut = done.get_future();
    std::string decodeError, genomeError, name;
    bool any = false;
    double t_begin = 0, t_decoded = 0, t_blocked = 0, t_genome = 0;
    // raised by the decoder thread when the target's file pieces are all on their way (or it has stopped): the genome is
    // needed when the target is finished, the pieces are needed now -- until then this target's genome leaves the cores, the
    // page-locking calls and PCIe to the pieces
    std::promise<void> piecesGone;
    bool piecesGoneSet = false;
    void raisePiecesGone() {
        if (!piecesGoneSet) {
            piecesGoneSet = true;
            piecesGone.set_value();
        }
    }
    // host decode: the storage of the batches the device thread has served comes back here
    std::vector<bam::ReadBatch> spare;
    std::mutex spareMu;
};

// one findJunctions run: what its steps hand to each other
struct JuncRun {
    std::vector<int32_t> with;    // the targets that hold alignments, in index order
    std::vector<int32_t> order;   // the order the workers take the targets in
    int total = 1, nthreads = 1;  // host threads in all; workers (one target each at a time)
    std::mutex mu;  // guards what follows
    std::vector<std::unique_ptr<DeviceThread>> deviceThreads;  // started by the first worker that asks for one
    size_t nextTask = 0;
    std::string firstError;
};

// host decode: the decode thread (with its inner pool) pushes batches straight to the device thread
void JunctionBuilder::decodeOnHost(DeviceThread& device, BamReader& reader, int32_t seq, DeferredTarget& dt) {
    auto send = [&](bam::ReadBatch& b) {
        const double tb0 = HostProfile::now();
        DeviceThread::Cmd c(DeviceThread::Cmd::BATCH, seq);
        std::swap(c.batch, b);
        c.spare = &dt.spare;
        c.spareMu = &dt.spareMu;
        dt.any = true;
        device.push(std::move(c));
        dt.t_blocked += HostProfile::now() - tb0;
        std::lock_guard<std::mutex> lk(dt.spareMu);
        if (!dt.spare.empty()) {
            std::swap(b, dt.spare.back());
            dt.spare.pop_back();
        }
    };
    if (innerThreads > 1) {
        reader.decodeRegionParallel(seq, innerThreads, batchRecords, send);
    } else {
        reader.setRegion(seq);
        bam::ReadBatch b;
        while (true) {
            b.clear();
            b.reserve(batchRecords);
            if (!reader.nextBatch(b, batchRecords)) break;
            send(b);
        }
    }
}

// device ingest, small target or small file: the target's bytes go over in one (pageable) block
void JunctionBuilder::sendWhole(DeviceThread& device, BamReader& reader, int32_t seq, DeferredTarget& dt, uint64_t fileOff, size_t nb, uint32_t firstU) {
    uint8_t* bytes = (uint8_t*)bam::bigAlloc(nb + 64);
    try {
        reader.readSpan(fileOff, nb, bytes, innerThreads);
    } catch (...) {
        bam::bigFree(bytes);
        throw;
    }
    std::promise<int64_t> got;
    std::future<int64_t> f = got.get_future();
    DeviceThread::Cmd c(DeviceThread::Cmd::BAM, seq);
    c.bamBytes = bytes;
    c.bamSize = nb;
    c.bamFirst = firstU;
    c.bamDone = &got;
    device.push(std::move(c));
    dt.any = f.get() > 0;
}

// device ingest, large target of a large file: the bytes go to the device in pieces through a small ring of
// page-locked buffers (page-locking a buffer per target costs ~0.15 s per GB); the copy of a piece runs while
// this thread reads the next one
void JunctionBuilder::streamPieces(DeviceThread& device, BamReader& reader, int32_t seq, DeferredTarget& dt, uint64_t fileOff, size_t nb, uint32_t firstU) {
    // This thread hands the pieces to the device itself (pjb_bam_begin / _piece are safe beside the device
    // thread's calls): queued behind genome uploads, finishes and record parsing on the device thread the
    // copies started late and PCIe idled between them.
    pjb_ctx* dctx = device.context();
    if (!dctx) return;  // (no context: nothing to read for; the FINISH reports why)
    const size_t piece = pinnedPool->piece();
    const double tg0 = HostProfile::now();
    const int slot = pinnedPool->enterTransfer(device.lane, transferRank(seq));
    g_prof.event(tg0, HostProfile::now(), "worker gate wait tid " + std::to_string(seq));
    struct Leave {
        PinnedPool* p;
        int lane, slot;
        ~Leave() { now(); }
        void now() {
            if (p) p->leaveTransfer(lane, slot);
            p = nullptr;
        }
    } leave{pinnedPool.get(), device.lane, slot};
    // One slot's target crosses straight out of the page cache: pieces of the file's mapping are page-locked
    // for their copy (2.5 ms per 64 MB, one thread; registration does not scale over threads) while the other
    // slot's readers copy theirs into the ring -- two different resources.
    size_t mapBytes = 0;
    const uint8_t* fileMap = slot == pinnedPool->registerSlot ? bam::BamReader::mapFile(prepData.getSortedBamFilePath(), mapBytes) : nullptr;
    const int readThreads = fileMap || pinnedPool->registerSlot < 0 ? pinnedPool->readThreads : pinnedPool->readThreads * 2;
    std::string readError;
    struct Mine {
        int64_t ticket;
        uint8_t* buf;  // a ring buffer, or
        void* reg;     // a registered range of the file's mapping
    };
    std::deque<Mine> mine;  // pieces of this target whose copy may still read the buffer
    auto releaseDone = [&](bool all) {
        int64_t done = 0;
        if (mine.empty()) return;
        if (pjb_bam_pieces_done(dctx, &done) != PJB_OK) done = all ? INT64_MAX : 0;
        for (int spin = 0; all && done < mine.back().ticket && spin < 20000; spin++) {  // (at most 2 s: the copies of a failed target)
            std::this_thread::sleep_for(std::chrono::microseconds(100));
            if (pjb_bam_pieces_done(dctx, &done) != PJB_OK) break;
        }
        if (all) done = INT64_MAX;
        while (!mine.empty() && mine.front().ticket <= done) {
            if (mine.front().reg) (void)pjb_host_unregister(mine.front().reg);
            else pinnedPool->release(mine.front().buf);
            mine.pop_front();
        }
    };
    const double tb0 = HostProfile::now();
    // (out of device memory: the device thread collects a chain -- its groups go target by target from then on --, and the call is repeated)
    int brc;
    while ((brc = pjb_bam_begin(dctx, seq, (int64_t)nb)) == PJB_ERR_NOMEM && device.askForRoom()) {
    }
    if (brc != PJB_OK) readError = std::string("pjb_bam_begin: ") + pjb_last_error(dctx) + (brc == PJB_ERR_NOMEM ? device.memoryAdvice(seq) : std::string());
    g_prof.event(tb0, HostProfile::now(), "worker bam_begin tid " + std::to_string(seq));
    // (with the mapping: pieces end on page boundaries of the FILE, so that no two pieces share a page)
    const size_t firstPiece = fileMap ? piece - (size_t)(fileOff & 4095) : piece;
    for (size_t off = 0, step = firstPiece; off < nb && readError.empty(); off += step, step = piece) {
        const size_t n = std::min(step, nb - off);
        const double ta0 = HostProfile::now();
        if (fileMap && fileOff + off + n <= mapBytes) {
            // [a, e): the pages that hold the piece (the first and the last page of a target may still be locked for
            // a neighbouring target's copy: then the piece is read like any other)
            const uintptr_t lo = (uintptr_t)(fileMap + fileOff + off), hi = lo + n;
            const uintptr_t a = lo & ~(uintptr_t)4095, e = (hi + 4095) & ~(uintptr_t)4095;
            while (mine.size() >= 6) {  // (at most six pieces' pages locked at a time)
                releaseDone(false);
                if (mine.size() >= 6) std::this_thread::sleep_for(std::chrono::microseconds(100));
            }
            if (pjb_host_register((void*)a, (size_t)(e - a)) == PJB_OK) {
                int64_t ticket = 0;
                if (pjb_bam_piece(dctx, seq, (const uint8_t*)lo, (int64_t)n, &ticket) != PJB_OK) {
                    readError = std::string("pjb_bam_piece: ") + pjb_last_error(dctx);
                    releaseDone(true);
                    (void)pjb_host_unregister((void*)a);
                    break;
                }
                mine.push_back(Mine{ticket, nullptr, (void*)a});
                g_prof.event(ta0, HostProfile::now(), "worker map piece tid " + std::to_string(seq) + " " + std::to_string(n >> 20) + " MB");
                releaseDone(false);
                continue;
            }
            // (a piece that cannot be registered -- its first page still locked for a copy in flight -- is read)
        }
        uint8_t* buf = nullptr;
        while (!(buf = pinnedPool->tryAcquire(piece))) {  // (this thread's finished copies may be what the ring waits for)
            releaseDone(false);
            std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
        const double ta1 = HostProfile::now();
        if (ta1 - ta0 > 1e-3) g_prof.event(ta0, ta1, "worker ring wait tid " + std::to_string(seq));
        try {
            reader.readSpan(fileOff + off, n, buf, readThreads);
            g_prof.event(ta1, HostProfile::now(), "worker read piece tid " + std::to_string(seq) + " " + std::to_string(n >> 20) + " MB");
        } catch (const std::exception& e) {
            pinnedPool->release(buf);
            readError = e.what();
            break;
        }
        int64_t ticket = 0;
        const double tp0 = HostProfile::now();
        const int prc = pjb_bam_piece(dctx, seq, buf, (int64_t)n, &ticket);
        if (HostProfile::now() - tp0 > 1e-3) g_prof.event(tp0, HostProfile::now(), "worker bam_piece call tid " + std::to_string(seq));
        if (prc != PJB_OK) {
            readError = std::string("pjb_bam_piece: ") + pjb_last_error(dctx);
            releaseDone(true);  // (a failing piece call has waited for the upload stream)
            pinnedPool->release(buf);
            break;
        }
        mine.push_back(Mine{ticket, buf, nullptr});
        releaseDone(false);
    }
    std::promise<int64_t> got;
    std::future<int64_t> f = got.get_future();
    DeviceThread::Cmd c(DeviceThread::Cmd::BAMEND, seq);  // (after a read error: fails with "n of m bytes arrived" and drops the staging)
    c.bamFirst = firstU;
    c.bamDone = &got;
    const double tq0 = HostProfile::now();
    device.push(std::move(c));
    if (HostProfile::now() - tq0 > 1e-3) g_prof.event(tq0, HostProfile::now(), "worker BAMEND push tid " + std::to_string(seq));
    leave.now();  // the next target's pieces cross while this one is inflated and parsed
    dt.raisePiecesGone();
    // (The push waits while the device thread's queue is full -- 0.4 s over a run, up to 0.13 s at a time -- and the slot
    // stays taken meanwhile.  Releasing the slot before the push and a queue of 32 were blamed in round 3 for runs that
    // stood still for a second or two (profiles/r03v_e2e_scheduling_ab.txt); those were runs right behind another
    // process (profiles/r06_e2e_pause.txt).  Measured again with a pause before every run, neither changes the wall:
    // medians 1.82 - 1.88 s for all four combinations, profiles/r06_e2e_slot_turnover.txt.  Left as it was.)
    // (the ring gets this target's buffers back as their copies complete, not when its records are parsed)
    while (f.wait_for(std::chrono::microseconds(200)) != std::future_status::ready) releaseDone(false);
    dt.any = f.get() > 0;
    releaseDone(true);  // (pjb_bam_end has waited for the copies)
    if (!readError.empty()) throw bam::BamException(readError);
}

// the target's genome: the record's bytes as they are in the FASTA file where that works, the filtered bases otherwise
void JunctionBuilder::uploadGenome(DeviceThread& device, GenomeMapper& gmap, int32_t seq, DeferredTarget& dt) {
    const double t0 = HostProfile::now();
    // large runs: the record's bytes go to the device as they are in the file (a pread into a page-locked buffer; the
    // device takes the line terminators out) -- parsing 3 GB of FASTA on the host was 6 core-seconds at the very moment
    // the file pieces of the first targets want the cores
    bool uploaded = false;
    bam::GenomeMapper::RawSpan span;
    if (genomePool && gmap.rawSpan(dt.name, span) && span.length == refs->at((size_t)seq)->length && span.bytes > 0) {
        uint8_t* buf = genomePool->acquire(span.bytes);
        if (buf) {
            const double t1 = HostProfile::now();
            bool whole = false;
            try {
                whole = gmap.readRaw(span, buf, std::max(innerThreads, 4));
            } catch (...) {
                genomePool->release(buf);
                throw;
            }
            g_prof.event(t0, t1, "worker genome buffer wait tid " + std::to_string(seq));
            g_prof.event(t1, HostProfile::now(), "worker genome raw read tid " + std::to_string(seq));
            if (!whole) {  // the file ends before the span the index describes: the record is not laid out that way
                genomePool->release(buf);
            } else {
                std::promise<bool> ok;
                std::future<bool> f = ok.get_future();
                DeviceThread::Cmd c(DeviceThread::Cmd::GENOME, seq);
                c.raw = buf;
                c.rawBytes = span.bytes;
                c.lineBases = span.lineBases;
                c.lineWidth = span.lineWidth;
                c.genomeLen = span.length;
                c.rawPool = genomePool.get();
                c.rawDone = &ok;
                device.push(std::move(c));
                uploaded = f.get();
                dt.t_genome = HostProfile::now() - t0;
            }
        }
    }
    if (!uploaded) {
        std::string contig = gmap.fetchContig(dt.name);
        dt.t_genome = HostProfile::now() - t0;
        g_prof.event(t0, t0 + dt.t_genome, "worker genome read tid " + std::to_string(seq));
        if ((int64_t)contig.size() != refs->at((size_t)seq)->length)
            throw JunctionBuilderException("Genome sequence " + dt.name + " has " + std::to_string(contig.size()) +
                                           " bases but the BAM header says " + std::to_string(refs->at((size_t)seq)->length));
        DeviceThread::Cmd c(DeviceThread::Cmd::GENOME, seq);
        c.genome = std::move(contig);
        device.push(std::move(c));
    }
}

// One target sequence: a second thread moves the target's records (or its file bytes) to the device thread,
// this thread reads the genome meanwhile, then asks for the contig to be finished.
void JunctionBuilder::findJuncs(DeviceThread& device, BamReader& reader, GenomeMapper& gmap, int32_t seq) {
    if (!reader.hasAlignments(seq)) return;  // nothing placed on this target: counters keep their neutral values
    auto dt = std::make_shared<DeferredTarget>();
    dt->t_begin = HostProfile::now();
    dt->name = refs->at((size_t)seq)->name;
    std::future<void> piecesGoneF = dt->piecesGone.get_future();
    std::thread decoder([&] {
        try {
            uint64_t fileOff = 0;
            size_t nb = 0;
            uint32_t firstU = 0;
            if (!deviceIngest) decodeOnHost(device, reader, seq, *dt);
            // the device inflates and parses: this thread only moves the target's file bytes
            else if (reader.regionSpan(seq, fileOff, nb, firstU)) {
                if (pinnedPool && pinnedPool->piece() > 0 && nb >= pieceMinTarget) streamPieces(device, reader, seq, *dt, fileOff, nb, firstU);
                else sendWhole(device, reader, seq, *dt, fileOff, nb, firstU);
            }
        } catch (const std::exception& e) {
            dt->decodeError = e.what();
        }
        dt->raisePiecesGone();
    });
    try {
        if (deviceIngest && pinnedPool) piecesGoneF.wait();
        uploadGenome(device, gmap, seq, *dt);
    } catch (const std::exception& e) {
        dt->genomeError = e.what();
    }
    decoder.join();
    dt->t_decoded = HostProfile::now();
    // always close the contig on the device, also after a host-side error
    DeviceThread::Cmd c(DeviceThread::Cmd::FINISH, seq);
    c.done = &dt->done;
    if (device.grouped()) c.seen = &dt->seen;
    device.push(std::move(c));
    if (device.grouped()) {
        dt->seen.get_future().wait();  // (the batches queued before the FINISH name this target's buffers)
        // the target's chain is queued when the last member of its group has been asked for: this worker goes on to its next target
        // (waiting here, a worker would hold the thread the group's other members need) and findJunctions takes the result later
        std::lock_guard<std::mutex> lk(deferredMu);
        deferredTargets[(size_t)seq] = dt;
        return;
    }
    completeTarget(seq, *dt);
}

// what a worker does once its target's chain has been collected (or failed)
void JunctionBuilder::completeTarget(int32_t seq, DeferredTarget& dt) {
    RegionResult& res = results[(size_t)seq];
    ContigDone d;
    std::string finishError;
    try {
        d = dt.fut.get();
    } catch (const std::exception& e) {
        finishError = e.what();
    }
    if (!dt.decodeError.empty()) throw JunctionBuilderException(dt.decodeError);
    if (!dt.genomeError.empty()) throw JunctionBuilderException(dt.genomeError);
    if (!finishError.empty()) throw JunctionBuilderException(finishError);
    if (!dt.any) return;
    res.js.appendRows(d.rows.data(), d.rows.size());
    res.rowBase = d.rowBase;
    res.splicedCount = d.rr.spliced;
    res.unsplicedCount = d.rr.unspliced;
    res.sumQueryLengths = d.rr.sum_len;
    res.minQueryLength = d.rr.min_len;
    res.maxQueryLength = d.rr.max_len;
    if (g_prof.on) {
        const double t_end = HostProfile::now();
        std::lock_guard<std::mutex> lk(g_prof.mu);
        cerr << "[host profile] " << dt.name << ": total " << (t_end - dt.t_begin) << " s = decode (incl. queueing) " << (dt.t_decoded - dt.t_begin)
             << " (of which blocked on the device queue " << dt.t_blocked << ") + finish/rows " << (t_end - dt.t_decoded)
             << "; genome read " << dt.t_genome << endl;
    }
}

// thread counts, the order the targets are taken in, the page-locked pools of a large device-ingest run
void JunctionBuilder::planIngest(JuncRun& run) {
    // `threads` host threads in total: one worker per target sequence in flight, the rest decode
    // inside the targets (a single big contig still uses every thread)
    {
        BamReader probe(prepData.getSortedBamFilePath());
        probe.open(useCsi);
        for (size_t i = 0; i < refs->size(); i++)
            if (probe.hasAlignments((int32_t)i)) run.with.push_back((int32_t)i);
    }
    const int withReads = (int)run.with.size();
    run.total = std::max<int>(1, hostThreads > 0 ? hostThreads : threads);
    run.nthreads = std::max(1, std::min(run.total, std::max(1, withReads)));
    innerThreads = std::max(1, run.total / run.nthreads);
    cout << "Creating " << run.nthreads << " threads, each with BAM and genome indicies loaded ...";
    cout.flush();
    std::vector<int32_t>& order = run.order;  // longest targets first: better balance across workers
    for (size_t i = 0; i < refs->size(); i++) {
        results[i].js.setRefs(refs);
        results[i].name = refs->at(i)->name;
        order.push_back((int32_t)i);
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return refs->at((size_t)a)->length > refs->at((size_t)b)->length; });
    // ... except that a smaller one goes first: the device has nothing to do until a target's last byte has crossed, and the
    // largest target takes longest to cross (first inflate 0.23 s after the contexts were ready; the smallest ones still end
    // the run: a short tail)
    if (order.size() >= 5) {
        const size_t k = order.size() * 4 / 5;
        const int32_t small = order[k];
        order.erase(order.begin() + (long)k);
        order.insert(order.begin(), small);
    }
    transferRanks.assign(refs->size(), 1 << 30);
    for (size_t k = 0; k < order.size(); k++) transferRanks[(size_t)order[k]] = (int)k;
    // large inputs: page-locked buffers for the file bytes (allocating them costs ~0.15 s per GB once, so small runs
    // keep the pageable path whose staging copy is cheaper than that)
    pinnedPool.reset();
    genomePool.reset();
    if (!deviceIngest) return;
    struct stat bst;
    const bool testPieces = env->pieceBytes >= 0;  // (tests: small files in small pieces)
    const uint64_t minFile = testPieces ? 0 : 8ull << 30;
    pieceMinTarget = testPieces ? 0 : (size_t)64 << 20;
    // 12 x 64 MB: 0.75 GB of page-locked memory in all (64 MB pieces measured best of 32 / 64 / 128)
    const size_t pieceBytes = testPieces ? (size_t)std::max(64, env->pieceBytes) : env->pieceMB << 20;
    if (stat(prepData.getSortedBamFilePath().c_str(), &bst) == 0 && (uint64_t)bst.st_size >= minFile) {
        pinnedPool.reset(new PinnedPool(env->pinnedBuffers, pieceBytes));
        genomePool.reset(new PinnedPool(3));  // (the FASTA records' bytes go up as they are: pjb_upload_contig_fasta)
    }
}

// one device thread per GPU in use and context on it, with the run's chain plan (called once, by the first worker that asks)
void JunctionBuilder::startDeviceThreads(JuncRun& run) {
    const int ndevWanted = devices > 0 ? devices : 0;
    // the device count is only known once HIP is up; until then assume one GPU per requested device
    int nd = 1;
    if (ndevWanted > 1 || devices == 0) {
        int visible = deviceCount.get();
        if (env->shareGpu && visible > 0 && ndevWanted > 0) visible = ndevWanted;
        nd = std::max(1, std::min(ndevWanted > 0 ? ndevWanted : visible, std::min(visible, run.nthreads)));
    }
    // two contexts (device threads, streams) per GPU: while one target's kernels run, the other target's
    // file bytes and genome cross PCIe
    // (With the file pieces streaming through one context -- whose inflates run on their own streams beside
    // everything else -- a second context only adds contention for the runtime's locks: 2.9-3.0 s against 3.2 s.)
    int per = env->ctxPerGpu >= 0 ? std::max(1, env->ctxPerGpu) : pinnedPool ? 1 : 2;
    per = std::max(1, std::min(per, run.nthreads / nd));
    if (extra) nd = per = 1;  // the name multiplicities and the depth hand-over between targets are file-wide: one context
    // The chain plan.  ONE context serves every target (the default for large inputs): the targets that hold alignments, in index
    // order, are finished in the groups pjb_plan_groups makes of them -- what bench.py's step does.  Several contexts take their
    // targets as the workers come (no telling which context a target goes to): a chain per target.  --extra (always one context)
    // takes groups as well -- the unspliced records of a group are kept in the coordinates of its virtual sequence -- but plans a
    // chain per target unless told otherwise (groups become its default when tools/bench_extra.py --targets shows them faster by more
    // than the per-target runs' spread).
    // PORTCULLIS_CHAIN_PLAN=targets | groups overrides (groups: only with one context); PORTCULLIS_GROUP_BASES sets the bases of a
    // group (tests: small genomes in several groups).
    std::vector<int32_t> lens;
    for (auto& r : *refs) lens.push_back(r->length);
    std::vector<std::vector<int32_t>> chainPlan;
    const bool wantGroups = env->chainGroups >= 0 ? env->chainGroups == 1 : (pinnedPool != nullptr && !extra);
    if (wantGroups && nd * per == 1) {
        std::vector<int32_t> groupOf(run.with.size(), 0);
        const int ng = pjb_plan_groups(lens.data(), run.with.data(), (int32_t)run.with.size(), env->groupBases, groupOf.data());
        if (ng > 0) {
            chainPlan.resize((size_t)ng);
            for (size_t k = 0; k < run.with.size(); k++) chainPlan[(size_t)groupOf[k]].push_back(run.with[k]);
        }
    }
    DeviceThread::Setup setup{orientation, strandSpecific, lens, deviceCount, extra, env->shareGpu, env->printPlan, 0, false, {}};
    // the budget of a GPU is divided evenly among the contexts on it
    setup.memLimit = deviceMem / (uint64_t)(env->shareGpu ? nd * per : per);
    if (deviceMem && !setup.memLimit) setup.memLimit = 1;
    setup.report = verbose || g_prof.on;
    for (auto& r : *refs) setup.names.push_back(r->name);
    for (int k = 0; k < per; k++)
        for (int d = 0; d < nd; d++) run.deviceThreads.emplace_back(new DeviceThread(d, setup, chainPlan));
    for (size_t k = 0; k < run.deviceThreads.size(); k++) run.deviceThreads[k]->lane = (int)k;
    // Targets whose pieces are on their way at once, over all contexts (PORTCULLIS_TRANSFER_SLOTS; 0: no limit), each read by
    // PORTCULLIS_READ_THREADS threads.  FEW readers: four threads pread 31.6 GB/s out of the page cache into page-locked
    // buffers, eight 25.0, fifteen 24.8 (profiles/r03ap_register_probe.txt), and the run with 2 x 2 readers takes 2.03 s
    // where 3 x 5 took 2.3 - 2.6 (profiles/r03aq_e2e_readers.txt).
    // (Round 6, every run behind a 3 s pause -- the stalls that made three slots look unstable were the process before the run,
    // profiles/r06_e2e_pause.txt --: three targets in transfer against two, medians of 8 / 8 / 14 runs in three calls: 1.61 / 1.63 /
    // 1.71 s against 1.68 / 1.64 / 1.68 s, and 1.69 s against 1.63 - 1.65 in the bench's own leg; four: as three.  A wash with the
    // wider spread on three's side: two stays.  profiles/r06_e2e_retune*.txt)
    if (pinnedPool && env->transferSlots > 0) {
        const int perLane = std::max(1, env->transferSlots / (int)run.deviceThreads.size());
        pinnedPool->setTransferSlots(perLane);
        pinnedPool->readThreads = env->readThreads >= 0 ? env->readThreads : std::min(2, run.total / (perLane * (int)run.deviceThreads.size()));
        pinnedPool->readThreads = std::max(1, pinnedPool->readThreads);  // (threads per target in transfer)
        pinnedPool->registerSlot = env->registerSlot;
    }
}

// a worker: its own readers, the device thread of its index, targets from the run's order until none is left
void JunctionBuilder::worker(JuncRun& run, int w) {
    try {
        GenomeMapper gmap(prepData.getGenomeFilePath());
        gmap.loadFastaIndex();
        BamReader reader(prepData.getSortedBamFilePath());
        reader.open(useCsi);
        reader.setNameHashes(extra);
        DeviceThread* dev = nullptr;
        {
            std::lock_guard<std::mutex> lk(run.mu);
            if (run.deviceThreads.empty()) startDeviceThreads(run);
            dev = run.deviceThreads[(size_t)w % run.deviceThreads.size()].get();
        }
        if (pinnedPool) dev->waitReady();
        while (true) {
            int32_t tid;
            {
                std::lock_guard<std::mutex> lk(run.mu);
                if (run.nextTask >= run.order.size() || !run.firstError.empty()) break;
                tid = run.order[run.nextTask++];
            }
            findJuncs(*dev, reader, gmap, tid);
        }
    } catch (const std::exception& e) {
        std::lock_guard<std::mutex> lk(run.mu);
        if (run.firstError.empty()) run.firstError = e.what();
    }
}

// group chains: every target has been asked for -- what still waits for the rest of its group goes now, then the results are taken
void JunctionBuilder::completeDeferred(JuncRun& run) {
    for (auto& dth : run.deviceThreads)
        if (dth->grouped()) {
            DeviceThread::Cmd c(DeviceThread::Cmd::FLUSH);
            dth->push(std::move(c));
        }
    // A few threads take the targets in index order: a target's rows become Junction objects as soon as its chain has been collected
    // -- the first groups' while the last group's chain still runs -- instead of all 250 000 behind the last chain on this thread
    // (50 ms of the run).  The first error in index order is the one reported, as before.
    std::vector<std::string> errs(deferredTargets.size());
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= deferredTargets.size()) break;
            if (!deferredTargets[i]) continue;
            try {
                completeTarget((int32_t)i, *deferredTargets[i]);
            } catch (const std::exception& e) {
                errs[i] = e.what();
                if (errs[i].empty()) errs[i] = "unknown error";
            }
            deferredTargets[i].reset();
        }
    };
    size_t waiting = 0;
    for (auto& d : deferredTargets) waiting += d ? 1 : 0;
    const size_t nt = std::min<size_t>(waiting, 16);
    if (nt <= 1) {
        work();
    } else {
        std::vector<std::thread> th;
        for (size_t t = 0; t < nt; t++) th.emplace_back(work);
        for (auto& x : th) x.join();
    }
    for (auto& e : errs)
        if (!e.empty() && run.firstError.empty()) run.firstError = e;
}

// calcExtraMetrics (src/junction_builder.cc:293-312): multiple mapping score, flanking alignments, coverage
void JunctionBuilder::calcExtraMetrics(JuncRun& run) {
    cout << "Calculating extra junction metrics:" << endl;
    try {
        std::promise<std::vector<pjb_extra_row>> got;
        std::future<std::vector<pjb_extra_row>> f = got.get_future();
        DeviceThread::Cmd c(DeviceThread::Cmd::EXTRA);
        c.extraDone = &got;
        run.deviceThreads[0]->push(std::move(c));
        const std::vector<pjb_extra_row> xr = f.get();
        for (auto& res : results) {
            const JunctionList& jl = res.js.getJunctions();
            for (size_t k = 0; k < jl.size(); k++) {
                const pjb_extra_row& x = xr.at(res.rowBase + k);
                jl[k]->setMultipleMappingScore(x.mm_score);
                jl[k]->setCoverage(x.coverage);
                jl[k]->setNbUpstreamFlankingAlignments(x.up_aln);
                jl[k]->setNbDownstreamFlankingAlignments(x.down_aln);
            }
        }
    } catch (const std::exception& e) {
        run.firstError = e.what();
    }
}

// Everything the device produced is on the host.  Taking the contexts down (every device buffer), and the page-locked
// rings with them, is 0.1-0.3 s of runtime and driver work that nothing waits for: it runs beside the merge and the
// writers instead of before them.
void JunctionBuilder::tearDown(JuncRun& run) {
    if (teardown && run.firstError.empty()) {
        // a driver that goes on in this process owns the two threads below and waits for them where its next stage needs the device
        // (also under PJB_NORMAL_EXIT: it has joined them before main returns)
        teardown->add(std::thread([pp = std::move(pinnedPool), gp = std::move(genomePool)]() mutable {
            pp.reset();
            gp.reset();
        }));
        teardown->add(std::thread([dts = std::move(run.deviceThreads)]() mutable { dts.clear(); }));
        return;
    }
    // (a process that will leave through exit handlers must not have a thread inside the runtime by then)
    if (!backgroundTeardown || env->normalExit || !run.firstError.empty()) {
        run.deviceThreads.clear();  // joins the device threads (destroys the contexts)
        return;
    }
    // The rings on one thread, the contexts on another (1.67 against 1.70 s on one thread, profiles/r06_e2e_host_tail2.txt).  The
    // page-locked rings start first: giving 1.6 GB of them back takes ~0.15 s here or in the kernel when the process leaves, a context's
    // device memory a third of that -- tools/debug/exit_probe.cc.
    // Giving the rings back EARLIER -- behind the last target's bytes, beside the last chains -- was measured twice and made the run
    // longer both times: the unregister calls hold up the chains' launches, profiles/r06_e2e_pools.txt, r06_e2e_early_free.txt.
    // (moved into the threads: the last owner frees, and that must not be this thread)
    std::thread([pp = std::move(pinnedPool), gp = std::move(genomePool)]() mutable {
        pp.reset();
        gp.reset();
    }).detach();
    std::thread([dts = std::move(run.deviceThreads)]() mutable { dts.clear(); }).detach();
}

double JuncTeardown::wait() {
    const double t0 = HostProfile::now();
    std::vector<std::thread> mine;
    {
        std::lock_guard<std::mutex> lk(mu);
        mine.swap(threads);
    }
    for (auto& t : mine) t.join();
    return HostProfile::now() - t0;
}

// the merge of the targets' systems and its console output (src/junction_builder.cc:258-290)
void JunctionBuilder::mergeResults() {
    cout << " - All threads completed." << endl << " - Combining results from threads." << endl << endl;
    uint64_t unsplicedCount = 0, splicedCount = 0, sumQueryLengths = 0;
    int32_t minQueryLength = INT32_MAX, maxQueryLength = 0;
    cout << std::left << std::setw(12) << "Sequence"
         << "\t" << std::right << std::setw(12) << "unspliced"
         << "\t" << std::right << std::setw(12) << "spliced"
         << "\t" << std::right << std::setw(12) << "total" << endl;
    {
        size_t total = 0;
        for (auto& res : results) total += res.js.getJunctions().size();
        junctionSystem.reserve(total);
    }
    for (auto& res : results) {
        junctionSystem.absorb(res.js);  // (the per-target systems keep their lists -- --extra walks them -- not their maps)
        unsplicedCount += res.unsplicedCount;
        splicedCount += res.splicedCount;
        sumQueryLengths += res.sumQueryLengths;
        minQueryLength = std::min(minQueryLength, res.minQueryLength);
        maxQueryLength = std::max(maxQueryLength, res.maxQueryLength);
        cout << std::left << std::setw(12) << res.name << "\t" << std::right << std::setw(12) << res.unsplicedCount << "\t"
             << std::right << std::setw(12) << res.splicedCount << "\t" << std::right << std::setw(12)
             << res.splicedCount + res.unsplicedCount << endl;
    }
    cout << endl << "Sorting and reindexing merged junctions...";
    cout.flush();
    junctionSystem.sort();
    junctionSystem.index();
    cout << " done." << endl << endl;
    const uint64_t totalAlignments = splicedCount + unsplicedCount;
    const double meanQueryLength = (double)sumQueryLengths / (double)totalAlignments;
    junctionSystem.setQueryLengthStats(minQueryLength, meanQueryLength, maxQueryLength);
    cout << "Final stats:" << endl
         << " - Processed " << totalAlignments << " alignments." << endl
         << " - Alignment query length statistics: min: " << minQueryLength << "; mean: " << meanQueryLength
         << "; max: " << maxQueryLength << ";" << endl
         << " - Found " << junctionSystem.size() << " junctions from " << splicedCount << " spliced alignments." << endl
         << " - Found " << unsplicedCount << " unspliced alignments." << endl;
}

void JunctionBuilder::findJunctions() {
    WallTimer timer;
    results.clear();
    results.resize(refs->size());
    if (!deviceCount.valid()) deviceCount = std::async(std::launch::async, [] { return pjb_device_count(); }).share();
    JuncRun run;
    planIngest(run);
    const double t_workers0 = HostProfile::now();
    g_prof.mark("workers start");
    cout << " done." << endl;
    cout << "Finding junctions and calculating basic metrics:" << endl;
    cout << " - Queueing " << refs->size() << " target sequences for processing in the thread pool" << endl;
    cout << " - Processing: " << endl;
    std::vector<std::thread> pool;
    deferredTargets.assign(refs->size(), nullptr);
    for (int w = 0; w < run.nthreads; w++) pool.emplace_back([this, &run, w] { worker(run, w); });
    for (auto& t : pool) t.join();
    completeDeferred(run);
    if (extra && run.firstError.empty() && !run.deviceThreads.empty()) calcExtraMetrics(run);
    tearDown(run);
    if (!run.firstError.empty()) throw JunctionBuilderException(run.firstError);
    const double t_workers1 = HostProfile::now();
    g_prof.mark("workers and device threads done");
    mergeResults();
    const double t_merge1 = HostProfile::now();
    if (junctionSystem.size() > 1) {
        cout << " - Calculating junctions stats that require comparisons with other junctions...";
        cout.flush();
        junctionSystem.calcJunctionStats();
        cout << " done." << endl;
    }
    if (g_prof.on)
        cerr << "[host profile] workers " << (t_workers1 - t_workers0) << " s, merge+sort+index " << (t_merge1 - t_workers1)
             << " s, calcJunctionStats " << (HostProfile::now() - t_merge1) << " s" << endl;
}

// command line of `portcullis junc` (src/junction_builder.cc:359-454); a small hand-rolled parser
// replaces boost::program_options.
int JunctionBuilder::main(int argc, char* argv[]) {
    std::string prepDir, output = DEFAULT_JUNC_OUTPUT, source = DEFAULT_JUNC_SOURCE, ori = "UNKNOWN", strand = "UNKNOWN";
    int threads = DEFAULT_JUNC_THREADS, devices = 0;
    size_t batch = 0;
    std::string ingest;
    uint64_t deviceMem = 0;
    bool haveDeviceMem = false;
    bool extra = false, separate = false, useCsi = false, exonGff = false, intronGff = false, verbose = false, help = false;
    auto need = [&](int& i) -> std::string {
        if (i + 1 >= argc) throw JunctionBuilderException(std::string("Missing value for option ") + argv[i]);
        return argv[++i];
    };
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-o" || a == "--output") output = need(i);
        else if (a == "-t" || a == "--threads") threads = atoi(need(i).c_str());
        else if (a == "--orientation") ori = need(i);
        else if (a == "--strandedness") strand = need(i);
        else if (a == "--source") source = need(i);
        else if (a == "--devices") devices = atoi(need(i).c_str());
        else if (a == "--batch") batch = (size_t)atol(need(i).c_str());
        else if (a == "--ingest") ingest = need(i);
        else if (a == "--device_mem") deviceMem = parseDeviceMem(need(i)), haveDeviceMem = true;
        else if (a == "--separate") separate = true;
        else if (a == "--extra") extra = true;
        else if (a == "-c" || a == "--use_csi") useCsi = true;
        else if (a == "--exon_gff") exonGff = true;
        else if (a == "--intron_gff") intronGff = true;
        else if (a == "-v" || a == "--verbose") verbose = true;
        else if (a == "--help" || a == "-h") help = true;
        else if (!a.empty() && a[0] == '-') throw JunctionBuilderException("Unknown option: " + a);
        else prepDir = a;
    }
    if (help || prepDir.empty()) {
        cout << title() << endl << endl << description() << endl << endl << "Usage: " << usage() << endl
             << "  -o, --output <prefix>      Output prefix for files generated by this program (default " << DEFAULT_JUNC_OUTPUT << ")" << endl
             << "  -t, --threads <n>          Host decode threads; one target sequence per thread at a time" << endl
             << "      --orientation <o>      SE, FR, RF, FF or UNKNOWN" << endl
             << "      --strandedness <s>     unstranded, firststrand, secondstrand or UNKNOWN" << endl
             << "      --source <name>        Source column of the BED/GFF output (default portcullis)" << endl
             << "      --exon_gff             Also write <prefix>.junctions.exon.gff3" << endl
             << "      --intron_gff           Also write <prefix>.junctions.intron.gff3" << endl
             << "  -c, --use_csi              Use the CSI index of the prepared BAM instead of the BAI" << endl
             << "      --devices <n>          Number of GPUs to use (default: all visible)" << endl
             << "      --ingest <device|host> Where BGZF inflate and BAM record parsing run (default device; env PORTCULLIS_INGEST)" << endl
             << "      --device_mem <size>    Device memory the run may hold on one GPU: an integer with an optional K, M or G (default: no" << endl
             << "                             budget; env PORTCULLIS_DEVICE_MEM).  Group chains that do not fit are finished target by target" << endl
             << "  -v, --verbose" << endl;
        return help ? 0 : 1;
    }
    WallTimer timer;
    cout << "Running portcullis in junction builder mode" << endl << "------------------------------------------" << endl << endl;
    // deliberately never destroyed: the program ends right after process() and freeing every junction object
    // one by one would only delay that
    JunctionBuilder& jb = *new JunctionBuilder(prepDir, output);
    jb.setThreads((uint16_t)std::max(1, threads));
    jb.setExtra(extra);
    jb.setSeparate(separate);
    jb.setSource(source);
    jb.setUseCsi(useCsi);
    jb.setOutputExonGFF(exonGff);
    jb.setOutputIntronGFF(intronGff);
    jb.setVerbose(verbose);
    jb.setOrientation(bam::orientationFromString(ori));
    jb.setStrandSpecific(bam::strandednessFromString(strand));
    if (devices > 0) jb.setDevices(devices);
    if (haveDeviceMem) jb.setDeviceMem(deviceMem);
    if (batch > 0) jb.setBatchRecords(batch);
    if (!ingest.empty()) {
        if (ingest != "host" && ingest != "device") throw JunctionBuilderException("--ingest takes host or device");
        jb.setDeviceIngest(ingest == "device");
    }
    jb.backgroundTeardown = true;  // (this program leaves through _exit)
    jb.process();
    if (g_prof.on) cerr << "[host profile] main: " << timer.elapsed() << " s until process() returned" << endl;
    return 0;
}

}  // namespace portcullis
