// Prepare (`portcullis_amd prep`): see prepare.hpp.  Mirrors src/prepare.cc:89-332 (Prepare::copy, genomeIndex, bamIndex,
// prepare) and 373- (Prepare::main) of the reference; the BAM index is built on the device instead of by `samtools index`,
// --merge (src/prepare.cc:154-195, `samtools merge`) merges coordinate-sorted inputs on the device, target by target, and --sort
// (Prepare::bamSort, `samtools sort`) sorts an unsorted input on the device, run by run, merging the runs where there are several.
// --build_csi makes every index built here a CSI (pjb_index_begin_csi / _end_csi; `samtools index -c`), which also covers targets of 2^29 bases or more.
#include <portcullis/bam/bam_writer.hpp>
#include <portcullis/bam/bam_reader.hpp>
#include <portcullis/bam/genome_mapper.hpp>
#include <portcullis/merge_header.hpp>
#include <portcullis/prepare.hpp>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <mutex>
#include <thread>

#include "../../../include/portcullis_amd.h"
#include "pinned_pool.hpp"

using std::cout;
using std::endl;
using std::string;

namespace portcullis {

namespace {

bool lexists(const string& p) {
    struct stat st;
    return lstat(p.c_str(), &st) == 0;
}
bool fileExists(const string& p) {  // (follows links: a dangling link is not a file)
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}
bool makeDirs(const string& dir) {
    string cur;
    for (size_t i = 0; i <= dir.size(); i++) {
        if (i == dir.size() || dir[i] == '/') {
            if (!cur.empty() && !fileExists(cur) && mkdir(cur.c_str(), 0777) != 0 && errno != EEXIST) return false;
        }
        if (i < dir.size()) cur += dir[i];
    }
    return true;
}
double nowSeconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

constexpr int64_t BAI_MAX_TARGET = (int64_t)1 << 29;  // reg2bin covers [0, 2^29)

// One BGZF block header at p (n bytes in reach): the block's size, 0 if the header is not complete yet; throws if it is none.
size_t bgzfBlockSize(const uint8_t* p, size_t n, int64_t fileOffset) {
    if (n < 18) return 0;
    if (p[0] != 31 || p[1] != 139 || p[2] != 8 || !(p[3] & 4)) throw PrepareException("Not a BGZF block header at byte " + std::to_string(fileOffset) + " of the BAM file");
    const size_t xlen = p[10] | (size_t)p[11] << 8;
    if (n < 12 + xlen) return 0;
    size_t bsize = 0;
    for (size_t x = 0; x + 4 <= xlen;) {
        const uint8_t* f = p + 12 + x;
        const size_t slen = f[2] | (size_t)f[3] << 8;
        if (f[0] == 'B' && f[1] == 'C' && slen == 2 && x + 6 <= xlen) bsize = (size_t)(f[4] | (size_t)f[5] << 8) + 1;
        x += 4 + slen;
    }
    if (bsize < xlen + 20) throw PrepareException("BGZF block at byte " + std::to_string(fileOffset) + " of the BAM file has no valid BC field");
    return bsize;
}

// What the indexer needs of a BAM file's header: the targets, and where the first alignment record starts.
struct BamHead {
    string text;  // the SAM header text
    std::vector<string> names;
    std::vector<int32_t> lens;
    int64_t firstBlock = 0;  // file offset of the block that holds the first record's first byte (or follows the header)
    int32_t firstUoffset = 0;
};

BamHead readBamHead(const string& bamFile) {
    FILE* f = fopen(bamFile.c_str(), "rb");
    if (!f) throw PrepareException("Could not open BAM file: " + bamFile);
    struct Closer {
        FILE* f;
        ~Closer() { fclose(f); }
    } closer{f};
    std::vector<uint8_t> head;              // inflated bytes so far
    std::vector<std::pair<int64_t, size_t>> blocks;  // (file offset, inflated bytes before it)
    int64_t at = 0;
    std::vector<uint8_t> out(65536);
    auto need = [&](size_t n) {
        while (head.size() < n) {
            uint8_t h[18 + 65536];
            if (fseeko(f, (off_t)at, SEEK_SET) != 0) throw PrepareException("Could not read BAM file: " + bamFile);
            const size_t got = fread(h, 1, sizeof h, f);
            const size_t bsize = got ? bgzfBlockSize(h, got, at) : 0;
            if (bsize == 0 || bsize > got) throw PrepareException("The header of BAM file " + bamFile + " is truncated");
            const size_t xlen = h[10] | (size_t)h[11] << 8;
            z_stream zs;
            memset(&zs, 0, sizeof zs);
            if (inflateInit2(&zs, -15) != Z_OK) throw PrepareException("zlib: inflateInit2 failed");
            zs.next_in = h + 12 + xlen;
            zs.avail_in = (uInt)(bsize - xlen - 20);
            zs.next_out = out.data();
            zs.avail_out = (uInt)out.size();
            const int zr = inflate(&zs, Z_FINISH);
            const size_t made = out.size() - zs.avail_out;
            inflateEnd(&zs);
            if (zr != Z_STREAM_END) throw PrepareException("Corrupt BGZF block at byte " + std::to_string(at) + " of " + bamFile);
            blocks.push_back({at, head.size()});
            head.insert(head.end(), out.begin(), out.begin() + (long)made);
            at += (int64_t)bsize;
        }
    };
    auto rd32 = [&](size_t o) { return (int32_t)((uint32_t)head[o] | (uint32_t)head[o + 1] << 8 | (uint32_t)head[o + 2] << 16 | (uint32_t)head[o + 3] << 24); };
    need(12);
    if (memcmp(head.data(), "BAM\1", 4) != 0) throw PrepareException("Not a BAM file: " + bamFile);
    const int32_t lText = rd32(4);
    if (lText < 0) throw PrepareException("Corrupt BAM header: " + bamFile);
    size_t p = 8 + (size_t)lText;
    need(p + 4);
    const int32_t nRef = rd32(p);
    p += 4;
    if (nRef < 0) throw PrepareException("Corrupt BAM header: " + bamFile);
    BamHead H;
    H.text.assign((const char*)&head[8], (size_t)lText);
    for (int32_t t = 0; t < nRef; t++) {
        need(p + 4);
        const int32_t lName = rd32(p);
        if (lName < 1) throw PrepareException("Corrupt BAM header: " + bamFile);
        p += 4;
        need(p + (size_t)lName + 4);
        H.names.emplace_back((const char*)&head[p], (size_t)lName - 1);
        p += (size_t)lName;
        H.lens.push_back(rd32(p));
        p += 4;
    }
    // the block in which inflated byte p lies; the block behind the header when the header ends with its block
    H.firstBlock = at;
    H.firstUoffset = 0;
    for (size_t b = 0; b < blocks.size(); b++) {
        const size_t end = b + 1 < blocks.size() ? blocks[b + 1].second : head.size();
        if (blocks[b].second <= p && p < end) {
            H.firstBlock = blocks[b].first;
            H.firstUoffset = (int32_t)(p - blocks[b].second);
        }
    }
    return H;
}

// The file's bytes in pieces of a ring of page-locked buffers, read ahead by a thread of its own.  A buffer holds two pieces'
// worth: the piece is read into its second half, and what the piece before it left unconsumed (a block cut by the piece's end,
// the block of a record that straddles it) is copied in front of it, so that the indexer sees whole blocks in one run of memory.
struct PieceReader {
    struct Piece {
        uint8_t* buf = nullptr;  // the ring buffer (nullptr: the end of the file, or an error)
        size_t got = 0;
        bool last = false;
    };
    PinnedPool pool;
    size_t piece;
    int fd;
    int64_t size, from;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Piece> ready;
    string error;
    std::thread th;

    PieceReader(int fd_, int64_t from_, int64_t size_, size_t pieceBytes) : pool(3, 2 * pieceBytes), piece(pieceBytes), fd(fd_), size(size_), from(from_) {
        th = std::thread([this] { run(); });
    }
    ~PieceReader() {  // (also an early exit: the reader gets every buffer back and sees `stop`)
        std::unique_lock<std::mutex> lk(mu);
        stop = true;
        for (;;) {
            while (!ready.empty()) {
                if (ready.front().buf) pool.release(ready.front().buf);
                ready.pop_front();
            }
            if (exited) break;
            cv.wait(lk);
        }
        lk.unlock();
        th.join();
    }
    void run() {
        struct Exit {
            PieceReader& r;
            ~Exit() {
                std::lock_guard<std::mutex> lk(r.mu);
                r.exited = true;
                r.cv.notify_all();
            }
        } onExit{*this};
        int64_t at = from;
        for (;;) {
            Piece pc;
            pc.buf = pool.acquire(2 * piece);
            if (!pc.buf) {
                push(Piece(), "Could not allocate page-locked memory for the BAM file's pieces");
                return;
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                if (stop) {
                    pool.release(pc.buf);
                    return;
                }
            }
            const size_t want = (size_t)std::min<int64_t>((int64_t)piece, size - at);
            size_t got = 0;
            while (got < want) {
                const ssize_t r = pread(fd, pc.buf + piece + got, want - got, (off_t)(at + (int64_t)got));
                if (r < 0 && errno == EINTR) continue;
                if (r <= 0) {
                    pool.release(pc.buf);
                    push(Piece(), "Could not read the BAM file");
                    return;
                }
                got += (size_t)r;
            }
            pc.got = got;
            at += (int64_t)got;
            pc.last = at >= size;
            const bool last = pc.last;
            push(pc, "");
            if (last) return;
        }
    }
    void push(const Piece& pc, const string& err) {
        std::lock_guard<std::mutex> lk(mu);
        if (!err.empty()) error = err;
        ready.push_back(pc);
        cv.notify_all();
    }
    Piece next() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !ready.empty(); });
        Piece pc = ready.front();
        ready.pop_front();
        if (!pc.buf) throw PrepareException(error);
        return pc;
    }
    void release(uint8_t* buf) { pool.release(buf); }
    bool stop = false, exited = false;
};

}  // namespace

Prepare::Prepare(const string& outputDir) : output(outputDir) {
    struct stat st;
    if (stat(outputDir.c_str(), &st) != 0) {
        if (!makeDirs(outputDir) || stat(outputDir.c_str(), &st) != 0) throw PrepareException("Could not create output directory at: " + outputDir);
    } else if (!S_ISDIR(st.st_mode))
        throw PrepareException("File exists with name of suggested output directory: " + outputDir);
}

void Prepare::clean() {
    for (const string& p : {output.getUnsortedBamFilePath(), output.getSortedBamFilePath(), output.getBamIndexFilePath(false), output.getBamIndexFilePath(true),
                            output.getGenomeFilePath(), output.getGenomeIndexFilePath()})
        if (lexists(p)) unlink(p.c_str());
}

bool Prepare::copy(const string& from, const string& to, const string& msg, bool requireInputFileExists) {
    if (lexists(to)) cout << "Prepped " << msg << " file detected: " << to << endl;
    else if (requireInputFileExists || lexists(from)) {
        if (useLinks) {
            char real[PATH_MAX];
            if (!realpath(from.c_str(), real)) throw PrepareException("Could not resolve " + msg + " file: " + from);
            if (symlink(real, to.c_str()) != 0) throw PrepareException("Could not create symlink from " + from + " to " + to);
            cout << "Created symlink from " << from << " to " << to << endl;
        } else {
            const double t0 = nowSeconds();
            cout << "Copying from " << from << " to " << to << " ... ";
            cout.flush();
            std::ifstream src(from, std::ios::binary);
            std::ofstream dst(to, std::ios::binary);
            if (!src || !dst) throw PrepareException("Could not copy " + from + " to " + to);
            dst << src.rdbuf();
            dst.close();
            if (!dst) throw PrepareException("Could not copy " + from + " to " + to);
            cout << "done." << endl;
            printf(" - Copy %s - Wall time taken: %.1fs\n\n", msg.c_str(), nowSeconds() - t0);
        }
    } else
        cout << "Existing " << msg << " not found.  Will create later." << endl;
    return lexists(to);
}

bool Prepare::genomeIndex() {
    const string indexFile = output.getGenomeIndexFilePath();
    if (lexists(indexFile)) cout << "Pre-indexed genome detected: " << indexFile << endl;
    else {
        const double t0 = nowSeconds();
        cout << "Indexing genome " << output.getGenomeFilePath() << " ... ";
        cout.flush();
        bam::GenomeMapper(output.getGenomeFilePath()).buildFastaIndex();
        cout << "done." << endl << "Genome index file created at: " << indexFile << endl;
        printf(" - Genome Index - Wall time taken: %.1fs\n\n", nowSeconds() - t0);
    }
    return fileExists(indexFile);
}

bool Prepare::bamIndex(bool indexCopied) {
    const string indexFile = output.getBamIndexFilePath(useCsi);
    if (indexCopied || lexists(indexFile)) cout << "Pre-indexed BAM detected: " << indexFile << endl;
    else {
        const double t0 = nowSeconds();
        cout << "Indexing " << output.getSortedBamFilePath() << " on the GPU ... ";
        cout.flush();
        buildIndexOnDevice(output.getSortedBamFilePath(), indexFile);
        cout << "done." << endl << "BAM index created at: " << indexFile << endl;
        printf(" - BAM Index - Wall time taken: %.1fs\n\n", nowSeconds() - t0);
    }
    return lexists(indexFile);
}

namespace {

const char* const NO_DEVICE_INDEX =
    "No MI355X (HIP device) is visible: the BAM index is built on the GPU and has no CPU fallback.  Put an index made elsewhere "
    "(samtools index) beside the BAM file, or run prep where the GPU is.";

// A file that is not in coordinate order: what `prep --sort` catches and sorts, and everything else passes on as the refusal it is.
struct UnsortedBam : PrepareException {
    explicit UnsortedBam(const string& m) : PrepareException(m) {}
};
string unsortedMessage(const string& deviceMessage, const string& bamFile, bool nameFile) {
    return "The BAM file is not in coordinate order: " + deviceMessage + ".  Sort it first (samtools sort), or pass --sort: prep then sorts it on the GPU." +
           (nameFile ? "  (" + bamFile + ")" : string());
}

// The one read of a BAM file in pieces, for whoever takes them (the index build, the sort): the file from the block of its first record on,
// through the ring of page-locked pieces, as runs of whole BGZF blocks in file order.  `feed(region, bytes, fileOffset, uoff, last, nv)`
// gets a run of blocks that starts at fileOffset, the offset of the first record not yet taken in its inflated bytes, and whether the
// file ends with it; it returns true and sets nv to the virtual offset (in the file) of the first record it did not take -- the next
// run starts with that record's block --, or false: its first record is longer than these blocks, which then come again with the
// next piece behind them.  `pieceCap` bounds the piece size (0: none).
template <typename Feed>
void walkPieces(const string& bamFile, const BamHead& H, size_t pieceCap, Feed feed) {
    const int fd = open(bamFile.c_str(), O_RDONLY);
    if (fd < 0) throw PrepareException("Could not open BAM file: " + bamFile);
    struct Fd {
        int fd;
        ~Fd() { close(fd); }
    } fdGuard{fd};
    struct stat st;
    if (fstat(fd, &st) != 0) throw PrepareException("Could not stat BAM file: " + bamFile);
    const int64_t size = (int64_t)st.st_size;
    // PORTCULLIS_PIECE_BYTES (tests) / PORTCULLIS_PIECE_MB as in junc: what is read and handed to the device at a time.  The default is
    // larger than junc's 64 MB: a piece is one inflate launch, and a launch takes ~27 ms whatever its size (a 3.4 GB file of 20 M records:
    // 1.91 s with pieces of 64 MB, 0.96 s with 256 MB, 1.03 s with 1 GB -- page-locking the ring then costs what the launches save).
    size_t piece = (size_t)std::max(1, getenv("PORTCULLIS_PIECE_MB") ? atoi(getenv("PORTCULLIS_PIECE_MB")) : 256) << 20;
    if (const char* e = getenv("PORTCULLIS_PIECE_BYTES"))
        if (atoi(e) > 0) piece = (size_t)std::max(64, atoi(e));
    if (pieceCap) piece = std::min(piece, std::max<size_t>(pieceCap, 64));
    piece = (size_t)std::min<int64_t>((int64_t)piece, std::max<int64_t>(size - H.firstBlock, 64));

    // `carry`: the bytes from file offset carryOff on that have been read and not consumed
    std::vector<uint8_t> carry, big;
    int64_t carryOff = H.firstBlock;
    int32_t uoff = H.firstUoffset;
    if (H.firstBlock >= size) {  // a header and nothing else (not even the EOF block)
        uint64_t nv = 0;
        feed((const uint8_t*)nullptr, (size_t)0, H.firstBlock, 0, true, nv);
        return;
    }
    PieceReader reader(fd, H.firstBlock, size, piece);
    for (bool done = false; !done;) {
        PieceReader::Piece pc = reader.next();
        struct Release {
            PieceReader& r;
            uint8_t* b;
            ~Release() { r.release(b); }
        } rel{reader, pc.buf};
        uint8_t* region;
        const size_t regionBytes = carry.size() + pc.got;
        if (carry.size() <= piece) {  // the usual case: in front of the piece, in its page-locked buffer
            region = pc.buf + piece - carry.size();
            if (!carry.empty()) memcpy(region, carry.data(), carry.size());
        } else {  // a block or a record longer than a piece: a run of pageable memory as long as it takes
            big.resize(regionBytes);
            memcpy(big.data(), carry.data(), carry.size());
            memcpy(big.data() + carry.size(), pc.buf + piece, pc.got);
            region = big.data();
        }
        // whole blocks
        size_t whole = 0;
        while (whole < regionBytes) {
            const size_t bs = bgzfBlockSize(region + whole, regionBytes - whole, carryOff + (int64_t)whole);
            if (bs == 0 || whole + bs > regionBytes) break;
            whole += bs;
        }
        if (pc.last && whole != regionBytes) throw PrepareException("The BAM file ends inside a BGZF block (truncated file): " + bamFile);
        size_t consumed = 0;
        if (whole > 0) {
            uint64_t nv = ~0ull;
            if (feed((const uint8_t*)region, whole, carryOff, uoff, pc.last, nv)) {
                consumed = (size_t)((int64_t)(nv >> 16) - carryOff);
                uoff = (int32_t)(nv & 0xffff);
            } else if (pc.last)
                throw PrepareException("The BAM file ends inside an alignment record (truncated file): " + bamFile);
            // (else: the first record is longer than these blocks: the same blocks again, with the next piece behind them)
        }
        if (pc.last) done = true;
        else {
            std::vector<uint8_t> rest(region + consumed, region + regionBytes);
            carry.swap(rest);
            carryOff += (int64_t)consumed;
        }
    }
}

struct DeviceCtx {  // a context without chains: what prep's index, merge and sort run on
    pjb_ctx* c = nullptr;
    DeviceCtx() {
        pjb_config cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.abi_version = PJB_ABI_VERSION;
        cfg.flags = PJB_FLAG_NO_CHAINS;
        if (pjb_create(&c, &cfg) != PJB_OK) throw PrepareException(string("pjb_create: ") + pjb_last_error(nullptr));
    }
    ~DeviceCtx() {
        if (c) pjb_destroy(c);
    }
    DeviceCtx(const DeviceCtx&) = delete;
    DeviceCtx& operator=(const DeviceCtx&) = delete;
};

const uint8_t BGZF_EOF_BLOCK[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
const int32_t BGZF_CUT = 0xff00;  // inflated bytes a member of a file written here holds
// host bytes -> BGZF members, deflated on the device (no EOF block)
std::vector<uint8_t> deflateMembers(pjb_ctx* c, const std::vector<uint8_t>& raw) {
    std::vector<uint8_t> packed(((raw.size() + BGZF_CUT - 1) / BGZF_CUT) * 65536);
    int64_t n = 0;
    if (pjb_deflate_bgzf(c, raw.data(), (int64_t)raw.size(), BGZF_CUT, packed.data(), (int64_t)packed.size(), &n, nullptr) != PJB_OK)
        throw PrepareException(string("pjb_deflate_bgzf: ") + pjb_last_error(c));
    packed.resize((size_t)n);
    return packed;
}

// The index of a coordinate-sorted BAM file, built on the device ...
struct BuiltIndex {
    bam::BaiBins bins;
    bam::BaiLinear lin;    // a BAI's
    bam::CsiLoffsets loff; // a CSI's, with its depth
    int32_t csiDepth = -1;
    std::vector<uint8_t> csiFile;  // the CSI as the bytes of its file: deflated on the context that built it
    int64_t records = 0, chunks = 0;
};
// (nameFile: the refusal of an unsorted file says which file -- prep --merge has several)
// (csi: a CSI of the depth htslib would choose, for targets of any length)
BuiltIndex buildIndex(const string& bamFile, bool nameFile, bool csi) {
    const BamHead H = readBamHead(bamFile);
    for (size_t t = 0; !csi && t < H.lens.size(); t++)
        if ((int64_t)H.lens[t] >= BAI_MAX_TARGET)
            throw PrepareException("BAI cannot index this target: " + H.names[t] + " has " + std::to_string(H.lens[t]) +
                                   " bases, and a BAI index reaches 2^29.  Index the file with `samtools index -c` and use the CSI index (junc --use_csi): writing "
                                   "CSI is not built into portcullis_amd prep.  Or pass --build_csi: prep then builds a CSI index on the GPU.");
    if (pjb_device_count() <= 0) throw PrepareException(NO_DEVICE_INDEX);
    DeviceCtx ctx;
    auto check = [&](int rc, const char* what) {
        if (rc == PJB_OK) return;
        const string msg = pjb_last_error(ctx.c);
        if (rc == PJB_ERR_UNSORTED) throw UnsortedBam(unsortedMessage(msg, bamFile, nameFile));
        if (rc == PJB_ERR_ARG && msg.find("BAI cannot index") != string::npos)
            throw PrepareException(msg + ".  Index the file with `samtools index -c` and use the CSI index (junc --use_csi), or pass --build_csi.");
        throw PrepareException(string(what) + ": " + msg);
    };
    check(pjb_set_refs(ctx.c, (int32_t)H.lens.size(), H.lens.data()), "pjb_set_refs");
    check(csi ? pjb_index_begin_csi(ctx.c, -1) : pjb_index_begin(ctx.c), csi ? "pjb_index_begin_csi" : "pjb_index_begin");
    walkPieces(bamFile, H, 0, [&](const uint8_t* region, size_t bytes, int64_t fileOffset, int32_t uoff, bool last, uint64_t& nv) {
        nv = ~0ull;
        const int rc = pjb_index_piece(ctx.c, region, (int64_t)bytes, fileOffset, uoff, last ? 1 : 0, &nv);
        if (rc == PJB_ERR_ARG && nv != ~0ull && !last) return false;  // the first record is longer than these blocks
        check(rc, "pjb_index_piece");
        return true;
    });
    const size_t nRef = H.lens.size();
    BuiltIndex X;
    X.bins.resize(nRef);
    if (csi) {
        pjb_csi_result res;
        check(pjb_index_end_csi(ctx.c, &res), "pjb_index_end_csi");
        X.loff.resize(nRef);
        for (int64_t k = 0; k < res.n_chunks; k++) {
            const pjb_index_chunk& ch = res.chunks[k];
            X.bins[(size_t)ch.tid][ch.bin].push_back({ch.vbeg, ch.vend});
            X.loff[(size_t)ch.tid][ch.bin] = res.loffset[k];
        }
        X.csiDepth = res.depth;
        X.records = res.n_records;
        X.chunks = res.n_chunks;
        // the file's bytes: the payload in BGZF members deflated on the device, the EOF block behind them
        X.csiFile = deflateMembers(ctx.c, bam::csiPayload(res.min_shift, res.depth, X.bins, X.loff));
        X.csiFile.insert(X.csiFile.end(), BGZF_EOF_BLOCK, BGZF_EOF_BLOCK + sizeof BGZF_EOF_BLOCK);
        return X;
    }
    pjb_index_result res;
    check(pjb_index_end(ctx.c, &res), "pjb_index_end");
    // the chunk list is ordered by (target, bin, file order): the maps below only group it
    X.lin.resize(nRef);
    for (int64_t k = 0; k < res.n_chunks; k++) {
        const pjb_index_chunk& ch = res.chunks[k];
        X.bins[(size_t)ch.tid][ch.bin].push_back({ch.vbeg, ch.vend});
    }
    for (size_t t = 0; t < nRef; t++) X.lin[t].assign(res.lin + res.lin_off[t], res.lin + res.lin_off[t + 1]);
    X.records = res.n_records;
    X.chunks = res.n_chunks;
    return X;
}

// ... and written as a .bai, or as the .csi it was built as
void writeIndex(const BuiltIndex& X, const string& baiFile) {
    const string tmp = baiFile + ".tmp";
    if (X.csiDepth >= 0) bam::writeCsi(tmp, X.csiFile);
    else bam::writeBai(tmp, X.bins, X.lin);
    if (rename(tmp.c_str(), baiFile.c_str()) != 0) throw PrepareException("Could not write BAM index: " + baiFile);
}

}  // namespace

void Prepare::buildIndexOnDevice(const string& bamFile, const string& baiFile) {
    const BuiltIndex X = buildIndex(bamFile, false, buildCsi);
    writeIndex(X, baiFile);
    if (verbose) {
        cout << endl << "Indexed " << X.records << " alignment records: " << X.chunks << " chunks";
        if (X.csiDepth >= 0) cout << ", a CSI of depth " << X.csiDepth;
        cout << "." << endl;
    }
}

// ---- prep --merge: several coordinate-sorted files into the prepared directory's one, target by target on the device ----------------
namespace {

struct Unlinker {  // the merge's temporary files: gone when it ends, however it ends
    std::vector<string> paths;
    ~Unlinker() {
        for (const string& p : paths) unlink(p.c_str());
    }
};
void writeAll(FILE* f, const void* p, size_t n, const string& path) {
    if (n && fwrite(p, 1, n, f) != n) throw PrepareException("Could not write to " + path);
}
void put32(std::vector<uint8_t>& v, int32_t x) {
    for (int k = 0; k < 4; k++) v.push_back((uint8_t)((uint32_t)x >> (8 * k)));
}
// the size of the whole BGZF block at `off` of a file (0: there is none, or it is not a plain one)
size_t followingBlock(const string& path, uint64_t off) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return 0;
    uint8_t h[18];
    struct stat st;
    size_t bs = 0;
    if (fstat(fileno(f), &st) == 0 && fseeko(f, (off_t)off, SEEK_SET) == 0 && fread(h, 1, 18, f) == 18 && h[0] == 31 && h[1] == 139 && h[2] == 8 && (h[3] & 4) &&
        h[10] == 6 && h[11] == 0 && h[12] == 'B' && h[13] == 'C')
        bs = (size_t)(h[16] | (size_t)h[17] << 8) + 1;
    fclose(f);
    return bs && off + bs <= (uint64_t)st.st_size ? bs : 0;
}
// the inflated bytes in front of a BAM file's first record
std::vector<uint8_t> bamHeaderBytes(const string& text, const std::vector<string>& names, const std::vector<int32_t>& lens) {
    std::vector<uint8_t> h = {'B', 'A', 'M', 1};
    put32(h, (int32_t)text.size());
    h.insert(h.end(), text.begin(), text.end());
    put32(h, (int32_t)names.size());
    for (size_t t = 0; t < names.size(); t++) {
        put32(h, (int32_t)names[t].size() + 1);
        h.insert(h.end(), names[t].begin(), names[t].end());
        h.push_back(0);
        put32(h, lens[t]);
    }
    return h;
}
// host bytes -> BGZF members (on the device) -> the file
void deflateToFile(pjb_ctx* c, const std::vector<uint8_t>& raw, FILE* out, const string& path) {
    if (raw.empty()) return;
    const std::vector<uint8_t> packed = deflateMembers(c, raw);
    writeAll(out, packed.data(), packed.size(), path);
}

const char* const NO_DEVICE_SORT =
    "No MI355X (HIP device) is visible: the BAM file is sorted on the GPU and there is no CPU fallback.  Sort it elsewhere (samtools sort) and pass the "
    "coordinate-sorted file, or run prep where the GPU is.";

// What a run of the sort held and made (-v)
struct SortRunInfo {
    string path;
    int64_t records = 0, unplaced = 0, compressedIn = 0;
    bool wasSorted = false;
    uint64_t peakHeld = 0;
};

// `prep --sort`: the records of an unsorted file in coordinate order, as one or several complete BAM files (runs: each holds a stretch
// of the input, stable-sorted by (refID as unsigned, pos), under the header `headerText`).  One read of the file through walkPieces; a
// run is closed before the compressed bytes handed over would pass `runBytes` (a piece is no longer than that; a run takes one piece at
// least), or when the device has no room for the next piece.  The run
// files are named by `runPath(k)` and listed in `tempPaths` before they are created.
std::vector<SortRunInfo> sortBamToRuns(const string& bamFile, const string& headerText, int64_t runBytes, const std::function<string(size_t)>& runPath, std::vector<string>& tempPaths) {
    const BamHead H = readBamHead(bamFile);
    if (pjb_device_count() <= 0) throw PrepareException(NO_DEVICE_SORT);
    DeviceCtx ctx;
    auto check = [&](int rc, const char* what) {
        if (rc != PJB_OK) throw PrepareException(string(what) + " (" + bamFile + "): " + pjb_last_error(ctx.c));
    };
    check(pjb_set_refs(ctx.c, (int32_t)H.lens.size(), H.lens.data()), "pjb_set_refs");
    const std::vector<uint8_t> head = bamHeaderBytes(headerText, H.names, H.lens);
    std::vector<SortRunInfo> runs;
    bool open = false;
    int64_t runIn = 0, runRecords = 0;
    auto closeRun = [&] {
        pjb_bam_sort_result res;
        const int rc = pjb_bam_sort_end(ctx.c, BGZF_CUT, &res);
        if (rc == PJB_ERR_NOMEM)
            throw PrepareException("prep --sort: a run of " + std::to_string(runIn) + " compressed bytes does not fit the device memory this run may hold (" +
                                   pjb_last_error(ctx.c) + ").  Set PORTCULLIS_SORT_RUN_BYTES to a smaller run, or sort the file elsewhere (samtools sort).");
        check(rc, "pjb_bam_sort_end");
        SortRunInfo info;
        info.path = runPath(runs.size());
        info.records = res.n_records;
        info.unplaced = res.n_unplaced;
        info.compressedIn = runIn;
        info.wasSorted = res.was_sorted != 0;
        unlink(info.path.c_str());  // (what a killed run left)
        tempPaths.push_back(info.path);
        FILE* out = fopen(info.path.c_str(), "wb");
        if (!out) throw PrepareException("Could not create " + info.path);
        struct Closer {
            FILE*& f;
            ~Closer() {
                if (f) fclose(f);
            }
        } closer{out};
        deflateToFile(ctx.c, head, out, info.path);
        writeAll(out, res.members, (size_t)res.member_bytes, info.path);
        writeAll(out, BGZF_EOF_BLOCK, sizeof BGZF_EOF_BLOCK, info.path);
        FILE* f = out;
        out = nullptr;
        if (fclose(f) != 0) throw PrepareException("Could not write to " + info.path);
        pjb_memory m;
        memset(&m, 0, sizeof m);
        (void)pjb_memory_info(ctx.c, &m);
        info.peakHeld = m.peak_held;
        runs.push_back(info);
        open = false;
        runIn = runRecords = 0;
    };
    walkPieces(bamFile, H, (size_t)std::min<int64_t>(runBytes, (int64_t)1 << 40), [&](const uint8_t* region, size_t bytes, int64_t fileOffset, int32_t uoff, bool last, uint64_t& nvFile) {
        if (open && runRecords > 0 && runIn + (int64_t)bytes > runBytes) closeRun();  // (these blocks would take the run past its size)
        for (;;) {
            if (!open) {
                check(pjb_bam_sort_begin(ctx.c), "pjb_bam_sort_begin");
                open = true;
            }
            uint64_t nv = ~0ull;
            int64_t n = 0;
            const int rc = pjb_bam_sort_piece(ctx.c, region, (int64_t)bytes, uoff, last ? 1 : 0, &nv, &n);
            if (rc == PJB_ERR_NOMEM) {  // the device is full: what the run holds is sorted and written, the piece goes to a fresh run
                if (runRecords == 0)
                    throw PrepareException("prep --sort: a piece of " + std::to_string(bytes) + " compressed bytes does not fit the device memory this run may hold (" +
                                           pjb_last_error(ctx.c) + ").  Set PORTCULLIS_PIECE_MB to a smaller piece, or sort the file elsewhere (samtools sort).");
                closeRun();
                continue;
            }
            if (rc == PJB_ERR_ARG && nv != ~0ull && !last) return false;  // the first record is longer than these blocks
            check(rc, "pjb_bam_sort_piece");
            runRecords += n;
            runIn += (int64_t)(nv >> 16);
            nvFile = (uint64_t)(fileOffset + (int64_t)(nv >> 16)) << 16 | (nv & 0xffff);
            if (runIn >= runBytes && !last) closeRun();
            return true;
        }
    });
    if (open || runs.empty()) {
        if (!open) check(pjb_bam_sort_begin(ctx.c), "pjb_bam_sort_begin");  // (a header and nothing else)
        open = true;
        closeRun();
    }
    return runs;
}

// the size of a run of `prep --sort`, in compressed bytes of input.  The default, 1 GB, inflates to 2 - 5 GB of records; with the sorted
// stream, 36 to 44 bytes a record for the sort and the deflate's scratch a run holds a few times that, far below the device's 288 GB
// (measured, profiles/prep_sort.json: a run of 1.07 GB, 10 M records, 2.1 GB inflated, held 8.3 GB at the most).
int64_t sortRunBytes() {
    if (const char* e = getenv("PORTCULLIS_SORT_RUN_BYTES"))
        if (atoll(e) > 0) return (int64_t)atoll(e);
    return (int64_t)1 << 30;
}

}  // namespace

// --sort: `bamFile` (found unsorted) as a list of coordinate-sorted files in the prepared directory, in input order; whoever owns
// `tempPaths` removes them.  (`first`: the number of the first run file, so that several inputs' runs do not meet.)
static std::vector<string> sortedRunsOf(const string& bamFile, const string& prepDir, size_t first, bool verbose, std::vector<string>& tempPaths) {
    const double t0 = nowSeconds();
    cout << "Sorting " << bamFile << " on the GPU ... ";
    cout.flush();
    BamHead H = readBamHead(bamFile);
    string text;
    try {
        text = mergeBamHeaders({BamHeaderInfo{bamFile, std::move(H.text), std::move(H.names), std::move(H.lens)}});  // (@HD ... SO:coordinate)
    } catch (const MergeHeaderException& e) {
        throw PrepareException(e.what());
    }
    const std::vector<SortRunInfo> runs =
        sortBamToRuns(bamFile, text, sortRunBytes(), [&](size_t k) { return prepDir + "/sortrun" + std::to_string(first + k) + ".bam"; }, tempPaths);
    cout << "done." << endl;
    std::vector<string> paths;
    int64_t records = 0, unplaced = 0;
    uint64_t peak = 0;
    for (const SortRunInfo& r : runs) {
        paths.push_back(r.path);
        records += r.records;
        unplaced += r.unplaced;
        peak = std::max(peak, r.peakHeld);
        if (verbose)
            cout << " - sort run " << paths.size() << ": " << r.records << " alignment records, " << r.unplaced << " of them unplaced, from " << r.compressedIn
                 << " compressed bytes" << (r.wasSorted ? " (in order already)" : "") << endl;
    }
    if (verbose)
        cout << " - sorted: " << records << " alignment records, " << unplaced << " of them unplaced, in " << runs.size() << (runs.size() == 1 ? " run" : " runs")
             << "; the device held at most " << peak << " bytes" << endl;
    printf(" - BAM Sort - Wall time taken: %.1fs\n\n", nowSeconds() - t0);
    return paths;
}

string Prepare::mergedHeaderText(const std::vector<string>& bamFiles) {
    std::vector<BamHeaderInfo> heads;
    for (const string& f : bamFiles) {
        BamHead H = readBamHead(f);
        heads.push_back(BamHeaderInfo{f, std::move(H.text), std::move(H.names), std::move(H.lens)});
    }
    try {
        return mergeBamHeaders(heads);
    } catch (const MergeHeaderException& e) {
        throw PrepareException(e.what());
    }
}

void Prepare::mergeBams(const std::vector<string>& bamFiles, const string& headerText) {
    const string sorted = output.getSortedBamFilePath();
    if (lexists(sorted)) {
        cout << "Pre-merged BAM detected: " << sorted << endl;
        return;
    }
    if (pjb_device_count() <= 0)
        throw PrepareException("No MI355X (HIP device) is visible: the BAM files are merged on the GPU and there is no CPU fallback.  Merge them elsewhere (samtools "
                               "merge) and pass the one coordinate-sorted file, or run prep where the GPU is.");
    const double t0 = nowSeconds();
    cout << "Merging " << bamFiles.size() << " BAM files on the GPU ... ";
    cout.flush();
    const size_t nFiles = bamFiles.size();
    Unlinker temps;
    // where each input's targets lie: the index beside it if there is one (trusted, as prep trusts one today), else one built on the device;
    // either way it is found beside a link to the input, under the reference's temp names
    std::vector<std::unique_ptr<bam::BamReader>> readers;
    for (size_t k = 0; k < nFiles; k++) {
        const string ext = buildCsi ? ".csi" : ".bai";
        const string link = output.getPrepDir() + "/temp" + std::to_string(k) + ".bam", bai = link + ext;
        char real[PATH_MAX];
        if (!realpath(bamFiles[k].c_str(), real)) throw PrepareException("Could not resolve BAM file: " + bamFiles[k]);
        unlink(link.c_str());  // (what a killed run left)
        unlink(bai.c_str());
        temps.paths.push_back(link);
        temps.paths.push_back(bai);
        if (symlink(real, link.c_str()) != 0) throw PrepareException("Could not create symlink from " + bamFiles[k] + " to " + link);
        if (fileExists(bamFiles[k] + ext)) {
            char realBai[PATH_MAX];
            if (!realpath((bamFiles[k] + ext).c_str(), realBai) || symlink(realBai, bai.c_str()) != 0)
                throw PrepareException("Could not create symlink from " + bamFiles[k] + ext + " to " + bai);
        } else
            writeIndex(buildIndex(bamFiles[k], true, buildCsi), bai);
        readers.emplace_back(new bam::BamReader(link));
        try {
            readers.back()->open(buildCsi);
        } catch (const std::exception& e) {
            throw PrepareException("Could not open " + bamFiles[k] + " with its index: " + e.what());
        }
    }
    const std::vector<bam::RefSeq>& targets = readers[0]->getTargets();
    std::vector<int32_t> lens;
    for (const bam::RefSeq& t : targets) lens.push_back(t.length);

    DeviceCtx ctx;
    auto check = [&](int rc, const char* what) {
        if (rc != PJB_OK) throw PrepareException(string(what) + ": " + pjb_last_error(ctx.c));
    };
    check(pjb_set_refs(ctx.c, (int32_t)lens.size(), lens.data()), "pjb_set_refs");

    const string tmp = sorted + ".tmp";
    temps.paths.push_back(tmp);  // (renamed away when all went well: the unlink then finds nothing)
    FILE* out = fopen(tmp.c_str(), "wb");
    if (!out) throw PrepareException("Could not create " + tmp);
    struct Closer {
        FILE*& f;
        ~Closer() {
            if (f) fclose(f);
        }
    } closer{out};
    const int32_t BLOCK = BGZF_CUT;
    auto deflateToFile = [&](const std::vector<uint8_t>& raw) { portcullis::deflateToFile(ctx.c, raw, out, tmp); };
    {  // the header
        std::vector<string> names;
        for (const bam::RefSeq& t : targets) names.push_back(t.name);
        deflateToFile(bamHeaderBytes(headerText, names, lens));
    }
    // target by target, in index order: what the device holds at a time is one target's records of all files
    std::vector<int64_t> perFile(nFiles, 0), unplacedPerFile(nFiles, 0);
    int64_t written = 0;
    for (size_t t = 0; t < targets.size(); t++) {
        std::vector<size_t> with;
        for (size_t k = 0; k < nFiles; k++)
            if (readers[k]->hasAlignments((int32_t)t)) with.push_back(k);
        if (with.empty()) continue;
        check(pjb_bam_merge_begin(ctx.c, (int32_t)t, (int32_t)nFiles), "pjb_bam_merge_begin");
        size_t targetBytes = 0;
        auto tooLarge = [&](int rc) {  // (no windowing inside a target: one that does not fit ends the run)
            if (rc != PJB_ERR_NOMEM) return;
            pjb_memory m;
            memset(&m, 0, sizeof m);
            (void)pjb_memory_info(ctx.c, &m);
            throw PrepareException("prep --merge: target " + targets[t].name + " does not fit the device memory this run may hold: its records of all files have to be there at "
                                   "once (" + std::to_string(targetBytes) + " compressed bytes; " + pjb_last_error(ctx.c) + "; held " + std::to_string(m.held) + ", limit " +
                                   (m.limit ? std::to_string(m.limit) + " bytes" : string("none: the device is full")) + ").  Merge the files elsewhere (samtools merge).");
        };
        for (size_t k : with) {
            uint64_t fileOff = 0;
            size_t bytes = 0;
            uint32_t firstU = 0;
            if (!readers[k]->regionSpan((int32_t)t, fileOff, bytes, firstU)) continue;
            // The span ends with the block in which the next target's first record begins.  If only a few bytes of that record lie in
            // it the device cannot tell whose it is: the block behind goes along (the device stops at the first foreign record).
            bytes += followingBlock(bamFiles[k], fileOff + bytes);
            uint8_t* buf = (uint8_t*)bam::bigAlloc(bytes);
            if (!buf) throw PrepareException("Out of memory reading " + bamFiles[k]);
            struct Free {
                uint8_t* p;
                ~Free() { bam::bigFree(p); }
            } fr{buf};
            readers[k]->readSpan(fileOff, bytes, buf, threads);
            targetBytes += bytes;
            int64_t n = 0;
            const int rc = pjb_bam_merge_file(ctx.c, (int32_t)k, buf, (int64_t)bytes, (int32_t)firstU, &n);
            tooLarge(rc);
            if (rc == PJB_ERR_UNSORTED)
                throw PrepareException(unsortedMessage(pjb_last_error(ctx.c), bamFiles[k], true));
            if (rc != PJB_OK) throw PrepareException("pjb_bam_merge_file (" + bamFiles[k] + "): " + pjb_last_error(ctx.c));
            perFile[k] += n;
        }
        pjb_bam_merge_result res;
        const int rc = pjb_bam_merge_end(ctx.c, BLOCK, &res);
        tooLarge(rc);
        check(rc, "pjb_bam_merge_end");
        writeAll(out, res.members, (size_t)res.member_bytes, tmp);
        written += res.n_records;
    }
    // the unplaced records behind each file's last placed one, file by file: carried over (bamfilt copies them, as the reference's does)
    const size_t PIECE = (size_t)64 << 20;
    for (size_t k = 0; k < nFiles; k++) {
        std::vector<uint8_t> raw, rec;
        readers[k]->seekUnplacedTail();
        while (readers[k]->nextRecord(rec)) {
            const int32_t refID = (int32_t)((uint32_t)rec[4] | (uint32_t)rec[5] << 8 | (uint32_t)rec[6] << 16 | (uint32_t)rec[7] << 24);
            if (refID >= 0)
                throw PrepareException("A placed alignment record follows the last one the index of " + bamFiles[k] + " names: the index does not belong to the file");
            raw.insert(raw.end(), rec.begin(), rec.end());
            unplacedPerFile[k]++;
            if (raw.size() >= PIECE) {  // (a multiple of the block size per piece would save a short member; records do not care)
                deflateToFile(raw);
                raw.clear();
            }
        }
        deflateToFile(raw);
    }
    writeAll(out, BGZF_EOF_BLOCK, sizeof BGZF_EOF_BLOCK, tmp);
    FILE* f = out;
    out = nullptr;
    if (fclose(f) != 0) throw PrepareException("Could not write to " + tmp);
    if (rename(tmp.c_str(), sorted.c_str()) != 0) throw PrepareException("Could not write merged BAM file: " + sorted);
    cout << "done." << endl << "Merged BAM file created at: " << sorted << endl;
    if (verbose) {
        int64_t unplaced = 0;
        for (size_t k = 0; k < nFiles; k++) {
            cout << " - " << bamFiles[k] << ": " << perFile[k] << " placed alignment records, " << unplacedPerFile[k] << " unplaced" << endl;
            unplaced += unplacedPerFile[k];
        }
        cout << " - written: " << written + unplaced << " alignment records, " << unplaced << " of them unplaced" << endl;
    }
    printf(" - BAM Merge - Wall time taken: %.1fs\n\n", nowSeconds() - t0);
}

void Prepare::prepare(const std::vector<string>& bamFiles, const string& genomeFile) {
    if (useCsi && !buildCsi)
        throw PrepareException("Writing CSI indexes is not built into portcullis_amd prep.  Build the directory without --use_csi (a BAI index covers targets "
                               "below 2^29 bases), or put a CSI index made with `samtools index -c` beside the BAM file and link the files by hand, or pass "
                               "--build_csi: prep then builds the CSI index on the GPU.");
    useCsi = buildCsi;  // (every index path below is the CSI's with --build_csi)
    const string indexExt = buildCsi ? ".csi" : ".bai";
    if (bamFiles.empty()) throw PrepareException("No BAM files to process");
    if (bamFiles.size() > 1 && !merge)
        throw PrepareException("More than one BAM file was given, and merging is not built into portcullis_amd prep.  Merge them first (samtools merge) and "
                               "pass the one coordinate-sorted file.");
    for (const string& b : bamFiles)
        if (!fileExists(b)) throw PrepareException("Could not find BAM file at: " + b);
    // --merge with several files: what their headers refuse is refused before a file is written or a device opened
    const bool merging = bamFiles.size() > 1;
    const string mergedText = merging ? mergedHeaderText(bamFiles) : string();
    if (force) {
        cout << "Cleaning output dir " << output.getPrepDir() << " ... ";
        cout.flush();
        clean();
        cout << "done." << endl;
    }
    if (!copy(genomeFile, output.getGenomeFilePath(), "genome", true)) throw PrepareException("Could not copy/symlink genome file to: " + output.getGenomeFilePath());
    copy(genomeFile + ".fai", output.getGenomeIndexFilePath(), "genome index", false);
    if (!genomeIndex()) throw PrepareException("Could not create genome index");
    Unlinker sortRuns;  // --sort: the sorted runs of unsorted inputs, gone however this ends
    if (merging) {
        // --sort --merge: every input found unsorted gives way, in its place, to its sorted run or runs (the reference's tempN.bam).  An index
        // beside an input is trusted, as everywhere; an input without one is probed by building its index
        std::vector<string> inputs;
        for (const string& b : bamFiles) {
            bool unsorted = false;
            if (sort && !lexists(output.getSortedBamFilePath()) && !fileExists(b + indexExt)) {
                try {
                    (void)buildIndex(b, true, buildCsi);
                } catch (const UnsortedBam&) {
                    unsorted = true;
                }
            }
            if (!unsorted) inputs.push_back(b);
            else
                for (const string& run : sortedRunsOf(b, output.getPrepDir(), sortRuns.paths.size(), verbose, sortRuns.paths)) inputs.push_back(run);
        }
        // the result is a regular file under the sorted BAM's name; its index is then built like any input's (a second inflate of the output)
        mergeBams(inputs, mergedText);
        if (!bamIndex(false)) throw PrepareException("Failed to index: " + output.getSortedBamFilePath());
        return;
    }
    const string sorted = output.getSortedBamFilePath();
    const bool bamWasThere = lexists(sorted);
    if (!copy(bamFiles[0], sorted, "BAM", true)) throw PrepareException("Could not copy/symlink BAM file to: " + sorted);
    // the index beside the input if there is one (src/prepare.cc:316), else it is built (no device is touched before this point)
    const bool indexCopied = copy(bamFiles[0] + indexExt, output.getBamIndexFilePath(buildCsi), "BAM index", false);
    try {
        if (!bamIndex(indexCopied)) throw PrepareException("Failed to index: " + sorted);
    } catch (const UnsortedBam&) {
        struct stat st;
        if (!sort || (bamWasThere && lstat(sorted.c_str(), &st) == 0 && !S_ISLNK(st.st_mode))) throw;  // (a file someone put there is not replaced)
        // --sort: the index build found the file unsorted.  What was linked or copied under the sorted file's name goes, and the sorted
        // file takes its place: the one run renamed, or the merge of several
        cout << "not in coordinate order." << endl;
        unlink(sorted.c_str());
        sortBam(bamFiles[0], sortRuns.paths);
        if (!bamIndex(false)) throw PrepareException("Failed to index: " + sorted);
    }
}

void Prepare::sortBam(const string& bamFile, std::vector<string>& tempPaths) {
    const string sorted = output.getSortedBamFilePath();
    const std::vector<string> runs = sortedRunsOf(bamFile, output.getPrepDir(), 0, verbose, tempPaths);
    if (runs.size() == 1) {
        if (rename(runs[0].c_str(), sorted.c_str()) != 0) throw PrepareException("Could not write sorted BAM file: " + sorted);
        cout << "Sorted BAM file created at: " << sorted << endl;
        return;
    }
    // several runs: each is a sorted file, and run order is input order, so the merge's tie rule (the earlier file first) keeps the sort
    // stable as a whole.  The merge indexes the runs on the device, as any input without an index.
    mergeBams(runs, mergedHeaderText({runs[0]}));
}

int Prepare::main(int argc, char* argv[]) {
    std::vector<string> positional;
    string outputDir = DEFAULT_PREP_OUTPUT_DIR;
    bool force = false, copy = false, useCsi = false, buildCsi = false, verbose = false, help = false, merge = false, sort = false;
    int threads = DEFAULT_PREP_THREADS;
    auto need = [&](int& i) -> string {
        if (i + 1 >= argc) throw PrepareException(string("Missing value for option ") + argv[i]);
        return argv[++i];
    };
    for (int i = 1; i < argc; i++) {
        const string a = argv[i];
        if (a == "-o" || a == "--output") outputDir = need(i);
        else if (a == "--force") force = true;
        else if (a == "--copy") copy = true;
        else if (a == "--merge") merge = true;
        else if (a == "--sort") sort = true;
        else if (a == "-c" || a == "--use_csi") useCsi = true;
        else if (a == "-C" || a == "--build_csi") buildCsi = true;
        else if (a == "-t" || a == "--threads") threads = atoi(need(i).c_str());
        else if (a == "-v" || a == "--verbose") verbose = true;
        else if (a == "--help" || a == "-h") help = true;
        else if (!a.empty() && a[0] == '-') throw PrepareException("Unknown option: " + a);
        else positional.push_back(a);
    }
    if (help || positional.size() < 2) {
        cout << title() << endl << endl << description() << endl << endl << "Usage: " << usage() << endl
             << "  -o, --output <dir>   Output directory for prepared files (default " << DEFAULT_PREP_OUTPUT_DIR << ")" << endl
             << "      --force          Clean the output directory first, so that everything is prepared again" << endl
             << "      --copy           Copy the input files into the output directory instead of linking them" << endl
             << "      --merge          Several coordinate-sorted BAM files may follow the genome: they are merged into one on the GPU" << endl
             << "                       (ties in position go to the file given first; without the flag a second BAM file is refused)" << endl
             << "      --sort           A BAM file that is not in coordinate order is sorted on the GPU (stable by target and position;" << endl
             << "                       unplaced records last; without the flag such a file is refused).  A sorted file is left as it is" << endl
             << "  -c, --use_csi        CSI instead of BAI indexing (refused without --build_csi; with it, the same as --build_csi)" << endl
             << "  -C, --build_csi      Every index prep builds is a CSI (<bam>.csi, no .bai), built on the GPU: min_shift 14 and the depth" << endl
             << "                       htslib chooses.  It also covers targets of 2^29 bases or more, which a BAI cannot.  A .csi beside" << endl
             << "                       the input is linked or copied instead.  Run junc with --use_csi on the result" << endl
             << "  -t, --threads <n>    Threads that read the BAM files for --merge and for the runs of --sort (index and sort run on the GPU)" << endl
             << "  -v, --verbose        Print extra information" << endl
             << "      --help           Produce this message" << endl;
        return help ? 0 : 1;
    }
    const string genomeFile = positional[0];
    const std::vector<string> bamFiles(positional.begin() + 1, positional.end());
    if (!lexists(genomeFile)) throw PrepareException("Could not find genome file at: " + genomeFile);
    const double t0 = nowSeconds();
    cout << "Running portcullis in prepare mode" << endl << "----------------------------------" << endl << endl;
    Prepare prep(outputDir);
    prep.setForce(force);
    prep.setUseLinks(!copy);
    prep.setUseCsi(useCsi);
    prep.setBuildCsi(buildCsi);
    prep.setMerge(merge);
    prep.setSort(sort);
    prep.setThreads((uint16_t)std::max(1, threads));
    prep.setVerbose(verbose);
    prep.prepare(bamFiles, genomeFile);
    prep.getOutput().valid(buildCsi);
    printf("\nPortcullis prep completed.\nTotal runtime: %.1fs\n\n", nowSeconds() - t0);
    return 0;
}

}  // namespace portcullis
