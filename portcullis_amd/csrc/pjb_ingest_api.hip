// pjb_ingest_api.hip -- the part of the C ABI that takes file bytes: BGZF inflate / deflate on the device, BAM record boundaries and transcoding
// (pjb_inflate_bgzf, pjb_deflate_bgzf, pjb_submit_bam, pjb_bam_begin / _piece / _end here; pjb_index_* in pjb_index_api.hip.h, pjb_bam_merge_* in
// pjb_merge_api.hip.h, pjb_bam_sort_* in pjb_sort_api.hip.h, host code included below, behind the drivers they share); kernels in pjb_ingest.hip.h,
// pjb_deflate.hip.h, pjb_index.hip.h and pjb_merge.hip.h.
#include "pjb_host.hip.h"
#include "pjb_deflate.hip.h"
#include "pjb_ingest.hip.h"
#include "pjb_index.hip.h"
#include "pjb_merge.hip.h"

void ingest_kernel_attributes() { (void)hipFuncSetAttribute((const void *)bgzf_decode, hipFuncAttributeMaxDynamicSharedMemorySize, I3_LDS_BYTES); }
int ingest_lds_bytes() { return I3_LDS_BYTES; }


// ---- device-side ingest ---------------------------------------------------------------------------
// Each step has one driver, whoever asks: bgzf_header (a block header through a byte reader: scan_bgzf over a buffer, stage_scan over
// pieces), inflate_queue (one inflate launch on a stream: inflate_on_device waits for it, inflate_early does not), walk_records (record
// boundaries of a target's region or, `all`, of an indexer's piece), upload_host (host bytes to the device), upload_padded + inflate_into
// (the piece prologue: a call's BGZF bytes up, padded, and inflated into the buffer the caller names), piece_records (every complete
// record of a piece: the index and the sort), write_members (ordered records -> BGZF members: the merge and the sort), op_leave (what a
// failing call of a piece-wise operation leaves).
const char *inf_text(int code) {
    switch (code) {
    case INF_ERR_BTYPE: return "reserved DEFLATE block type";
    case INF_ERR_STORED: return "stored block length check failed";
    case INF_ERR_CODELENS: return "invalid code length set";
    case INF_ERR_CODE: return "invalid Huffman code";
    case INF_ERR_DIST: return "match distance before the start of the block";
    case INF_ERR_OVERRUN: return "block inflates or reads past its declared size";
    case INF_ERR_SIZE: return "block inflates to fewer bytes than its ISIZE";
    default: return "bad block";
    }
}

// One BGZF block header (bgzf.c:348-356 check_header, BSIZE from the BC extra subfield).  `at(o)` reads byte o of the stream, the block
// starts at `off`, the bytes before `end` have arrived, the stream ends at `total`.  PJB_OK: `b` (but for out_off) and `bsize` are set;
// BGZF_SHORT_*: that part of the block has not all arrived; else the error.
enum { BGZF_SHORT_HEADER = 1, BGZF_SHORT_EXTRA, BGZF_SHORT_FOOTER };
template <typename At>
static int bgzf_header(pjb_ctx *c, At at, int64_t off, int64_t end, int64_t total, InfBlock &b, int64_t &bsize) {
    auto le16 = [&](int64_t o) { return (uint32_t)at(o) | (uint32_t)at(o + 1) << 8; };
    if (off + 18 > end) return BGZF_SHORT_HEADER;
    if (at(off) != 31 || at(off + 1) != 139 || at(off + 2) != 8 || !(at(off + 3) & 4))
        return fail(c, PJB_ERR_BGZF, "not a BGZF block header at byte %lld", (long long)off);
    const uint32_t xlen = le16(off + 10);
    if (off + 12 + xlen > end) return BGZF_SHORT_EXTRA;
    bsize = -1;
    for (uint32_t x = 0; x + 4 <= xlen;) {
        const int64_t f = off + 12 + x;
        const uint32_t slen = le16(f + 2);
        if (at(f) == 'B' && at(f + 1) == 'C' && slen == 2 && x + 6 <= xlen) bsize = (int64_t)le16(f + 4) + 1;
        x += 4 + slen;
    }
    if (bsize < 0) return fail(c, PJB_ERR_BGZF, "BGZF block at byte %lld has no BC field", (long long)off);
    if (bsize < (int64_t)xlen + 20 || off + bsize > total)
        return fail(c, PJB_ERR_BGZF, "BGZF block at byte %lld has an impossible size %lld", (long long)off, (long long)bsize);
    if (off + bsize > end) return BGZF_SHORT_FOOTER;
    const uint32_t isize = le16(off + bsize - 4) | le16(off + bsize - 2) << 16;
    if (isize > 65536u) return fail(c, PJB_ERR_BGZF, "BGZF block at byte %lld declares %u inflated bytes", (long long)off, isize);
    b.in_off = (iu64)(off + 12 + xlen);
    b.in_len = (iu32)(bsize - xlen - 20);
    b.out_len = isize;
    return PJB_OK;
}

// hop over the BGZF block headers of a whole buffer
int scan_bgzf(pjb_ctx *c, const uint8_t *comp, int64_t n, std::vector<InfBlock> &blocks, int64_t &total_out) {
    total_out = 0;
    for (int64_t off = 0, bsize = 0; off < n; off += bsize) {
        InfBlock b;
        const int rc = bgzf_header(c, [&](int64_t o) { return comp[o]; }, off, n, n, b, bsize);
        if (rc > 0) return fail(c, PJB_ERR_BGZF, rc == BGZF_SHORT_HEADER ? "truncated BGZF block header at byte %lld" : "truncated BGZF extra field at byte %lld", (long long)off);
        if (rc) return rc;
        b.out_off = (iu64)total_out;
        blocks.push_back(b);
        total_out += b.out_len;
    }
    return PJB_OK;
}

// pageable host memory -> device through the two page-locked staging buffers: a few threads memcpy a
// piece into one buffer while the DMA engine drains the other
int upload_staged(pjb_ctx *c, void *dst, const uint8_t *src, size_t bytes) {
    const size_t PIECE = (size_t)64 << 20;
    for (size_t off = 0; off < bytes; off += PIECE) {
        const size_t nb = std::min(PIECE, bytes - off);
        const unsigned si = c->stage_next++ & 1u;
        if (c->stage_busy[si]) {
            HIP_TRY(c, hipEventSynchronize(c->stage_ev[si]));
            c->stage_busy[si] = false;
        }
        if (c->stage_cap[si] < nb) {
            if (c->stage[si]) (void)hipHostFree(c->stage[si]);
            c->stage[si] = nullptr;
            c->stage_cap[si] = 0;
            if (hipHostMalloc((void **)&c->stage[si], PIECE, hipHostMallocDefault) != hipSuccess)
                return fail(c, PJB_ERR_NOMEM, "cannot allocate %zu bytes of page-locked staging memory", PIECE);
            c->stage_cap[si] = PIECE;
        }
        if (!c->stage_ev[si]) HIP_TRY(c, hipEventCreateWithFlags(&c->stage_ev[si], hipEventDisableTiming));
        parallel_copy(c->stage[si], src + off, nb);
        HIP_TRY(c, hipMemcpyAsync((uint8_t *)dst + off, c->stage[si], nb, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(c->stage_ev[si], c->stream));
        c->stage_busy[si] = true;
    }
    return PJB_OK;
}

// host memory -> device on the main stream: page-locked input (pjb_host_alloc) is one DMA without a staging copy
int upload_host(pjb_ctx *c, void *dst, const uint8_t *src, size_t bytes) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, src) == hipSuccess && at.type == hipMemoryTypeHost) {
        HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
        return PJB_OK;
    }
    (void)hipGetLastError();
    return upload_staged(c, dst, src, bytes);
}

// the status words of a finished bgzf_inflate (d_status[nb] = "some block failed")
int inflate_status(pjb_ctx *c, const std::vector<InfBlock> &blocks, const int *d_status) {
    const size_t nb = blocks.size();
    int any = 0;
    HIP_TRY(c, hipMemcpy(&any, d_status + nb, 4, hipMemcpyDeviceToHost));
    if (!any) return PJB_OK;
    std::vector<int> status(nb);
    HIP_TRY(c, hipMemcpy(status.data(), d_status, nb * 4, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < nb; b++)
        if (status[b])
            return fail(c, PJB_ERR_BGZF, "BGZF block %zu (payload at byte %llu): %s", b, (unsigned long long)blocks[b].in_off, inf_text(status[b]));
    return fail(c, PJB_ERR_BGZF, "BGZF inflate failed");
}

// One launch inflates a list of blocks: as many lanes as the chip holds at once (two 64-lane workgroups per CU: the tables' LDS), each
// taking block after block from a counter.
static size_t inflate_lanes(pjb_ctx *c, size_t nb) {
    size_t lanes = (size_t)c->inflate_lanes;
    if (const char *e = getenv("PJB_INF_BLOCKS_PER_LAUNCH")) lanes = (size_t)std::max(64, atoi(e)) / 64 * 64; // tests: few lanes, long lists
    return std::min<size_t>((nb + 63) / 64 * 64, lanes);
}

// Queues the inflate of `blocks` (d_comp: their bytes, padded) on `st`: the block table and the control words go up (`ctl` must live
// until that copy is over), then decode (lane per block: literals in place, a token + a bitmap bit per match) and the copies (wave per
// block).  Waits for nothing and fails nothing: the caller decides what an error means.  Buffers for nb blocks: InfBlock[nb] | int[nb]
// status, "some block failed", the block counter | INF_SCRATCH_PER_LANE per lane | INF_BITMAP_WORDS u64 per block.
static hipError_t inflate_queue(pjb_ctx *c, hipStream_t st, const uint8_t *d_comp, const std::vector<InfBlock> &blocks, size_t lanes, iu32 *ctl,
                                const Buf &b_blocks, const Buf &b_status, const Buf &b_scratch, const Buf &b_bitmap, uint8_t *d_out) {
    const size_t nb = blocks.size();
    int *d_status = (int *)b_status.p;
    int *d_any = d_status + nb;
    iu32 *d_next = (iu32 *)(d_any + 1);
    ctl[0] = 0u;
    ctl[1] = (iu32)lanes;
    hipError_t e;
    if ((e = hipMemcpyAsync(b_blocks.p, blocks.data(), nb * sizeof(InfBlock), hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemcpyAsync(d_any, ctl, 8, hipMemcpyHostToDevice, st)) != hipSuccess ||
        (e = hipMemsetAsync(b_bitmap.p, 0, nb * INF_BITMAP_WORDS * 8, st)) != hipSuccess)
        return e;
    const bool t_dec = st == c->stream && ktime_wanted(c, "bgzf_decode"), t_res = st == c->stream && ktime_wanted(c, "bgzf_resolve");
    if (t_dec) ev_begin(c, "bgzf_decode");
    hipLaunchKernelGGL(bgzf_decode, dim3((unsigned)(lanes / 64)), dim3(64), I3_LDS_BYTES, st, d_comp, (const InfBlock *)b_blocks.p, (iu32)nb, d_out,
                       (uint8_t *)b_scratch.p, d_status, d_any, d_next, (iu64 *)b_bitmap.p, 8);
    if (t_dec) ev_end(c);
    if (t_res) ev_begin(c, "bgzf_resolve");
    hipLaunchKernelGGL(bgzf_resolve, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st, (const InfBlock *)b_blocks.p, (iu32)nb, d_out,
                       (const iu64 *)b_bitmap.p, (const int *)d_status);
    if (t_res) ev_end(c);
    return hipGetLastError();
}

// comp already on the device (padded); blocks on the host
int inflate_on_device(pjb_ctx *c, const uint8_t *d_comp, const std::vector<InfBlock> &blocks, uint8_t *d_out) {
    int rc;
    const size_t nb = blocks.size();
    if (nb == 0) return PJB_OK;
    const size_t lanes = inflate_lanes(c, nb);
    if ((rc = ensure(c, c->b_inf_blocks, nb * sizeof(InfBlock))) || (rc = ensure(c, c->b_inf_status, nb * 4 + 16)) ||
        (rc = ensure(c, c->b_inf_scratch, lanes * INF_SCRATCH_PER_LANE)) || (rc = ensure(c, c->b_inf_bitmap, nb * INF_BITMAP_WORDS * 8)))
        return rc;
    iu32 ctl[2];
    HIP_TRY(c, inflate_queue(c, c->stream, d_comp, blocks, lanes, ctl, c->b_inf_blocks, c->b_inf_status, c->b_inf_scratch, c->b_inf_bitmap, d_out));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->ktime) ev_collect(c, MISC_POOL);
    return inflate_status(c, blocks, (const int *)c->b_inf_status.p);
}

extern "C" int pjb_inflate_bgzf(pjb_ctx *c, const uint8_t *comp, int64_t comp_bytes, uint8_t *out, int64_t out_cap,
                                int64_t *out_bytes) {
    if (!c || !out_bytes || comp_bytes < 0 || (comp_bytes && !comp)) return fail(c, PJB_ERR_ARG, "inflate_bgzf: bad arguments");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    std::vector<InfBlock> blocks;
    int64_t total = 0;
    int rc = scan_bgzf(c, comp, comp_bytes, blocks, total);
    if (rc) return rc;
    *out_bytes = total;
    if (total > out_cap) return fail(c, PJB_ERR_ARG, "inflate_bgzf: output needs %lld bytes, capacity is %lld", (long long)total, (long long)out_cap);
    if (blocks.empty()) return PJB_OK;
    if (total && !out) return fail(c, PJB_ERR_ARG, "inflate_bgzf: no output buffer"); // (blocks of ISIZE 0 are decoded too: their streams must be valid)
    if ((rc = ensure(c, c->b_inf_comp, (size_t)comp_bytes + INF_PAD))) return rc;
    if ((rc = ensure(c, c->b_inf_out, (size_t)total + 64))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->b_inf_comp.p, comp, (size_t)comp_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync((uint8_t *)c->b_inf_comp.p + comp_bytes, 0, INF_PAD, c->stream));
    if ((rc = inflate_on_device(c, (const uint8_t *)c->b_inf_comp.p, blocks, (uint8_t *)c->b_inf_out.p))) return rc;
    if (total) HIP_TRY(c, hipMemcpy(out, c->b_inf_out.p, (size_t)total, hipMemcpyDeviceToHost));
    return PJB_OK;
}

// BGZF deflate on the device (pjb_deflate.hip.h): at most DFL_LAUNCH_BLOCKS blocks per launch (1 GB of symbol scratch)
constexpr int64_t DFL_LAUNCH_BLOCKS = 4096;
// The launches of one deflate, whoever asks (pjb_deflate_bgzf: `host_in`, copied to b_dfl_in launch by launch; write_members: `dev_in`,
// a stream that lies on the device already).  `n_bytes` are cut every `block_bytes`; for every launch `sink(b0, sizes, total, dst)` is
// told the first block's number, the members' sizes and their sum, and says where in host memory the packed members go.
template <typename Sink>
static int deflate_launches(pjb_ctx *c, const uint8_t *host_in, const uint8_t *dev_in, int64_t n_bytes, int32_t block_bytes, Sink sink) {
    hipStream_t st = c->stream;
    const int64_t n_blocks = (n_bytes + block_bytes - 1) / block_bytes;
    int rc;
    std::vector<u32> sizes;
    std::vector<iu64> offs;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += DFL_LAUNCH_BLOCKS) {
        const int64_t nb = std::min<int64_t>(DFL_LAUNCH_BLOCKS, n_blocks - b0);
        const int64_t in_off = b0 * block_bytes, in_len = std::min<int64_t>(n_bytes - in_off, nb * block_bytes);
        if ((host_in && (rc = ensure(c, c->b_dfl_in, (size_t)in_len + 64))) || (rc = ensure(c, c->b_dfl_sym, (size_t)nb * DFL_SYM_STRIDE * 4)) ||
            (rc = ensure(c, c->b_dfl_slots, (size_t)nb * DFL_SLOT)) || (rc = ensure(c, c->b_dfl_size, (size_t)nb * 4)) ||
            (rc = ensure(c, c->b_dfl_off, (size_t)nb * 8)))
            return rc;
        if (host_in) HIP_TRY(c, hipMemcpyAsync(c->b_dfl_in.p, host_in + in_off, (size_t)in_len, hipMemcpyHostToDevice, st));
        const uint8_t *d_in = host_in ? (const uint8_t *)c->b_dfl_in.p : dev_in + in_off;
        LAUNCH(c, "bgzf_deflate", bgzf_deflate, dim3((unsigned)nb), dim3(64), d_in, (iu64)in_len, (u32)block_bytes, (u32)nb,
               (u32 *)c->b_dfl_sym.p, (uint8_t *)c->b_dfl_slots.p, (u32 *)c->b_dfl_size.p);
        sizes.resize((size_t)nb);
        HIP_TRY(c, hipMemcpyAsync(sizes.data(), c->b_dfl_size.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        offs.resize((size_t)nb);
        iu64 total = 0;
        for (int64_t k = 0; k < nb; k++) {
            if (sizes[(size_t)k] < 26 || sizes[(size_t)k] > 65536) return fail(c, PJB_ERR_STATE, "deflate_bgzf: block %lld came out with %u bytes", (long long)(b0 + k), sizes[(size_t)k]);
            offs[(size_t)k] = total;
            total += sizes[(size_t)k];
        }
        uint8_t *dst = nullptr;
        if ((rc = sink(b0, sizes, total, dst))) return rc;
        if ((rc = ensure(c, c->b_dfl_packed, (size_t)total + 64))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->b_dfl_off.p, offs.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));
        LAUNCH(c, "bgzf_pack", bgzf_pack, dim3((unsigned)nb), dim3(256), (const uint8_t *)c->b_dfl_slots.p, (const u32 *)c->b_dfl_size.p,
               (const iu64 *)c->b_dfl_off.p, (u32)nb, (uint8_t *)c->b_dfl_packed.p);
        HIP_TRY(c, hipMemcpyAsync(dst, c->b_dfl_packed.p, (size_t)total, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    if (c->ktime) ev_collect(c, MISC_POOL);
    return PJB_OK;
}

extern "C" int pjb_deflate_bgzf(pjb_ctx *c, const uint8_t *in, int64_t n_bytes, int32_t block_bytes, uint8_t *out, int64_t out_cap, int64_t *out_bytes,
                                uint32_t *member_size) {
    if (!c || !out_bytes || n_bytes < 0 || (n_bytes && (!in || !out))) return fail(c, PJB_ERR_ARG, "deflate_bgzf: bad arguments");
    if (block_bytes < 4 || block_bytes > (int32_t)DFL_IN_MAX || (block_bytes & 3))
        return fail(c, PJB_ERR_ARG, "deflate_bgzf: block_bytes must be a multiple of 4 between 4 and %u", DFL_IN_MAX);
    *out_bytes = 0;
    if (n_bytes == 0) return PJB_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int64_t written = 0;
    const int rc = deflate_launches(c, in, nullptr, n_bytes, block_bytes, [&](int64_t b0, const std::vector<u32> &sizes, iu64 total, uint8_t *&dst) {
        if (member_size)
            for (size_t k = 0; k < sizes.size(); k++) member_size[(size_t)b0 + k] = sizes[k];
        if (written + (int64_t)total > out_cap) return fail(c, PJB_ERR_ARG, "deflate_bgzf: the output needs more than %lld bytes", (long long)out_cap);
        dst = out + written;
        written += (int64_t)total;
        return (int)PJB_OK;
    });
    if (rc) return rc;
    *out_bytes = written;
    return PJB_OK;
}

// ---- record boundaries ------------------------------------------------------------------------------------------
// `total` inflated bytes at U whose first record starts at `first`; tid -1: no target's in particular (the indexer)
static BamRegion bam_region(pjb_ctx *c, const uint8_t *U, int64_t total, int32_t first, int32_t tid) {
    BamRegion R;
    R.U = U;
    R.total = (iu64)total;
    R.first = (iu64)first;
    R.tid = tid;
    R.ref_len = tid < 0 ? 0 : c->ref_len[(size_t)tid];
    R.n_ref = (int32_t)c->ref_len.size();
    return R;
}

// What a walk over the inflated bytes R found.  The records' offsets are in b_bam_rec.
struct RecordWalk {
    size_t n = 0;                   // records
    uint32_t end_seg = 0xffffffffu; // the segment in which the target ended (a record of another target, or past the target's end)
    uint32_t cut_seg = 0xffffffffu; // the first segment whose walk met a record the data ends in
    iu64 next_u = 0;                // all: the first byte that belongs to no complete record (R.total: the data ends on a record's end)
};

// The one driver of the record kernels (pjb_ingest.hip.h): a start guessed per 64 KB segment, the walks from start to start counted and
// verified (a start that a verified walk contradicts is replaced by the boundary that walk reached, at most 16 times), the segments behind
// the stop trimmed, the counts scanned, the offsets filled in.  `all`: the indexer's walk -- records of every target, up to the record
// the data ends in; else the records of target R.tid, up to the first record that is not the target's.  `where` places the errors.
static int walk_records(pjb_ctx *c, const BamRegion &R, bool all, const char *where, RecordWalk &w) {
    hipStream_t st = c->stream;
    int rc;
    const uint32_t NONE = 0xffffffffu;
    const uint32_t n_seg = (uint32_t)((R.total + BAM_SEG - 1) / BAM_SEG);
    const dim3 seg_grid((n_seg + 255) / 256), seg_block(256);
    // seg_start u64 | seg_base u64 | land u64 | seg_n u32
    if ((rc = ensure(c, c->b_bam_seg, (size_t)n_seg * 28 + 64)) || (rc = ensure(c, c->b_bam_ctl, 64))) return rc;
    iu64 *seg_start = (iu64 *)c->b_bam_seg.p;
    iu64 *seg_base = seg_start + n_seg;
    iu64 *land = seg_base + n_seg;
    iu32 *seg_n = (iu32 *)(land + n_seg);
    // [0] the target ended, [1] mismatch, [2] bad segment, [3] repair failed, [4..5] u64 total of the scan, [6] the data ends in a record
    iu32 *ctl = (iu32 *)c->b_bam_ctl.p;
    iu64 *d_total = (iu64 *)(ctl + 4);
    BamWalkOut O;
    O.seg_n = seg_n;
    O.land = land;
    O.rec_off = nullptr;
    O.seg_base = seg_base;
    O.ctl = ctl;
    LAUNCH(c, "bam_find_starts", bam_find_starts, dim3(n_seg), dim3(64), R, n_seg, seg_start);
    if (const char *e = getenv("PJB_TEST_FALSE_START")) { // test hook: damage the guessed start of one segment
        const uint32_t k = (uint32_t)atoi(e);
        if (k > 0 && k < n_seg) {
            iu64 v = 0;
            HIP_TRY(c, hipMemcpyAsync(&v, seg_start + k, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            if (v != BAM_NONE) {
                v += 1;
                HIP_TRY(c, hipMemcpyAsync(seg_start + k, &v, 8, hipMemcpyHostToDevice, st));
                HIP_TRY(c, hipStreamSynchronize(st));
            }
        }
    }
    uint32_t h_ctl[8];
    uint32_t stop = NONE; // the segment behind which nothing counts
    for (int attempt = 0;; attempt++) {
        HIP_TRY(c, hipMemsetAsync(ctl, 0xff, 32, st));
        if (all) LAUNCH(c, "bam_walk_all_count", bam_walk_all<false>, seg_grid, seg_block, R, n_seg, (const iu64 *)seg_start, O);
        else LAUNCH(c, "bam_walk_count", bam_walk<false>, seg_grid, seg_block, R, n_seg, (const iu64 *)seg_start, O);
        HIP_TRY(c, hipMemcpyAsync(h_ctl, ctl, 32, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        stop = h_ctl[all ? 6 : 0];
        if (h_ctl[2] != NONE && h_ctl[2] <= stop && (h_ctl[1] == NONE || h_ctl[2] <= h_ctl[1]))
            return fail(c, PJB_ERR_BGZF, "Invalid BAM record layout %s (inflated offset %llu..)", where, (unsigned long long)h_ctl[2] * BAM_SEG);
        if (h_ctl[1] == NONE || h_ctl[1] > stop) break; // every walk up to the stop landed on the next start
        // a guessed start was not a record boundary: replace it by the boundary the verified walk reached, walk again
        if (attempt >= 16)
            return fail(c, PJB_ERR_BGZF, "BAM record chain %s is inconsistent near inflated offset %llu", where, (unsigned long long)h_ctl[1] * BAM_SEG);
        LAUNCH(c, "bam_repair_start", bam_repair_start, dim3(1), dim3(1), seg_start, n_seg, h_ctl[1], (const iu64 *)land, R.total, ctl);
        HIP_TRY(c, hipMemcpyAsync(h_ctl, ctl, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (h_ctl[3] != NONE) return fail(c, PJB_ERR_BGZF, "Invalid BAM record %s (inflated offset %llu..)", where, (unsigned long long)h_ctl[3] * BAM_SEG);
    }
    w.end_seg = h_ctl[0];
    w.cut_seg = h_ctl[6];
    w.next_u = R.total;
    if (stop != NONE) {
        // what the segments behind the stop found are not records: they lie inside the cut record, or are not the target's
        if (all) HIP_TRY(c, hipMemcpyAsync(ctl, &stop, 4, hipMemcpyHostToDevice, st)); // (bam_trim_segments reads ctl[0])
        LAUNCH(c, "bam_trim_segments", bam_trim_segments, seg_grid, seg_block, seg_n, n_seg, (const iu32 *)ctl);
        if (all) HIP_TRY(c, hipMemcpyAsync(&w.next_u, land + stop, 8, hipMemcpyDeviceToHost, st));
    }
    if ((rc = run_scan(c, "bam_seg", SegCountFn{seg_n}, SegBaseSink{seg_base}, n_seg, d_total))) return rc;
    iu64 n64 = 0;
    HIP_TRY(c, hipMemcpyAsync(&n64, d_total, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    w.n = (size_t)n64;
    if (n64 == 0 || n64 >= 0xffffff00ull) return PJB_OK; // (more than the callers take: nothing to fill)
    if ((rc = ensure(c, c->b_bam_rec, w.n * 8))) return rc;
    O.rec_off = (iu64 *)c->b_bam_rec.p;
    if (all) LAUNCH(c, "bam_walk_all_fill", bam_walk_all<true>, seg_grid, seg_block, R, n_seg, (const iu64 *)seg_start, O);
    else LAUNCH(c, "bam_walk_fill", bam_walk<true>, seg_grid, seg_block, R, n_seg, (const iu64 *)seg_start, O);
    return PJB_OK;
}

// ---- what the calls that take BGZF bytes share --------------------------------------------------------------------
// The piece prologue in two halves (pjb_submit_bam times them apart): a call's BGZF bytes to b_inf_comp, INF_PAD zeroed bytes behind them;
// then `blocks` of d_comp inflated into `out` -- b_inf_out or a Buf of the caller's, grown under the category the caller names -- with 64
// zeroed bytes behind the `total` inflated ones.
static int upload_padded(pjb_ctx *c, const uint8_t *comp, int64_t comp_bytes) {
    int rc;
    if ((rc = ensure(c, c->b_inf_comp, (size_t)comp_bytes + INF_PAD)) || (rc = upload_host(c, c->b_inf_comp.p, comp, (size_t)comp_bytes))) return rc;
    HIP_TRY(c, hipMemsetAsync((uint8_t *)c->b_inf_comp.p + comp_bytes, 0, INF_PAD, c->stream));
    return PJB_OK;
}
static int inflate_into(pjb_ctx *c, const uint8_t *d_comp, const std::vector<InfBlock> &blocks, int64_t total, Buf &out, MemCat cat) {
    if (const int rc = ensure_cat(c, out, (size_t)total + 64, cat)) return rc;
    HIP_TRY(c, hipMemsetAsync((uint8_t *)out.p + total, 0, 64, c->stream));
    return inflate_on_device(c, d_comp, blocks, (uint8_t *)out.p);
}

// Every complete record of a piece, of whatever target (pjb_index_piece, pjb_bam_sort_piece): the blocks' layout, the inflated bytes in
// `out`, the records' offsets in b_bam_rec, and how the piece ended -- PIECE_TAKEN: records up to next_u (`total`: the data ends on a
// record's end; less: the rest starts the next piece); PIECE_CUT_AT_EOF: the last piece ends inside a record; PIECE_RECORD_TOO_LONG: the
// first record is longer than the piece, nothing was taken.  The callers word what a cut means, each with its own offsets.
enum PieceEnd { PIECE_TAKEN, PIECE_CUT_AT_EOF, PIECE_RECORD_TOO_LONG };
struct PieceRecords {
    std::vector<InfBlock> blocks;
    int64_t total = 0; // inflated bytes
    size_t n = 0;      // records
    iu64 next_u = 0;   // the first byte that belongs to no complete record
    PieceEnd end = PIECE_TAKEN;
};
// `who` heads the refusals; `held` records are the caller's already, and `too_many` refuses more than the ordinals hold
static int piece_records(pjb_ctx *c, const char *who, const uint8_t *comp, int64_t comp_bytes, int32_t first_uoffset, int32_t last, Buf &out, MemCat cat, size_t held,
                         const char *too_many, PieceRecords &P) {
    int rc = scan_bgzf(c, comp, comp_bytes, P.blocks, P.total);
    if (rc) return rc;
    if ((int64_t)first_uoffset > P.total) return fail(c, PJB_ERR_ARG, "%s: first_uoffset %d lies behind the piece's %lld inflated bytes", who, first_uoffset, (long long)P.total);
    P.next_u = (iu64)first_uoffset;
    if ((int64_t)first_uoffset < P.total) {
        if ((rc = upload_padded(c, comp, comp_bytes)) || (rc = inflate_into(c, (const uint8_t *)c->b_inf_comp.p, P.blocks, P.total, out, cat))) return rc;
        RecordWalk w;
        if ((rc = walk_records(c, bam_region(c, (const uint8_t *)out.p, P.total, first_uoffset, -1), true, "in the piece", w))) return rc;
        if (w.n >= 0xffffff00ull || held + w.n >= 0xffffff00ull) return fail(c, PJB_ERR_ARG, "%s", too_many);
        P.n = w.n;
        P.next_u = w.next_u;
    }
    if (P.next_u < (iu64)P.total) P.end = last ? PIECE_CUT_AT_EOF : P.n == 0 ? PIECE_RECORD_TOO_LONG : PIECE_TAKEN;
    return PJB_OK;
}

// What a piece-wise operation's state (IndexState, MergeState, SortRun) starts with, and what a failing call leaves of it: nothing to go
// on with -- begin again -- unless the call set keep_on_error or, `spare_nomem`, ran out of device memory (the call can be repeated).
struct PieceOp {
    bool active = false;
    bool keep_on_error = false; // the failing call left the operation as it was
};
static int op_leave(pjb_ctx *c, PieceOp *s, int rc, bool spare_nomem) {
    if (rc && !(spare_nomem && rc == PJB_ERR_NOMEM) && !s->keep_on_error) {
        (void)hipStreamSynchronize(c->stream);
        s->active = false;
    }
    return rc;
}
template <typename State>
static void op_clear(pjb_ctx *c, State *&s) { // (pjb_destroy: every state releases its own buffers)
    if (s) s->release_all(c);
    delete s;
    s = nullptr;
}

// Ordered records as BGZF members (pjb_bam_merge_end, pjb_bam_sort_end): what the writer holds on the device and the result on the host.
struct MemberWriter {
    Buf dst, stream;                // every record's offset in the stream | the stream, 64 bytes of slack behind it
    std::vector<uint32_t> r_size;   // the result: the members' sizes
    std::vector<uint8_t> r_members; // and the members back to back
    void release_all(pjb_ctx *c) { release(c, dst), release(c, stream); } // (a device buffer added above is added here)
    void clear_result() { r_size.clear(), r_members.clear(); }
    static int check_block_bytes(pjb_ctx *c, const char *who, int32_t block_bytes) {
        if (block_bytes >= 4 && block_bytes <= (int32_t)DFL_IN_MAX && !(block_bytes & 3)) return PJB_OK;
        return fail(c, PJB_ERR_ARG, "%s: block_bytes must be a multiple of 4 between 4 and %u", who, DFL_IN_MAX);
    }
    template <typename Result>
    void result_to(Result *out) const { // (pjb_bam_merge_result, pjb_bam_sort_result)
        out->n_members = (int32_t)r_size.size();
        out->member_size = r_size.data();
        out->members = r_members.data();
        out->member_bytes = (int64_t)r_members.size();
    }
};
// Records i = 0 .. n - 1 of `size[i]` bytes at `src[i]`, taken in `order` (null: as they are), gathered into one stream and deflated in
// members of `block_bytes`: the scan (timed as `scan_label`, its total in `d_total`) places them, mg_gather copies them.
static int write_members(pjb_ctx *c, MemberWriter &w, const iu32 *size, const iu64 *src, const iu32 *order, size_t n, const char *scan_label, u64 *d_total,
                         int32_t block_bytes, int64_t *raw_bytes) {
    hipStream_t st = c->stream;
    int rc;
    if ((rc = ensure(c, w.dst, n * 8))) return rc;
    if ((rc = run_scan(c, scan_label, MgSizeFn{size, order}, MgOffsetSink{(iu64 *)w.dst.p}, n, d_total))) return rc;
    iu64 raw = 0;
    HIP_TRY(c, hipMemcpyAsync(&raw, d_total, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if ((rc = ensure_cat(c, w.stream, (size_t)raw + 64, MEM_STAGING))) return rc;
    LAUNCH(c, "mg_gather", mg_gather, dim3((unsigned)((n + 3) / 4)), dim3(256), src, size, order, (const iu64 *)w.dst.p, (iu64)n, (uint8_t *)w.stream.p);
    rc = deflate_launches(c, nullptr, (const uint8_t *)w.stream.p, (int64_t)raw, block_bytes, [&](int64_t, const std::vector<u32> &sizes, iu64 total, uint8_t *&dst) {
        const size_t had = w.r_members.size();
        w.r_size.insert(w.r_size.end(), sizes.begin(), sizes.end());
        w.r_members.resize(had + (size_t)total);
        dst = w.r_members.data() + had;
        return (int)PJB_OK;
    });
    if (rc) w.clear_result();
    else *raw_bytes = (int64_t)raw;
    return rc;
}

// the inflated bytes of one target's region (d_out, `total` of them followed by 64 zero bytes) -> the SoA batch of the target
static int ingest_parse(pjb_ctx *c, int32_t tid, OpenContig &oc, const uint8_t *d_out, size_t n_blocks, int64_t comp_bytes, int64_t total,
                        int32_t first_uoffset, int64_t *n_records, double t_scan, double t_up, double t_inf) {
    const bool prof = getenv("PJB_PROFILE_HOST") != nullptr;
    double t0 = wall_now(), t_walk;
    hipStream_t st = c->stream;
    int rc;
    const BamRegion R = bam_region(c, d_out, total, first_uoffset, tid);
    RecordWalk w;
    if ((rc = walk_records(c, R, false, ("on target " + std::to_string(tid)).c_str(), w))) return rc;
    // The data ends inside a record of this target and no record of another target (or past the target's end) was seen:
    // the bytes handed over stop short of the target's last alignment (a stale index, a truncated file).  The reference
    // fails on a truncated file too (bgzf_read / bam_read1); dropping the tail silently would change counts.
    if (w.end_seg == 0xffffffffu && w.cut_seg != 0xffffffffu)
        return fail(c, PJB_ERR_BGZF, "the data for target %d ends inside an alignment record (inflated offset %llu..): truncated "
                                     "file, or the index's span for the target is too short", tid, (unsigned long long)w.cut_seg * BAM_SEG);
    t_walk = wall_now() - t0;
    t0 = wall_now();
    if (w.n == 0) return PJB_OK;
    if (w.n >= 0xffffff00ull) return fail(c, PJB_ERR_ARG, "submit_bam: more than 2^32 alignments on one target are not supported");
    const size_t n = w.n;
    iu64 *d_total = (iu64 *)((iu32 *)c->b_bam_ctl.p + 4); // (the scans' total)

    // ---- SoA arrays in the target's slabs (same packing as a host-submitted batch)
    // (150-base paired-end records: fields + operations + 4- and 2-bit bases of the spliced third are 0.28 of the inflated bytes)
    if (oc.slabs.empty()) oc.slab_hint = (((size_t)total / 100 * 32) + ((size_t)32 << 20)) & ~(((size_t)1 << 20) - 1);
    const size_t fixed[8] = {n * 4, n * 2, n, n, n * 4, n * 4, n * 4, (n + 1) * 4}; // pos flag mapq xs l_qseq mtid mpos cig_off
    size_t offs[9], tot_b = 0;
    for (int k = 0; k < 8; k++) {
        offs[k] = tot_b;
        tot_b += (std::max<size_t>(fixed[k], 16) + 255) & ~(size_t)255;
    }
    offs[8] = tot_b; // seq_off
    tot_b += (((n + 1) * 4) + 255) & ~(size_t)255;
    uint8_t *dev = (uint8_t *)slab_alloc(c, oc, tot_b);
    if (!dev) return nomem(c, "submit_bam: the alignments' fields", tot_b);
    BamSoA B;
    B.pos = (int32_t *)(dev + offs[0]);
    B.flag = (uint16_t *)(dev + offs[1]);
    B.mapq = dev + offs[2];
    B.xs = dev + offs[3];
    B.l_qseq = (int32_t *)(dev + offs[4]);
    B.mtid = (int32_t *)(dev + offs[5]);
    B.mpos = (int32_t *)(dev + offs[6]);
    B.cig_off = (iu32 *)(dev + offs[7]);
    B.seq_off = (iu32 *)(dev + offs[8]);
    B.cigar = nullptr;
    B.seq4 = nullptr;
    B.name_hash = nullptr;
    B.seq2 = nullptr;
    B.seq_exc = nullptr;
    if (c->extra) {
        B.name_hash = (iu64 *)slab_alloc(c, oc, n * 8 + 16);
        if (!B.name_hash) return nomem(c, "submit_bam: name codes", n * 8 + 16);
    }
    if ((rc = run_scan(c, "bam_sizes", BamSizesFn{R.U, (const iu64 *)c->b_bam_rec.p}, BamOffsetsSink{B.cig_off, B.seq_off}, n, d_total)))
        return rc;
    iu64 tot = 0;
    HIP_TRY(c, hipMemcpyAsync(&tot, d_total, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const uint32_t n_ops = (uint32_t)(tot >> 32), n_words = (uint32_t)tot;
    // (a carry out of the low half would mean 2^32 sequence words: 16 GB of bases on one target)
    const uint32_t tails[2] = {n_ops, n_words};
    HIP_TRY(c, hipMemcpyAsync(B.cig_off + n, &tails[0], 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(B.seq_off + n, &tails[1], 4, hipMemcpyHostToDevice, st));
    B.cigar = (iu32 *)slab_alloc(c, oc, (size_t)n_ops * 4 + 16);
    B.seq4 = (uint8_t *)slab_alloc(c, oc, (size_t)n_words * 4 + 16);
    if (!B.cigar || !B.seq4) return nomem(c, "submit_bam: CIGARs / bases", ((size_t)n_ops + n_words) * 4 + 32);
    static const bool no_seq2 = getenv("PJB_NO_SEQ2") && atoi(getenv("PJB_NO_SEQ2")) != 0;
    if (!no_seq2) { // the bases in 2 bits as well (what pjb_batch.seq2 / .seq_exc hold): written where the 4-bit bases are
        B.seq2 = (unsigned short *)slab_alloc(c, oc, ((size_t)n_words + 2) * 2 + 16);
        B.seq_exc = (iu32 *)slab_alloc(c, oc, ((n + 31) / 32) * 4 + 16);
        if (!B.seq2 || !B.seq_exc) return nomem(c, "submit_bam: the 2-bit bases", ((size_t)n_words + 2) * 2 + ((n + 31) / 32) * 4 + 32);
    }
    LAUNCH(c, "bam_transcode", bam_transcode, dim3((unsigned)((n + 255) / 256)), dim3(256), R.U, (const iu64 *)c->b_bam_rec.p, (iu64)n, B);
    HIP_TRY(c, hipStreamSynchronize(st)); // `tails` is on this stack frame
    if (c->ktime) ev_collect(c, MISC_POOL);
    if (prof)
        fprintf(stderr, "[host profile] submit_bam tid %d: %zu blocks, %.1f MB -> %.1f MB, %zu records: header scan %.3f, upload %.3f, inflate %.3f, "
                        "boundaries %.3f, fill+sizes+transcode %.3f s\n",
                tid, n_blocks, comp_bytes / 1e6, total / 1e6, n, t_scan, t_up, t_inf, t_walk, wall_now() - t0);
    DevBatch d;
    memset(&d, 0, sizeof d);
    d.n = (int64_t)n;
    d.base = 0;
    d.pos = B.pos; d.flag = B.flag; d.mapq = B.mapq; d.xs = B.xs; d.l_qseq = B.l_qseq; d.mtid = B.mtid; d.mpos = B.mpos;
    d.cig_off = B.cig_off; d.cigar = B.cigar; d.seq_off = B.seq_off; d.seq4 = B.seq4;
    d.name_hash = (const u64 *)B.name_hash;
    d.seq2 = (const uint32_t *)B.seq2;
    d.seq_exc = B.seq_exc;
    oc.on_main_stream = true;
    oc.batches.push_back(d);
    oc.last_known.push_back(0);
    oc.last_pos.push_back(INT32_MIN);
    if (n_records) *n_records = (int64_t)n;
    return PJB_OK;
}

// the part of pjb_submit_bam behind the upload: `d_comp` holds the target's BGZF bytes (padded), `blocks` their layout
static int ingest_staged(pjb_ctx *c, int32_t tid, OpenContig &oc, const uint8_t *d_comp, const std::vector<InfBlock> &blocks, int64_t comp_bytes,
                         int64_t total, int32_t first_uoffset, int64_t *n_records, double t_scan, double t_up) {
    const double t0 = wall_now();
    const int rc = inflate_into(c, d_comp, blocks, total, c->b_inf_out, MEM_SCRATCH);
    if (rc) return rc;
    return ingest_parse(c, tid, oc, (const uint8_t *)c->b_inf_out.p, blocks.size(), comp_bytes, total, first_uoffset, n_records, t_scan, t_up, wall_now() - t0);
}

static int submit_bam_body(pjb_ctx *c, int32_t tid, OpenContig &oc, const uint8_t *comp, int64_t comp_bytes, int32_t first_uoffset, int64_t *n_records);

extern "C" int pjb_submit_bam(pjb_ctx *c, int32_t tid, const uint8_t *comp, int64_t comp_bytes, int32_t first_uoffset,
                              int64_t *n_records) {
    if (!c) return PJB_ERR_ARG;
    if (n_records) *n_records = 0;
    if (comp_bytes < 0 || (comp_bytes && !comp) || first_uoffset < 0) return fail(c, PJB_ERR_ARG, "submit_bam: bad arguments");
    if (tid < 0 || (size_t)tid >= c->ref_len.size()) return fail(c, PJB_ERR_ARG, "submit_bam: bad tid %d", tid);
    c->cur_tid = tid;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    OpenContig &oc = c->open[tid];
    if (!oc.batches.empty()) return fail(c, PJB_ERR_STATE, "submit_bam: target %d already has batches (one call per target)", tid);
    const SlabMark mark = slab_mark(c, oc);
    const int rc = submit_bam_body(c, tid, oc, comp, comp_bytes, first_uoffset, n_records);
    if (rc == PJB_ERR_NOMEM) slab_rollback(c, oc, mark); // (retryable: the target is as it was)
    return rc;
}

static int submit_bam_body(pjb_ctx *c, int32_t tid, OpenContig &oc, const uint8_t *comp, int64_t comp_bytes, int32_t first_uoffset, int64_t *n_records) {
    const bool prof = getenv("PJB_PROFILE_HOST") != nullptr;
    double t0 = wall_now(), t_scan, t_up;
    std::vector<InfBlock> blocks;
    int64_t total = 0;
    int rc = scan_bgzf(c, comp, comp_bytes, blocks, total);
    if (rc) return rc;
    if (total == 0 || (int64_t)first_uoffset >= total) return PJB_OK;
    t_scan = wall_now() - t0;
    t0 = wall_now();
    if ((rc = upload_padded(c, comp, comp_bytes))) return rc;
    if (prof) (void)hipStreamSynchronize(c->stream);
    t_up = wall_now() - t0;
    return ingest_staged(c, tid, oc, (const uint8_t *)c->b_inf_comp.p, blocks, comp_bytes, total, first_uoffset, n_records, t_scan, t_up);
}

// ---- the same in pieces -----------------------------------------------------------------------------------------
// (pjb_bam_begin / pjb_bam_piece / pjb_bam_pieces_done / pjb_bam_end, see the header)
struct BamStage {
    Buf dev;                 // the target's BGZF bytes on the device (from the context's pool)
    int64_t total = 0, got = 0;
    std::vector<InfBlock> blocks;
    int64_t total_out = 0;
    int64_t next = 0;        // file-relative offset of the next block header to look at
    uint8_t keep[65536 + 64]; // bytes [keep_at, got) of what arrived, for a block whose header or footer straddles two pieces
    int64_t keep_at = 0, keep_n = 0;
    double t_scan = 0, t_up = 0;
    // the inflate launched at the last piece (launched: ev_inf follows the kernel on its stream)
    bool launched = false;
    iu32 ctl[2] = {0, 0}; // { "some block failed", lanes }: copied to the device asynchronously, so it lives here and not on a stack
    Buf out, d_blocks, d_status, d_scratch, d_bitmap;
    hipEvent_t ev_inf = nullptr, ev_last = nullptr;
};

// a buffer of at least `bytes` from a pool (the smallest that fits), else a new one
static int pool_take(pjb_ctx *c, std::vector<Buf> &pool, Buf &b, size_t bytes) {
    int best = -1;
    for (size_t k = 0; k < pool.size(); k++)
        if (pool[k].cap >= bytes && (best < 0 || pool[k].cap < pool[(size_t)best].cap)) best = (int)k;
    if (best >= 0) {
        b = pool[(size_t)best];
        pool.erase(pool.begin() + best);
        std::lock_guard<std::mutex> lk(c->mem.mu);
        c->mem.pooled_stage -= std::min(b.cap, c->mem.pooled_stage);
        return PJB_OK;
    }
    return ensure_cat(c, b, bytes, MEM_STAGING);
}
static void pool_give(pjb_ctx *c, std::vector<Buf> &pool, Buf &b) {
    if (b.p) {
        pool.push_back(b);
        std::lock_guard<std::mutex> lk(c->mem.mu);
        c->mem.pooled_stage += b.cap;
    }
    b.p = nullptr;
    b.cap = 0;
}
static void stage_release(pjb_ctx *c, BamStage &st) { // (after the work that uses the buffers has completed)
    pool_give(c, c->stage_pool, st.dev);
    pool_give(c, c->out_pool, st.out);
    pool_give(c, c->misc_pool, st.d_blocks);
    pool_give(c, c->misc_pool, st.d_status);
    pool_give(c, c->misc_pool, st.d_scratch);
    pool_give(c, c->out_pool, st.d_bitmap); // (output-sized: an eighth of the inflated bytes)
    if (st.ev_inf) (void)hipEventDestroy(st.ev_inf);
    if (st.ev_last) (void)hipEventDestroy(st.ev_last);
    st.ev_inf = st.ev_last = nullptr;
}

// every byte of the target has been queued for copying and every block header seen: inflate on a stream of its own, behind
// the last copy.  Nothing here waits; a failure just leaves the inflate to pjb_bam_end.
static void inflate_early(pjb_ctx *c, BamStage &st) {
    const size_t nb = st.blocks.size();
    if (st.launched || nb == 0 || st.total_out <= 0) return;
    const size_t lanes = inflate_lanes(c, nb);
    if (pool_take(c, c->out_pool, st.out, (size_t)st.total_out + 64) || pool_take(c, c->misc_pool, st.d_blocks, nb * sizeof(InfBlock)) ||
        pool_take(c, c->misc_pool, st.d_status, nb * 4 + 16) || pool_take(c, c->misc_pool, st.d_scratch, lanes * INF_SCRATCH_PER_LANE) ||
        pool_take(c, c->out_pool, st.d_bitmap, nb * INF_BITMAP_WORDS * 8)) {
        std::lock_guard<std::mutex> lk(c->err_mu); // (a failure here just leaves the inflate to pjb_bam_end)
        c->err.clear();
        return;
    }
    hipStream_t &is = c->inf_streams[c->inf_next++ & 3u];
    if (!is) {
        // The inflate streams have the lowest priority: a launch holds every LDS byte of the chip for ~50 ms, and the short
        // kernels beside it -- record parsing, genome uploads, the junc chains of the targets before it -- are what the one
        // host thread that serves all targets waits for (end to end 2.73 -> 2.44 s)
        int lo = 0, hi = 0; // (least, greatest priority)
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (hipStreamCreateWithPriority(&is, hipStreamNonBlocking, lo) != hipSuccess) return;
    }
    if (hipEventCreateWithFlags(&st.ev_last, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&st.ev_inf, hipEventDisableTiming) != hipSuccess) return;
    const bool ok = hipEventRecord(st.ev_last, c->stream_up) == hipSuccess && hipStreamWaitEvent(is, st.ev_last, 0) == hipSuccess &&
                    hipMemsetAsync((uint8_t *)st.out.p + st.total_out, 0, 64, is) == hipSuccess &&
                    inflate_queue(c, is, (const uint8_t *)st.dev.p, st.blocks, lanes, st.ctl, st.d_blocks, st.d_status, st.d_scratch, st.d_bitmap,
                                  (uint8_t *)st.out.p) == hipSuccess &&
                    hipEventRecord(st.ev_inf, is) == hipSuccess;
    if (!ok) { // whatever was queued must be over before the buffers are used again
        (void)hipStreamSynchronize(is);
        (void)hipGetLastError();
        return;
    }
    st.launched = true;
}

// block headers that are complete with the bytes received so far (the last `avail` bytes of the stream are at `p`, the
// first of them is byte `p_at` of the target's bytes); leaves st.next at the first block it cannot finish yet
static int stage_scan(pjb_ctx *c, BamStage &st, const uint8_t *p, int64_t p_at, int64_t avail) {
    // what lies before this piece is in the kept tail, which ends where the piece begins
    if (st.next < p_at && (st.next < st.keep_at || st.keep_at + st.keep_n != p_at))
        return fail(c, PJB_ERR_STATE, "bam_piece: internal: header byte %lld out of reach", (long long)st.next);
    auto byte_at = [&](int64_t off) { return off >= p_at ? p[off - p_at] : st.keep[off - st.keep_at]; };
    while (st.next < st.total) {
        InfBlock b;
        int64_t bsize = 0;
        const int rc = bgzf_header(c, byte_at, st.next, p_at + avail, st.total, b, bsize);
        if (rc > 0) break; // the rest of it has not arrived
        if (rc) return rc;
        b.out_off = (iu64)st.total_out;
        st.blocks.push_back(b);
        st.total_out += b.out_len;
        st.next += bsize;
    }
    return PJB_OK;
}

extern "C" int pjb_bam_begin(pjb_ctx *c, int32_t tid, int64_t total_bytes) {
    if (!c) return PJB_ERR_ARG;
    if (tid < 0 || (size_t)tid >= c->ref_len.size() || total_bytes <= 0) return fail(c, PJB_ERR_ARG, "bam_begin: bad arguments (tid %d)", tid);
    BamLock lk(c);
    if (c->bam_stage.count(tid)) return fail(c, PJB_ERR_STATE, "bam_begin: target %d is being staged already", tid);
    // (that the target has no batches yet is checked by pjb_bam_end, on the thread that owns the open targets)
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    std::unique_ptr<BamStage> st(new (std::nothrow) BamStage());
    if (!st) return fail(c, PJB_ERR_NOMEM, "bam_begin: out of host memory");
    int rc = pool_take(c, c->stage_pool, st->dev, (size_t)total_bytes + INF_PAD);
    if (rc) return rc;
    st->total = total_bytes;
    hipError_t he = hipSuccess;
    if (!c->stream_up) he = hipStreamCreateWithFlags(&c->stream_up, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipMemsetAsync((uint8_t *)st->dev.p + total_bytes, 0, INF_PAD, c->stream_up);
    if (he != hipSuccess) {
        pool_give(c, c->stage_pool, st->dev);
        return fail(c, PJB_ERR_HIP, "bam_begin: %s", hipGetErrorString(he));
    }
    c->bam_stage[tid] = st.release();
    return PJB_OK;
}

static int bam_piece_body(pjb_ctx *c, int32_t tid, BamStage &st, const uint8_t *piece, int64_t bytes, int64_t *ticket);

extern "C" int pjb_bam_piece(pjb_ctx *c, int32_t tid, const uint8_t *piece, int64_t bytes, int64_t *ticket) {
    if (!c || !piece || bytes <= 0) return fail(c, PJB_ERR_ARG, "bam_piece: bad arguments");
    BamLock lk(c);
    auto it = c->bam_stage.find(tid);
    if (it == c->bam_stage.end()) return fail(c, PJB_ERR_STATE, "bam_piece: target %d was not begun (pjb_bam_begin)", tid);
    const int rc = bam_piece_body(c, tid, *it->second, piece, bytes, ticket);
    if (rc) { // the target's staging is dropped: it has to be begun again
        (void)hipStreamSynchronize(c->stream_up);
        for (auto &is : c->inf_streams)
            if (is) (void)hipStreamSynchronize(is);
        stage_release(c, *it->second);
        delete it->second;
        c->bam_stage.erase(it);
    }
    return rc;
}

static int bam_piece_body(pjb_ctx *c, int32_t tid, BamStage &st, const uint8_t *piece, int64_t bytes, int64_t *ticket) {
    if (st.got + bytes > st.total) return fail(c, PJB_ERR_ARG, "bam_piece: target %d: more bytes than announced", tid);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    double t0 = wall_now();
    // the copy first (asynchronous, on the upload stream), the header hop meanwhile
    HIP_TRY(c, hipMemcpyAsync((uint8_t *)st.dev.p + st.got, piece, (size_t)bytes, hipMemcpyHostToDevice, c->stream_up));
    const int64_t tk = ++c->up_ticket;
    hipEvent_t &ev = c->up_events[(size_t)(tk % (int64_t)PJB_UP_EVENTS)];
    if (!ev) HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    else if (tk - c->up_done >= (int64_t)PJB_UP_EVENTS) { // the ring is full: its oldest copy must have completed
        HIP_TRY(c, hipEventSynchronize(ev));
        c->up_done = std::max<int64_t>(c->up_done, tk - (int64_t)PJB_UP_EVENTS);
    }
    HIP_TRY(c, hipEventRecord(ev, c->stream_up));
    st.t_up += wall_now() - t0;
    t0 = wall_now();
    int rc = stage_scan(c, st, piece, st.got, bytes);
    if (rc) return rc;
    st.got += bytes;
    // keep what the next piece's first block may still need: everything from st.next on, if it is short (a block is
    // at most 64 KB), else nothing (the block then starts in a later piece)
    if (st.next < st.got) {
        const int64_t from = st.next;
        const int64_t n = st.got - from;
        if (n > (int64_t)sizeof st.keep) return fail(c, PJB_ERR_BGZF, "BGZF block at byte %lld is longer than 64 KB", (long long)from);
        uint8_t tmp[sizeof st.keep];
        for (int64_t k = 0; k < n; k++) {
            const int64_t off = from + k;
            tmp[k] = off >= st.got - bytes ? piece[off - (st.got - bytes)] : st.keep[off - st.keep_at];
        }
        memcpy(st.keep, tmp, (size_t)n);
        st.keep_at = from;
        st.keep_n = n;
    } else
        st.keep_n = 0;
    st.t_scan += wall_now() - t0;
    if (ticket) *ticket = tk;
    if (st.got == st.total && st.next == st.total) inflate_early(c, st);
    return PJB_OK;
}

extern "C" int pjb_bam_inflate_done(pjb_ctx *c, int32_t tid) {
    if (!c) return 1;
    BamLock lk(c);
    auto it = c->bam_stage.find(tid);
    if (it == c->bam_stage.end() || !it->second->launched) return 1; // (nothing in flight: pjb_bam_end does all the work)
    const bool done = hipEventQuery(it->second->ev_inf) == hipSuccess;
    (void)hipGetLastError();
    return done ? 1 : 0;
}

extern "C" int pjb_bam_pieces_done(pjb_ctx *c, int64_t *completed_ticket) {
    if (!c || !completed_ticket) return PJB_ERR_ARG;
    BamLock lk(c);
    while (c->up_done < c->up_ticket) {
        hipEvent_t ev = c->up_events[(size_t)((c->up_done + 1) % (int64_t)PJB_UP_EVENTS)];
        if (!ev || hipEventQuery(ev) != hipSuccess) break;
        c->up_done++;
    }
    (void)hipGetLastError(); // (hipErrorNotReady is not an error here)
    *completed_ticket = c->up_done;
    return PJB_OK;
}

static int bam_end_body(pjb_ctx *c, int32_t tid, BamStage &stage, int32_t first_uoffset, int64_t *n_records, bool *keep);

extern "C" int pjb_bam_end(pjb_ctx *c, int32_t tid, int32_t first_uoffset, int64_t *n_records) {
    if (!c) return PJB_ERR_ARG;
    if (n_records) *n_records = 0;
    std::unique_ptr<BamStage> st;
    {
        BamLock lk(c);
        auto it = c->bam_stage.find(tid);
        if (it == c->bam_stage.end()) return fail(c, PJB_ERR_STATE, "bam_end: target %d was not begun (pjb_bam_begin)", tid);
        st.reset(it->second);
        c->bam_stage.erase(it);
    }
    struct Return { // the device buffer goes back to the pool whatever happens (after the work that reads it) -- unless the call ran out of
                    // device memory: then the stage is the context's again, pieces and inflate as they are, and the call can be repeated
        pjb_ctx *c;
        std::unique_ptr<BamStage> &st;
        int32_t tid;
        bool keep;
        ~Return() {
            (void)hipStreamSynchronize(c->stream);
            if (st->launched) (void)hipEventSynchronize(st->ev_inf); // (the inflate waited for the target's last copy)
            else if (c->stream_up) (void)hipStreamSynchronize(c->stream_up); // early returns: the copies may still read the caller's buffers
            BamLock lk(c);
            if (keep) c->bam_stage[tid] = st.release();
            else stage_release(c, *st);
        }
    } ret{c, st, tid, false};
    const int rc = bam_end_body(c, tid, *st, first_uoffset, n_records, &ret.keep);
    return rc;
}

// (*keep: the call failed with PJB_ERR_NOMEM behind its argument checks; the target's slabs are as they were)
static int bam_end_body(pjb_ctx *c, int32_t tid, BamStage &stage, int32_t first_uoffset, int64_t *n_records, bool *keep) {
    BamStage *st = &stage;
    c->cur_tid = tid;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (first_uoffset < 0) return fail(c, PJB_ERR_ARG, "bam_end: bad first_uoffset");
    if (st->got != st->total) return fail(c, PJB_ERR_ARG, "bam_end: target %d: %lld of %lld bytes arrived", tid, (long long)st->got, (long long)st->total);
    if (st->next != st->total) return fail(c, PJB_ERR_BGZF, "truncated BGZF block at byte %lld", (long long)st->next);
    OpenContig &oc = c->open[tid];
    if (!oc.batches.empty()) return fail(c, PJB_ERR_STATE, "bam_end: target %d already has batches (one call per target)", tid);
    if (st->total_out == 0 || (int64_t)first_uoffset >= st->total_out) return PJB_OK;
    const SlabMark mark = slab_mark(c, oc);
    int rc;
    if (st->launched) { // the inflate started with the last piece: wait for it, look at its status words, go on with the records
        const double t0 = wall_now();
        HIP_TRY(c, hipEventSynchronize(st->ev_inf));
        rc = inflate_status(c, st->blocks, (const int *)st->d_status.p);
        if (rc) return rc;
        rc = ingest_parse(c, tid, oc, (const uint8_t *)st->out.p, st->blocks.size(), st->total, st->total_out, first_uoffset, n_records, st->t_scan, st->t_up,
                          wall_now() - t0);
    } else {
        // the service stream picks up behind the last copy
        if (!c->ev_up) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->ev_up, c->stream_up));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_up, 0));
        rc = ingest_staged(c, tid, oc, (const uint8_t *)st->dev.p, st->blocks, st->total, st->total_out, first_uoffset, n_records, st->t_scan, st->t_up);
    }
    if (rc == PJB_ERR_NOMEM) { // (retryable: the target and its stage are as they were)
        slab_rollback(c, oc, mark);
        if (n_records) *n_records = 0;
        *keep = true;
    }
    return rc;
}


// ---- prep's operations: a header each, host code over the drivers above ----------------------------------------
#include "pjb_index_api.hip.h" // pjb_index_*: the BAI / CSI of a sorted file
#include "pjb_merge_api.hip.h" // pjb_bam_merge_*: one target of several sorted files
#include "pjb_sort_api.hip.h"  // pjb_bam_sort_*: an unsorted file, run by run

void bam_stage_clear(pjb_ctx *c) {
    op_clear(c, c->index);
    op_clear(c, c->merge);
    op_clear(c, c->sort_run);
    for (auto &is : c->inf_streams)
        if (is) (void)hipStreamSynchronize(is);
    for (auto &kv : c->bam_stage) {
        stage_release(c, *kv.second);
        delete kv.second;
    }
    c->bam_stage.clear();
    release_pooled_stage(c);
    for (auto &is : c->inf_streams)
        if (is) (void)hipStreamDestroy(is);
    for (auto &ev : c->up_events)
        if (ev) (void)hipEventDestroy(ev);
    if (c->ev_up) (void)hipEventDestroy(c->ev_up);
    if (c->stream_up) (void)hipStreamDestroy(c->stream_up);
}
