// pjb_ingest_api.hip -- the part of the C ABI that takes file bytes: BGZF inflate / deflate on the device, BAM record boundaries and transcoding
// (pjb_inflate_bgzf, pjb_deflate_bgzf, pjb_submit_bam, pjb_bam_*, pjb_index_*, pjb_bam_merge_*, pjb_bam_sort_*); kernels in pjb_ingest.hip.h, pjb_deflate.hip.h,
// pjb_index.hip.h and pjb_merge.hip.h.
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
// boundaries of a target's region or, `all`, of an indexer's piece), upload_host (host bytes to the device).
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
// The launches of one deflate, whoever asks (pjb_deflate_bgzf: `host_in`, copied to b_dfl_in launch by launch; pjb_bam_merge_end: `dev_in`,
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
    int rc;
    if ((rc = ensure(c, c->b_inf_out, (size_t)total + 64))) return rc;
    HIP_TRY(c, hipMemsetAsync((uint8_t *)c->b_inf_out.p + total, 0, 64, c->stream));
    if ((rc = inflate_on_device(c, d_comp, blocks, (uint8_t *)c->b_inf_out.p))) return rc;
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
    hipStream_t st = c->stream;
    if ((rc = ensure(c, c->b_inf_comp, (size_t)comp_bytes + INF_PAD))) return rc;
    if ((rc = upload_host(c, c->b_inf_comp.p, comp, (size_t)comp_bytes))) return rc;
    HIP_TRY(c, hipMemsetAsync((uint8_t *)c->b_inf_comp.p + comp_bytes, 0, INF_PAD, st));
    if (prof) (void)hipStreamSynchronize(st);
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

static void index_clear(pjb_ctx *c);
static void merge_clear(pjb_ctx *c);
static void sort_clear(pjb_ctx *c);
void bam_stage_clear(pjb_ctx *c) {
    index_clear(c);
    merge_clear(c);
    sort_clear(c);
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


// ---- the BAM index of a sorted file, piece by piece (pjb_index_begin / _piece / _end, see the header; kernels in pjb_index.hip.h) ---------
struct IndexState {
    bool active = false, saw_last = false;
    bool keep_on_error = false;   // the failing piece call left the index as it was
    int csi_depth = -1;           // < 0: a BAI; 0 .. 6: a CSI of that depth (pjb_index_begin_csi)
    int64_t n_records = 0;
    iu64 prev_sort = 0;           // (refID unsigned) << 32 | pos of the last record seen
    iu64 open_key = BAI_NOKEY;    // (target, bin) of the run the last record belongs to: its chunk is the list's last, its end open
    iu64 win_carry = 0;           // running window maximum
    iu64 end_voffset = 0;         // where the data ended (the last piece)
    size_t n_chunks = 0;
    Buf chunks;                   // BaiChunk[n_chunks], file order
    Buf lin, ref_len, lin_off;    // u64 per window of every target (0: untouched) | i32[n_ref] | u64[n_ref + 1]
    size_t lin_total = 0;
    std::vector<iu64> h_lin_cap;  // lin_off on the host
    Buf key, vs, win, w0, heads, tab, ctl, tile_max; // a piece's scratch
    Buf q[4], tid_start, sorted;  // pjb_index_end (q[3]: the seventh level, a CSI of depth 6)
    Buf loff;                     // pjb_index_end_csi: u64 per ordered chunk
    // the result
    std::vector<pjb_index_chunk> r_chunks;
    std::vector<int64_t> r_lin_off;
    std::vector<uint64_t> r_lin;
    std::vector<uint64_t> r_loff;
};
static_assert(sizeof(BaiChunk) == sizeof(pjb_index_chunk) && sizeof(pjb_index_chunk) == 24, "chunk layout");

static void index_clear(pjb_ctx *c) {
    IndexState *x = c->index;
    if (!x) return;
    for (Buf *b : {&x->chunks, &x->lin, &x->ref_len, &x->lin_off, &x->key, &x->vs, &x->win, &x->w0, &x->heads, &x->tab, &x->ctl, &x->tile_max, &x->q[0], &x->q[1],
                   &x->q[2], &x->q[3], &x->tid_start, &x->sorted, &x->loff})
        release(c, *b);
    delete x;
    c->index = nullptr;
}

extern "C" int pjb_csi_depth(const int32_t *ref_len, int32_t n_ref) {
    int64_t longest = 0;
    for (int32_t t = 0; ref_len && t < n_ref; t++) longest = std::max<int64_t>(longest, ref_len[t]);
    longest += 256; // (htslib's margin, sam.c bam_index_build: the smallest depth whose root bin covers the longest target + 256)
    int depth = 0;
    for (int64_t s = 1ll << CSI_MIN_SHIFT; s < longest; s <<= 3) depth++;
    return depth;
}

static int index_begin_body(pjb_ctx *c, int csi_depth) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (!c->index) c->index = new (std::nothrow) IndexState();
    IndexState *x = c->index;
    if (!x) return fail(c, PJB_ERR_NOMEM, "index_begin: out of host memory");
    x->active = false;
    x->saw_last = false;
    x->csi_depth = csi_depth;
    x->n_records = 0;
    x->prev_sort = 0;
    x->open_key = BAI_NOKEY;
    x->win_carry = 0;
    x->end_voffset = 0;
    x->n_chunks = 0;
    x->r_chunks.clear();
    x->r_lin_off.clear();
    x->r_lin.clear();
    x->r_loff.clear();
    // a window of 16 kb per 2^14 bases of every target reg2bin covers (a record on a longer one is refused when it is met); of
    // every target for a CSI
    const size_t n_ref = c->ref_len.size();
    x->h_lin_cap.assign(n_ref + 1, 0);
    for (size_t t = 0; t < n_ref; t++) {
        const int32_t len = c->ref_len[t];
        x->h_lin_cap[t + 1] = x->h_lin_cap[t] + (len > 0 && (csi_depth >= 0 || len < BAI_MAX_LEN) ? ((iu64)len + 16383) >> 14 : 0);
    }
    x->lin_total = (size_t)x->h_lin_cap[n_ref];
    int rc;
    if ((rc = ensure(c, x->lin, x->lin_total * 8 + 8)) || (rc = ensure(c, x->ref_len, n_ref * 4 + 4)) || (rc = ensure(c, x->lin_off, (n_ref + 1) * 8)) ||
        (rc = ensure(c, x->ctl, BAI_CTL_WORDS * 8)))
        return rc;
    hipStream_t st = c->stream;
    HIP_TRY(c, hipMemsetAsync(x->lin.p, 0, x->lin_total * 8 + 8, st));
    if (n_ref) HIP_TRY(c, hipMemcpyAsync(x->ref_len.p, c->ref_len.data(), n_ref * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(x->lin_off.p, x->h_lin_cap.data(), (n_ref + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    x->active = true;
    return PJB_OK;
}

extern "C" int pjb_index_begin(pjb_ctx *c) {
    if (!c) return PJB_ERR_ARG;
    return index_begin_body(c, -1);
}

extern "C" int pjb_index_begin_csi(pjb_ctx *c, int32_t depth) {
    if (!c) return PJB_ERR_ARG;
    if (c->index) c->index->active = false; // (as pjb_index_begin: an index that was being built is dropped, whatever comes of this call)
    if (depth > CSI_MAX_DEPTH) return fail(c, PJB_ERR_ARG, "index_begin_csi: a depth of %d is not supported (0 .. %d, or a negative one for the smallest that fits)", depth, CSI_MAX_DEPTH);
    if (depth < 0) depth = pjb_csi_depth(c->ref_len.data(), (int32_t)c->ref_len.size());
    if (depth > CSI_MAX_DEPTH) return fail(c, PJB_ERR_ARG, "index_begin_csi: no depth up to %d covers the longest target", CSI_MAX_DEPTH);
    // the BAI's rule (BAI_MAX_LEN) at every depth: a target of 2^(14 + 3 depth) bases or more is not binned.  Depth 0 has the one bin
    // that holds whatever there is.
    for (size_t t = 0; depth > 0 && t < c->ref_len.size(); t++)
        if ((int64_t)c->ref_len[t] >= 1ll << (CSI_MIN_SHIFT + 3 * depth))
            return fail(c, PJB_ERR_ARG, "index_begin_csi: a CSI of depth %d bins targets of less than 2^%d bases, target %zu has %d", depth,
                        CSI_MIN_SHIFT + 3 * depth, t, c->ref_len[t]);
    return index_begin_body(c, depth);
}

// a chunk list that must hold `need` chunks: a larger buffer takes over what the list holds
static int index_grow_chunks(pjb_ctx *c, IndexState *x, size_t need) {
    if (need * sizeof(BaiChunk) <= x->chunks.cap && x->chunks.p) return PJB_OK;
    Buf nb;
    int rc = ensure(c, nb, std::max<size_t>(need * 2, 4096) * sizeof(BaiChunk));
    if (rc) return rc;
    if (x->n_chunks) HIP_TRY(c, hipMemcpyAsync(nb.p, x->chunks.p, x->n_chunks * sizeof(BaiChunk), hipMemcpyDeviceToDevice, c->stream));
    if (x->chunks.p) bury(c, x->chunks.p); // (the copy is on the stream: freed where a wait costs nothing)
    x->chunks = nb;
    return PJB_OK;
}

static int index_piece_body(pjb_ctx *c, IndexState *x, const uint8_t *comp, int64_t comp_bytes, int64_t file_offset, int32_t first_uoffset, int32_t last,
                            uint64_t *next_voffset) {
    std::vector<InfBlock> blocks;
    int64_t total = 0;
    int rc = scan_bgzf(c, comp, comp_bytes, blocks, total);
    if (rc) return rc;
    if ((int64_t)first_uoffset > total) return fail(c, PJB_ERR_ARG, "index_piece: first_uoffset %d lies behind the piece's %lld inflated bytes", first_uoffset, (long long)total);
    // block starts: inflated offset | file offset, + the sentinel "end of the data, the file's next block"
    const size_t nb = blocks.size();
    std::vector<iu64> tab(2 * (nb + 1));
    {
        int64_t off = 0;
        for (size_t b = 0; b < nb; b++) {
            tab[b] = blocks[b].out_off;
            tab[nb + 1 + b] = (iu64)(file_offset + off);
            off = (int64_t)blocks[b].in_off + blocks[b].in_len + 8; // (the payload, CRC32 and ISIZE: the next block's first byte)
        }
        tab[nb] = (iu64)total;
        tab[2 * nb + 1] = (iu64)(file_offset + comp_bytes);
    }
    auto voffset_of = [&](iu64 u) -> uint64_t { // bai_block_of on the host
        size_t lo = 0, hi = nb + 1;
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (tab[mid] < u) lo = mid + 1;
            else hi = mid;
        }
        if ((lo == nb + 1 || tab[lo] > u) && lo > 0) lo--;
        return tab[nb + 1 + lo] << 16 | (u - tab[lo]);
    };
    size_t n = 0;
    iu64 next_u = (iu64)first_uoffset;
    hipStream_t st = c->stream;
    if ((int64_t)first_uoffset < total) {
        if ((rc = ensure(c, c->b_inf_comp, (size_t)comp_bytes + INF_PAD))) return rc;
        if ((rc = upload_host(c, c->b_inf_comp.p, comp, (size_t)comp_bytes))) return rc;
        HIP_TRY(c, hipMemsetAsync((uint8_t *)c->b_inf_comp.p + comp_bytes, 0, INF_PAD, st));
        if ((rc = ensure(c, c->b_inf_out, (size_t)total + 64))) return rc;
        HIP_TRY(c, hipMemsetAsync((uint8_t *)c->b_inf_out.p + total, 0, 64, st));
        if ((rc = inflate_on_device(c, (const uint8_t *)c->b_inf_comp.p, blocks, (uint8_t *)c->b_inf_out.p))) return rc;
        // every record that lies completely in the inflated bytes, of whatever target
        RecordWalk w;
        if ((rc = walk_records(c, bam_region(c, (const uint8_t *)c->b_inf_out.p, total, first_uoffset, -1), true, "in the piece", w))) return rc;
        if (w.n >= 0xffffff00ull) return fail(c, PJB_ERR_ARG, "index_piece: more than 2^32 alignments in one piece are not supported");
        n = w.n;
        next_u = w.next_u;
    }
    if (next_u < (iu64)total) { // the data ends inside a record
        if (last) return fail(c, PJB_ERR_BGZF, "the data ends inside an alignment record (virtual offset 0x%llx): truncated file", (unsigned long long)voffset_of(next_u));
        if (n == 0) { // nothing was indexed and nothing changed: the caller may hand the same blocks over again with more behind them
            x->keep_on_error = true;
            if (next_voffset) *next_voffset = voffset_of(next_u);
            return fail(c, PJB_ERR_ARG, "index_piece: the alignment record at virtual offset 0x%llx is longer than the piece (%lld bytes): hand over more blocks at once",
                        (unsigned long long)voffset_of(next_u), (long long)comp_bytes);
        }
    }
    if (n > 0) {
        if ((rc = ensure(c, x->key, n * 8)) || (rc = ensure(c, x->vs, n * 8)) || (rc = ensure(c, x->win, n * 8)) || (rc = ensure(c, x->w0, n * 4)) ||
            (rc = ensure(c, x->heads, n * 4)) || (rc = ensure(c, x->tab, tab.size() * 8)))
            return rc;
        iu64 *ctl = (iu64 *)x->ctl.p;
        HIP_TRY(c, hipMemsetAsync(ctl, 0xff, BAI_CTL_WORDS * 8, st));
        HIP_TRY(c, hipMemcpyAsync(x->tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
        BaiTable T;
        T.out_off = (const iu64 *)x->tab.p;
        T.cstart = T.out_off + nb + 1;
        T.n = (iu32)(nb + 1);
        BaiRecOut O;
        O.key = (iu64 *)x->key.p;
        O.vs = (iu64 *)x->vs.p;
        O.win = (iu64 *)x->win.p;
        O.w0 = (iu32 *)x->w0.p;
        O.ctl = ctl;
        const iu64 *rec_off = (const iu64 *)c->b_bam_rec.p;
        const unsigned grid = (unsigned)((n + 255) / 256);
        LAUNCH(c, "bai_records", bai_records, dim3(grid), dim3(256), (const uint8_t *)c->b_inf_out.p, rec_off, (iu64)n, T, (const int32_t *)x->ref_len.p,
               (int32_t)c->ref_len.size(), x->prev_sort, x->csi_depth, O);
        if ((rc = run_scan(c, "bai_head", BaiHeadFn{O.key, x->open_key}, ExclusiveU32Sink{(u32 *)x->heads.p}, n, (u64 *)(ctl + BAI_CTL_HEADS)))) return rc;
        iu64 h[BAI_CTL_WORDS];
        HIP_TRY(c, hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        // the first offender decides (a record that cannot be is usually out of order as well)
        const iu64 first_err = std::min(h[BAI_CTL_UNSORTED], std::min(h[BAI_CTL_BAD], h[BAI_CTL_LONG]));
        if (first_err != ~0ull) {
            const long long ord = (long long)(x->n_records + (int64_t)first_err);
            if (h[BAI_CTL_BAD] == first_err)
                return fail(c, PJB_ERR_BGZF, "alignment record %lld names a target or a position the header does not have (refID beyond the %zu targets, or pos outside its target)",
                            ord, c->ref_len.size());
            if (h[BAI_CTL_LONG] == first_err)
                return fail(c, PJB_ERR_ARG, "BAI cannot index this target: alignment record %lld lies on a target of 2^29 bases or more (a CSI index is needed)", ord);
            return fail(c, PJB_ERR_UNSORTED, "%s (alignment record %lld lies before its predecessor)", err_text(PJB_ERR_UNSORTED), ord);
        }
        const size_t n_heads = (size_t)h[BAI_CTL_HEADS];
        if (x->n_chunks + n_heads >= 0xffffff00ull) return fail(c, PJB_ERR_ARG, "index_piece: more than 2^32 chunks are not supported");
        if ((rc = index_grow_chunks(c, x, x->n_chunks + n_heads))) return rc;
        LAUNCH(c, "bai_chunks", bai_chunks, dim3(grid), dim3(256), (const iu64 *)O.key, (const iu64 *)O.vs, (const iu32 *)x->heads.p, (iu64)n, x->open_key,
               (BaiChunk *)x->chunks.p, (iu64)x->n_chunks, (iu64)(x->n_chunks + n_heads));
        const iu32 nt = (iu32)((n + SCAN_TILE - 1) / SCAN_TILE);
        if ((rc = ensure(c, x->tile_max, (size_t)nt * 8))) return rc;
        LAUNCH(c, "bai_win_reduce", bai_win_reduce, dim3(nt), dim3(256), (const iu64 *)O.win, (iu64)n, (iu64 *)x->tile_max.p);
        LAUNCH(c, "bai_win_tiles", bai_win_tiles, dim3(1), dim3(1024), (iu64 *)x->tile_max.p, nt, x->win_carry, ctl + BAI_CTL_WINMAX);
        LAUNCH(c, "bai_win_apply", bai_win_apply, dim3(nt), dim3(256), (const iu64 *)O.win, (const iu32 *)O.w0, (const iu64 *)O.vs, (iu64)n,
               (const iu64 *)x->tile_max.p, (const iu64 *)x->lin_off.p, (iu64 *)x->lin.p, (iu64)x->lin_total);
        iu64 win_max = 0;
        HIP_TRY(c, hipMemcpyAsync(&win_max, ctl + BAI_CTL_WINMAX, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (c->ktime) ev_collect(c, MISC_POOL);
        x->n_chunks += n_heads;
        x->n_records += (int64_t)n;
        x->prev_sort = h[BAI_CTL_LASTSORT];
        x->open_key = h[BAI_CTL_LASTKEY];
        x->win_carry = win_max;
    }
    const uint64_t nv = voffset_of(next_u);
    if (next_voffset) *next_voffset = nv;
    if (last) {
        x->saw_last = true;
        x->end_voffset = nv;
    }
    return PJB_OK;
}

extern "C" int pjb_index_piece(pjb_ctx *c, const uint8_t *comp, int64_t comp_bytes, int64_t file_offset, int32_t first_uoffset, int32_t last,
                               uint64_t *next_voffset) {
    if (!c) return PJB_ERR_ARG;
    IndexState *x = c->index;
    if (!x || !x->active) return fail(c, PJB_ERR_STATE, "index_piece: no index is being built (pjb_index_begin)");
    if (x->saw_last) return fail(c, PJB_ERR_STATE, "index_piece: the last piece has been handed over (pjb_index_end)");
    if (comp_bytes < 0 || (comp_bytes && !comp) || file_offset < 0 || first_uoffset < 0) return fail(c, PJB_ERR_ARG, "index_piece: bad arguments");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    x->keep_on_error = false;
    const int rc = index_piece_body(c, x, comp, comp_bytes, file_offset, first_uoffset, last, next_voffset);
    if (rc && !x->keep_on_error) { // the index is dropped: begin again
        (void)hipStreamSynchronize(c->stream);
        x->active = false;
    }
    return rc;
}

// closes the last chunk and orders the list by (target, bin, file order) into x->sorted, the copy to x->r_chunks queued
static int index_order_chunks(pjb_ctx *c, IndexState *x) {
    hipStream_t st = c->stream;
    const size_t n = x->n_chunks, n_ref = c->ref_len.size();
    int rc;
    x->r_chunks.assign(n, pjb_index_chunk());
    if (n) {
        BaiChunk *chunks = (BaiChunk *)x->chunks.p;
        // the last run ends where the data ends
        if (x->open_key != BAI_NOKEY) HIP_TRY(c, hipMemcpyAsync(&chunks[n - 1].vend, &x->end_voffset, 8, hipMemcpyHostToDevice, st));
        const int n_scans = x->csi_depth > 5 ? 4 : 3; // two levels a scan
        for (int p = 0; p < n_scans; p++)
            if ((rc = ensure(c, x->q[p], (n + 1) * 8))) return rc;
        if ((rc = ensure(c, x->tid_start, (n_ref + 1) * 4)) || (rc = ensure(c, x->sorted, n * sizeof(BaiChunk)))) return rc;
        iu64 *ctl = (iu64 *)x->ctl.p;
        for (int p = 0; p < n_scans; p++)
            if ((rc = run_scan(c, "bai_level", BaiLevelFn{chunks, (iu64)n, (iu32)p}, BaiLevelSink{(iu64 *)x->q[p].p}, n + 1, (u64 *)(ctl + BAI_CTL_HEADS)))) return rc;
        LAUNCH(c, "bai_tid_starts", bai_tid_starts, dim3((unsigned)((n + 256) / 256)), dim3(256), (const BaiChunk *)chunks, (iu64)n, (int32_t)n_ref, (iu32 *)x->tid_start.p);
        LAUNCH(c, "bai_partition", bai_partition, dim3((unsigned)((n + 255) / 256)), dim3(256), (const BaiChunk *)chunks, (iu64)n, (int32_t)n_ref,
               (const iu32 *)x->tid_start.p, (const iu64 *)x->q[0].p, (const iu64 *)x->q[1].p, (const iu64 *)x->q[2].p, (const iu64 *)(n_scans > 3 ? x->q[3].p : nullptr), (BaiChunk *)x->sorted.p);
        HIP_TRY(c, hipMemcpyAsync(x->r_chunks.data(), x->sorted.p, n * sizeof(BaiChunk), hipMemcpyDeviceToHost, st));
    }
    return PJB_OK;
}

extern "C" int pjb_index_end(pjb_ctx *c, pjb_index_result *out) {
    if (!c || !out) return fail(c, PJB_ERR_ARG, "index_end: bad arguments");
    IndexState *x = c->index;
    if (!x || !x->active) return fail(c, PJB_ERR_STATE, "index_end: no index is being built (pjb_index_begin)");
    if (x->csi_depth >= 0) return fail(c, PJB_ERR_STATE, "index_end: a CSI is being built (pjb_index_end_csi)");
    if (!x->saw_last) return fail(c, PJB_ERR_STATE, "index_end: the last piece has not been handed over (pjb_index_piece with last != 0)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    x->active = false;
    hipStream_t st = c->stream;
    const size_t n = x->n_chunks, n_ref = c->ref_len.size();
    int rc;
    if ((rc = index_order_chunks(c, x))) return rc;
    // the windows: per target up to the last one a record touched (every touched window holds a virtual offset, and none is 0)
    std::vector<uint64_t> all(x->lin_total);
    if (x->lin_total) HIP_TRY(c, hipMemcpyAsync(all.data(), x->lin.p, x->lin_total * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    x->r_lin_off.assign(n_ref + 1, 0);
    x->r_lin.clear();
    for (size_t t = 0; t < n_ref; t++) {
        const size_t a = (size_t)x->h_lin_cap[t];
        size_t k = (size_t)x->h_lin_cap[t + 1] - a;
        while (k > 0 && all[a + k - 1] == 0) k--;
        x->r_lin.insert(x->r_lin.end(), all.begin() + (long)a, all.begin() + (long)(a + k));
        x->r_lin_off[t + 1] = (int64_t)x->r_lin.size();
    }
    out->n_records = x->n_records;
    out->n_chunks = (int64_t)n;
    out->chunks = x->r_chunks.data();
    out->lin_off = x->r_lin_off.data();
    out->lin = x->r_lin.data();
    return PJB_OK;
}

extern "C" int pjb_index_end_csi(pjb_ctx *c, pjb_csi_result *out) {
    if (!c || !out) return fail(c, PJB_ERR_ARG, "index_end_csi: bad arguments");
    IndexState *x = c->index;
    if (!x || !x->active) return fail(c, PJB_ERR_STATE, "index_end_csi: no index is being built (pjb_index_begin_csi)");
    if (x->csi_depth < 0) return fail(c, PJB_ERR_STATE, "index_end_csi: a BAI is being built (pjb_index_end)");
    if (!x->saw_last) return fail(c, PJB_ERR_STATE, "index_end_csi: the last piece has not been handed over (pjb_index_piece with last != 0)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    x->active = false;
    hipStream_t st = c->stream;
    const size_t n = x->n_chunks, n_ref = c->ref_len.size();
    int rc;
    if ((rc = index_order_chunks(c, x))) return rc;
    x->r_loff.assign(n, 0);
    if (n && x->lin_total) {
        // the windows filled from the left (tid_start is index_order_chunks'), then every chunk's bin reads its first one
        if ((rc = ensure(c, x->loff, n * 8))) return rc;
        const iu32 nt = (iu32)((x->lin_total + SCAN_TILE - 1) / SCAN_TILE);
        if ((rc = ensure(c, x->tile_max, (size_t)nt * 8))) return rc;
        iu64 *ctl = (iu64 *)x->ctl.p, *lin = (iu64 *)x->lin.p;
        LAUNCH(c, "csi_seed", csi_seed, dim3((unsigned)((n_ref + 255) / 256)), dim3(256), (const BaiChunk *)x->chunks.p, (const iu32 *)x->tid_start.p, (int32_t)n_ref,
               (const iu64 *)x->lin_off.p, lin, (iu64)x->lin_total);
        LAUNCH(c, "bai_win_reduce", bai_win_reduce, dim3(nt), dim3(256), (const iu64 *)lin, (iu64)x->lin_total, (iu64 *)x->tile_max.p);
        LAUNCH(c, "bai_win_tiles", bai_win_tiles, dim3(1), dim3(1024), (iu64 *)x->tile_max.p, nt, (iu64)0, ctl + BAI_CTL_WINMAX);
        LAUNCH(c, "csi_fill_apply", csi_fill_apply, dim3(nt), dim3(256), lin, (iu64)x->lin_total, (const iu64 *)x->tile_max.p);
        LAUNCH(c, "csi_loffset", csi_loffset, dim3((unsigned)((n + 255) / 256)), dim3(256), (const BaiChunk *)x->sorted.p, (iu64)n, (int32_t)n_ref, x->csi_depth,
               (const iu64 *)x->lin_off.p, (const iu64 *)lin, (iu64)x->lin_total, (iu64 *)x->loff.p);
        HIP_TRY(c, hipMemcpyAsync(x->r_loff.data(), x->loff.p, n * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    out->n_records = x->n_records;
    out->n_chunks = (int64_t)n;
    out->chunks = x->r_chunks.data();
    out->loffset = x->r_loff.data();
    out->min_shift = CSI_MIN_SHIFT;
    out->depth = x->csi_depth;
    return PJB_OK;
}


// ---- several sorted files' records of one target as one stream (pjb_bam_merge_begin / _file / _end, see the header; kernels in pjb_merge.hip.h) ----
struct MergeFile {
    bool given = false;
    size_t n = 0;       // its records on the target
    Buf out;            // its inflated bytes, 64 zeroed bytes behind them
    Buf key, size, src; // per record: pos | 4 + block_size | where it lies in `out`
};
struct MergeState {
    bool active = false;
    int32_t tid = -1;
    std::vector<MergeFile> files;
    SortU32 sort;                              // all files' keys, file after file, and what the passes need
    Buf size, src;                             // all files' sizes and places
    Buf dst, ctl, stream;                      // offsets in the merged stream | MG_CTL_* and the passes' record count | the merged stream
    uint32_t h_n = 0;                          // (copied to the device asynchronously)
    // the result
    std::vector<uint32_t> r_size;
    std::vector<uint8_t> r_members;
};

static void merge_file_release(pjb_ctx *c, MergeFile &f) {
    for (Buf *b : {&f.out, &f.key, &f.size, &f.src}) release(c, *b);
}
static void merge_clear(pjb_ctx *c) {
    MergeState *m = c->merge;
    if (!m) return;
    for (MergeFile &f : m->files) merge_file_release(c, f);
    SortU32 &s = m->sort;
    for (Buf *b : {&s.key[0], &s.key[1], &s.idx[0], &s.idx[1], &s.hist, &s.hist_part, &s.hist_scan, &s.bin_total, &m->size, &m->src, &m->dst, &m->ctl, &m->stream})
        release(c, *b);
    delete m;
    c->merge = nullptr;
}
// what a failing call leaves: nothing to go on with, except after PJB_ERR_NOMEM (the call can be repeated)
static int merge_leave(pjb_ctx *c, MergeState *m, int rc) {
    if (rc && rc != PJB_ERR_NOMEM) {
        (void)hipStreamSynchronize(c->stream);
        m->active = false;
    }
    return rc;
}

extern "C" int pjb_bam_merge_begin(pjb_ctx *c, int32_t tid, int32_t n_files) {
    if (!c) return PJB_ERR_ARG;
    if (c->merge) c->merge->active = false;
    if (tid < 0 || (size_t)tid >= c->ref_len.size() || n_files < 1) return fail(c, PJB_ERR_ARG, "bam_merge_begin: bad arguments (tid %d, %d files)", tid, n_files);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (!c->merge) c->merge = new (std::nothrow) MergeState();
    MergeState *m = c->merge;
    if (!m) return fail(c, PJB_ERR_NOMEM, "bam_merge_begin: out of host memory");
    for (size_t k = (size_t)n_files; k < m->files.size(); k++) merge_file_release(c, m->files[k]);
    m->files.resize((size_t)n_files);
    for (MergeFile &f : m->files) {
        f.given = false;
        f.n = 0;
    }
    m->r_size.clear();
    m->r_members.clear();
    int rc = ensure(c, m->ctl, MG_CTL_WORDS * 8);
    if (rc) return rc;
    m->tid = tid;
    m->active = true;
    return PJB_OK;
}

static int merge_file_body(pjb_ctx *c, MergeState *m, int32_t file, const uint8_t *comp, int64_t comp_bytes, int32_t first_uoffset, int64_t *n_records) {
    MergeFile &f = m->files[(size_t)file];
    const int32_t tid = m->tid;
    std::vector<InfBlock> blocks;
    int64_t total = 0;
    int rc = scan_bgzf(c, comp, comp_bytes, blocks, total);
    if (rc) return rc;
    if (total == 0 || (int64_t)first_uoffset >= total) {
        f.given = true;
        return PJB_OK;
    }
    hipStream_t st = c->stream;
    if ((rc = ensure(c, c->b_inf_comp, (size_t)comp_bytes + INF_PAD))) return rc;
    if ((rc = upload_host(c, c->b_inf_comp.p, comp, (size_t)comp_bytes))) return rc;
    HIP_TRY(c, hipMemsetAsync((uint8_t *)c->b_inf_comp.p + comp_bytes, 0, INF_PAD, st));
    if ((rc = ensure_cat(c, f.out, (size_t)total + 64, MEM_STAGING))) return rc;
    HIP_TRY(c, hipMemsetAsync((uint8_t *)f.out.p + total, 0, 64, st));
    if ((rc = inflate_on_device(c, (const uint8_t *)c->b_inf_comp.p, blocks, (uint8_t *)f.out.p))) return rc;
    // the target's records: up to the first one of another target.  (The walk's other end test, a position past the target's end, is
    // off: such a record is an error here, found by mg_keys.)
    BamRegion R = bam_region(c, (const uint8_t *)f.out.p, total, first_uoffset, tid);
    const int32_t ref_len = R.ref_len;
    R.ref_len = INT32_MAX;
    RecordWalk w;
    if ((rc = walk_records(c, R, false, ("in file " + std::to_string(file) + " on target " + std::to_string(tid)).c_str(), w))) return rc;
    if (w.end_seg == 0xffffffffu && w.cut_seg != 0xffffffffu) {
        // The data ends inside a record and no record of another target was seen.  The walk asks for a record's 36 fixed bytes before it
        // looks at it; a span that ends with the block in which the NEXT target begins may hold fewer of that target's first record.
        // With its refID in reach (8 bytes) that record says itself whose it is.
        const uint32_t n_seg = (uint32_t)(((iu64)total + BAM_SEG - 1) / BAM_SEG);
        const iu64 *land = (const iu64 *)c->b_bam_seg.p + 2 * (size_t)n_seg; // (walk_records: seg_start | seg_base | land)
        iu64 at = 0;
        HIP_TRY(c, hipMemcpyAsync(&at, land + w.cut_seg, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        int32_t head[2] = {0, tid};
        if (at + 8 <= (iu64)total) HIP_TRY(c, hipMemcpy(head, (const uint8_t *)f.out.p + at, 8, hipMemcpyDeviceToHost));
        if (head[1] == tid)
            return fail(c, PJB_ERR_BGZF, "file %d: the data for target %d ends inside an alignment record (inflated offset %llu..): truncated "
                                         "file, or the index's span for the target is too short", file, tid, (unsigned long long)at);
    }
    if (w.n >= 0xffffff00ull) return fail(c, PJB_ERR_ARG, "bam_merge_file: more than 2^32 alignments on one target are not supported");
    const size_t n = w.n;
    if (n) {
        if ((rc = ensure(c, f.key, n * 4)) || (rc = ensure(c, f.size, n * 4)) || (rc = ensure(c, f.src, n * 8))) return rc;
        iu64 *ctl = (iu64 *)m->ctl.p;
        HIP_TRY(c, hipMemsetAsync(ctl, 0xff, MG_CTL_WORDS * 8, st));
        LAUNCH(c, "mg_keys", mg_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), (const uint8_t *)f.out.p, (const iu64 *)c->b_bam_rec.p, (iu64)n, ref_len,
               (iu32 *)f.key.p, (iu32 *)f.size.p, (iu64 *)f.src.p, ctl);
        iu64 h[MG_CTL_WORDS];
        HIP_TRY(c, hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (c->ktime) ev_collect(c, MISC_POOL);
        // the first offender decides
        if (h[MG_CTL_BAD] != ~0ull && h[MG_CTL_BAD] <= h[MG_CTL_UNSORTED])
            return fail(c, PJB_ERR_BGZF, "file %d: alignment record %llu on target %d has a position outside the target", file, (unsigned long long)h[MG_CTL_BAD], tid);
        if (h[MG_CTL_UNSORTED] != ~0ull)
            return fail(c, PJB_ERR_UNSORTED, "%s (file %d: alignment record %llu on target %d lies before its predecessor)", err_text(PJB_ERR_UNSORTED), file,
                        (unsigned long long)h[MG_CTL_UNSORTED], tid);
    }
    f.n = n;
    f.given = true;
    if (n_records) *n_records = (int64_t)n;
    return PJB_OK;
}

extern "C" int pjb_bam_merge_file(pjb_ctx *c, int32_t file, const uint8_t *comp, int64_t comp_bytes, int32_t first_uoffset, int64_t *n_records) {
    if (!c) return PJB_ERR_ARG;
    if (n_records) *n_records = 0;
    MergeState *m = c->merge;
    if (!m || !m->active) return fail(c, PJB_ERR_STATE, "bam_merge_file: no merge is open (pjb_bam_merge_begin)");
    if (file < 0 || (size_t)file >= m->files.size() || comp_bytes < 0 || (comp_bytes && !comp) || first_uoffset < 0)
        return merge_leave(c, m, fail(c, PJB_ERR_ARG, "bam_merge_file: bad arguments (file %d of %zu)", file, m->files.size()));
    if (m->files[(size_t)file].given) return merge_leave(c, m, fail(c, PJB_ERR_STATE, "bam_merge_file: file %d was handed over already", file));
    c->cur_tid = m->tid;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    return merge_leave(c, m, merge_file_body(c, m, file, comp, comp_bytes, first_uoffset, n_records));
}

static int merge_end_body(pjb_ctx *c, MergeState *m, int32_t block_bytes, pjb_bam_merge_result *out) {
    hipStream_t st = c->stream;
    int rc;
    std::vector<MergeFile *> parts; // the files that have records, in file order
    iu64 n64 = 0;
    for (MergeFile &f : m->files)
        if (f.given && f.n) {
            parts.push_back(&f);
            n64 += f.n;
        }
    if (n64 >= 0xffffff00ull) return fail(c, PJB_ERR_ARG, "bam_merge_end: more than 2^32 alignments on one target are not supported");
    const size_t n = (size_t)n64;
    if (n == 0) return PJB_OK;
    iu64 *ctl = (iu64 *)m->ctl.p;
    const iu32 *order = nullptr, *size = (const iu32 *)parts[0]->size.p;
    const iu64 *src = (const iu64 *)parts[0]->src.p;
    const int32_t ref_len = c->ref_len[(size_t)m->tid];
    const int key_bits = ref_len > 1 ? bits_of((uint64_t)ref_len - 1) : 0;
    if (parts.size() > 1) {
        // one ordinal space, file after file
        const size_t slack = n + RS_TILE; // (rs_scatter loads whole tiles unguarded)
        if ((rc = ensure(c, m->sort.key[0], slack * 4)) || (rc = ensure(c, m->sort.key[1], slack * 4)) || (rc = ensure(c, m->sort.idx[0], slack * 4)) ||
            (rc = ensure(c, m->sort.idx[1], slack * 4)) || (rc = ensure(c, m->size, n * 4)) || (rc = ensure(c, m->src, n * 8)))
            return rc;
        size_t at = 0;
        for (MergeFile *f : parts) {
            HIP_TRY(c, hipMemcpyAsync((iu32 *)m->sort.key[0].p + at, f->key.p, f->n * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(c, hipMemcpyAsync((iu32 *)m->size.p + at, f->size.p, f->n * 4, hipMemcpyDeviceToDevice, st));
            HIP_TRY(c, hipMemcpyAsync((iu64 *)m->src.p + at, f->src.p, f->n * 8, hipMemcpyDeviceToDevice, st));
            at += f->n;
        }
        size = (const iu32 *)m->size.p;
        src = (const iu64 *)m->src.p;
        if (key_bits > 0) { // (a target of one base: every key is 0, the ordinals are in order)
            u32 *d_n = (u32 *)(ctl + MG_CTL_WORDS - 1);
            m->h_n = (uint32_t)n;
            HIP_TRY(c, hipMemcpyAsync(d_n, &m->h_n, 4, hipMemcpyHostToDevice, st));
            int cur = 0;
            if ((rc = sort_u32_pairs(c, m->sort, d_n, n, key_bits, &cur))) return rc;
            order = (const iu32 *)m->sort.idx[cur].p;
        }
    }
    // where every record goes, and how long the stream is
    if ((rc = ensure(c, m->dst, n * 8))) return rc;
    if ((rc = run_scan(c, "mg_off", MgSizeFn{size, order}, MgOffsetSink{(iu64 *)m->dst.p}, n, (u64 *)(ctl + MG_CTL_TOTAL)))) return rc;
    iu64 raw = 0;
    HIP_TRY(c, hipMemcpyAsync(&raw, ctl + MG_CTL_TOTAL, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if ((rc = ensure_cat(c, m->stream, (size_t)raw + 64, MEM_STAGING))) return rc;
    LAUNCH(c, "mg_gather", mg_gather, dim3((unsigned)((n + 3) / 4)), dim3(256), src, size, order, (const iu64 *)m->dst.p, (iu64)n, (uint8_t *)m->stream.p);
    rc = deflate_launches(c, nullptr, (const uint8_t *)m->stream.p, (int64_t)raw, block_bytes, [&](int64_t, const std::vector<u32> &sizes, iu64 total, uint8_t *&dst) {
        const size_t had = m->r_members.size();
        m->r_size.insert(m->r_size.end(), sizes.begin(), sizes.end());
        m->r_members.resize(had + (size_t)total);
        dst = m->r_members.data() + had;
        return (int)PJB_OK;
    });
    if (rc) {
        m->r_size.clear();
        m->r_members.clear();
        return rc;
    }
    out->n_records = (int64_t)n;
    out->raw_bytes = (int64_t)raw;
    return PJB_OK;
}

extern "C" int pjb_bam_merge_end(pjb_ctx *c, int32_t block_bytes, pjb_bam_merge_result *out) {
    if (!c) return PJB_ERR_ARG;
    MergeState *m = c->merge;
    if (!m || !m->active) return fail(c, PJB_ERR_STATE, "bam_merge_end: no merge is open (pjb_bam_merge_begin)");
    if (!out) return merge_leave(c, m, fail(c, PJB_ERR_ARG, "bam_merge_end: bad arguments"));
    if (block_bytes < 4 || block_bytes > (int32_t)DFL_IN_MAX || (block_bytes & 3))
        return merge_leave(c, m, fail(c, PJB_ERR_ARG, "bam_merge_end: block_bytes must be a multiple of 4 between 4 and %u", DFL_IN_MAX));
    c->cur_tid = m->tid;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    memset(out, 0, sizeof *out);
    const int rc = merge_leave(c, m, merge_end_body(c, m, block_bytes, out));
    if (rc) return rc;
    m->active = false;
    out->n_members = (int32_t)m->r_size.size();
    out->member_size = m->r_size.data();
    out->members = m->r_members.data();
    out->member_bytes = (int64_t)m->r_members.size();
    return PJB_OK;
}


// ---- an unsorted file's records in coordinate order, run by run (pjb_bam_sort_begin / _piece / _end, see the header; sr_keys in pjb_merge.hip.h) ----
struct SortRun {
    bool active = false;
    bool keep_on_error = false;      // the failing piece call left the run as it was
    int pos_bits = 0, key_bits = 0;  // bits_of(longest target - 1) | + bits_of(n_ref): what the sort runs over
    bool wide = false;               // key_bits > 32: 64-bit keys
    size_t n = 0, cap = 0;           // records taken | room in sort.key[0], size, src
    int64_t n_unplaced = 0;
    iu64 prev = 0;                   // the key of the last record taken
    iu64 descent = ~0ull;            // the first ordinal whose key lies below its predecessor's
    bool ordered = false;            // pjb_bam_sort_end has run the passes: the order lies in sort.idx[order_in]
    int order_in = 0;
    std::vector<Buf> pieces;         // every piece's inflated bytes, 64 zeroed bytes behind them
    SortU32 sort;                    // key[0]: the run's keys in input order
    Buf size, src;                   // per record: 4 + block_size | where it lies in its piece
    Buf ref_len, dst, ctl, stream;   // i32[n_ref] | offsets in the sorted stream | SR_CTL_* | the sorted stream
    uint32_t h_n = 0;                // (copied to the device asynchronously)
    // the result
    std::vector<uint32_t> r_size;
    std::vector<uint8_t> r_members;
};

static void sort_drop_pieces(pjb_ctx *c, SortRun *r) {
    for (Buf &b : r->pieces) release(c, b);
    r->pieces.clear();
}
static void sort_clear(pjb_ctx *c) {
    SortRun *r = c->sort_run;
    if (!r) return;
    sort_drop_pieces(c, r);
    SortU32 &s = r->sort;
    for (Buf *b : {&s.key[0], &s.key[1], &s.idx[0], &s.idx[1], &s.hist, &s.hist_part, &s.hist_scan, &s.bin_total, &r->size, &r->src, &r->ref_len, &r->dst, &r->ctl, &r->stream})
        release(c, *b);
    delete r;
    c->sort_run = nullptr;
}
// what a failing call leaves: nothing to go on with, except after PJB_ERR_NOMEM and a first record longer than its piece
static int sort_leave(pjb_ctx *c, SortRun *r, int rc) {
    if (rc && rc != PJB_ERR_NOMEM && !r->keep_on_error) {
        (void)hipStreamSynchronize(c->stream);
        r->active = false;
        sort_drop_pieces(c, r);
    }
    return rc;
}

extern "C" int pjb_bam_sort_begin(pjb_ctx *c) {
    if (!c) return PJB_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (!c->sort_run) c->sort_run = new (std::nothrow) SortRun();
    SortRun *r = c->sort_run;
    if (!r) return fail(c, PJB_ERR_NOMEM, "bam_sort_begin: out of host memory");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    r->active = false;
    sort_drop_pieces(c, r);
    r->n = 0;
    r->n_unplaced = 0;
    r->prev = 0;
    r->descent = ~0ull;
    r->ordered = false;
    r->r_size.clear();
    r->r_members.clear();
    const size_t n_ref = c->ref_len.size();
    int32_t longest = 0;
    for (int32_t len : c->ref_len) longest = std::max(longest, len);
    r->pos_bits = longest > 1 ? bits_of((uint64_t)longest - 1) : 0;
    r->key_bits = r->pos_bits + bits_of((uint64_t)n_ref);
    const bool wide = r->key_bits > 32;
    if (wide != r->wide) { // the keys' buffers are typed by what they hold
        for (Buf *b : {&r->sort.key[0], &r->sort.key[1]}) release(c, *b);
        r->cap = 0;
        r->wide = wide;
    }
    int rc;
    if ((rc = ensure(c, r->ctl, SR_CTL_WORDS * 8)) || (rc = ensure(c, r->ref_len, n_ref * 4 + 4))) return rc;
    if (n_ref) HIP_TRY(c, hipMemcpy(r->ref_len.p, c->ref_len.data(), n_ref * 4, hipMemcpyHostToDevice));
    r->active = true;
    return PJB_OK;
}

// room for `need` records in the run's arrays: larger buffers take over what the arrays hold
static int sort_grow(pjb_ctx *c, SortRun *r, size_t need) {
    if (need <= r->cap && r->sort.key[0].p) return PJB_OK;
    const size_t cap = std::max<size_t>(need + need / 2, (size_t)1 << 16), ksz = r->wide ? 8 : 4;
    Buf nk, ns, nr;
    int rc;
    if ((rc = ensure(c, nk, (cap + RS_TILE) * ksz)) || (rc = ensure(c, ns, cap * 4)) || (rc = ensure(c, nr, cap * 8))) {
        for (Buf *b : {&nk, &ns, &nr}) release(c, *b);
        return rc;
    }
    hipStream_t st = c->stream;
    if (r->n) {
        HIP_TRY(c, hipMemcpyAsync(nk.p, r->sort.key[0].p, r->n * ksz, hipMemcpyDeviceToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(ns.p, r->size.p, r->n * 4, hipMemcpyDeviceToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(nr.p, r->src.p, r->n * 8, hipMemcpyDeviceToDevice, st));
    }
    for (Buf *b : {&r->sort.key[0], &r->size, &r->src})
        if (b->p) bury(c, b->p); // (the copies are on the stream: freed where a wait costs nothing)
    r->sort.key[0] = nk;
    r->size = ns;
    r->src = nr;
    r->cap = cap;
    return PJB_OK;
}

static int sort_piece_body(pjb_ctx *c, SortRun *r, Buf &out, const uint8_t *comp, int64_t comp_bytes, int32_t first_uoffset, int32_t last, uint64_t *next_voffset,
                           int64_t *n_records) {
    std::vector<InfBlock> blocks;
    int64_t total = 0;
    int rc = scan_bgzf(c, comp, comp_bytes, blocks, total);
    if (rc) return rc;
    if ((int64_t)first_uoffset > total) return fail(c, PJB_ERR_ARG, "bam_sort_piece: first_uoffset %d lies behind the piece's %lld inflated bytes", first_uoffset, (long long)total);
    const size_t nb = blocks.size();
    // inflated byte u of the piece as (offset of its block in the piece) << 16 | offset in the block; the end of the data: the piece's end
    auto voffset_of = [&](iu64 u) -> uint64_t {
        if (u >= (iu64)total) return (uint64_t)comp_bytes << 16;
        size_t lo = 0, hi = nb;
        while (lo < hi) { // the first block that begins behind u; the one before it holds u (empty blocks lie before the block they share a start with)
            const size_t mid = lo + (hi - lo) / 2;
            if (blocks[mid].out_off <= u) lo = mid + 1;
            else hi = mid;
        }
        const size_t k = lo - 1;
        const iu64 start = k == 0 ? 0 : blocks[k - 1].in_off + blocks[k - 1].in_len + 8; // (behind the payload, CRC32 and ISIZE of the block before)
        return (uint64_t)start << 16 | (u - blocks[k].out_off);
    };
    size_t n = 0;
    iu64 next_u = (iu64)first_uoffset;
    hipStream_t st = c->stream;
    if ((int64_t)first_uoffset < total) {
        if ((rc = ensure(c, c->b_inf_comp, (size_t)comp_bytes + INF_PAD))) return rc;
        if ((rc = upload_host(c, c->b_inf_comp.p, comp, (size_t)comp_bytes))) return rc;
        HIP_TRY(c, hipMemsetAsync((uint8_t *)c->b_inf_comp.p + comp_bytes, 0, INF_PAD, st));
        if ((rc = ensure_cat(c, out, (size_t)total + 64, MEM_STAGING))) return rc;
        HIP_TRY(c, hipMemsetAsync((uint8_t *)out.p + total, 0, 64, st));
        if ((rc = inflate_on_device(c, (const uint8_t *)c->b_inf_comp.p, blocks, (uint8_t *)out.p))) return rc;
        RecordWalk w;
        if ((rc = walk_records(c, bam_region(c, (const uint8_t *)out.p, total, first_uoffset, -1), true, "in the piece", w))) return rc;
        if (w.n >= 0xffffff00ull || r->n + w.n >= 0xffffff00ull) return fail(c, PJB_ERR_ARG, "bam_sort_piece: 2^32 - 256 alignments or more in one run are not supported");
        n = w.n;
        next_u = w.next_u;
    }
    if (next_u < (iu64)total) { // the data ends inside a record
        if (last) return fail(c, PJB_ERR_BGZF, "the data ends inside an alignment record (inflated offset %llu of the last piece): truncated file", (unsigned long long)next_u);
        if (n == 0) { // nothing was taken and nothing changed: the caller may hand the same blocks over again with more behind them
            r->keep_on_error = true;
            if (next_voffset) *next_voffset = voffset_of(next_u);
            return fail(c, PJB_ERR_ARG, "bam_sort_piece: the alignment record at inflated offset %llu is longer than the piece (%lld bytes): hand over more blocks at once",
                        (unsigned long long)next_u, (long long)comp_bytes);
        }
    }
    if (n > 0) {
        if ((rc = sort_grow(c, r, r->n + n))) return rc;
        iu64 *ctl = (iu64 *)r->ctl.p;
        HIP_TRY(c, hipMemsetAsync(ctl, 0xff, SR_CTL_WORDS * 8, st));
        HIP_TRY(c, hipMemsetAsync(ctl + SR_CTL_UNPLACED, 0, 8, st));
        const dim3 grid((unsigned)((n + 255) / 256));
        const iu64 *rec_off = (const iu64 *)c->b_bam_rec.p;
        if (r->wide)
            LAUNCH(c, "sr_keys", sr_keys<u64>, grid, dim3(256), (const uint8_t *)out.p, rec_off, (iu64)n, (const int32_t *)r->ref_len.p, (int32_t)c->ref_len.size(), r->pos_bits,
                   r->prev, (u64 *)r->sort.key[0].p + r->n, (iu32 *)r->size.p + r->n, (iu64 *)r->src.p + r->n, ctl);
        else
            LAUNCH(c, "sr_keys", sr_keys<u32>, grid, dim3(256), (const uint8_t *)out.p, rec_off, (iu64)n, (const int32_t *)r->ref_len.p, (int32_t)c->ref_len.size(), r->pos_bits,
                   r->prev, (u32 *)r->sort.key[0].p + r->n, (iu32 *)r->size.p + r->n, (iu64 *)r->src.p + r->n, ctl);
        iu64 h[SR_CTL_WORDS];
        HIP_TRY(c, hipMemcpyAsync(h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (c->ktime) ev_collect(c, MISC_POOL);
        // the first offender decides
        if (h[SR_CTL_BAD_TID] != ~0ull && h[SR_CTL_BAD_TID] <= h[SR_CTL_BAD_POS])
            return fail(c, PJB_ERR_BGZF, "alignment record %llu names a target the header does not have (its refID lies outside the %zu targets)",
                        (unsigned long long)(r->n + h[SR_CTL_BAD_TID]), c->ref_len.size());
        if (h[SR_CTL_BAD_POS] != ~0ull)
            return fail(c, PJB_ERR_BGZF, "alignment record %llu has a position outside its target", (unsigned long long)(r->n + h[SR_CTL_BAD_POS]));
        if (h[SR_CTL_DESCENT] != ~0ull) r->descent = std::min(r->descent, (iu64)r->n + h[SR_CTL_DESCENT]);
        r->prev = h[SR_CTL_LAST];
        r->n_unplaced += (int64_t)h[SR_CTL_UNPLACED];
        r->n += n;
        r->pieces.push_back(out);
        out = Buf();
    }
    if (next_voffset) *next_voffset = voffset_of(next_u);
    if (n_records) *n_records = (int64_t)n;
    return PJB_OK;
}

extern "C" int pjb_bam_sort_piece(pjb_ctx *c, const uint8_t *comp, int64_t comp_bytes, int32_t first_uoffset, int32_t last, uint64_t *next_voffset,
                                  int64_t *n_records) {
    if (!c) return PJB_ERR_ARG;
    if (n_records) *n_records = 0;
    SortRun *r = c->sort_run;
    if (!r || !r->active) return fail(c, PJB_ERR_STATE, "bam_sort_piece: no run is open (pjb_bam_sort_begin)");
    r->keep_on_error = false;
    if (comp_bytes < 0 || (comp_bytes && !comp) || first_uoffset < 0) return sort_leave(c, r, fail(c, PJB_ERR_ARG, "bam_sort_piece: bad arguments"));
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    Buf out;
    const int rc = sort_piece_body(c, r, out, comp, comp_bytes, first_uoffset, last, next_voffset, n_records);
    if (out.p) { // the piece was not taken: its bytes go when nothing reads them any more
        (void)hipStreamSynchronize(c->stream);
        release(c, out);
    }
    return sort_leave(c, r, rc);
}

static int sort_end_body(pjb_ctx *c, SortRun *r, int32_t block_bytes, pjb_bam_sort_result *out) {
    hipStream_t st = c->stream;
    int rc;
    const size_t n = r->n;
    out->was_sorted = r->descent == ~0ull;
    if (n == 0) return PJB_OK;
    iu64 *ctl = (iu64 *)r->ctl.p;
    const iu32 *order = nullptr;
    if (!out->was_sorted) { // (a descent needs two different keys: key_bits > 0)
        const size_t slack = n + RS_TILE, ksz = r->wide ? 8 : 4; // (rs_scatter loads whole tiles unguarded)
        if ((rc = ensure(c, r->sort.key[1], slack * ksz)) || (rc = ensure(c, r->sort.idx[0], slack * 4)) || (rc = ensure(c, r->sort.idx[1], slack * 4))) return rc;
        u32 *d_n = (u32 *)(ctl + SR_CTL_N);
        r->h_n = (uint32_t)n;
        HIP_TRY(c, hipMemcpyAsync(d_n, &r->h_n, 4, hipMemcpyHostToDevice, st));
        // (the passes leave key[0] permuted: a call repeated after PJB_ERR_NOMEM goes on with the order it has)
        if (!r->ordered && (rc = r->wide ? sort_u64_pairs(c, r->sort, d_n, n, r->key_bits, &r->order_in) : sort_u32_pairs(c, r->sort, d_n, n, r->key_bits, &r->order_in)))
            return rc;
        r->ordered = true;
        order = (const iu32 *)r->sort.idx[r->order_in].p;
    }
    if ((rc = ensure(c, r->dst, n * 8))) return rc;
    if ((rc = run_scan(c, "sr_off", MgSizeFn{(const iu32 *)r->size.p, order}, MgOffsetSink{(iu64 *)r->dst.p}, n, (u64 *)(ctl + SR_CTL_TOTAL)))) return rc;
    iu64 raw = 0;
    HIP_TRY(c, hipMemcpyAsync(&raw, ctl + SR_CTL_TOTAL, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if ((rc = ensure_cat(c, r->stream, (size_t)raw + 64, MEM_STAGING))) return rc;
    LAUNCH(c, "mg_gather", mg_gather, dim3((unsigned)((n + 3) / 4)), dim3(256), (const iu64 *)r->src.p, (const iu32 *)r->size.p, order, (const iu64 *)r->dst.p, (iu64)n,
           (uint8_t *)r->stream.p);
    rc = deflate_launches(c, nullptr, (const uint8_t *)r->stream.p, (int64_t)raw, block_bytes, [&](int64_t, const std::vector<u32> &sizes, iu64 total, uint8_t *&dst) {
        const size_t had = r->r_members.size();
        r->r_size.insert(r->r_size.end(), sizes.begin(), sizes.end());
        r->r_members.resize(had + (size_t)total);
        dst = r->r_members.data() + had;
        return (int)PJB_OK;
    });
    if (rc) {
        r->r_size.clear();
        r->r_members.clear();
        return rc;
    }
    out->n_records = (int64_t)n;
    out->raw_bytes = (int64_t)raw;
    out->n_unplaced = r->n_unplaced;
    return PJB_OK;
}

extern "C" int pjb_bam_sort_end(pjb_ctx *c, int32_t block_bytes, pjb_bam_sort_result *out) {
    if (!c) return PJB_ERR_ARG;
    SortRun *r = c->sort_run;
    if (!r || !r->active) return fail(c, PJB_ERR_STATE, "bam_sort_end: no run is open (pjb_bam_sort_begin)");
    r->keep_on_error = false;
    if (!out) return sort_leave(c, r, fail(c, PJB_ERR_ARG, "bam_sort_end: bad arguments"));
    if (block_bytes < 4 || block_bytes > (int32_t)DFL_IN_MAX || (block_bytes & 3))
        return sort_leave(c, r, fail(c, PJB_ERR_ARG, "bam_sort_end: block_bytes must be a multiple of 4 between 4 and %u", DFL_IN_MAX));
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    memset(out, 0, sizeof *out);
    const int rc = sort_leave(c, r, sort_end_body(c, r, block_bytes, out));
    if (rc) return rc;
    r->active = false;
    (void)hipStreamSynchronize(c->stream);
    sort_drop_pieces(c, r); // (the stream has been copied out: the run's inflated bytes make room for the next run's)
    out->n_members = (int32_t)r->r_size.size();
    out->member_size = r->r_size.data();
    out->members = r->r_members.data();
    out->member_bytes = (int64_t)r->r_members.size();
    return PJB_OK;
}
