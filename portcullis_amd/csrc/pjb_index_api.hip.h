// pjb_index_api.hip.h -- the BAM index of a sorted file, piece by piece, as a BAI or a CSI: pjb_csi_depth, pjb_index_begin / _begin_csi /
// _piece / _end / _end_csi (see the ABI header); kernels in pjb_index.hip.h.  Host code only, included by pjb_ingest_api.hip behind its
// shared drivers (piece_records, op_leave, op_clear) and by nothing else.
#pragma once

struct IndexState : PieceOp {     // (keep_on_error: the failing piece call left the index as it was)
    bool saw_last = false;
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
    void release_all(pjb_ctx *c) { // (a device buffer added above is added here)
        for (Buf *b : {&chunks, &lin, &ref_len, &lin_off, &key, &vs, &win, &w0, &heads, &tab, &ctl, &tile_max, &q[0], &q[1], &q[2], &q[3], &tid_start, &sorted, &loff})
            release(c, *b);
    }
    // the result
    std::vector<pjb_index_chunk> r_chunks;
    std::vector<int64_t> r_lin_off;
    std::vector<uint64_t> r_lin;
    std::vector<uint64_t> r_loff;
};
static_assert(sizeof(BaiChunk) == sizeof(pjb_index_chunk) && sizeof(pjb_index_chunk) == 24, "chunk layout");

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
    PieceRecords P;
    int rc = piece_records(c, "index_piece", comp, comp_bytes, first_uoffset, last, c->b_inf_out, MEM_SCRATCH, 0,
                           "index_piece: more than 2^32 alignments in one piece are not supported", P);
    if (rc) return rc;
    // block starts: inflated offset | file offset, + the sentinel "end of the data, the file's next block"
    const std::vector<InfBlock> &blocks = P.blocks;
    const size_t nb = blocks.size(), n = P.n;
    std::vector<iu64> tab(2 * (nb + 1));
    {
        int64_t off = 0;
        for (size_t b = 0; b < nb; b++) {
            tab[b] = blocks[b].out_off;
            tab[nb + 1 + b] = (iu64)(file_offset + off);
            off = (int64_t)blocks[b].in_off + blocks[b].in_len + 8; // (the payload, CRC32 and ISIZE: the next block's first byte)
        }
        tab[nb] = (iu64)P.total;
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
    const uint64_t nv = voffset_of(P.next_u);
    if (P.end == PIECE_CUT_AT_EOF) return fail(c, PJB_ERR_BGZF, "the data ends inside an alignment record (virtual offset 0x%llx): truncated file", (unsigned long long)nv);
    if (P.end == PIECE_RECORD_TOO_LONG) { // nothing was indexed and nothing changed: the caller may hand the same blocks over again with more behind them
        x->keep_on_error = true;
        if (next_voffset) *next_voffset = nv;
        return fail(c, PJB_ERR_ARG, "index_piece: the alignment record at virtual offset 0x%llx is longer than the piece (%lld bytes): hand over more blocks at once",
                    (unsigned long long)nv, (long long)comp_bytes);
    }
    hipStream_t st = c->stream;
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
    // the index is dropped by whatever fails, out of memory included: begin again
    return op_leave(c, x, index_piece_body(c, x, comp, comp_bytes, file_offset, first_uoffset, last, next_voffset), false);
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
