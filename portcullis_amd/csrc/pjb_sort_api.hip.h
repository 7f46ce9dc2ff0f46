// pjb_sort_api.hip.h -- an unsorted file's records in coordinate order, run by run: pjb_bam_sort_begin / _piece / _end (see the ABI header);
// sr_keys and mg_gather in pjb_merge.hip.h, the sort passes in pjb_api.hip (sort_u32_pairs / sort_u64_pairs).  Host code only, included by
// pjb_ingest_api.hip behind its shared drivers (piece_records, MemberWriter, op_leave) and by nothing else.
#pragma once

struct SortRun : PieceOp {           // (keep_on_error: the failing piece call left the run as it was)
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
    Buf ref_len, ctl;                // i32[n_ref] | SR_CTL_*
    MemberWriter w;                  // the sorted stream and the result
    uint32_t h_n = 0;                // (copied to the device asynchronously)
    void drop_pieces(pjb_ctx *c) {
        for (Buf &b : pieces) release(c, b);
        pieces.clear();
    }
    void release_all(pjb_ctx *c) { // (a device buffer added above is added here)
        drop_pieces(c);
        sort.release_all(c);
        w.release_all(c);
        for (Buf *b : {&size, &src, &ref_len, &ctl}) release(c, *b);
    }
};

// what a failing call leaves: nothing to go on with, and no piece held, except after PJB_ERR_NOMEM and a first record longer than its piece
static int sort_leave(pjb_ctx *c, SortRun *r, int rc) {
    if (op_leave(c, r, rc, true) && !r->active) r->drop_pieces(c);
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
    r->drop_pieces(c);
    r->n = 0;
    r->n_unplaced = 0;
    r->prev = 0;
    r->descent = ~0ull;
    r->ordered = false;
    r->w.clear_result();
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
    PieceRecords P;
    int rc = piece_records(c, "bam_sort_piece", comp, comp_bytes, first_uoffset, last, out, MEM_STAGING, r->n,
                           "bam_sort_piece: 2^32 - 256 alignments or more in one run are not supported", P);
    if (rc) return rc;
    const std::vector<InfBlock> &blocks = P.blocks;
    const size_t nb = blocks.size(), n = P.n;
    // inflated byte u of the piece as (offset of its block in the piece) << 16 | offset in the block; the end of the data: the piece's end
    auto voffset_of = [&](iu64 u) -> uint64_t {
        if (u >= (iu64)P.total) return (uint64_t)comp_bytes << 16;
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
    if (P.end == PIECE_CUT_AT_EOF)
        return fail(c, PJB_ERR_BGZF, "the data ends inside an alignment record (inflated offset %llu of the last piece): truncated file", (unsigned long long)P.next_u);
    if (P.end == PIECE_RECORD_TOO_LONG) { // nothing was taken and nothing changed: the caller may hand the same blocks over again with more behind them
        r->keep_on_error = true;
        if (next_voffset) *next_voffset = voffset_of(P.next_u);
        return fail(c, PJB_ERR_ARG, "bam_sort_piece: the alignment record at inflated offset %llu is longer than the piece (%lld bytes): hand over more blocks at once",
                    (unsigned long long)P.next_u, (long long)comp_bytes);
    }
    hipStream_t st = c->stream;
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
    if (next_voffset) *next_voffset = voffset_of(P.next_u);
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
    if ((rc = write_members(c, r->w, (const iu32 *)r->size.p, (const iu64 *)r->src.p, order, n, "sr_off", (u64 *)(ctl + SR_CTL_TOTAL), block_bytes, &out->raw_bytes))) return rc;
    out->n_records = (int64_t)n;
    out->n_unplaced = r->n_unplaced;
    return PJB_OK;
}

extern "C" int pjb_bam_sort_end(pjb_ctx *c, int32_t block_bytes, pjb_bam_sort_result *out) {
    if (!c) return PJB_ERR_ARG;
    SortRun *r = c->sort_run;
    if (!r || !r->active) return fail(c, PJB_ERR_STATE, "bam_sort_end: no run is open (pjb_bam_sort_begin)");
    r->keep_on_error = false;
    if (!out) return sort_leave(c, r, fail(c, PJB_ERR_ARG, "bam_sort_end: bad arguments"));
    if (int rc = MemberWriter::check_block_bytes(c, "bam_sort_end", block_bytes)) return sort_leave(c, r, rc);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    memset(out, 0, sizeof *out);
    const int rc = sort_leave(c, r, sort_end_body(c, r, block_bytes, out));
    if (rc) return rc;
    r->active = false;
    (void)hipStreamSynchronize(c->stream);
    r->drop_pieces(c); // (the stream has been copied out: the run's inflated bytes make room for the next run's)
    r->w.result_to(out);
    return PJB_OK;
}
