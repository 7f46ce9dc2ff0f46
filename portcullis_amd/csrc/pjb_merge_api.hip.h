// pjb_merge_api.hip.h -- several sorted files' records of one target as one stream: pjb_bam_merge_begin / _file / _end (see the ABI header);
// kernels in pjb_merge.hip.h, the sort passes in pjb_api.hip (sort_u32_pairs).  Host code only, included by pjb_ingest_api.hip behind its
// shared drivers (upload_padded, inflate_into, MemberWriter, op_leave) and by nothing else.
#pragma once

struct MergeFile {
    bool given = false;
    size_t n = 0;       // its records on the target
    Buf out;            // its inflated bytes, 64 zeroed bytes behind them
    Buf key, size, src; // per record: pos | 4 + block_size | where it lies in `out`
    void release_all(pjb_ctx *c) { for (Buf *b : {&out, &key, &size, &src}) release(c, *b); }
};
struct MergeState : PieceOp {
    int32_t tid = -1;
    std::vector<MergeFile> files;
    SortU32 sort;       // all files' keys, file after file, and what the passes need
    Buf size, src;      // all files' sizes and places
    Buf ctl;            // MG_CTL_* and the passes' record count
    MemberWriter w;     // the merged stream and the result
    uint32_t h_n = 0;   // (copied to the device asynchronously)
    void release_all(pjb_ctx *c) { // (a device buffer added above is added here)
        for (MergeFile &f : files) f.release_all(c);
        sort.release_all(c);
        w.release_all(c);
        for (Buf *b : {&size, &src, &ctl}) release(c, *b);
    }
};

// what a failing call leaves: nothing to go on with, except after PJB_ERR_NOMEM (the call can be repeated)
static int merge_leave(pjb_ctx *c, MergeState *m, int rc) { return op_leave(c, m, rc, true); }

extern "C" int pjb_bam_merge_begin(pjb_ctx *c, int32_t tid, int32_t n_files) {
    if (!c) return PJB_ERR_ARG;
    if (c->merge) c->merge->active = false;
    if (tid < 0 || (size_t)tid >= c->ref_len.size() || n_files < 1) return fail(c, PJB_ERR_ARG, "bam_merge_begin: bad arguments (tid %d, %d files)", tid, n_files);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (!c->merge) c->merge = new (std::nothrow) MergeState();
    MergeState *m = c->merge;
    if (!m) return fail(c, PJB_ERR_NOMEM, "bam_merge_begin: out of host memory");
    for (size_t k = (size_t)n_files; k < m->files.size(); k++) m->files[k].release_all(c);
    m->files.resize((size_t)n_files);
    for (MergeFile &f : m->files) {
        f.given = false;
        f.n = 0;
    }
    m->w.clear_result();
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
    if ((rc = upload_padded(c, comp, comp_bytes)) || (rc = inflate_into(c, (const uint8_t *)c->b_inf_comp.p, blocks, total, f.out, MEM_STAGING))) return rc;
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
    if ((rc = write_members(c, m->w, size, src, order, n, "mg_off", (u64 *)(ctl + MG_CTL_TOTAL), block_bytes, &out->raw_bytes))) return rc;
    out->n_records = (int64_t)n;
    return PJB_OK;
}

extern "C" int pjb_bam_merge_end(pjb_ctx *c, int32_t block_bytes, pjb_bam_merge_result *out) {
    if (!c) return PJB_ERR_ARG;
    MergeState *m = c->merge;
    if (!m || !m->active) return fail(c, PJB_ERR_STATE, "bam_merge_end: no merge is open (pjb_bam_merge_begin)");
    if (!out) return merge_leave(c, m, fail(c, PJB_ERR_ARG, "bam_merge_end: bad arguments"));
    if (int rc = MemberWriter::check_block_bytes(c, "bam_merge_end", block_bytes)) return merge_leave(c, m, rc);
    c->cur_tid = m->tid;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    memset(out, 0, sizeof *out);
    const int rc = merge_leave(c, m, merge_end_body(c, m, block_bytes, out));
    if (rc) return rc;
    m->active = false;
    m->w.result_to(out);
    return PJB_OK;
}
