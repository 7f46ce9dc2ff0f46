// pjb_extra_api.hip -- the part of the C ABI behind `junc --extra` (depth, flanking counts, name multiplicities: pjb_extra_finish), `bamfilt`
// (pjb_filter_*); kernels in pjb_extra.hip.h.
#include "pjb_host.hip.h"
#include "pjb_extra.hip.h"

// The name codes of a chain's spliced records, in BAM order, to `codes`; their number to cnt->n_spliced.  Through the tile lists the
// chain's first kernels left in its slot (tile numbers run through the chain).
static int spliced_codes(pjb_ctx *c, const Flight &f, ExtraCounters *cnt, u64 *codes) {
    CtlSlot &S = c->sl[f.slot];
    u32 n_tiles = 0;
    for (auto &b : f.batches) n_tiles = std::max<u32>(n_tiles, b.tile_base + (u32)((b.n + K1_TILE - 1) / K1_TILE));
    int rc;
    if ((rc = ensure(c, c->x_tileoff, (size_t)n_tiles * 4 + 16))) return rc;
    LAUNCH(c, "kx_spliced_offsets", kx_spliced_offsets, dim3(1), dim3(1024), (const TileStats *)S.tile_stats.p, n_tiles, (u32 *)c->x_tileoff.p, cnt);
    for (auto &b : f.batches)
        LAUNCH(c, "kx_spliced_codes", kx_spliced_codes, dim3((unsigned)((b.n + K1_TILE - 1) / K1_TILE)), dim3(256), b, (const TileStats *)S.tile_stats.p,
               (const u32 *)S.splidx.p, (const u32 *)c->x_tileoff.p, codes);
    return PJB_OK;
}

// a lone target through the depth vector (the dense path of pjb_extra.hip.h)
static int extra_contig_dense(pjb_ctx *c, Flight &f, u64 n_spliced, u32 P, u32 J, size_t row_base, bool codes_in_table) {
    hipStream_t st = c->stream;
    const int32_t tid = f.tid;
    std::vector<DevBatch> &batches = f.batches;
    const int32_t L = c->ref_len[(size_t)tid];
    const size_t N = (size_t)f.n_reads;
    ExtraContig X;
    X.dense = true;
    X.codes_in_table = codes_in_table;
    X.tid = tid;
    X.len = L;
    X.row_base = row_base;
    X.n_rows = J;
    X.n_pairs = P;
    int rc;
    if ((rc = ensure(c, c->b_xtotal, 8))) return rc;
    if ((rc = ensure(c, c->x_pos, N * 4 + 16))) return rc;
    if ((rc = ensure(c, c->x_endx, N * 4 + 16))) return rc;
    if ((rc = ensure(c, c->x_q, N + 16))) return rc;
    if ((rc = ensure(c, c->x_prefq, (N + 1) * 4))) return rc;
    if ((rc = ensure(c, c->x_ce, ((size_t)L + 2) * 4))) return rc;
    if ((rc = ensure(c, c->x_zlist, (size_t)X_ZCAP * 4))) return rc;
    if ((rc = ensure(c, c->x_cnt, sizeof(ExtraCounters)))) return rc;
    struct Guard { // frees what this contig allocated unless it is handed over to the context
        pjb_ctx *c;
        ExtraContig *x;
        ~Guard() {
            if (!x) return;
            (void)dev_free(c, x->cover);
            (void)dev_free(c, x->xr);
            (void)dev_free(c, x->pair_code);
            (void)dev_free(c, x->pair_row);
            (void)dev_free(c, x->spl_codes);
        }
    } guard{c, &X};
    if (!(X.cover = (u32 *)dev_alloc(c, MEM_OTHER, ((size_t)L + 2) * 4))) return nomem(c, "extra: depth array", ((size_t)L + 2) * 4);
    if (!(X.spl_codes = (u64 *)dev_alloc(c, MEM_OTHER, std::max<size_t>((size_t)n_spliced, 1) * 8)))
        return nomem(c, "extra: name codes", std::max<size_t>((size_t)n_spliced, 1) * 8);
    HIP_TRY(c, hipMemsetAsync(X.cover, 0, ((size_t)L + 2) * 4, st));
    HIP_TRY(c, hipMemsetAsync(c->x_ce.p, 0, ((size_t)L + 2) * 4, st));
    HIP_TRY(c, hipMemsetAsync((uint8_t *)c->x_q.p + N, 0, 1, st));
    ExtraCounters hc;
    memset(&hc, 0, sizeof hc);
    hc.hot_first = 0xffffffffu;
    HIP_TRY(c, hipMemcpyAsync(c->x_cnt.p, &hc, sizeof hc, hipMemcpyHostToDevice, st));
    ExtraCounters *d_cnt = (ExtraCounters *)c->x_cnt.p;
    int32_t *x_pos = (int32_t *)c->x_pos.p, *x_endx = (int32_t *)c->x_endx.p;
    uint8_t *x_q = (uint8_t *)c->x_q.p;
    u32 *prefq = (u32 *)c->x_prefq.p, *ce = (u32 *)c->x_ce.p;
    for (auto &b : batches)
        LAUNCH(c, "kx_classify", kx_classify, dim3((unsigned)((b.n + 255) / 256)), dim3(256), b, L, x_pos, x_endx, x_q, ce,
               (int32_t *)X.cover, (u32 *)c->x_zlist.p, X_ZCAP, d_cnt);
    if ((rc = spliced_codes(c, f, d_cnt, X.spl_codes))) return rc;
    if ((rc = run_scan(c, "kx_ends", ArrU32Fn{ce}, ExclusiveU32Sink{ce}, (u64)L + 2, (u64 *)c->b_xtotal.p))) return rc;
    if ((rc = run_scan(c, "kx_unspl", ArrU8Bit0Fn{x_q}, ExclusiveU32Sink{prefq}, (u64)N + 1, (u64 *)c->b_xtotal.p))) return rc;
    LAUNCH(c, "kx_cap_bound", kx_cap_bound, dim3((unsigned)((N + 255) / 256)), dim3(256), (const int32_t *)x_pos, (const uint8_t *)x_q,
           (const u32 *)prefq, (const u32 *)ce, (u32)N, L, (u32 *)nullptr, d_cnt);
    u32 n_unspl = 0;
    HIP_TRY(c, hipMemcpyAsync(&hc, d_cnt, sizeof hc, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&n_unspl, prefq + N, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (hc.n_zero > X_ZCAP)
        return fail(c, PJB_ERR_ARG, "extra: target %d has %u mapped records without a reference span (limit %u)", tid, hc.n_zero, X_ZCAP);
    if (hc.max_buffered + hc.n_zero + 2 > PLP_MAXCNT) { // the pileup's record cap may bite: replay it over the hot span
        if ((rc = ensure(c, c->x_bound, N * 4 + 16))) return rc;
        if ((rc = ensure(c, c->x_de, ((size_t)L + 2) * 4))) return rc;
        if ((rc = ensure(c, c->x_dropped, N + 16))) return rc;
        HIP_TRY(c, hipMemsetAsync(c->x_de.p, 0, ((size_t)L + 2) * 4, st));
        HIP_TRY(c, hipMemsetAsync(c->x_dropped.p, 0, N + 16, st));
        LAUNCH(c, "kx_cap_bound", kx_cap_bound, dim3((unsigned)((N + 255) / 256)), dim3(256), (const int32_t *)x_pos,
               (const uint8_t *)x_q, (const u32 *)prefq, (const u32 *)ce, (u32)N, L, (u32 *)c->x_bound.p, d_cnt);
        LAUNCH(c, "kx_cap_replay", kx_cap_replay, dim3(1), dim3(64), (const int32_t *)x_pos, (const int32_t *)x_endx, (const uint8_t *)x_q,
               (const u32 *)c->x_bound.p, (u32)N, L, (u32 *)c->x_de.p, (uint8_t *)c->x_dropped.p, d_cnt);
        for (auto &b : batches)
            LAUNCH(c, "kx_undo_dropped", kx_undo_dropped, dim3((unsigned)((b.n + 255) / 256)), dim3(256), b, L,
                   (const uint8_t *)c->x_dropped.p, (int32_t *)X.cover);
    }
    if ((rc = run_scan(c, "kx_depth", ArrI32Fn{(const int32_t *)X.cover}, InclusiveU32Sink{X.cover}, (u64)L + 1, (u64 *)c->b_xtotal.p)))
        return rc;
    X.has_unspliced = n_unspl > 0;
    X.n_spl = hc.n_spliced;
    if (J > 0) {
        if (!(X.xr = (ExtraRow *)dev_alloc(c, MEM_OTHER, (size_t)J * sizeof(ExtraRow)))) return nomem(c, "extra: rows", (size_t)J * sizeof(ExtraRow));
        HIP_TRY(c, hipMemsetAsync(X.xr, 0, (size_t)J * sizeof(ExtraRow), st));
        LAUNCH(c, "kx_flank", kx_flank, dim3((J + 255) / 256), dim3(256), (const pjb_junction_row *)c->sl[f.slot].rows.p, J, (const int32_t *)x_pos,
               (u32)N, (const u32 *)prefq, (const u32 *)ce, L, (const u32 *)c->x_zlist.p, (const ExtraCounters *)d_cnt, X_ZCAP, X.xr);
        if (!(X.pair_code = (u64 *)dev_alloc(c, MEM_OTHER, (size_t)P * 8)) || !(X.pair_row = (u32 *)dev_alloc(c, MEM_OTHER, (size_t)P * 4)))
            return nomem(c, "extra: pair codes", (size_t)P * 12);
        LAUNCH(c, "kx_pair_codes", kx_pair_codes, dim3((P + 255) / 256), dim3(256), f.sidx, f.jid_sorted, f.pr.g,
               (const DevBatch *)c->sl[f.slot].batches.p, (int)batches.size(), P, (u32)row_base, X.pair_code, X.pair_row);
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    c->xc.push_back(X);
    guard.x = nullptr;
    return PJB_OK;
}

#define XTRACE(what)                                                                                                              \
    do {                                                                                                                          \
        if (xtrace) {                                                                                                             \
            (void)hipStreamSynchronize(st);                                                                                       \
            const auto now_ = std::chrono::steady_clock::now();                                                                   \
            fprintf(stderr, "[xtrace] %-28s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now_ - xt0).count());     \
            xt0 = now_;                                                                                                           \
        }                                                                                                                         \
    } while (0)
// room in the name table for `add` more codes (load <= 1/2): a larger table takes over the old one's names
static int name_table_reserve(pjb_ctx *c, size_t add) {
    hipStream_t st = c->stream;
    const size_t need = (c->x_tab_n + add) + (c->x_tab_n + add) / 2 + 1; // load <= 2/3
    if (c->x_tab_n == 0 && c->x_tab_slots >= need) { // first codes of a file: wipe
        if (add) HIP_TRY(c, hipMemsetAsync(c->x_tab.p, 0xff, c->x_tab_slots * sizeof(NameSlot), st));
        return PJB_OK;
    }
    if (c->x_tab_slots >= need) return PJB_OK;
    if (need > 0xfffffff0ull) return fail(c, PJB_ERR_ARG, "extra: more than 2^31 spliced records");
    const size_t slots = std::min<size_t>(std::max<size_t>(2 * need + 16, 1024), 0xfffffff0ull); // (twice what is needed now: a file's targets arrive one by one)
    Buf nb;
    int rc = ensure(c, nb, slots * sizeof(NameSlot));
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(nb.p, 0xff, slots * sizeof(NameSlot), st));
    if (c->x_tab_n)
        LAUNCH(c, "kx_name_rehash", kx_name_rehash, dim3((unsigned)((c->x_tab_slots + 255) / 256)), dim3(256), (const NameSlot *)c->x_tab.p,
               (u32)c->x_tab_slots, (NameSlot *)nb.p, (u32)slots);
    if (c->x_tab.p) {
        HIP_TRY(c, hipStreamSynchronize(st));
        release(c, c->x_tab);
    }
    c->x_tab = nb;
    c->x_tab_slots = slots;
    return PJB_OK;
}
static int name_table_insert(pjb_ctx *c, const u64 *codes, u32 n) {
    if (!n) return PJB_OK;
    int rc = name_table_reserve(c, n);
    if (rc) return rc;
    LAUNCH(c, "kx_name_insert", kx_name_insert4, dim3((n + 1023) / 1024), dim3(256), codes, n, (NameSlot *)c->x_tab.p, (u32)c->x_tab_slots);
    c->x_tab_n += n;
    return PJB_OK;
}

// The same work without an array of the target's length (pjb_extra.hip.h, "the sparse path"), in two parts, for a CHAIN: a lone
// target, or a group of targets finished as one chain -- one such target in the coordinates of its virtual sequence (members_of; a lone
// target is the chain of one member at offset 0).  extra_pre needs the records only: queued on the service stream when the chain is
// queued, it runs beside the chains.  extra_contig needs the chain's rows and sorted pairs: queued when the chain is collected, beside
// the chains queued after this one; one wait at its end.  The launches depend on the number of batches, not on the number of members.
//   Where the sparse answer does not stand (SparseCounters::need_dense) a lone target goes through extra_contig_dense instead; a group
// (extra_group_apart) is taken apart by its caller, and its members come back here one by one.
static XMembers members_of(const pjb_ctx *c, const Flight &f) {
    XMembers M;
    memset(&M, 0, sizeof M);
    M.n = (int32_t)f.tids.size();
    for (size_t m = 0; m < f.tids.size(); m++) {
        M.tid[m] = f.tids[m];
        M.voff[m] = f.voff[m];
        M.len[m] = c->ref_len[(size_t)f.tids[m]];
    }
    return M;
}
int extra_pre(pjb_ctx *c, Flight &f) {
    if (f.x_pre || c->extra_dense_only || f.empty) return PJB_OK;
    hipStream_t st = c->stream;
    CtlSlot &S = c->sl[f.slot];
    const size_t N = (size_t)f.n_reads;
    const bool group = f.tids.size() > 1;
    int rc;
    f.x_gap_cap = (u32)std::min<size_t>(N / 16 + 1024, 0x7fffffffu);
    f.x_spos = (int32_t *)xarena_alloc(c, N * 4 + 16); // (compacted: the records with a span)
    f.x_send = (int32_t *)xarena_alloc(c, N * 4 + 16);
    f.x_gapoff = (u32 *)xarena_alloc(c, (N / 256 + 2) * 4);
    f.x_gaps = (Gap *)xarena_alloc(c, (size_t)f.x_gap_cap * sizeof(Gap));
    if (!f.x_spos || !f.x_send || !f.x_gapoff || !f.x_gaps)
        return fail(c, PJB_ERR_NOMEM, "extra: no device memory for what target %d keeps (%zu records)", f.tid, N);
    if ((rc = ensure(c, S.x_q, N + 16)) || (rc = ensure(c, S.x_spos, N * 4 + 16)) || (rc = ensure(c, S.x_send, N * 4 + 16)) ||
        (rc = ensure(c, S.x_gapoff, (N / 256 + 2) * 4)) || (rc = ensure(c, S.x_zlist, (size_t)X_ZCAP * 8)) ||
        (rc = ensure(c, S.x_scnt, X_SCNT_BYTES)))
        return rc;
    uint8_t *q = (uint8_t *)S.x_q.p;
    SparseCounters *d_cnt = (SparseCounters *)S.x_scnt.p;
    if (f.x_k1) HIP_TRY(c, hipStreamWaitEvent(st, S.ev_xk1, 0)); // (the chain's k1_count classified the records)
    else {
        // Only a group comes here.  queue_chain calls queue_contig first, and queue_contig has k1_count classify the records of every lone
        // target of a context that gets this far (no "extra_dense") the first time its chain is queued: x_k1 is set, a repeat keeps it, and
        // the members of a group that came apart are fresh flights that go through queue_contig like any other.
        const XOut xo{(int32_t *)S.x_spos.p, (int32_t *)S.x_send.p, q, (u32 *)S.x_zlist.p, X_ZCAP, d_cnt};
        HIP_TRY(c, hipMemsetAsync(q + N, 0, 1, st));
        HIP_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(SparseCounters) + sizeof(ExtraCounters), st));
        for (auto &b : f.batches)
            if (b.n > 0)
                LAUNCH(c, "kx_classify_sparse", kx_classify_sparse, dim3((unsigned)((b.n + 255) / 256)), dim3(256), b, f.voff[(size_t)b.member],
                       c->ref_len[(size_t)f.tids[(size_t)b.member]], group, xo);
    }
    if ((rc = run_scan(c, "kx_spans", SparseFn{q},
                       SparseSink{f.x_spos, f.x_send, (u32 *)S.x_gapoff.p, f.x_gapoff, (const int32_t *)S.x_spos.p, (const int32_t *)S.x_send.p, q}, (u64)N + 1,
                       &d_cnt->total)))
        return rc;
    for (auto &b : f.batches)
        if (b.n > 0)
        {
            const u32 nblk = (u32)((((u64)b.base + (u64)b.n + 255) >> 8) - (b.base >> 8));
            LAUNCH(c, "kx_gaps", kx_gaps, dim3(std::min<u32>(nblk, 2048)), dim3(256), b, f.voff[(size_t)b.member], (const uint8_t *)q, (u32)N,
                   (const u32 *)S.x_gapoff.p, f.x_gaps, f.x_gap_cap, d_cnt, nblk);
        }
    if (N >= PLP_MAXCNT)
        LAUNCH(c, "kx_cap_check", kx_cap_check, dim3((unsigned)((N + 255) / 256)), dim3(256), (const int32_t *)f.x_spos, d_cnt);
    if (group) // (which members have records with a span; a lone target has if there are any: extra_contig)
        LAUNCH(c, "kx_member_spans", kx_member_spans, dim3(1), dim3(64), (const int32_t *)f.x_spos, (const SparseCounters *)d_cnt, members_of(c, f),
               (GroupCounters *)((uint8_t *)S.x_scnt.p + sizeof(SparseCounters) + sizeof(ExtraCounters)));
    f.x_pre = true;
    return PJB_OK;
}

// Does the sparse answer stand for the group in fl[0]?  Asked when its chain has completed and BEFORE anything of the group is
// committed (name table, c->xc, rows): *apart is set when a member needs the depth vector -- the pileup's cap may bite (a false alarm
// where two members' records lie within max_span of each other in virtual coordinates only costs this), a record with more gaps than
// a byte counts, the gap list full -- or holds a record that leaves its sequence, or when the group has more records without a span than
// the list holds.  The members then go one by one through the path of a target finished alone, which decides for each of them.
int extra_group_apart(pjb_ctx *c, Flight &f, bool *apart) {
    *apart = false;
    if (c->extra_dense_only || f.empty) return PJB_OK;
    int rc;
    if ((rc = extra_pre(c, f))) return rc;
    CtlSlot &S = c->sl[f.slot];
    SparseCounters &hc = *(SparseCounters *)(S.pub + PUB_XCNT_AT);
    HIP_TRY(c, hipMemcpyAsync(&hc, S.x_scnt.p, sizeof(SparseCounters), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *apart = hc.need_dense != 0 || hc.n_zero > X_ZCAP;
    return PJB_OK;
}

// The rows part, once for the whole chain, and one ExtraContig per member -- the hand-over of the coverage in pjb_extra_finish goes
// target by target -- that share the chain's records.
int extra_contig(pjb_ctx *c, Flight &f, const pjb_region_result *res, u64 n_spliced, u32 P, u32 J, size_t row_base) {
    if (c->extra_dense_only) return extra_contig_dense(c, f, n_spliced, P, J, row_base, false); // (lone targets only: begin_flight)
    int rc;
    if ((rc = extra_pre(c, f))) return rc;
    hipStream_t st = c->stream;
    CtlSlot &S = c->sl[f.slot];
    const size_t n_members = f.tids.size();
    const bool lone = n_members == 1;
    const char *who = lone ? "target" : "the group from target";
    // rows and sorted pairs are in the order of the junction ids, member after member: how many each member holds (a lone target: all)
    std::vector<std::pair<size_t, u32>> share(n_members, std::make_pair((size_t)J, P));
    if (!lone) {
        u64 pairs = 0, juncs = 0;
        for (size_t m = 0; m < n_members; m++) {
            share[m] = std::make_pair((size_t)res[m].n_junctions, (u32)res[m].n_pairs);
            pairs += (u64)res[m].n_pairs, juncs += (u64)res[m].n_junctions;
        }
        if (pairs != P || juncs != J)
            return fail(c, PJB_ERR_STATE, "extra: the members of the group from target %d hold %llu pairs / %llu junctions, the chain %u / %u", f.tid,
                        (unsigned long long)pairs, (unsigned long long)juncs, P, J);
    }
    ExtraRow *xr = J ? (ExtraRow *)xarena_alloc(c, (size_t)J * sizeof(ExtraRow)) : nullptr;
    u64 *pair_code = J ? (u64 *)xarena_alloc(c, (size_t)P * 8 + 16) : nullptr;
    u32 *pair_row = J ? (u32 *)xarena_alloc(c, (size_t)P * 4 + 16) : nullptr;
    if (J && (!xr || !pair_code || !pair_row)) return fail(c, PJB_ERR_NOMEM, "extra: no device memory for the pairs of %s %d", who, f.tid);
    if ((rc = ensure(c, S.x_codes, std::max<size_t>((size_t)n_spliced, 1) * 8))) return rc;
    const bool xtrace = getenv("PJB_XTRACE") != nullptr;
    auto xt0 = std::chrono::steady_clock::now();
    XTRACE("post: pre-part done");
    SparseCounters *d_cnt = (SparseCounters *)S.x_scnt.p;
    // the spliced records' name codes -> the name table
    if ((rc = spliced_codes(c, f, (ExtraCounters *)(d_cnt + 1), (u64 *)S.x_codes.p))) return rc;
    XTRACE("post: codes");
    if ((rc = name_table_insert(c, (const u64 *)S.x_codes.p, (u32)n_spliced))) return rc;
    XTRACE("post: insert");
    if (J > 0) {
        HIP_TRY(c, hipMemsetAsync(xr, 0, (size_t)J * sizeof(ExtraRow), st));
        LAUNCH(c, "kx_flank_sparse", kx_flank_sparse, dim3((J + 255) / 256), dim3(256), (const pjb_junction_row *)S.rows.p, J, (const int32_t *)f.x_spos,
               (const int32_t *)f.x_send, members_of(c, f), (const u32 *)S.x_zlist.p, (const SparseCounters *)d_cnt, X_ZCAP, xr);
        LAUNCH(c, "kx_pair_codes", kx_pair_codes, dim3((P + 255) / 256), dim3(256), f.sidx, f.jid_sorted, f.pr.g, (const DevBatch *)S.batches.p,
               (int)f.batches.size(), P, (u32)row_base, pair_code, pair_row);
    }
    // one wait: the counters decide whether the sparse answer stands
    SparseCounters &hc = *(SparseCounters *)(S.pub + PUB_XCNT_AT);
    ExtraCounters &hx = *(ExtraCounters *)(S.pub + PUB_XCNT_AT + sizeof(SparseCounters));
    GroupCounters &hg = *(GroupCounters *)(S.pub + PUB_XCNT_AT + sizeof(SparseCounters) + sizeof(ExtraCounters));
    XTRACE("post: flank + pair codes");
    HIP_TRY(c, hipMemcpyAsync(&hc, d_cnt, X_SCNT_BYTES, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    XTRACE("post: counters");
    if (c->ktime) ev_collect(c, MISC_POOL);
    // What depends on the number of members, all of it here.  A lone target with more records without a span than the list holds is
    // refused, and one that needs the depth vector -- the pileup's cap may bite, or the gap list is too small -- gets it; for a group
    // extra_group_apart has said no to both before anything was committed.  Whether a member has unspliced records with a span: a lone
    // target has if the chain has any, a group's members were asked by kx_member_spans (extra_pre).
    if (lone && hc.n_zero > X_ZCAP)
        return fail(c, PJB_ERR_ARG, "extra: target %d has %u mapped records without a reference span (limit %u)", f.tid, hc.n_zero, X_ZCAP);
    if (hx.n_spliced != (u32)n_spliced)
        return fail(c, PJB_ERR_STATE, "extra: %s %d: %u spliced records in the tile lists, the chain counted %llu", who, f.tid, hx.n_spliced,
                    (unsigned long long)n_spliced);
    if (lone && hc.need_dense) return extra_contig_dense(c, f, n_spliced, P, J, row_base, true);
    if (hc.need_dense || hc.n_zero > X_ZCAP) return fail(c, PJB_ERR_STATE, "extra: the group from target %d needs the depth vector", f.tid);
    const u32 has_spans = lone ? ((u32)hc.total > 0 ? 1u : 0u) : hg.has_spans;
    const SparseDepth D{f.x_spos, f.x_send, f.x_gaps, f.x_gapoff, (u32)hc.total, (u32)(hc.total >> 32), hc.max_span, hc.max_gap};
    size_t row_at = 0, pair_at = 0;
    for (size_t m = 0; m < n_members; m++) {
        ExtraContig X;
        X.tid = f.tids[m];
        X.len = c->ref_len[(size_t)X.tid];
        X.voff = f.voff[m];
        X.row_base = row_base + row_at;
        X.n_rows = share[m].first;
        X.n_pairs = share[m].second;
        X.xr = X.n_rows ? xr + row_at : nullptr;
        X.pair_code = X.n_rows ? pair_code + pair_at : nullptr;
        X.pair_row = X.n_rows ? pair_row + pair_at : nullptr;
        X.codes_in_table = true;
        X.has_unspliced = (has_spans >> m) & 1u;
        X.sparse = D;
        row_at += X.n_rows;
        pair_at += X.n_pairs;
        c->xc.push_back(X);
    }
    return PJB_OK;
}

extern "C" {
int pjb_extra_finish(pjb_ctx *c, const pjb_extra_row **rows_out, int64_t *n_out) {
    if (!c || !rows_out || !n_out) return PJB_ERR_ARG;
    const bool xtrace = getenv("PJB_XTRACE") != nullptr;
    auto xt0 = std::chrono::steady_clock::now();
    if (!c->extra) return fail(c, PJB_ERR_STATE, "pjb_extra_finish: the context was not created with PJB_FLAG_EXTRA");
    if (!c->open.empty()) return fail(c, PJB_ERR_STATE, "pjb_extra_finish: target %d is still open", c->open.begin()->first);
    if (c->n_fl) return fail(c, PJB_ERR_STATE, "pjb_extra_finish: target %d is still queued", c->fl[0].tid);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    int rc;
    const size_t Jall = c->rows_n;
    *rows_out = c->xrows_pinned;
    *n_out = (int64_t)Jall;
    if (Jall == 0) return PJB_OK;
    if (Jall > c->xrows_pinned_cap) {
        if (c->xrows_pinned) (void)hipHostFree(c->xrows_pinned);
        c->xrows_pinned = nullptr;
        c->xrows_pinned_cap = 0;
        const size_t cap = Jall + Jall / 4 + 1024;
        HIP_TRY(c, hipHostMalloc((void **)&c->xrows_pinned, cap * sizeof(pjb_extra_row), hipHostMallocDefault));
        c->xrows_pinned_cap = cap;
    }
    *rows_out = c->xrows_pinned;
    // every target's flanking counts into one table, parallel to the row table in HBM (which the kernels below read)
    if ((rc = ensure(c, c->x_xrall, Jall * (sizeof(ExtraRow) + sizeof(pjb_extra_row))))) return rc;
    ExtraRow *xr = (ExtraRow *)c->x_xrall.p;
    pjb_extra_row *xout = (pjb_extra_row *)(xr + Jall);
    HIP_TRY(c, hipMemsetAsync(xr, 0, Jall * sizeof(ExtraRow), st));
    for (auto &x : c->xc)
        if (x.n_rows) HIP_TRY(c, hipMemcpyAsync(xr + x.row_base, x.xr, x.n_rows * sizeof(ExtraRow), hipMemcpyDeviceToDevice, st));
    XTRACE("finish: memset + copies");
    // ---- splicedAlignmentMap over every spliced record of the file (src/junction_builder.cc:168-176): the targets' codes went
    // into the table as the targets were collected (a target of the dense path: now)
    for (auto &x : c->xc)
        if (!x.codes_in_table) {
            if ((rc = name_table_insert(c, (const u64 *)x.spl_codes, x.n_spl))) return rc;
            x.codes_in_table = true;
        }
    if (c->x_tab_n)
        for (auto &x : c->xc)
            if (x.n_pairs && x.n_rows)
                LAUNCH(c, "kx_name_sum", kx_name_sum, dim3((x.n_pairs + 1023) / 1024), dim3(256), (const u64 *)x.pair_code, (const u32 *)x.pair_row,
                       x.n_pairs, (const NameSlot *)c->x_tab.p, (u32)c->x_tab_slots, xr);
    // ---- JunctionSystem::calcCoverage (lib/src/junction_system.cc:231-242).  DepthParser::loadNextBatch
    // (lib/src/depth_parser.cc:112-164) returns the vector of the target it started in, but by then `last`
    // names the target the pileup has moved on to, and getCurrentRefIndex() selects THAT target's junctions:
    // every batch is applied to the junctions of the next target that has unspliced records; only the final
    // batch (the pileup ended inside it) meets its own junctions, after they were first given the previous
    // target's.  Targets without unspliced records never appear.
    XTRACE("finish: name sums");
    std::vector<const ExtraContig *> T;
    for (auto &x : c->xc)
        if (x.has_unspliced) T.push_back(&x);
    std::sort(T.begin(), T.end(), [](const ExtraContig *a, const ExtraContig *b) { return a->tid < b->tid; });
    const pjb_junction_row *rows = c->rows_table;
    for (size_t k = 0; k < T.size(); k++) {
        const ExtraContig &x = *T[k];
        if (!x.n_rows) continue;
        const ExtraContig *src = (k + 1 == T.size()) ? &x : (k > 0 ? T[k - 1] : nullptr);
        if (!src) continue; // the first target's junctions are never visited (unless it is also the last)
        if (src->dense)
            LAUNCH(c, "kx_coverage", kx_coverage, dim3((unsigned)((x.n_rows + 255) / 256)), dim3(256), rows, (u32)x.row_base, (u32)x.n_rows,
                   (const u32 *)src->cover, src->len, xr);
        else
            LAUNCH(c, "kx_coverage_sparse", kx_coverage_sparse, dim3((unsigned)((x.n_rows + 255) / 256)), dim3(256), rows, (u32)x.row_base,
                   (u32)x.n_rows, src->sparse, src->len, src->voff, xr);
    }
    XTRACE("finish: coverage");
    LAUNCH(c, "kx_rows_out", kx_rows_out, dim3((unsigned)((Jall + 255) / 256)), dim3(256), rows, (const ExtraRow *)xr, (u32)Jall, xout);
    XTRACE("finish: rows_out");
    HIP_TRY(c, hipMemcpyAsync(c->xrows_pinned, xout, Jall * sizeof(pjb_extra_row), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    XTRACE("finish: D2H");
    if (c->ktime) ev_collect(c, MISC_POOL);
    return PJB_OK;
}

int pjb_filter_set_junctions(pjb_ctx *c, int32_t tid, const uint64_t *sorted_keys, int64_t n_keys) {
    if (!c) return PJB_ERR_ARG;
    if (tid < 0 || n_keys < 0 || n_keys > 0xfffffff0ll || (n_keys > 0 && !sorted_keys))
        return fail(c, PJB_ERR_ARG, "pjb_filter_set_junctions: bad arguments (tid %d)", tid);
    for (int64_t i = 1; i < n_keys; i++)
        if (sorted_keys[i - 1] >= sorted_keys[i]) return fail(c, PJB_ERR_ARG, "pjb_filter_set_junctions: keys must be strictly ascending");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    auto it = c->filter_keys.find(tid);
    if (it != c->filter_keys.end()) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (it->second.first) (void)dev_free(c, it->second.first);
        c->filter_keys.erase(it);
    }
    u64 *d = nullptr;
    if (n_keys) {
        if (!(d = (u64 *)dev_alloc(c, MEM_OTHER, (size_t)n_keys * 8))) return nomem(c, "pjb_filter_set_junctions", (size_t)n_keys * 8);
        hipError_t e = hipMemcpy(d, sorted_keys, (size_t)n_keys * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)dev_free(c, d);
            return fail(c, PJB_ERR_HIP, "pjb_filter_set_junctions: %s", hipGetErrorString(e));
        }
    }
    c->filter_keys[tid] = std::make_pair(d, (u32)n_keys);
    return PJB_OK;
}

int pjb_filter_batch(pjb_ctx *c, int32_t tid, const pjb_batch *b, int32_t clip_mode, uint8_t *codes_out) {
    if (!c) return PJB_ERR_ARG;
    if (!b || b->n_reads < 0 || (b->n_reads > 0 && (!b->pos || !b->cig_off || !b->cigar || !codes_out)))
        return fail(c, PJB_ERR_ARG, "pjb_filter_batch: bad batch");
    if (clip_mode < PJB_CLIP_HARD || clip_mode > PJB_CLIP_COMPLETE) return fail(c, PJB_ERR_ARG, "pjb_filter_batch: bad clip mode %d", clip_mode);
    if (b->n_reads == 0) return PJB_OK;
    if (b->n_reads > 0xfffffff0ll) return fail(c, PJB_ERR_ARG, "pjb_filter_batch: batch too large");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)b->n_reads, n_ops = b->cig_off[n];
    int rc;
    if ((rc = ensure(c, c->f_pos, n * 4))) return rc;
    if ((rc = ensure(c, c->f_cigoff, (n + 1) * 4))) return rc;
    if ((rc = ensure(c, c->f_cigar, n_ops * 4 + 16))) return rc;
    if ((rc = ensure(c, c->f_codes, n + 16))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->f_pos.p, b->pos, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->f_cigoff.p, b->cig_off, (n + 1) * 4, hipMemcpyHostToDevice, st));
    if (n_ops) HIP_TRY(c, hipMemcpyAsync(c->f_cigar.p, b->cigar, n_ops * 4, hipMemcpyHostToDevice, st));
    const u64 *keys = nullptr;
    u32 n_keys = 0;
    auto it = c->filter_keys.find(tid);
    if (it != c->filter_keys.end()) {
        keys = it->second.first;
        n_keys = it->second.second;
    }
    LAUNCH(c, "kf_filter", kf_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), (const int32_t *)c->f_pos.p, (const u32 *)c->f_cigoff.p,
           (const u32 *)c->f_cigar.p, (u32)n, keys, n_keys, (int)clip_mode, (uint8_t *)c->f_codes.p);
    HIP_TRY(c, hipMemcpyAsync(codes_out, c->f_codes.p, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    return PJB_OK;
}

} // extern "C"
