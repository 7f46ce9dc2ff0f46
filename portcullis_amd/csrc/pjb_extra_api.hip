// pjb_extra_api.hip -- the part of the C ABI behind `junc --extra` (depth, flanking counts, name multiplicities: pjb_extra_finish), `bamfilt`
// (pjb_filter_*), `filt`'s feature rows and forest (pjb_filt_features, pjb_forest_*, pjb_filt_scores) and `train`'s growing of one
// (pjb_forest_grow) and self-training's nearest neighbours (pjb_knn); kernels in pjb_extra.hip.h, pjb_forest.hip.h, pjb_grow.hip.h
// and pjb_knn.hip.h.
#include "pjb_host.hip.h"
#include "pjb_extra.hip.h"
#include "pjb_forest.hip.h"
#include "pjb_grow.hip.h"
#include "pjb_knn.hip.h"

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
        ExtraContig *x;
        ~Guard() {
            if (!x) return;
            if (x->cover) (void)hipFree(x->cover);
            if (x->xr) (void)hipFree(x->xr);
            if (x->pair_code) (void)hipFree(x->pair_code);
            if (x->pair_row) (void)hipFree(x->pair_row);
            if (x->spl_codes) (void)hipFree(x->spl_codes);
        }
    } guard{&X};
    if (hipMalloc((void **)&X.cover, ((size_t)L + 2) * 4) != hipSuccess) return fail(c, PJB_ERR_NOMEM, "extra: depth array of target %d", tid);
    if (hipMalloc((void **)&X.spl_codes, std::max<size_t>((size_t)n_spliced, 1) * 8) != hipSuccess)
        return fail(c, PJB_ERR_NOMEM, "extra: name codes of target %d", tid);
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
    if ((rc = run_scan(c, "kx_unspl", ArrU8Fn{x_q}, ExclusiveU32Sink{prefq}, (u64)N + 1, (u64 *)c->b_xtotal.p))) return rc;
    LAUNCH(c, "kx_cap_bound", kx_cap_bound, dim3((unsigned)((N + 255) / 256)), dim3(256), (const int32_t *)x_pos, (const uint8_t *)x_q,
           (const u32 *)prefq, (const u32 *)ce, (u32)N, L, (u32 *)nullptr, d_cnt);
    u32 n_unspl = 0;
    HIP_TRY(c, hipMemcpyAsync(&hc, d_cnt, sizeof hc, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&n_unspl, prefq + N, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (hc.n_zero > X_ZCAP)
        return fail(c, PJB_ERR_ARG, "extra: target %d has %u mapped records without a reference span (limit %u)", tid, hc.n_zero, X_ZCAP);
    if (hc.max_buffered + 2 > PLP_MAXCNT) { // the pileup's record cap may bite: replay it over the hot span
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
        if (hipMalloc((void **)&X.xr, (size_t)J * sizeof(ExtraRow)) != hipSuccess) return fail(c, PJB_ERR_NOMEM, "extra: rows of target %d", tid);
        HIP_TRY(c, hipMemsetAsync(X.xr, 0, (size_t)J * sizeof(ExtraRow), st));
        LAUNCH(c, "kx_flank", kx_flank, dim3((J + 255) / 256), dim3(256), (const pjb_junction_row *)c->sl[f.slot].rows.p, J, (const int32_t *)x_pos,
               (u32)N, (const u32 *)prefq, (const u32 *)ce, L, (const u32 *)c->x_zlist.p, (const ExtraCounters *)d_cnt, X_ZCAP, X.xr);
        if (hipMalloc((void **)&X.pair_code, (size_t)P * 8) != hipSuccess || hipMalloc((void **)&X.pair_row, (size_t)P * 4) != hipSuccess)
            return fail(c, PJB_ERR_NOMEM, "extra: pair codes of target %d", tid);
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
        release(c->x_tab);
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

// The device work of one contig, queued in one go.  The host does not learn a single count while the kernels run:
// buffers and grids are sized from LIMITS (pair_limit, junc_limit, the key format kf), the kernels read the actual
// counts from the control block in device memory (ContigStats) and stand still when a limit is exceeded.  Nothing
// here waits for the device: the last kernels (rows stream) write rows and control block into page-locked host memory
// and pjb_finish_contig_end waits for their event -- by which time the next contig may be queued behind this one.
// `filt`: uploads the junctions and the models and queues kg_features on the context's stream; the rows are in c->g_out, the "a genome is
// missing" flag in c->g_bad.  Nothing waits here (rows and models are pageable: the caller's wait comes before it returns).
static int features_queue(pjb_ctx *c, const pjb_junction_row *rows, size_t n, double mean_read_length, uint32_t l95, const pjb_markov_models *models) {
    hipStream_t st = c->stream;
    int rc;
    if ((rc = ensure(c, c->g_rows, n * sizeof(pjb_junction_row)))) return rc;
    if ((rc = ensure(c, c->g_models, ((size_t)6 * PJB_KMER_TABLE + 2 * PJB_PW_LEN * 5) * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->g_refs, std::max<size_t>(c->contigs.size(), 1) * sizeof(GenomeRef)))) return rc;
    if ((rc = ensure(c, c->g_out, n * PJB_N_FEATURES * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->g_bad, sizeof(int)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->g_rows.p, rows, n * sizeof(pjb_junction_row), hipMemcpyHostToDevice, st));
    DevModels M;
    memset(&M, 0, sizeof M);
    double *dm = (double *)c->g_models.p;
    const double *src[8] = {models->exon, models->intron, models->donor_t, models->donor_f, models->acceptor_t, models->acceptor_f,
                            models->donor_pw, models->acceptor_pw};
    const double **dst[8] = {&M.exon, &M.intron, &M.don_t, &M.don_f, &M.acc_t, &M.acc_f, &M.don_pw, &M.acc_pw};
    size_t at = 0;
    for (int k = 0; k < 8; k++) {
        const size_t cnt = k < 6 ? (size_t)PJB_KMER_TABLE : (size_t)PJB_PW_LEN * 5;
        if (src[k]) {
            HIP_TRY(c, hipMemcpyAsync(dm + at, src[k], cnt * sizeof(double), hipMemcpyHostToDevice, st));
            *dst[k] = dm + at;
        }
        at += cnt;
    }
    M.exon_size = models->exon ? models->exon_size : 0;
    M.intron_size = models->intron ? models->intron_size : 0;
    M.don_pw_size = models->donor_pw ? models->donor_pw_size : 0;
    M.acc_pw_size = models->acceptor_pw ? models->acceptor_pw_size : 0;
    std::vector<GenomeRef> refs(std::max<size_t>(c->contigs.size(), 1));
    for (size_t t = 0; t < c->contigs.size(); t++) {
        refs[t].d = c->contigs[t].present ? c->contigs[t].d : nullptr;
        refs[t].len = (int32_t)c->contigs[t].len;
    }
    HIP_TRY(c, hipMemcpyAsync(c->g_refs.p, refs.data(), refs.size() * sizeof(GenomeRef), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync(c->g_bad.p, 0, sizeof(int), st));
    LAUNCH(c, "kg_features", kg_features, dim3((unsigned)((n + 255) / 256)), dim3(256), (const pjb_junction_row *)c->g_rows.p, (u32)n,
           (const GenomeRef *)c->g_refs.p, (int)c->contigs.size(), M, mean_read_length, (u32)l95, (double *)c->g_out.p, (int *)c->g_bad.p);
    return PJB_OK;
}

// queues the walk of the context's forest over n rows of `data` (device; `stride` doubles a row); predictions to c->r_pred
static int forest_queue(pjb_ctx *c, const double *data, size_t n, u32 stride, const int32_t *colmap) {
    int rc;
    if ((rc = ensure(c, c->r_pred, n * (size_t)c->r_classes * sizeof(double)))) return rc;
    const size_t lds = (size_t)FOREST_BLOCK * (size_t)c->r_classes * sizeof(double) + (size_t)c->r_vars * sizeof(int32_t);
    LAUNCH_LDS(c, "kr_forest", kr_forest, dim3((unsigned)((n + FOREST_BLOCK - 1) / FOREST_BLOCK)), dim3(FOREST_BLOCK), lds, (const ForestNode *)c->r_nodes.p,
               (const u32 *)c->r_roots.p, (u32)c->r_trees, (u32)c->r_classes, (u32)c->r_vars, (const double *)c->r_leaf.p, data, (u32)n, stride, colmap,
               (double *)c->r_pred.p);
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
        if (it->second.first) (void)hipFree(it->second.first);
        c->filter_keys.erase(it);
    }
    u64 *d = nullptr;
    if (n_keys) {
        if (hipMalloc((void **)&d, (size_t)n_keys * 8) != hipSuccess) return fail(c, PJB_ERR_NOMEM, "pjb_filter_set_junctions: %lld keys", (long long)n_keys);
        hipError_t e = hipMemcpy(d, sorted_keys, (size_t)n_keys * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
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

int pjb_filt_features(pjb_ctx *c, const pjb_junction_row *rows, int64_t n_rows, double mean_read_length, uint32_t l95,
                      const pjb_markov_models *models, double *features_out) {
    if (!c) return PJB_ERR_ARG;
    if (n_rows < 0 || (n_rows > 0 && (!rows || !features_out)) || !models || n_rows > 0xfffffff0ll)
        return fail(c, PJB_ERR_ARG, "pjb_filt_features: bad arguments");
    if (n_rows == 0) return PJB_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_rows;
    int rc;
    if ((rc = features_queue(c, rows, n, mean_read_length, l95, models))) return rc;
    int bad = 0;
    HIP_TRY(c, hipMemcpyAsync(features_out, c->g_out.p, n * PJB_N_FEATURES * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&bad, c->g_bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    if (bad) return fail(c, PJB_ERR_STATE, "pjb_filt_features: a junction lies on a target whose genome was not uploaded");
    return PJB_OK;
}

int pjb_forest_check(const pjb_forest *f, char *msg, int len) {
    auto no = [&](const char *fmt, long long a, long long b) {
        if (msg && len > 0) snprintf(msg, (size_t)len, fmt, a, b);
        return PJB_ERR_ARG;
    };
    if (!f) return no("pjb_forest_check: no forest", 0, 0);
    if (f->n_trees < 1) return no("forest: %lld trees (at least one is needed)", f->n_trees, 0);
    if (f->n_classes < 1 || f->n_classes > PJB_FOREST_MAX_CLASSES) return no("forest: %lld classes (1 to %lld can be walked)", f->n_classes, PJB_FOREST_MAX_CLASSES);
    if (f->n_vars < 1 || f->n_vars > PJB_FOREST_MAX_VARS) return no("forest: %lld variables (1 to %lld can be walked)", f->n_vars, PJB_FOREST_MAX_VARS);
    if (f->dependent_var < 0 || f->dependent_var >= f->n_vars) return no("forest: dependent variable %lld of %lld variables", f->dependent_var, f->n_vars);
    if (!f->tree_off || !f->left || !f->right || !f->split_var || !f->split_value || !f->count_off || (!f->counts && f->n_counts > 0) || f->n_counts < 0)
        return no("forest: an array is missing", 0, 0);
    if (f->is_ordered)
        for (int32_t v = 0; v < f->n_vars; v++)
            if (!f->is_ordered[v]) return no("forest: variable %lld is unordered (only ordered variables can be walked)", v, 0);
    if (f->tree_off[0] != 0) return no("forest: the first tree starts at node %lld", (long long)f->tree_off[0], 0);
    if (f->tree_off[f->n_trees] > 0x7ffffff0ll) return no("forest: %lld nodes", (long long)f->tree_off[f->n_trees], 0);
    std::vector<uint8_t> has_parent;
    for (int32_t t = 0; t < f->n_trees; t++) {
        const int64_t base = f->tree_off[t], n = f->tree_off[t + 1] - base;
        if (n < 1 || n > 0x7ffffff0ll) return no("forest: tree %lld has %lld nodes", t, (long long)n);
        has_parent.assign((size_t)n, 0);
        for (int64_t k = 0; k < n; k++) {
            const int64_t l = f->left[base + k], r = f->right[base + k];
            if (l < 0 && r < 0) { // terminal
                const int64_t at = f->count_off[base + k];
                if (at < 0 || at > f->n_counts - f->n_classes) return no("forest: tree %lld, node %lld: a terminal node without its class counts", t, (long long)k);
                continue;
            }
            if (l < 0 || r < 0) return no("forest: tree %lld, node %lld has one child only", t, (long long)k);
            if (l >= n || r >= n) return no("forest: tree %lld, node %lld: a child lies outside the tree", t, (long long)k);
            if (l <= k || r <= k) return no("forest: tree %lld, node %lld: a child is not behind its parent", t, (long long)k);
            if (l == r || has_parent[(size_t)l] || has_parent[(size_t)r]) return no("forest: tree %lld, node %lld: a child has two parents", t, (long long)k);
            has_parent[(size_t)l] = has_parent[(size_t)r] = 1;
            const int32_t v = f->split_var[base + k];
            if (v < 0 || v >= f->n_vars) return no("forest: tree %lld, node %lld splits on a variable the data does not have", t, (long long)k);
            if (v == f->dependent_var) return no("forest: tree %lld, node %lld splits on the dependent variable", t, (long long)k);
        }
    }
    return PJB_OK;
}

int pjb_forest_load(pjb_ctx *c, const pjb_forest *f) {
    if (!c) return PJB_ERR_ARG;
    char msg[200] = "";
    if (pjb_forest_check(f, msg, (int)sizeof msg) != PJB_OK) return fail(c, PJB_ERR_ARG, "pjb_forest_load: %s", msg);
    // pack: each tree breadth first from its root, so that the two children of a node are neighbours (nodes nothing leads to are dropped)
    std::vector<ForestNode> nodes;
    std::vector<double> leaf;
    std::vector<u32> roots((size_t)f->n_trees);
    std::vector<int64_t> order;
    nodes.reserve((size_t)f->tree_off[f->n_trees]);
    for (int32_t t = 0; t < f->n_trees; t++) {
        const int64_t base = f->tree_off[t];
        const size_t first = nodes.size();
        roots[(size_t)t] = (u32)first;
        order.assign(1, 0);
        for (size_t at = 0; at < order.size(); at++) {
            const int64_t k = base + order[at];
            ForestNode nd;
            if (f->left[k] < 0) {
                nd.split = 0.0;
                nd.child = (u32)(leaf.size() / (size_t)f->n_classes);
                nd.var = FOREST_LEAF;
                for (int32_t cl = 0; cl < f->n_classes; cl++) leaf.push_back(f->counts[f->count_off[k] + cl] / (double)f->n_trees);
            } else {
                nd.split = f->split_value[k];
                nd.child = (u32)(first + order.size());
                nd.var = (u32)f->split_var[k];
                order.push_back(f->left[k]);
                order.push_back(f->right[k]);
            }
            nodes.push_back(nd);
        }
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    HIP_TRY(c, hipStreamSynchronize(st)); // (the arrays below are pageable, and a walk of the old forest may be queued)
    c->r_trees = 0;
    int rc;
    if ((rc = ensure(c, c->r_nodes, nodes.size() * sizeof(ForestNode)))) return rc;
    if ((rc = ensure(c, c->r_leaf, leaf.size() * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->r_roots, roots.size() * sizeof(u32)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->r_nodes.p, nodes.data(), nodes.size() * sizeof(ForestNode), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->r_leaf.p, leaf.data(), leaf.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->r_roots.p, roots.data(), roots.size() * sizeof(u32), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    c->r_trees = f->n_trees;
    c->r_classes = f->n_classes;
    c->r_vars = f->n_vars;
    c->r_dep = f->dependent_var;
    return PJB_OK;
}

int pjb_forest_predict(pjb_ctx *c, const double *data, int64_t n_rows, int32_t n_cols, double *pred) {
    if (!c) return PJB_ERR_ARG;
    if (!c->r_trees) return fail(c, PJB_ERR_STATE, "pjb_forest_predict: no forest was loaded (pjb_forest_load)");
    if (n_rows < 0 || n_rows > 0xfffffff0ll || (n_rows > 0 && (!data || !pred))) return fail(c, PJB_ERR_ARG, "pjb_forest_predict: bad arguments");
    if (n_cols != c->r_vars) return fail(c, PJB_ERR_ARG, "pjb_forest_predict: the data has %d columns, the forest %d variables", n_cols, c->r_vars);
    if (n_rows == 0) return PJB_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_rows;
    int rc;
    if ((rc = ensure(c, c->r_data, n * (size_t)n_cols * sizeof(double)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->r_data.p, data, n * (size_t)n_cols * sizeof(double), hipMemcpyHostToDevice, st));
    if ((rc = forest_queue(c, (const double *)c->r_data.p, n, (u32)n_cols, nullptr))) return rc;
    HIP_TRY(c, hipMemcpyAsync(pred, c->r_pred.p, n * (size_t)c->r_classes * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (c->ktime) ev_collect(c, MISC_POOL);
    return PJB_OK;
}

int pjb_filt_scores(pjb_ctx *c, const pjb_junction_row *rows, int64_t n_rows, double mean_read_length, uint32_t l95,
                    const pjb_markov_models *models, const int32_t *var_feature, double *pred, double *features_out) {
    if (!c) return PJB_ERR_ARG;
    if (!c->r_trees) return fail(c, PJB_ERR_STATE, "pjb_filt_scores: no forest was loaded (pjb_forest_load)");
    if (n_rows < 0 || (n_rows > 0 && (!rows || !pred)) || !models || !var_feature || n_rows > 0xfffffff0ll)
        return fail(c, PJB_ERR_ARG, "pjb_filt_scores: bad arguments");
    std::vector<int32_t> colmap((size_t)c->r_vars, 0);
    for (int32_t v = 0; v < c->r_vars; v++) {
        if (v == c->r_dep) continue; // (never read)
        if (var_feature[v] < 0 || var_feature[v] >= PJB_N_FEATURES)
            return fail(c, PJB_ERR_ARG, "pjb_filt_scores: variable %d is column %d of a feature row of %d", v, var_feature[v], PJB_N_FEATURES);
        colmap[(size_t)v] = var_feature[v];
    }
    if (n_rows == 0) return PJB_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    const size_t n = (size_t)n_rows;
    int rc;
    if ((rc = ensure(c, c->r_colmap, colmap.size() * sizeof(int32_t)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->r_colmap.p, colmap.data(), colmap.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if ((rc = features_queue(c, rows, n, mean_read_length, l95, models))) return rc;
    if ((rc = forest_queue(c, (const double *)c->g_out.p, n, (u32)PJB_N_FEATURES, (const int32_t *)c->r_colmap.p))) return rc;
    int bad = 0;
    HIP_TRY(c, hipMemcpyAsync(pred, c->r_pred.p, n * (size_t)c->r_classes * sizeof(double), hipMemcpyDeviceToHost, st));
    if (features_out) HIP_TRY(c, hipMemcpyAsync(features_out, c->g_out.p, n * PJB_N_FEATURES * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&bad, c->g_bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st)); // (the one wait; colmap is pageable and lives until here)
    if (c->ktime) ev_collect(c, MISC_POOL);
    if (bad) return fail(c, PJB_ERR_STATE, "pjb_filt_scores: a junction lies on a target whose genome was not uploaded");
    return PJB_OK;
}

// Device memory one batch of trees may take (lists, nodes, candidates, scores); more trees than fit are grown batch after batch.
static constexpr size_t GROW_POOL_BYTES = (size_t)6 << 30;

// Forest::grow for ForestProbability as ModelFeatures::trainInstance sets it up: see include/portcullis_amd.h and pjb_grow.hip.h.
int pjb_forest_grow(pjb_ctx *c, const double *data, int64_t n_rows, int32_t n_cols, const pjb_grow_params *p, pjb_grow_result *out) {
    if (!c) return PJB_ERR_ARG;
    if (!p || !out) return fail(c, PJB_ERR_ARG, "pjb_forest_grow: bad arguments");
    if (p->n_trees < 1) return fail(c, PJB_ERR_ARG, "pjb_forest_grow: %d trees (at least one is needed)", p->n_trees);
    if (n_rows < 1) return fail(c, PJB_ERR_ARG, "pjb_forest_grow: %lld rows (at least one is needed)", (long long)n_rows);
    if (n_cols < 2) return fail(c, PJB_ERR_ARG, "pjb_forest_grow: %d columns (the labels and one variable at least)", n_cols);
    if (n_cols > PJB_FOREST_MAX_VARS) return fail(c, PJB_ERR_ARG, "pjb_forest_grow: %d variables (1 to %d can be walked)", n_cols, PJB_FOREST_MAX_VARS);
    if (!data || n_rows > (1ll << 28) || p->n_trees > (1 << 24)) return fail(c, PJB_ERR_ARG, "pjb_forest_grow: bad arguments");
    if (p->dependent_col < 0 || p->dependent_col >= n_cols)
        return fail(c, PJB_ERR_ARG, "pjb_forest_grow: dependent column %d of %d columns", p->dependent_col, n_cols);
    if (p->mtry < 0 || p->min_node_size < 0) return fail(c, PJB_ERR_ARG, "pjb_forest_grow: mtry %d, node size %d", p->mtry, p->min_node_size);
    // ForestProbability::initInternal (ForestProbability.cpp:64-75)
    const u32 mtry = p->mtry ? (u32)p->mtry : std::max<u32>(1, (u32)sqrt((double)(n_cols - 1)));
    const u32 min_node = p->min_node_size ? (u32)p->min_node_size : 10u;
    if (mtry >= (u32)n_cols / 2)
        return fail(c, PJB_ERR_ARG, "pjb_forest_grow: mtry %u of %d columns: from n_cols / 2 on ranger draws by Knuth's algorithm, which is not built", mtry, n_cols);
    const size_t n = (size_t)n_rows, C = (size_t)n_cols, dep = (size_t)p->dependent_col;
    std::vector<double> colmajor(C * n);
    std::vector<uint8_t> label(n);
    u32 label_sum = 0;
    for (size_t r = 0; r < n; r++)
        for (size_t k = 0; k < C; k++) {
            const double v = data[r * C + k];
            if (!std::isfinite(v)) return fail(c, PJB_ERR_ARG, "pjb_forest_grow: row %zu, column %zu is not finite", r, k);
            if (k == dep) {
                if (v != 0.0 && v != 1.0) return fail(c, PJB_ERR_ARG, "pjb_forest_grow: row %zu has the label %g (0 or 1)", r, v);
                label[r] = v == 1.0;
                label_sum += label[r];
            }
            colmajor[k * n + r] = v;
        }
    // one sort per column, shared by all trees (Data::sort's order of values; rows of one value in row order)
    std::vector<u32> sorted(C * n);
    for (size_t k = 0; k < C; k++) {
        u32 *s = sorted.data() + k * n;
        for (size_t r = 0; r < n; r++) s[r] = (u32)r;
        if (k == dep) continue;
        const double *v = colmajor.data() + k * n;
        std::stable_sort(s, s + n, [v](u32 a, u32 b) { return v[a] < v[b]; });
    }
    // the room of one batch of T trees
    const size_t M = 2 * n;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t shared_bytes = up(C * n * 8) + up(n) + up(C * n * 4) + 256;
    const size_t tree_bytes = 2 * C * n * 4 + n * 4 + M * (5 * 4 + 8) + M * mtry * (2 + sizeof(GrowBest)) + (GROW_MT_N + 1) * 8 + 2 * 4;
    size_t batch = c->grow_batch ? c->grow_batch : std::max<size_t>(1, GROW_POOL_BYTES / tree_bytes);
    batch = std::min<size_t>(std::min<size_t>(batch, (size_t)p->n_trees), 32768);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    int rc;
    if ((rc = ensure(c, c->w_pool, shared_bytes + batch * tree_bytes + 16 * 256))) return rc;
    uint8_t *at = (uint8_t *)c->w_pool.p;
    auto carve = [&](size_t bytes) {
        uint8_t *q = at;
        at += up(bytes);
        return q;
    };
    double *d_col = (double *)carve(C * n * 8);
    uint8_t *d_label = carve(n);
    u32 *d_sorted = (u32 *)carve(C * n * 4);
    u32 *d_new = (u32 *)carve(4);
    u32 *d_lists[2] = {(u32 *)carve(batch * C * n * 4), (u32 *)carve(batch * C * n * 4)};
    u32 *d_node_of = (u32 *)carve(batch * n * 4);
    GrowNodes nd;
    nd.start = (u32 *)carve(batch * M * 4);
    nd.count = (u32 *)carve(batch * M * 4);
    nd.sum = (u32 *)carve(batch * M * 4);
    nd.child = (u32 *)carve(batch * M * 4);
    nd.var = (u32 *)carve(batch * M * 4);
    nd.val = (double *)carve(batch * M * 8);
    uint16_t *d_cand = (uint16_t *)carve(batch * M * mtry * 2);
    GrowBest *d_best = (GrowBest *)carve(batch * M * mtry * sizeof(GrowBest));
    u64 *d_state = (u64 *)carve(batch * (GROW_MT_N + 1) * 8);
    u32 *d_lvl = (u32 *)carve(batch * 2 * 4);
    HIP_TRY(c, hipMemcpyAsync(d_col, colmajor.data(), C * n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_label, label.data(), n, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_sorted, sorted.data(), C * n * 4, hipMemcpyHostToDevice, st));

    pjb_ctx::GrowOut &G = c->grow_out;
    G = pjb_ctx::GrowOut();
    G.is_ordered.assign(C, 1);
    if (label_sum < n) G.class_values.push_back(0.0);
    if (label_sum > 0) G.class_values.push_back(1.0);
    const size_t K = G.class_values.size();
    G.tree_off.push_back(0);
    std::vector<u32> lvl, h_child, h_var, h_count, h_sum;
    std::vector<double> h_val;
    std::vector<u64> off;
    for (size_t t0 = 0; t0 < (size_t)p->n_trees; t0 += batch) {
        const u32 T = (u32)std::min<size_t>(batch, (size_t)p->n_trees - t0);
        LAUNCH(c, "kt_seed", kt_seed, dim3((T + 63) / 64), dim3(64), d_state, T, (u32)t0, (u32)p->seed, nd, (u32)M, d_lvl, (u32)n, label_sum);
        const u64 total = (u64)T * C * n;
        LAUNCH(c, "kt_fill", kt_fill, dim3((unsigned)((total + 255) / 256)), dim3(256), (const u32 *)d_sorted, d_lists[0], (u64)(C * n), total);
        HIP_TRY(c, hipMemsetAsync(d_node_of, 0, (size_t)T * n * 4, st));
        int cur = 0;
        // one trip per level: at most n_rows levels (every split leaves both children smaller); the one read-back says whether nodes were made
        for (size_t level = 0; level <= n; level++) {
            u32 n_new = 0;
            HIP_TRY(c, hipMemsetAsync(d_new, 0, 4, st));
            LAUNCH(c, "kt_draw", kt_draw, dim3((T + GROW_DRAW_TREES - 1) / GROW_DRAW_TREES), dim3(GROW_DRAW_TREES), d_state, T, (const u32 *)d_lvl, (u32)C, (u32)dep,
                   mtry, d_cand, (u32)M);
            LAUNCH(c, "kt_split", kt_split, dim3((unsigned)C, T), dim3(64), (const u32 *)d_lists[cur], (const u32 *)d_node_of, (const double *)d_col,
                   (const uint8_t *)d_label, (const u32 *)d_lvl, T, nd, (const uint16_t *)d_cand, d_best, (u32)n, (u32)C, (u32)dep, mtry, (u32)M);
            LAUNCH(c, "kt_decide", kt_decide, dim3(T), dim3(64), (const u32 *)d_lists[cur], (const double *)d_col, d_lvl, T, nd, (const uint16_t *)d_cand,
                   (const GrowBest *)d_best, (u32)n, (u32)C, mtry, (u32)M, min_node, d_new);
            HIP_TRY(c, hipMemcpyAsync(&n_new, d_new, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(c, hipStreamSynchronize(st));
            if (c->ktime) ev_collect(c, MISC_POOL);
            if (!n_new) break;
            LAUNCH(c, "kt_partition", kt_partition, dim3((unsigned)C, T), dim3(64), (const u32 *)d_lists[cur], d_lists[cur ^ 1], (const u32 *)d_node_of,
                   (const double *)d_col, (const u32 *)d_lvl, T, nd, (u32)n, (u32)C, (u32)dep, (u32)M);
            LAUNCH(c, "kt_assign", kt_assign, dim3((unsigned)((n + 255) / 256), T), dim3(256), d_node_of, (const double *)d_col, nd, (u32)n, (u32)M);
            cur ^= 1;
        }
        // the trees' nodes, packed one tree after the other
        lvl.resize((size_t)2 * T);
        HIP_TRY(c, hipMemcpyAsync(lvl.data(), d_lvl, (size_t)2 * T * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        off.assign((size_t)T + 1, 0);
        u32 most = 0;
        for (u32 t = 0; t < T; t++) {
            const u32 nodes = lvl[(size_t)T + t]; // (the end of the last level: the tree's node count)
            if (lvl[t] != nodes || nodes < 1 || nodes >= M) return fail(c, PJB_ERR_STATE, "pjb_forest_grow: tree %zu did not finish (%u nodes)", t0 + t, nodes);
            off[t + 1] = off[t] + nodes;
            most = std::max(most, nodes);
        }
        const size_t N = (size_t)off[T];
        if ((rc = ensure(c, c->w_pack, up((T + 1) * 8) + 4 * up(N * 4) + up(N * 8)))) return rc;
        uint8_t *q = (uint8_t *)c->w_pack.p;
        u64 *d_off = (u64 *)q;
        q += up((T + 1) * 8);
        u32 *p_child = (u32 *)q, *p_var = (u32 *)(q + up(N * 4)), *p_count = (u32 *)(q + 2 * up(N * 4)), *p_sum = (u32 *)(q + 3 * up(N * 4));
        double *p_val = (double *)(q + 4 * up(N * 4));
        HIP_TRY(c, hipMemcpyAsync(d_off, off.data(), (T + 1) * 8, hipMemcpyHostToDevice, st));
        LAUNCH(c, "kt_pack", kt_pack, dim3((most + 255) / 256, T), dim3(256), nd, (u32)M, (const u64 *)d_off, p_child, p_var, p_val, p_count, p_sum);
        h_child.resize(N), h_var.resize(N), h_count.resize(N), h_sum.resize(N), h_val.resize(N);
        HIP_TRY(c, hipMemcpyAsync(h_child.data(), p_child, N * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h_var.data(), p_var, N * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h_count.data(), p_count, N * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h_sum.data(), p_sum, N * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(h_val.data(), p_val, N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (c->ktime) ev_collect(c, MISC_POOL);
        for (u32 t = 0; t < T; t++) {
            for (u64 k = off[t]; k < off[t + 1]; k++) {
                if (h_child[k]) {
                    G.left.push_back((int32_t)h_child[k]);
                    G.right.push_back((int32_t)h_child[k] + 1);
                    G.count_off.push_back(-1);
                } else { // addToTerminalNodes: count[class] / n, one division each
                    G.left.push_back(-1);
                    G.right.push_back(-1);
                    G.count_off.push_back((int64_t)G.counts.size());
                    const double cnt = (double)h_count[k], ones = (double)h_sum[k];
                    if (K == 2) G.counts.push_back((cnt - ones) / cnt);
                    G.counts.push_back((K == 2 || label_sum > 0 ? ones : cnt) / cnt);
                }
                G.split_var.push_back((int32_t)h_var[k]);
                G.split_value.push_back(h_val[k]);
            }
            G.tree_off.push_back((int64_t)G.left.size());
        }
    }
    pjb_forest &f = out->forest;
    memset(&f, 0, sizeof f);
    f.n_trees = p->n_trees;
    f.n_classes = (int32_t)K;
    f.n_vars = n_cols;
    f.dependent_var = p->dependent_col;
    f.is_ordered = G.is_ordered.data();
    f.tree_off = G.tree_off.data();
    f.left = G.left.data();
    f.right = G.right.data();
    f.split_var = G.split_var.data();
    f.split_value = G.split_value.data();
    f.count_off = G.count_off.data();
    f.counts = G.counts.data();
    f.n_counts = (int64_t)G.counts.size();
    out->class_values = G.class_values.data();
    char msg[200] = "";
    if (pjb_forest_check(&f, msg, (int)sizeof msg) != PJB_OK) return fail(c, PJB_ERR_STATE, "pjb_forest_grow: the grown forest cannot be walked: %s", msg);
    return PJB_OK;
}

// Waves the default chunking of pjb_knn aims at: 256 CUs x 4 SIMDs x 4 waves, so that scalar-load latency has other waves to hide behind.
static constexpr size_t KNN_WAVES = 4096;
// A chunk shorter than this spends its time filling the lists (every one of the first rows of a chunk is an insertion).
static constexpr size_t KNN_MIN_CHUNK = 256;
// |value| <= this: 32 squared differences cannot overflow (32 * (2e153)^2 = 1.28e308), so every distance is finite and ordered.
static constexpr double KNN_MAX_ABS = 1e153;
static_assert(KN_LIST == PJB_KNN_MAX_K, "the lists of pjb_knn.hip.h hold PJB_KNN_MAX_K entries");

// KNN::execute (lib/src/knn.cc): see include/portcullis_amd.h and pjb_knn.hip.h.
int pjb_knn(pjb_ctx *c, const double *data, int64_t n_rows, int32_t n_cols, int32_t k, uint32_t *nn_out) {
    if (!c) return PJB_ERR_ARG;
    if (!data || !nn_out) return fail(c, PJB_ERR_ARG, "pjb_knn: bad arguments");
    if (n_cols < 1 || n_cols > PJB_KNN_MAX_COLS) return fail(c, PJB_ERR_ARG, "pjb_knn: %d columns (1 to %d)", n_cols, PJB_KNN_MAX_COLS);
    if (n_rows < 1 || n_rows > (1ll << 22)) return fail(c, PJB_ERR_ARG, "pjb_knn: %lld rows (1 to %d)", (long long)n_rows, 1 << 22);
    if (k < 1 || k > PJB_KNN_MAX_K || k > n_rows)
        return fail(c, PJB_ERR_ARG, "pjb_knn: k = %d (1 to %d, and no more than the %lld rows)", k, PJB_KNN_MAX_K, (long long)n_rows);
    const size_t n = (size_t)n_rows, C = (size_t)n_cols;
    const size_t NC = n_cols <= 28 ? 28 : 32; // the compiled widths: the 28 features of self-training, and the limit
    std::vector<double> padded(n * NC, 0.0);
    for (size_t r = 0; r < n; r++)
        for (size_t j = 0; j < C; j++) {
            const double v = data[r * C + j];
            if (!(fabs(v) <= KNN_MAX_ABS)) // (a NaN too)
                return fail(c, PJB_ERR_ARG, "pjb_knn: row %zu, column %zu is %g: not finite, or so large that a distance could overflow", r, j, v);
            padded[r * NC + j] = v;
        }
    size_t chunk = c->knn_chunk;
    if (!chunk) {
        const size_t row_waves = (n + 63) / 64;
        const size_t want = (KNN_WAVES + row_waves - 1) / row_waves;
        chunk = std::max(KNN_MIN_CHUNK, (n + want - 1) / want);
    }
    chunk = std::min(chunk, n);
    const size_t n_chunks = (n + chunk - 1) / chunk;
    if (n_chunks > 65535) return fail(c, PJB_ERR_ARG, "pjb_knn: knn_chunk %zu makes %zu chunks of %zu rows (65535 at most)", chunk, n_chunks, n);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    hipStream_t st = c->stream;
    int rc;
    if ((rc = ensure(c, c->n_data, n * NC * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->n_part_d, n_chunks * KN_LIST * n * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->n_part_i, n_chunks * KN_LIST * n * sizeof(u32)))) return rc;
    if ((rc = ensure(c, c->n_out, n * (size_t)k * sizeof(u32)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->n_data.p, padded.data(), n * NC * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)n_chunks);
    if (NC == 28)
        LAUNCH(c, "kn_partial", kn_partial<28>, grid, dim3(64), (const double *)c->n_data.p, (u32)n, (u32)chunk, (double *)c->n_part_d.p, (u32 *)c->n_part_i.p);
    else
        LAUNCH(c, "kn_partial", kn_partial<32>, grid, dim3(64), (const double *)c->n_data.p, (u32)n, (u32)chunk, (double *)c->n_part_d.p, (u32 *)c->n_part_i.p);
    LAUNCH(c, "kn_merge", kn_merge, dim3((unsigned)((n + 255) / 256)), dim3(256), (const double *)c->n_part_d.p, (const u32 *)c->n_part_i.p, (u32)n,
           (u32)n_chunks, (u32)k, (u32 *)c->n_out.p);
    HIP_TRY(c, hipMemcpyAsync(nn_out, c->n_out.p, n * (size_t)k * sizeof(u32), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st)); // (the one wait; `padded` is pageable and lives until here)
    if (c->ktime) ev_collect(c, MISC_POOL);
    return PJB_OK;
}

} // extern "C"
