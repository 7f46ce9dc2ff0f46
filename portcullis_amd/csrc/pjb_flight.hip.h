// pjb_flight.hip.h -- a flight (a target, or a group of targets finished as one chain) from begin to end: begin_flight checks the call,
// takes a control slot, prepares the flight and queues its chain; end_flight collects the oldest one -- collect_flight as named stages over
// one state (Collect): wait, relimit, apart, results, timing, commit -- and queues what waited behind it.  What a chain is queued with,
// and with what after an overflow, is pjb_limits.hip.h's; this file applies it.  Host code only, included by pjb_api.hip behind
// pjb_chain.hip.h and by nothing else.
#pragma once
#include "pjb_limits.hip.h"

static void aux_streams(pjb_ctx *c) { // the rows stream and the row mirror's (15 - 20 ms each to create)
    if (!c->stream3) (void)hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking);
    if (!c->stream4) (void)hipStreamCreateWithFlags(&c->stream4, hipStreamNonBlocking);
}

// a contig without junctions still reports its counters through the row mirror
static void mirror_fold(pjb_ctx *c, const pjb_region_result &R, size_t new_rows) {
    c->mirror_rows += new_rows;
    c->mirror_acc[0] += (int64_t)R.spliced;
    c->mirror_acc[1] += (int64_t)R.unspliced;
    c->mirror_acc[2] += (int64_t)R.sum_len;
    c->mirror_acc[3] = std::min<int64_t>(c->mirror_acc[3], R.min_len);
    c->mirror_acc[4] = std::max<int64_t>(c->mirror_acc[4], R.max_len);
    int64_t *h = c->mirror_hdr;
    h[0] = (int64_t)c->mirror_rows;
    for (int k = 0; k < 5; k++) h[1 + k] = c->mirror_acc[k];
    h[6] = h[7] = 0;
}
static void mirror_reset(pjb_ctx *c) {
    c->mirror_rows = 0;
    c->mirror_acc[0] = c->mirror_acc[1] = c->mirror_acc[2] = 0;
    c->mirror_acc[3] = INT32_MAX;
    c->mirror_acc[4] = 0;
}
static int mirror_header_only(pjb_ctx *c, const pjb_region_result &R) {
    if (!c->mirror) return PJB_OK;
    aux_streams(c);
    mirror_fold(c, R, 0);
    HIP_TRY(c, hipMemcpyAsync(c->mirror, c->mirror_hdr, PJB_MIRROR_HEADER_BYTES, hipMemcpyHostToDevice, c->stream4));
    HIP_TRY(c, hipStreamSynchronize(c->stream4));
    return PJB_OK;
}

// the host's row table holds `need` rows (the first c->rows_n of them are kept)
static int rows_pinned_reserve(pjb_ctx *c, size_t need) {
    if (need <= c->rows_pinned_cap && c->rows_pinned) return PJB_OK;
    int rc = rows_sync(c); // (a DMA into the table that is about to move)
    if (rc) return rc;
    const size_t ncap = std::max<size_t>(need * 3 / 2, 1024);
    pjb_junction_row *np = nullptr;
    const hipError_t e = hipHostMalloc((void **)&np, ncap * sizeof(pjb_junction_row), hipHostMallocPortable);
    if (e != hipSuccess) return fail(c, PJB_ERR_NOMEM, "hipHostMalloc(rows): %s", hipGetErrorString(e));
    if (c->rows_pinned && c->rows_n) memcpy(np, c->rows_pinned, std::min(c->rows_n, c->rows_pinned_cap) * sizeof(pjb_junction_row));
    if (c->rows_pinned) (void)hipHostFree(c->rows_pinned);
    c->rows_pinned = np;
    c->rows_pinned_cap = ncap;
    return PJB_OK;
}

// The contigs queued behind fl[0] are taken back (after an overflow or an error of fl[0] their rows are in the wrong
// place): their device work is allowed to finish and is thrown away; their own pjb_finish_contig_end queues them again.
static void unqueue_followers(pjb_ctx *c) {
    for (int k = 1; k < c->n_fl; k++) {
        Flight &g = c->fl[k];
        if (!g.queued) continue;
        wait_flight(c, g);
        if (g.forked) (void)hipStreamSynchronize(c->sl[g.slot].side);
        g.queued = false;
        g.forked = false;
        ev_drop(c, g.slot);
    }
}

// fl[0]'s chain -- waited for by the caller -- is taken back, and with it everything queued behind it: what it left on its side stream
// is allowed to finish, and the chain may be queued again
static void flight_take_back(pjb_ctx *c, Flight &f) {
    unqueue_followers(c);
    if (f.forked) (void)hipStreamSynchronize(c->sl[f.slot].side);
    f.queued = f.forked = false;
}

static void pop_flight(pjb_ctx *c) {
    if (c->n_fl <= 0) return;
    c->slot_busy[c->fl[0].slot] = false;
    for (int k = 1; k < c->n_fl; k++) c->fl[k - 1] = c->fl[k];
    c->n_fl--;
    c->fl[c->n_fl] = Flight();
}

// The flight's batch list, virtual offsets, tile ranges and limits from the open targets named in f.tids.
static void prepare_flight(pjb_ctx *c, Flight &f) {
    f.batches.clear();
    f.batch_member.clear();
    f.voff.assign(f.tids.size(), 0);
    f.tile_lo.assign(f.tids.size() + 1, 0);
    f.m_reads.assign(f.tids.size(), 0);
    f.n_tiles = 0;
    f.n_reads = 0;
    int64_t at = 0;
    bool genomes_ok = true;
    for (size_t m = 0; m < f.tids.size(); m++) {
        const int32_t tid = f.tids[m];
        const int32_t ref_len = c->ref_len[(size_t)tid];
        f.voff[m] = (int32_t)at;
        at += group_span(ref_len);
        f.tile_lo[m] = f.n_tiles;
        const Contig &G = c->contigs[(size_t)tid];
        auto open_it = c->open.find(tid);
        if (open_it == c->open.end() || open_it->second.batches.empty()) continue;
        // without the target's genome only the counting stage may run: any pair then shows up as an overflow
        if (!G.present || G.len != ref_len) genomes_ok = false;
        OpenContig &oc = open_it->second;
        int32_t prev_pos = INT32_MIN;
        const int32_t *prev_ptr = nullptr;
        for (size_t k = 0; k < oc.batches.size(); k++) {
            DevBatch b = oc.batches[k];
            b.base = (uint32_t)f.n_reads; // read ordinals and tile numbers run through the whole group
            b.tile_base = f.n_tiles;
            f.n_tiles += (u32)((b.n + K1_TILE - 1) / K1_TILE);
            b.prev_pos = prev_pos;
            b.prev_pos_ptr = prev_ptr; // sortedness across batches: the last position of the previous batch, wherever it is known
            f.n_reads += b.n;
            f.m_reads[m] += b.n;
            if (oc.last_known[k]) {
                prev_pos = oc.last_pos[k];
                prev_ptr = nullptr;
            } else
                prev_ptr = b.pos + (b.n - 1);
            b.member = (int32_t)m;
            f.batches.push_back(b);
            f.batch_member.push_back((int)m);
        }
    }
    f.tile_lo[f.tids.size()] = f.n_tiles;
    f.vlen = f.tids.size() > 1 ? at : c->ref_len[(size_t)f.tid];
    f.empty = f.batches.empty();
    f.lim = first_limits(LimitInputs{f.n_reads, (int)f.tids.size(), f.vlen, genomes_ok, c->junc_seen, c->lbits_seen, c->junc_per_read, c->sort_floor,
                                     c->dense_ids, c->run_sort});
}

// streams and events of a control slot, at its first use (a context that never queues eight chains never pays for them)
static int slot_init(pjb_ctx *c, int k) {
    CtlSlot &S = c->sl[k];
    if (S.ev_done) return PJB_OK;
    for (auto &ev : S.ev) HIP_TRY(c, hipEventCreate(&ev));
    HIP_TRY(c, hipEventCreateWithFlags(&S.ev_rows, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&S.ev_done, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&S.ev_k1, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&S.ev_xk1, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&S.ev_fork, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&S.ev_join, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&S.ev_fork2, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&S.ev_join2, hipEventDisableTiming));
    // (main before side, slot after slot: the order in which streams are created decides which hardware queue they share, and
    // every other order tried -- side first, all mains first, one to three streams created before -- cost the configs[2] step
    // 5 - 12 %: profiles/r03z_stream_order.txt)
    HIP_TRY(c, hipStreamCreateWithFlags(&S.main, hipStreamNonBlocking));
    HIP_TRY(c, hipStreamCreateWithFlags(&S.side, hipStreamNonBlocking));
    return PJB_OK;
}

// the chain and, with PJB_FLAG_EXTRA, the part of the extra metrics that needs the records only (service stream, beside the chain)
static int queue_chain(pjb_ctx *c, Flight &f) {
    int rc = queue_contig(c, f);
    if (!rc && c->extra) rc = extra_pre(c, f);
    return rc;
}

// what a call of pjb_finish_contig_begin / pjb_finish_group_begin must satisfy, in the order in which a bad call learns of it
static int begin_check(pjb_ctx *c, const int32_t *tids, int32_t n, const char *who) {
    if (!c) return PJB_ERR_ARG;
    if (!tids || n < 1 || n > GROUP_MAX) return fail(c, PJB_ERR_ARG, "%s: 1 to %d targets", who, GROUP_MAX);
    aux_streams(c);
    for (int32_t k = 0; k < n; k++) {
        if (tids[k] < 0 || (size_t)tids[k] >= c->ref_len.size()) return fail(c, PJB_ERR_ARG, "%s: bad tid %d", who, tids[k]);
        for (int32_t q = 0; q < k; q++)
            if (tids[q] == tids[k]) return fail(c, PJB_ERR_ARG, "%s: target %d named twice", who, tids[k]);
    }
    if (c->n_fl >= PJB_MAX_QUEUED)
        return fail(c, PJB_ERR_STATE, "%s: %d chains are queued already (oldest: target %d); collect one first", who, c->n_fl, c->fl[0].tid);
    for (int k = 0; k < c->n_fl; k++)
        for (int32_t t : c->fl[k].tids)
            for (int32_t q = 0; q < n; q++)
                if (t == tids[q]) return fail(c, PJB_ERR_STATE, "%s: target %d is queued already", who, t);
    if (n > 1) {
        // what a group needs (a caller that gets PJB_ERR_ARG here finishes the targets one by one)
        if (c->extra && c->extra_dense_only)
            return fail(c, PJB_ERR_ARG, "%s: a PJB_FLAG_EXTRA context with \"extra_dense\" 1 builds a depth vector per target: finish them one by one", who);
        int64_t vlen = 0;
        for (int32_t k = 0; k < n; k++) {
            const Contig &G = c->contigs[(size_t)tids[k]];
            vlen += group_span(c->ref_len[(size_t)tids[k]]);
            auto it = c->open.find(tids[k]);
            const bool has_reads = it != c->open.end() && !it->second.batches.empty();
            if (has_reads && (!G.present || G.len != c->ref_len[(size_t)tids[k]]))
                return fail(c, PJB_ERR_ARG, "%s: the genome of target %d has not been uploaded", who, tids[k]);
            if (has_reads && (!G.codes || G.has_x))
                return fail(c, PJB_ERR_ARG, "%s: target %d has characters outside the 16-letter alphabet: finish it alone", who, tids[k]);
        }
        if (vlen >= (int64_t)INT32_MAX - (1 << 20)) return fail(c, PJB_ERR_ARG, "%s: the group's targets add up to %lld bases (limit 2^31)", who, (long long)vlen);
    }
    return PJB_OK;
}

static int begin_flight(pjb_ctx *c, const int32_t *tids, int32_t n, const char *who) {
    int rc = begin_check(c, tids, n, who);
    if (rc) return rc;
    c->cur_tid = tids[0];
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    Flight &f = c->fl[c->n_fl];
    int slot = 0;
    while (slot < PJB_MAX_QUEUED && c->slot_busy[slot]) slot++;
    if (slot >= PJB_MAX_QUEUED) return fail(c, PJB_ERR_STATE, "%s: no free control slot", who);
    if ((rc = slot_init(c, slot))) return rc;
    f = Flight();
    f.slot = slot;
    f.tid = tids[0];
    f.tids.assign(tids, tids + n);
    c->slot_busy[slot] = true;
    prepare_flight(c, f);
    c->n_fl++;
    if (f.empty) return PJB_OK;
    // a chain that was taken back goes first (rows are in queue order): the end of the oldest one queues them all
    for (int k = 0; k + 1 < c->n_fl; k++)
        if (!c->fl[k].queued && !c->fl[k].empty) return PJB_OK;
    rc = queue_chain(c, f);
    if (rc) { // nothing of this chain stays behind
        (void)hipDeviceSynchronize();
        c->n_fl--;
        c->slot_busy[c->fl[c->n_fl].slot] = false;
        std::vector<int32_t> members = c->fl[c->n_fl].tids;
        c->fl[c->n_fl] = Flight();
        for (int32_t t : members) close_contig(c, t);
    }
    return rc;
}

// What the stages of collect_flight share: the chain in fl[0], what it published, and what became of it.  collect_flight fills it once.
struct Collect {
    pjb_ctx *c;
    Flight &f;
    CtlSlot &S;
    pjb_region_result *res; // one per member
    bool group;
    int32_t ref_len; // the sequence the chain works on: the target itself, or the group's virtual sequence
    ContigStats cs;  // the control block of the last attempt
    u64 herr = ~0ull;
    int64_t repeats = 0, repeat_reasons = 0;
    bool apart = false; // the group is taken apart: nothing of it is committed
};

// 1. wait: the chain -- queued here if it was taken back -- has run; its control block and error word; the members' genomes
static int collect_wait(Collect &co) {
    pjb_ctx *c = co.c;
    Flight &f = co.f;
    int rc;
    if (!f.queued && (rc = queue_chain(c, f))) return rc;
    wait_flight(c, f);
    memcpy(&co.cs, co.S.pub, sizeof co.cs);
    memcpy(&co.herr, co.S.pub + PUB_ERR_AT, 8);
    if ((rc = check_device_error(c, co.herr))) return rc;
    for (size_t m = 0; m < f.tids.size() && co.cs.n_pairs > 0; m++) {
        const Contig &G = c->contigs[(size_t)f.tids[m]];
        if (f.m_reads[m] == 0) continue;
        if (!G.present) return fail(c, PJB_ERR_STATE, "finish: genome of target %d was not uploaded", f.tids[m]);
        if (G.len != c->ref_len[(size_t)f.tids[m]])
            return fail(c, PJB_ERR_ARG, "finish: genome of target %d has %lld bases, header says %d", f.tids[m], (long long)G.len, c->ref_len[(size_t)f.tids[m]]);
    }
    return PJB_OK;
}

// 2. relimit: a limit was too small.  The control block says by how much; everything is queued again, and so are the chains queued
// behind this one: their rows went where this one's belong.
static int collect_relimit(Collect &co) {
    pjb_ctx *c = co.c;
    Flight &f = co.f;
    const ContigStats &cs = co.cs;
    if (!attempt_budget(cs.overflow, f.attempt, f.list_attempt))
        return fail(c, PJB_ERR_STATE, "finish: limits of target %d did not settle (overflow bits %u)", f.tid, cs.overflow);
    co.repeats++;
    co.repeat_reasons |= (int64_t)cs.overflow;
    const Relimit v = relimit(f.lim, cs, co.ref_len, co.group);
    if (v.run_sort_off) { // (for this chain, those taken back behind it and those to come)
        c->run_sort = false;
        for (int k = 0; k < c->n_fl; k++) c->fl[k].lim.run_sort = false;
    }
    flight_take_back(c, f);
    if (v.what == Relimit::TOO_MANY_PAIRS) return fail(c, PJB_ERR_ARG, "%s", too_many_pairs_text(co.group));
    co.apart = v.what == Relimit::APART;
    return PJB_OK;
}

// 3. apart: --extra answers a group from its members' records in virtual coordinates; where that answer does not stand the group is taken
// apart before anything of it is committed.  (Its rows are in the table and the cursor has moved: the chains behind it are taken back, and
// the members' chains are queued with their place given.)
static int collect_apart(Collect &co) {
    pjb_ctx *c = co.c;
    if (!c->extra || !co.group) return PJB_OK;
    const int rc = extra_group_apart(c, co.f, &co.apart);
    if (rc) return rc;
    if (co.apart) flight_take_back(c, co.f);
    return PJB_OK;
}

// 4. results: one per member, the chain's counts against the members', and what the context learns for the chains to come
static int collect_results(Collect &co) {
    pjb_ctx *c = co.c;
    Flight &f = co.f;
    const ContigStats &cs = co.cs;
    const int n_members = (int)f.tids.size();
    const u32 J = cs.J;
    if (!f.lim.kf.raw) c->lbits_seen = std::max(c->lbits_seen, std::max(1, bits_of((uint64_t)cs.max_nlen)));
    if (!co.group) {
        pjb_region_result &R = co.res[0];
        R.spliced = cs.spliced;
        R.unspliced = cs.unspliced;
        R.sum_len = cs.sum_len;
        R.min_len = cs.min_len;
        R.max_len = cs.max_len;
        R.n_reads = f.n_reads;
        R.n_pairs = (int64_t)cs.n_pairs;
        R.n_junctions = J;
    } else {
        const MemberStats *ms = (const MemberStats *)(co.S.pub + PUB_MEMBERS_AT);
        u64 pairs = 0, juncs = 0;
        for (int m = 0; m < n_members; m++) {
            pjb_region_result &R = co.res[m];
            memset(&R, 0, sizeof R);
            R.min_len = INT32_MAX;
            if (f.m_reads[(size_t)m] == 0) continue;
            R.spliced = ms[m].spliced;
            R.unspliced = ms[m].unspliced;
            R.sum_len = ms[m].sum_len;
            R.min_len = ms[m].min_len;
            R.max_len = ms[m].max_len;
            R.n_reads = f.m_reads[(size_t)m];
            R.n_pairs = (int64_t)ms[m].n_pairs;
            R.n_junctions = ms[m].n_junc;
            pairs += ms[m].n_pairs;
            juncs += ms[m].n_junc;
        }
        if (pairs != cs.n_pairs || juncs != J)
            return fail(c, PJB_ERR_STATE, "finish_group: members hold %llu pairs / %llu junctions, the chain %llu / %u", (unsigned long long)pairs,
                        (unsigned long long)juncs, (unsigned long long)cs.n_pairs, J);
    }
    c->junc_seen = std::max(c->junc_seen, co.group ? J / (u32)n_members : J);
    if (f.n_reads > 0) c->junc_per_read = std::max(c->junc_per_read, (double)J / (double)f.n_reads);
    return PJB_OK;
}

// 5. timing: what pjb_get_timing says of this chain (the events' times: collect_commit, when its rows are on their way)
static void collect_timing(Collect &co) {
    pjb_timing &T = co.c->timing;
    const uint8_t *pub = co.S.pub;
    T.sort_passes = co.f.n_pass;
    T.repeats = co.repeats;
    T.repeat_reasons = co.repeat_reasons;
    T.generic_pairs = 0;
    T.generic_reads = 0;
    T.checked_reads = *(const u32 *)(pub + PUB_CHECKED_AT);
    for (u32 k = 0; k < GEN_SHARDS; k++) {
        T.generic_pairs += ((const u32 *)(pub + PUB_GEN_AT))[k];
        T.generic_reads += ((const u32 *)(pub + PUB_GREADS_AT))[k];
    }
    T.position_runs = co.cs.R;
    T.candidates = co.f.lim.dense ? co.cs.n_cand : 0;
}

// 6. commit: the chain's rows are the context's -- their place checked, the row mirror's header, the DMA to the host table, --extra
static int collect_commit(Collect &co) {
    pjb_ctx *c = co.c;
    Flight &f = co.f;
    CtlSlot &S = co.S;
    const ContigStats &cs = co.cs;
    const u32 J = cs.J;
    const size_t old = c->rows_n;
    int rc;
    {
        u32 at[2];
        memcpy(at, S.pub + PUB_BASE_AT, 8);
        if (at[0] != (u32)old || (c->mirror && at[1] != (u32)c->mirror_rows))
            return fail(c, PJB_ERR_STATE, "finish: rows of target %d went to %u (exchange slot %u), expected %zu (%zu)", f.tid, at[0], at[1], old, c->mirror_rows);
    }
    if (c->mirror) { // the rows are in the exchange slot already (k6_rows_out); the header follows, covered by a small wait
        const size_t need = PJB_MIRROR_HEADER_BYTES + (c->mirror_rows + J) * sizeof(pjb_junction_row);
        if (need > c->mirror_cap) return fail(c, PJB_ERR_ARG, "finish: %zu rows do not fit the row mirror (%zu bytes)", c->mirror_rows + J, c->mirror_cap);
        pjb_region_result Rsum; // (the chain's counters: a group's members add up to them)
        memset(&Rsum, 0, sizeof Rsum);
        Rsum.spliced = cs.spliced;
        Rsum.unspliced = cs.unspliced;
        Rsum.sum_len = cs.sum_len;
        Rsum.min_len = cs.min_len;
        Rsum.max_len = cs.max_len;
        mirror_fold(c, Rsum, J);
        HIP_TRY(c, hipMemcpyAsync(c->mirror, c->mirror_hdr, PJB_MIRROR_HEADER_BYTES, hipMemcpyHostToDevice, c->stream4));
        HIP_TRY(c, hipStreamSynchronize(c->stream4));
    }
    if (J) { // the chain's rows: HBM table -> host table, by DMA, behind whatever the caller does next
        if ((rc = rows_pinned_reserve(c, old + J))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->rows_pinned + old, c->rows_table + old, (size_t)J * sizeof(pjb_junction_row), hipMemcpyDeviceToHost, c->stream4));
        c->rows_copy_pending = true;
    }
    c->cur_slot = f.slot;
    if (c->extra && (rc = extra_contig(c, f, co.res, cs.spliced, cs.P, J, old))) return rc;
    c->rows_n = old + J;
    c->last_rows_n = J;
    c->last_slot = f.slot;
    if (c->ktime) ev_collect(c, f.slot);
    if (c->ktime && c->ktime_only.empty())
        for (int k = 0; k < 7; k++) (void)hipEventElapsedTime(&c->timing.stage_ms[k], S.ev[k], S.ev[k + 1]);
    (void)hipEventElapsedTime(&c->timing.total_ms, S.ev[0], S.ev[7]);
    return PJB_OK;
}

// Collects the chain in fl[0] -- waits for it, repeats it when a limit it was queued with turned out too small -- and
// fills one result per member.  A group whose members turn out to hold alignments outside their own sequence is taken
// apart: *redo_single is set and nothing is committed.
static int collect_flight(pjb_ctx *c, pjb_region_result *res, bool *redo_single) {
    Flight &f = c->fl[0];
    const bool group = f.tids.size() > 1;
    Collect co{c, f, c->sl[f.slot], res, group, group ? (int32_t)f.vlen : c->ref_len[(size_t)f.tid]};
    int rc;
    for (;;) {
        if ((rc = collect_wait(co))) return rc;
        if (!co.cs.overflow) break;
        if ((rc = collect_relimit(co))) return rc;
        if (co.apart) break;
    }
    if (!co.apart && (rc = collect_apart(co))) return rc;
    if (co.apart) {
        *redo_single = true;
        return PJB_OK;
    }
    if ((rc = collect_results(co))) return rc;
    collect_timing(co);
    return collect_commit(co);
}

// A member of the group in fl[0] holds alignments outside its own sequence: the members go through one by one, in this chain's slot.
static int flight_members_singly(pjb_ctx *c, pjb_region_result *res) {
    const Flight whole = c->fl[0];
    size_t rows_total = 0;
    if (c->extra) HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the group's extra_pre reads the slot's scratch, which the members' chains write)
    for (size_t m = 0; m < whole.tids.size(); m++) {
        Flight one = Flight();
        one.slot = whole.slot;
        one.tid = whole.tids[m];
        one.tids.assign(1, one.tid);
        prepare_flight(c, one);
        c->fl[0] = one;
        if (one.empty) continue;
        bool again = false;
        const int rc = collect_flight(c, &res[m], &again);
        if (rc) {
            c->fl[0] = whole; // (the caller's guard releases every member)
            return rc;
        }
        rows_total += c->last_rows_n;
    }
    c->fl[0] = whole;
    c->fl[0].queued = c->fl[0].forked = false;
    c->last_rows_n = rows_total; // (pjb_collect_device covers the last member only: a caller of groups uses pjb_collect)
    c->timing.repeat_reasons |= 32; // (the rest of the timing is the last member's chain)
    return PJB_OK;
}

// followers that were taken back (or waited for the chain in fl[0]) are queued now, in order, the first one's place known
static void flight_requeue_followers(pjb_ctx *c) {
    c->fl[0].queued = false; // (fl[0] is still the collected chain: its rows are in the table, it is not "ahead" of anything)
    for (int k = 1; k < c->n_fl; k++) {
        Flight &g = c->fl[k];
        if (g.queued || g.empty) continue;
        // a follower that cannot be queued here is queued again -- and reports its error -- by its own _end; the chain in fl[0]
        // is collected and its rows are in the table
        if (queue_chain(c, g)) break;
    }
}

// a call of pjb_finish_contig_end / pjb_finish_group_end names the oldest queued chain
static int end_check(pjb_ctx *c, const int32_t *tids, int32_t n, const char *who) {
    if (!c) return PJB_ERR_ARG;
    if (!tids || n < 1) return fail(c, PJB_ERR_ARG, "%s: no targets", who);
    bool same = c->n_fl > 0 && (int32_t)c->fl[0].tids.size() == n;
    for (int32_t k = 0; same && k < n; k++) same = c->fl[0].tids[(size_t)k] == tids[k];
    if (!same)
        return fail(c, PJB_ERR_STATE, "%s: target %d (and the %d named with it) is not the oldest queued chain (begin first; collect in the same order, "
                                      "with the same targets)", who, tids[0], n - 1);
    return PJB_OK;
}

static int end_flight(pjb_ctx *c, const int32_t *tids, int32_t n, pjb_region_result *res, const char *who) {
    int rc = end_check(c, tids, n, who);
    if (rc) return rc;
    c->cur_tid = tids[0];
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    struct Closer { // also on every error path: the side stream (k4b_generic) may still read the contig's batches
        pjb_ctx *c;
        bool ok = false;
        ~Closer() {
            if (!ok) { // whatever is queued is in an unknown place now
                (void)hipDeviceSynchronize();
                flight_take_back(c, c->fl[0]);
            }
            const std::vector<int32_t> members = c->fl[0].tids;
            pop_flight(c);
            for (int32_t t : members) close_contig(c, t);
        }
    } closer{c};
    std::vector<pjb_region_result> tmp((size_t)n);
    for (auto &R : tmp) {
        memset(&R, 0, sizeof R);
        R.min_len = INT32_MAX;
    }
    memset(&c->timing, 0, sizeof c->timing);
    c->last_rows_n = 0;
    if (res) memcpy(res, tmp.data(), tmp.size() * sizeof(pjb_region_result));
    if (c->fl[0].empty) {
        rc = mirror_header_only(c, tmp[0]);
        closer.ok = rc == PJB_OK;
        return rc;
    }
    bool redo_single = false;
    if ((rc = collect_flight(c, tmp.data(), &redo_single))) return rc;
    if (redo_single && (rc = flight_members_singly(c, tmp.data()))) return rc;
    if (res) memcpy(res, tmp.data(), tmp.size() * sizeof(pjb_region_result));
    closer.ok = true;
    flight_requeue_followers(c);
    return PJB_OK;
}
