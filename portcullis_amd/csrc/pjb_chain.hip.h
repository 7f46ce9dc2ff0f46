// pjb_chain.hip.h -- the launcher of a `junc` chain: queue_contig as named stages over one chain state (Chain).  Host code only, included by
// pjb_api.hip behind pjb_kernels.hip.h -- and before pjb_flight.hip.h, which calls queue_contig -- and by nothing else.  The stages run in the order they stand in: plan (no HIP call), room (every
// allocation of the chain), front, K1, K2d, sort, the runs (dense ids or full keys), rows.
#pragma once

constexpr unsigned K6_BLOCKS = 128;

// rows of the contigs collected so far plus the most the queued ones can add
static size_t rows_upper_bound(const pjb_ctx *c) {
    size_t n = c->rows_n;
    for (int k = 0; k < c->n_fl; k++)
        if (c->fl[k].queued) n += c->fl[k].lim.junc_limit;
    return n;
}

// blocks until the contig's rows and control block are on the host
static void wait_flight(pjb_ctx *c, Flight &f) {
    if (f.queued) (void)hipEventSynchronize(c->sl[f.slot].ev_done);
}

// The row table lives twice, both grow-only: in HBM, where the rows stream appends each contig's rows (k6_rows_out),
// and in page-locked host memory, filled by a DMA per contig once its row count is known (pjb_finish_contig_end).
// (The kernel used to write the host table itself: 2 MB of PCIe stores per contig that slowed whatever ran beside
// them -- the next contig's k1_count by 40 %.)
// The HBM table has room for the most the queued chains can bring (JL is a bound, 5 - 20 x what a chain brings); the host table
// grows when a chain is collected, to what it brought (rows_pinned_reserve) -- page-locking costs ~0.1 s per GB, and sized by the
// bound the host table of the first 1-Gb chain was 400 MB: 70 ms on the thread that queues the chains, with every copy of the
// program's run waiting behind it, for 17 MB of rows.
static int rows_table_reserve(pjb_ctx *c, Flight &f, u32 JL) {
    size_t old = rows_upper_bound(c);
    if (old + JL <= c->rows_cap) return PJB_OK;
    for (int k = 0; k < c->n_fl; k++) // (the table moves: nothing may be writing to it)
        if (c->fl[k].queued && &c->fl[k] != &f) wait_flight(c, c->fl[k]);
    int rc = rows_sync(c);
    if (rc) return rc;
    old = std::min(old, c->rows_cap);
    const size_t ncap = std::max<size_t>((old + JL) * 3 / 2, 1024);
    pjb_junction_row *nd = (pjb_junction_row *)dev_alloc(c, MEM_ROWS, ncap * sizeof(pjb_junction_row));
    if (!nd) return nomem(c, "row table", ncap * sizeof(pjb_junction_row));
    if (old) {
        // (a device-to-device hipMemcpy may return before it has run, and the chains' streams do not wait for the null stream: without
        // the wait the rows a chain appends below `old` -- `old` is a bound -- could be overwritten by the tail of this copy.  The
        // hipFree that used to follow waited for the whole device; this waits for the copy.)
        HIP_TRY(c, hipMemcpyAsync(nd, c->rows_table, old * sizeof(pjb_junction_row), hipMemcpyDeviceToDevice, c->stream4));
        HIP_TRY(c, hipStreamSynchronize(c->stream4));
    }
    if (c->rows_table) bury(c, c->rows_table); // (nothing reads it any more; hipFree would wait for the device)
    c->rows_table = nd;
    c->rows_cap = ncap;
    return PJB_OK;
}

// What the stages of one chain share.  queue_contig fills it once (chain_plan: everything that is known at entry; chain_room: the
// pointers into the buffers it has made room in) and hands it to every stage.
struct Chain {
    pjb_ctx *c;
    Flight &f;
    CtlSlot &S;
    hipStream_t st, service; // the chain's stream ("overlap" off: the service stream itself); the stream the call came in on
    GroupTab GT;
    bool group, fast_codes, any_x, stage_events, xk1, dense_moved, entropy_forked;
    int n_members;
    int32_t ref_len; // the sequence the chain works on: the target itself, or the group's virtual sequence (every member at its offset)
    KeyFmt kf;
    u32 PL, JL, SL; // (SL: ids the sort's digits cover)
    u32 n_tiles, pair_blocks, range_blocks, slots_lim, n_slices_lim, gen_cap, pack_nn;
    int range_shift; // slices a range of k4_pairs, as a shift (frag_slot)
    size_t n_words;
    int64_t row_base, mirror_base;
    // the sort's plan: as few passes as the widest digit allows, bits spread evenly; the run route (ContigLimits::run_sort) sorts its
    // run list instead of the pairs -- fewer tiles (plan_tiles), the digits those of the run list's keys
    u32 rs_tiles, run_cap, ro_tiles, plan_tiles;
    bool run_route, first_hist_done;
    int sort_bits, n_pass, pass_bits[16], cur; // (radix_max_bits >= 4 and keys of 64 bits: 16 passes at most)
    RunOut ro;
    u64 *ro_total, *ro_key[2];
    u32 *run_dest, *ro_idx[2];
    // into the slot's buffers (chain_room)
    u64 *d_err;
    ContigStats *d_cs;
    const u32 *d_P, *d_J, *d_slots;
    MemberStats *d_members;
    u32 *d_member_junc, *d_tile_lo, *d_gen_cnt;
    Pairs pr;
};

// c->stream, c->scan_tiles and c->cur_pool as they were, on every return path: everything the LAUNCH macro and run_scan do follows them
struct ChainScope {
    pjb_ctx *c;
    hipStream_t stream = c->stream;
    Buf *scan_tiles = c->scan_tiles;
    int pool = c->cur_pool;
    ~ChainScope() {
        c->stream = stream;
        c->scan_tiles = scan_tiles;
        c->cur_pool = pool;
    }
};

// stage boundaries are timed only under full instrumentation: an event between two kernels costs a ~6 us bubble
#define STAGE_EVENT(k)                                                     \
    do {                                                                   \
        if (ch.stage_events) HIP_TRY(c, hipEventRecord(S.ev[k], ch.st));   \
    } while (0)

// `fn` beside what follows on the chain's stream: the side stream waits for `ev_fork`, recorded here, runs fn (LAUNCH follows c->stream)
// and records `ev_join`; `forked` tells whoever needs fn's results to wait for that.  "overlap" off: fn where it stands.
template <typename Fn>
static int chain_fork(Chain &ch, hipEvent_t ev_fork, hipEvent_t ev_join, bool &forked, Fn fn) {
    pjb_ctx *c = ch.c;
    if (!c->side_stream) return fn(ch);
    HIP_TRY(c, hipEventRecord(ev_fork, ch.st));
    HIP_TRY(c, hipStreamWaitEvent(ch.S.side, ev_fork, 0));
    c->stream = ch.S.side;
    forked = true;
    const int rc = fn(ch);
    c->stream = ch.st;
    if (rc) return rc;
    HIP_TRY(c, hipEventRecord(ev_join, ch.S.side));
    return PJB_OK;
}

// 1. plan: what the chain is, from the flight and its limits alone -- no HIP call
static int chain_plan(Chain &ch) {
    pjb_ctx *c = ch.c;
    Flight &f = ch.f;
    const ContigLimits &lim = f.lim;
    ch.service = c->stream;
    ch.st = c->side_stream ? ch.S.main : c->stream;
    ch.n_tiles = f.n_tiles;
    ch.n_members = (int)f.tids.size();
    ch.group = ch.n_members > 1;
    ch.ref_len = ch.group ? (int32_t)f.vlen : c->ref_len[(size_t)f.tid];
    GroupTab &GT = ch.GT;
    memset(&GT, 0, sizeof GT);
    GT.n = ch.n_members;
    bool all_codes = true;
    ch.any_x = false;
    for (int m = 0; m < ch.n_members; m++) {
        const Contig &g = c->contigs[(size_t)f.tids[(size_t)m]];
        GT.voff[m] = f.voff[(size_t)m];
        GT.len[m] = (int32_t)g.len;
        GT.tid[m] = f.tids[(size_t)m];
        GT.d[m] = g.d;
        GT.codes[m] = g.codes;
        GT.codes2[m] = g.codes2;
        if (g.any_exc) GT.exc_members |= 1u << m;
        all_codes = all_codes && g.codes != nullptr;
        ch.any_x = ch.any_x || g.has_x;
    }
    ch.fast_codes = all_codes && !ch.any_x; // (else: no read is "simple", every pair takes k4b_generic's byte-wise walks)
    ch.kf = lim.kf;
    const u32 PL = ch.PL = lim.pair_limit, JL = ch.JL = lim.junc_limit;
    ch.SL = lim.sort_limit && lim.sort_limit < JL ? lim.sort_limit : JL;
    // the place of this contig's rows: known here if nothing is queued ahead of it, else it follows on the device
    bool ahead = false;
    for (int k = 0; k < c->n_fl; k++) ahead |= c->fl[k].queued && &c->fl[k] != &f;
    ch.row_base = ahead ? -1 : (int64_t)c->rows_n;
    ch.mirror_base = ahead ? -1 : (int64_t)c->mirror_rows;
    ch.pair_blocks = std::max<u32>(1, (PL + 255) / 256);
    // entries per sub-list (list_cap_forced: the test hook pjb_set_option("list_cap", n) -- a first attempt with a room that overflows)
    ch.gen_cap = lim.list_cap ? lim.list_cap : (c->list_cap_forced ? c->list_cap_forced : gen_list_cap(PL));
    ch.pack_nn = (u64)ch.n_tiles * K1_TILE < (1ull << 28) ? 1u : 0u; // (EmitLists::pack_nn: the slots of the tiles' spliced lists fit 28 bits)
    ch.range_shift = c->pair_range_shift;
    ch.slots_lim = frag_slots_limit(JL, PL, ch.range_shift);
    ch.range_blocks = std::max<u32>(1, (frag_ranges(PL, ch.range_shift) + 3) / 4); // k4_pairs: a wavefront a range
    ch.n_slices_lim = (PL + 63) / 64 + 1;
    ch.n_words = ((size_t)std::max(ch.ref_len, 1) + 63) / 64; // K2d's bitmap
    ch.stage_events = c->ktime && c->ktime_only.empty();
    // with PJB_FLAG_EXTRA k1_count also leaves what the records span, the first time (a chain that is queued again leaves that alone: the
    // service stream may be reading it)
    ch.xk1 = c->extra && !c->extra_dense_only && !ch.group && !f.x_k1 && !f.x_pre;
    // ---- the sort.  The run route's list has room for an eighth of the pair limit and 64 entries a tile (chains have 0.4 % of their pairs)
    ch.rs_tiles = std::max<u32>(1, (PL + RS_TILE - 1) / RS_TILE);
    ch.run_route = lim.dense && lim.run_sort;
    ch.run_cap = (u32)std::min<u64>((u64)PL / 8 + 64ull * ch.rs_tiles, 0xfff00000ull);
    ch.ro_tiles = (ch.run_cap + RS_TILE - 1) / RS_TILE;
    if (ch.run_route) { // (else: all of `ro` stays zero, and window 0 tells kd_assign to count the first digit)
        ch.ro.cap = ch.run_cap;
        ch.ro.window = c->run_window ? std::min<u32>(c->run_window, RUN_W) : RUN_W;
        ch.ro.tile_bits = std::max(1, bits_of((uint64_t)ch.rs_tiles));
    }
    // (dense ids: the sort works on 15-19 bits instead of the keys' 46-48; kd_assign counts the first digit, or, on the run route, leaves
    // the tiles' id runs)
    ch.sort_bits = lim.dense ? std::max(1, bits_of((uint64_t)ch.SL)) + (ch.run_route ? ch.ro.tile_bits : 0) : ch.kf.total_bits;
    ch.plan_tiles = ch.run_route ? ch.ro_tiles : ch.rs_tiles;
    ch.first_hist_done = lim.dense && !ch.run_route;
    ch.n_pass = std::max(1, (ch.sort_bits + c->radix_max_bits - 1) / c->radix_max_bits);
    for (int p = 0; p < ch.n_pass; p++) ch.pass_bits[p] = ch.sort_bits / ch.n_pass + (p < ch.sort_bits % ch.n_pass ? 1 : 0);
    return PJB_OK;
}

// the run route's scratch, carved from one buffer of the slot: counters, the tiles' entries, the run list, its sort's ping-pong buffers
// (one tile of slack each: rs_scatter loads whole tiles unguarded)
static RunOut run_carve(Chain &ch, int &rc) {
    pjb_ctx *c = ch.c;
    CtlSlot &S = ch.S;
    RunOut ro = ch.ro;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const u32 rs_tiles = ch.rs_tiles, run_cap = ch.run_cap;
    const size_t slack = (size_t)run_cap + RS_TILE;
    const size_t at_tf = 256, at_tn = at_tf + al((size_t)rs_tiles * 4), at_key = at_tn + al((size_t)rs_tiles * 4), at_cnt = at_key + al(slack * 8),
                 at_dest = at_cnt + al((size_t)run_cap * 4), at_k0 = at_dest + al((size_t)run_cap * 4), at_k1 = at_k0 + al(slack * 8),
                 at_i0 = at_k1 + al(slack * 8), at_i1 = at_i0 + al(slack * 4), at_end = at_i1 + al(slack * 4);
    if ((rc = ensure(c, S.runs, at_end))) return ro;
    uint8_t *b = (uint8_t *)S.runs.p;
    ro.n_runs = (u32 *)b;
    ch.ro_total = (u64 *)(b + 8);
    ro.tile_first = (u32 *)(b + at_tf);
    ro.tile_n = (u32 *)(b + at_tn);
    ro.key = (u64 *)(b + at_key);
    ro.cnt = (u32 *)(b + at_cnt);
    ch.run_dest = (u32 *)(b + at_dest);
    ch.ro_key[0] = (u64 *)(b + at_k0);
    ch.ro_key[1] = (u64 *)(b + at_k1);
    ch.ro_idx[0] = (u32 *)(b + at_i0);
    ch.ro_idx[1] = (u32 *)(b + at_i1);
    return ro;
}

// 2. room: every buffer of the chain at its size -- all of them follow from the limits --, so that a failed allocation returns before
// anything of the chain is on a stream (an outgrown buffer is buried, not freed: an earlier chain that still reads it is not disturbed)
static int chain_room(Chain &ch) {
    pjb_ctx *c = ch.c;
    Flight &f = ch.f;
    CtlSlot &S = ch.S;
    const std::vector<DevBatch> &batches = f.batches;
    const u32 PL = ch.PL, JL = ch.JL, n_tiles = ch.n_tiles;
    const size_t n_words = ch.n_words, N = (size_t)f.n_reads;
    const u32 plan_tiles = ch.plan_tiles;
    const int dbits = ch.pass_bits[0]; // (the first digit is the widest)
    const bool dense = f.lim.dense;
    int rc;
    if (batches.size() + 2 > S.batches_pinned_cap) { // (+ 2 descriptors' worth of room for a group's tile ranges: 33 words)
        if (S.batches_pinned) (void)hipHostFree(S.batches_pinned);
        S.batches_pinned = nullptr;
        S.batches_pinned_cap = 0;
        const size_t cap = std::max<size_t>(batches.size() * 2 + 2, 16);
        HIP_TRY(c, hipHostMalloc((void **)&S.batches_pinned, cap * sizeof(DevBatch), hipHostMallocDefault));
        S.batches_pinned_cap = cap;
    }
    memcpy(S.batches_pinned, batches.data(), batches.size() * sizeof(DevBatch));
    // zeroed when they are made, once per slot (the cursor: per context): the chain's kernels leave them as the next chain needs them
    const struct { Buf *b; size_t bytes; bool whole; } once[] = {
        {&S.scan_parts, sizeof(ScanPart) * K1S_BLOCKS, false},
        {&c->b_cursor, sizeof(RowCursor), false}, // (blocks_done)
        {&S.members, GROUP_MAX * sizeof(MemberStats) + GROUP_MAX * 4 + (GROUP_MAX + 1) * 4, true}, // (member_junc: k6_rows_out (publish_chain) leaves it zeroed for the next chain)
    };
    for (const auto &o : once) {
        if (o.b->p) continue;
        if ((rc = ensure(c, *o.b, o.bytes))) return rc;
        HIP_TRY(c, hipMemset(o.b->p, 0, o.whole ? o.b->cap : o.bytes));
        HIP_TRY(c, hipStreamSynchronize(nullptr));
    }
    const void *was[3] = {S.bitmap.p, S.ends.p, S.pagecnt.p};
    const struct { Buf *b; size_t bytes; bool on = true; } room[] = { // (on: the row's condition)
        {&S.batches, batches.size() * sizeof(DevBatch)},
        {&S.cstats, sizeof(ContigStats)},
        {&S.err, 8},
        {&S.tile_cnt, (size_t)n_tiles * 4},
        {&S.tile_stats, (size_t)n_tiles * sizeof(TileStats)},
        {&S.tile_soff, ((size_t)n_tiles + 1) * 4},
        {&S.chunk_tile, ((size_t)n_tiles * (K1_TILE / 256) + 4) * 4},
        {&S.splidx, (size_t)n_tiles * K1_TILE * 4},
        {&S.splpoff, (size_t)n_tiles * K1_TILE * 4},
        {&S.splrec, (size_t)n_tiles * K1_TILE * 16},
        {&S.total, 8},
        // ---- pair-sized buffers (one sort tile of slack: rs_scatter loads whole tiles unguarded)
        {&S.okey, ((size_t)PL + RS_TILE) * 8}, // the pairs' keys as emitted (BAM order): kept, the sort works on copies
        {&S.key[0], ((size_t)PL + RS_TILE) * 8},
        {&S.key[1], ((size_t)PL + RS_TILE) * 8},
        {&S.idx[0], ((size_t)PL + RS_TILE) * 4},
        {&S.idx[1], ((size_t)PL + RS_TILE) * 4},
        {&S.rec, ((size_t)PL + 1) * sizeof(PairRec)},
        {&S.jid, (size_t)PL * 4 + 16},
        {&S.jidbam, ((size_t)PL + RS_TILE) * 4}, // (the sort's first pass loads whole tiles)
        {&S.g, (size_t)PL * 4 + 16, c->extra},
        {&S.seg, ((size_t)PL + 1) * 4},
        {&S.runfirst, ((size_t)PL + 1) * 4},
        {&S.runstart, ((size_t)PL + 1) * 4},
        {&S.ent, (size_t)PL * 8 + 16},
        {&S.genlist, (size_t)ch.gen_cap * GEN_SHARDS * 8 * 3}, // (three lists: EmitLists)
        {&S.gencount, GEN_SHARDS * GEN_CNT_STRIDE * 4},        // a line per sub-list: reads, pairs
        // ---- junction-sized buffers
        {&S.frag, (size_t)ch.slots_lim * F_WORDS * 4},
        {&S.fragj, (size_t)ch.slots_lim * 4},
        {&S.acc, (size_t)JL * F_WORDS * 4 + 16},
        {&S.ancl, (size_t)JL * 4 + 16},
        {&S.ancr, (size_t)JL * 4 + 16},
        {&S.jkey, (size_t)JL * 8 + 16},
        {&S.rows, (size_t)JL * sizeof(pjb_junction_row) + 16},
        {&S.entsum, (size_t)JL * 8 + 16},
        // ---- K2d's bitmap and end slots, the dense tail's boundary masks
        {&S.bitmap, n_words * 8 + 16, dense},
        {&S.wrank, n_words * 4 + 16, dense},
        {&S.pagecnt, ((n_words >> KD_PAGE_SHIFT) + 1) * 4 + 16, dense},
        {&S.pagerank, ((n_words >> KD_PAGE_SHIFT) + 1) * 4 + 16, dense},
        {&S.ends, (size_t)JL * DENSE_ENDS * 4 + 32, dense},
        {&S.firstid, (size_t)JL * 4 + 16, dense},
        {&S.masks, (size_t)ch.n_slices_lim * 8 * 2 + (size_t)ch.n_slices_lim * 4, dense},
        // ---- the sort's digit tables
        {&S.hist, (size_t)plan_tiles * (1u << dbits) * 4},
        {&S.hist_scan, (size_t)plan_tiles * (1u << dbits) * 4},
        {&S.bintotal, (size_t)4 << dbits},
        {&S.hist_part, (size_t)((plan_tiles + RSP_TILES - 1) / RSP_TILES) * (1u << dbits) * 4},
        // ---- --extra: what the records span (XOut)
        {&S.x_q, N + 16, ch.xk1},
        {&S.x_spos, N * 4 + 16, ch.xk1},
        {&S.x_send, N * 4 + 16, ch.xk1},
        {&S.x_zlist, (size_t)X_ZCAP * 8, ch.xk1},
        {&S.x_scnt, X_SCNT_BYTES, ch.xk1},
    };
    for (const auto &r : room)
        if (r.on && (rc = ensure(c, *r.b, r.bytes))) return rc;
    ch.dense_moved = was[0] != S.bitmap.p || was[1] != S.ends.p || was[2] != S.pagecnt.p;
    if (ch.run_route) {
        ch.ro = run_carve(ch, rc);
        if (rc) return rc;
    }
    if ((rc = rows_table_reserve(c, f, JL))) return rc;
    if (!S.pub) {
        HIP_TRY(c, hipHostMalloc((void **)&S.pub, PUB_BYTES, hipHostMallocMapped | hipHostMallocPortable));
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, S.pub, 0) != hipSuccess || !dp) return fail(c, PJB_ERR_HIP, "hipHostGetDevicePointer(control block) failed");
        S.pub_dev = (uint8_t *)dp;
    }
    ch.d_members = (MemberStats *)S.members.p;
    ch.d_member_junc = (u32 *)(ch.d_members + GROUP_MAX);
    ch.d_tile_lo = ch.d_member_junc + GROUP_MAX;
    ch.d_err = (u64 *)S.err.p;
    ch.d_cs = (ContigStats *)S.cstats.p;
    ch.d_P = &ch.d_cs->P;
    ch.d_J = &ch.d_cs->J;
    ch.d_slots = &ch.d_cs->n_slots;
    ch.d_gen_cnt = (u32 *)S.gencount.p;
    ch.pr.key = (u64 *)S.okey.p;
    ch.pr.rec = (PairRec *)S.rec.p;
    ch.pr.g = c->extra ? (u32 *)S.g.p : (u32 *)nullptr;
    return PJB_OK;
}

// 3. front: the chain's inputs and the rest state of what it counts in
static int chain_front(Chain &ch) {
    pjb_ctx *c = ch.c;
    Flight &f = ch.f;
    CtlSlot &S = ch.S;
    const hipStream_t st = ch.st;
    const size_t n_batches = f.batches.size();
    // (records still being produced on the service stream -- host copies, BAM ingest -- come first)
    bool on_service = false;
    for (int32_t t : f.tids) {
        auto oit = c->open.find(t);
        on_service = on_service || (oit != c->open.end() && oit->second.on_main_stream);
    }
    if (st != ch.service && on_service) {
        HIP_TRY(c, hipEventRecord(c->ev_front, ch.service));
        HIP_TRY(c, hipStreamWaitEvent(st, c->ev_front, 0));
    }
    HIP_TRY(c, hipMemcpyAsync(S.batches.p, S.batches_pinned, n_batches * sizeof(DevBatch), hipMemcpyHostToDevice, st));
    if (ch.group) { // (the tile ranges of the members; lives behind the batch descriptors in the page-locked staging block)
        u32 *h_lo = (u32 *)(S.batches_pinned + n_batches);
        for (int m = 0; m <= ch.n_members; m++) h_lo[m] = f.tile_lo[(size_t)m];
        HIP_TRY(c, hipMemcpyAsync(ch.d_tile_lo, h_lo, (size_t)(ch.n_members + 1) * 4, hipMemcpyHostToDevice, st));
    }
    if (!S.at_rest) {
        HIP_TRY(c, hipMemsetAsync(S.err.p, 0xff, 8, st));
        HIP_TRY(c, hipMemsetAsync(S.gencount.p, 0, GEN_SHARDS * GEN_CNT_STRIDE * 4, st));
        HIP_TRY(c, hipMemsetAsync(ch.d_member_junc, 0, GROUP_MAX * 4, st));
    }
    S.at_rest = false; // until k6_rows_out (publish_chain) is queued
    HIP_TRY(c, hipEventRecord(S.ev[0], st));
    // K2d's bitmap and end slots (all-clear at rest): k1_emit sets the bits
    if (f.lim.dense) {
        if (!S.dense_at_rest || ch.dense_moved) { // (first use, new memory, or a chain that broke off)
            HIP_TRY(c, hipMemsetAsync(S.bitmap.p, 0, S.bitmap.cap, st));
            HIP_TRY(c, hipMemsetAsync(S.pagecnt.p, 0, S.pagecnt.cap, st));
            HIP_TRY(c, hipMemsetAsync(S.ends.p, 0xff, S.ends.cap, st));
        }
        S.dense_at_rest = false; // until kd_reset is queued
    }
    f.pr = ch.pr;
    return PJB_OK;
}

// 4. K1: count, scan, emit -- and the reads k1_emit left
static int chain_k1(Chain &ch) {
    pjb_ctx *c = ch.c;
    Flight &f = ch.f;
    CtlSlot &S = ch.S;
    const std::vector<DevBatch> &batches = f.batches;
    const hipStream_t st = ch.st;
    const GroupTab &GT = ch.GT;
    const KeyFmt kf = ch.kf;
    const u32 n_tiles = ch.n_tiles;
    const bool k1_late = getenv("PJB_K1_SERIAL_LATE") != nullptr; // (experiment: the next chain's K1 behind k1_generic)
    // ---- K1a: count (a group's members: a tile whose alignments leave the member's own sequence is flagged); with
    // PJB_FLAG_EXTRA the first time also what the records span
    XOut xo = {nullptr, nullptr, nullptr, nullptr, 0, nullptr};
    if (ch.xk1) {
        const size_t N = (size_t)f.n_reads;
        HIP_TRY(c, hipMemsetAsync((uint8_t *)S.x_q.p + N, 0, 1, c->stream));
        HIP_TRY(c, hipMemsetAsync(S.x_scnt.p, 0, sizeof(SparseCounters) + sizeof(ExtraCounters), c->stream));
        xo = XOut{(int32_t *)S.x_spos.p, (int32_t *)S.x_send.p, (uint8_t *)S.x_q.p, (u32 *)S.x_zlist.p, X_ZCAP, (SparseCounters *)S.x_scnt.p};
    }
    // K1 of one chain fills the chip: the chains' K1 stages follow each other (this chain's waits for the last queued chain's),
    // and what comes behind a chain's K1 -- many small kernels -- runs beside the NEXT chain's K1 instead of beside its own twin
    if (c->k1_serial && c->last_k1_ev) HIP_TRY(c, hipStreamWaitEvent(st, c->last_k1_ev, 0));
    // (one launch over the chain's tiles: a block finds its batch from the tile index)
    if (ch.xk1)
        LAUNCH(c, "k1_count", k1_count<true>, dim3(n_tiles), dim3(K1C_T), (const DevBatch *)S.batches.p, (int)batches.size(), (u32 *)S.tile_cnt.p, (TileStats *)S.tile_stats.p,
               (u32 *)S.splidx.p, (u32 *)S.splpoff.p, (uint4 *)S.splrec.p, ch.d_err, GT, 0, xo);
    else
        LAUNCH(c, "k1_count", k1_count<false>, dim3(n_tiles), dim3(K1C_T), (const DevBatch *)S.batches.p, (int)batches.size(), (u32 *)S.tile_cnt.p, (TileStats *)S.tile_stats.p,
               (u32 *)S.splidx.p, (u32 *)S.splpoff.p, (uint4 *)S.splrec.p, ch.d_err, GT, ch.group ? 1 : 0, xo);
    if (ch.xk1) {
        HIP_TRY(c, hipEventRecord(S.ev_xk1, c->stream));
        f.x_k1 = true;
    }
    LAUNCH(c, "k1_scan_tiles", k1_scan_tiles, dim3(c->k1s_blocks_forced ? (u32)c->k1s_blocks_forced : k1s_blocks(n_tiles)), dim3(K1S_THREADS), (u32 *)S.tile_cnt.p, (const TileStats *)S.tile_stats.p,
           n_tiles, ch.d_cs, ch.PL, kf, ch.group ? INT32_MAX - 1 : ch.ref_len, (const u64 *)nullptr, (u32 *)S.tile_soff.p, (u32 *)S.chunk_tile.p,
           (ScanPart *)S.scan_parts.p, ++S.scan_epoch, c->window_skip ? 1u : 0u);
    // ---- K1b: emit (coordinates in the group's virtual sequence): keys, the pairs' records -- complete for reads of the
    // simple shape --, K2d's candidate keys (free until the first scatter; they are used up before it), the list of
    // reads for k4b_generic
    EmitLists el;
    el.cand = f.lim.dense ? (u64 *)S.key[1].p : (u64 *)nullptr;
    el.bitmap = f.lim.dense ? (u64 *)S.bitmap.p : (u64 *)nullptr;
    el.page_cnt = f.lim.dense ? (u32 *)S.pagecnt.p : (u32 *)nullptr;
    el.cand_anc = (u64 *)S.ent.p; // (a pair-sized scratch buffer nothing else uses at this point)
    el.gen_list = (u64 *)S.genlist.p;
    el.gen_cnt = ch.d_gen_cnt;
    el.gen_cap = ch.gen_cap;
    el.pack_nn = ch.pack_nn;
    // (one launch per chain -- per K1E_MAXB batches --: the blocks stride over the batches' trips of 256 spliced reads; a tile holds
    // ~300 spliced reads = 1.2 trips: a grid of half the tiles keeps two or three trips per block)
    for (size_t b0 = 0; b0 < batches.size(); b0 += K1E_MAXB) {
        const size_t nb = std::min<size_t>(K1E_MAXB, batches.size() - b0);
        u64 reads = 0;
        for (size_t bi = b0; bi < b0 + nb; bi++) reads += (u64)batches[bi].n;
        const u32 nt = (u32)std::min<u64>((reads + K1_TILE - 1) / K1_TILE + nb, 0x7fffffffu);
        // (tiles of reads per block: 2 / 4 / 8 / 16 = 9.17 / 8.96 / 8.94 / 9.05 ms a step, profiles/r05q_*; with round 6's 2-bit compare
        // 4 / 8 / 12 / 16 / 32 / 64 = 7.25 - 7.37 / 7.15 - 7.17 / 7.32 / 7.32 / 7.37 / 8.02: fewer, longer blocks make the kernel itself
        // faster still -- 970 us a chain in the step at 16 against 1 085 at 8 -- but the step no shorter: profiles/r06_k1_experiments.txt)
        static const u32 tiles_per_block = getenv("PJB_K1E_TILES") ? (u32)std::max(1, atoi(getenv("PJB_K1E_TILES"))) : 8u;
        const u32 grid = std::max<u32>(1, std::min<u32>(nt, std::max<u32>(1024, nt / tiles_per_block)));
        LAUNCH(c, "k1_emit", k1_emit, dim3(grid), dim3(256), (const DevBatch *)S.batches.p + b0, (int)nb, n_tiles, (const u32 *)S.tile_cnt.p,
               (const u32 *)S.tile_soff.p, (const u32 *)S.chunk_tile.p, (const u32 *)S.splidx.p, (const u32 *)S.splpoff.p, (const uint4 *)S.splrec.p, ch.pr, el, kf,
               GT, ch.fast_codes ? 1 : 0, (int)c->cfg.orientation, ch.d_err, ch.d_cs);
    }
    // (the next chain's K1 may start here: k1_generic -- a few reads walked by a few wavefronts, waiting for their loads -- runs beside
    // its k1_count, which is a stream)
    if (c->k1_serial && !k1_late) {
        HIP_TRY(c, hipEventRecord(S.ev_k1, st));
        c->last_k1_ev = S.ev_k1;
    }
    // (per-member counters of a group: off the K1 stage -- beside the next chain's k1_count -- and before k5_finalize counts the
    // members' junctions into them)
    if (ch.group)
        LAUNCH(c, "kg_member_stats", kg_member_stats, dim3((unsigned)ch.n_members), dim3(256), (const u32 *)S.tile_cnt.p, (const TileStats *)S.tile_stats.p,
               (const u32 *)ch.d_tile_lo, ch.n_members, ch.d_members, n_tiles, (const ContigStats *)ch.d_cs);
    // the reads k1_emit left: one launch over the chain's third list (the blocks stride over it)
    LAUNCH(c, "k1_generic", k1_generic, dim3(std::min<u32>(std::max<u32>(1, (u32)(((u64)ch.gen_cap * GEN_SHARDS + K1E_T - 1) / K1E_T)), 1536u /* six blocks a CU; 512 .. 3072 measured: no difference */)), dim3(K1E_T),
           (const DevBatch *)S.batches.p, (int)batches.size(), (const u32 *)S.splidx.p, (const uint4 *)S.splrec.p, ch.pr, el, kf, GT, ch.fast_codes ? 1 : 0,
           (int)c->cfg.orientation, ch.d_err, ch.d_cs);
    if (c->k1_serial && k1_late) {
        HIP_TRY(c, hipEventRecord(S.ev_k1, st));
        c->last_k1_ev = S.ev_k1;
    }
    STAGE_EVENT(1);
    return PJB_OK;
}

// k4b_generic: the pairs that need the generic walks, in BAM order, as soon as junction ids and anchors exist
static int chain_k4b(Chain &ch) {
    pjb_ctx *c = ch.c;
    CtlSlot &S = ch.S;
    const u32 gen_grid = std::min<u32>(2 * (u32)(((u64)ch.gen_cap * GEN_SHARDS + 255) / 256), 2560u); // (the blocks stride over the lists' entries)
    LAUNCH(c, "k4b_generic", k4b_generic, dim3(gen_grid), dim3(256), (const u64 *)S.genlist.p, (const u32 *)ch.d_gen_cnt, ch.gen_cap, (const u64 *)ch.pr.key,
           ch.pr.rec, (const u32 *)S.jidbam.p, ch.kf, (const DevBatch *)S.batches.p, (int)ch.f.batches.size(), (const int32_t *)S.ancl.p, (const int32_t *)S.ancr.p,
           ch.GT, ch.any_x ? 1 : 0, ch.any_x ? 0 : 1, ch.d_err, (const ContigStats *)ch.d_cs, ch.pack_nn, (const u32 *)S.splidx.p, (const uint4 *)S.splrec.p);
    return PJB_OK;
}

// 5. K2d: ordered dense junction ids (a chain that sorts the full keys has none), k4b_generic beside the sort on the side stream
static int chain_k2d(Chain &ch) {
    pjb_ctx *c = ch.c;
    Flight &f = ch.f;
    CtlSlot &S = ch.S;
    if (!f.lim.dense) return PJB_OK;
    const KeyFmt kf = ch.kf;
    const u32 JL = ch.JL;
    const size_t n_words = ch.n_words;
    int rc;
    const u32 cand_blocks = std::min<u32>(ch.pair_blocks, 1024u); // (a few candidates per junction: these kernels stride)
    const u64 *okey = (const u64 *)ch.pr.key;
    u64 *cand = (u64 *)S.key[1].p; // (k1_emit left the candidate keys here, and their starts' bits in the bitmap)
    // (ranks of the bitmap's words: a prefix sum over the pages' counts of starts, then the words of the pages that hold one)
    const u32 n_pages = (u32)((n_words + ((size_t)1 << KD_PAGE_SHIFT) - 1) >> KD_PAGE_SHIFT);
    if ((rc = run_scan(c, "kd_rank", ArrU32Fn{(const u32 *)S.pagecnt.p}, ExclusiveU32Sink{(u32 *)S.pagerank.p}, (u64)n_pages, (u64 *)S.total.p)))
        return rc;
    LAUNCH(c, "kd_rank_pages", kd_rank_pages, dim3((n_pages + 3) / 4), dim3(256), (const u64 *)S.bitmap.p, (const u32 *)S.pagecnt.p, (const u32 *)S.pagerank.p,
           (u32 *)S.wrank.p, n_pages, (u32)n_words);
    u32 *cand_rank = (u32 *)S.idx[1].p; // (free until the first scatter as well)
    LAUNCH(c, "kd_ends", kd_ends, dim3(cand_blocks), dim3(256), (const u64 *)cand, kf, (const u64 *)S.bitmap.p, (const u32 *)S.wrank.p, JL,
           (u32 *)S.ends.p, cand_rank, ch.d_cs);
    if ((rc = run_scan(c, "kd_first", EndsCountFn{(const u32 *)S.ends.p}, FirstIdSink{(u32 *)S.firstid.p, (int32_t *)S.ancl.p, (int32_t *)S.ancr.p},
                       (u64)JL, (u64 *)S.total.p)))
        return rc;
    LAUNCH(c, "kd_table", kd_table, dim3(cand_blocks), dim3(256), (const u64 *)cand, (const u64 *)S.ent.p, (const u32 *)cand_rank, kf, JL,
           (const u32 *)S.ends.p, (const u32 *)S.firstid.p, (const u64 *)S.total.p, (u64 *)S.jkey.p, (int32_t *)S.ancl.p, (int32_t *)S.ancr.p, ch.d_cs,
           (const u32 *)ch.d_gen_cnt, ch.gen_cap, ch.SL, ch.ro.n_runs, ch.range_shift);
    // (a block per tile of the sort: it leaves the tile's counts of the ids' first digit -- the first pass of the sort has no rs_hist --,
    // or, on the run route, the tile's id runs)
    LAUNCH(c, "kd_assign", kd_assign, dim3(ch.rs_tiles), dim3(256), okey, ch.d_P, kf, (const u64 *)S.bitmap.p, (const u32 *)S.wrank.p,
           (const u32 *)S.ends.p, (const u32 *)S.firstid.p, JL, (const u64 *)S.total.p, (u32 *)S.jidbam.p, (u32 *)S.acc.p, (const u64 *)S.jkey.p,
           (const int32_t *)S.ancl.p, (const int32_t *)S.ancr.p, ch.d_err, ch.d_cs, ch.run_route ? 0 : ch.pass_bits[0], (u32 *)S.hist.p, ch.ro);
    // (the main stream has just produced jid_bam and the anchors)
    if ((rc = chain_fork(ch, S.ev_fork, S.ev_join, f.forked, chain_k4b))) return rc;
    LAUNCH(c, "kd_reset", kd_reset, dim3(cand_blocks), dim3(256), (const u64 *)cand, (const u32 *)cand_rank, kf, JL, (const ContigStats *)ch.d_cs,
           (u64 *)S.bitmap.p, (u32 *)S.ends.p, (u32 *)S.pagecnt.p);
    S.dense_at_rest = true;
    return PJB_OK;
}

// (the run route's launches go by names of their own, kept in this table: bench.py's byte formulas are written for the pair-sized
// passes and describe none of them -- they appear under its kernels_without_formula)
static const char *const rs_names[4] = {"rs_hist", "rs_panel_sums", "rs_panel_scan", "rs_scatter"};
static const char *const ro_names[6] = {"ro_hist", "ro_panel_sums", "ro_panel_scan", "ro_scatter", "ro_offsets", "rs_place"};

// one digit pass over keys of type K and their pair indices
template <typename K>
static int sort_pass(Chain &ch, const void *kin_v, void *kout_v, const u32 *vin, u32 *vout, int shift, int bits, const u32 *d_n, u32 tiles,
                     const char *const *names) {
    pjb_ctx *c = ch.c;
    CtlSlot &S = ch.S;
    const K *kin = (const K *)kin_v;
    K *kout = (K *)kout_v;
    if (!(shift == 0 && ch.first_hist_done)) // (dense ids: kd_assign counted the first digit)
        LAUNCH(c, names[0], rs_hist<K>, dim3(tiles), dim3(256), kin, d_n, shift, bits, (u32 *)S.hist.p, tiles);
    {
        const u32 nb = 1u << bits, n_panels = (tiles + RSP_TILES - 1) / RSP_TILES;
        LAUNCH(c, names[1], rs_panel_sums, dim3(n_panels, (nb + 255) / 256), dim3(256), (const u32 *)S.hist.p, tiles, nb, (u32 *)S.hist_part.p);
        LAUNCH(c, names[2], rs_panel_scan, dim3(n_panels, (nb + 255) / 256), dim3(256), (const u32 *)S.hist.p, (const u32 *)S.hist_part.p, tiles, nb,
               (u32 *)S.hist_scan.p, (u32 *)S.bintotal.p);
    }
#define RS_SCATTER(B)                                                                                                                          \
    LAUNCH_LDS(c, names[3], (rs_scatter<B, K>), dim3(tiles), dim3(256), rs_scatter_lds_bytes(bits, sizeof(K)), kin, vin, kout, vout, d_n, \
               shift, bits, (const u32 *)S.hist_scan.p, (const u32 *)S.bintotal.p, tiles)
    switch (bits) { // the usual digit widths get an unrolled match loop
    case 9: RS_SCATTER(9); break;
    case 10: RS_SCATTER(10); break;
    case 11: RS_SCATTER(11); break;
    default: RS_SCATTER(0); break;
    }
#undef RS_SCATTER
    return PJB_OK;
}

// 6. sort: radix sort of (key, pair index).  Dense ids are 32-bit keys: pass 0 reads them where kd_assign left them (BAM order;
// k4b_generic reads that array beside the sort, so no pass writes to it), the ping-pong buffers are the first halves of the 64-bit key
// buffers.  The run route sorts its run list -- 64-bit keys whatever the chain's size, its length is on the device -- and places the pairs
// in one pass.
static int chain_sort(Chain &ch) {
    pjb_ctx *c = ch.c;
    Flight &f = ch.f;
    CtlSlot &S = ch.S;
    const RunOut &ro = ch.ro;
    int rc = PJB_OK, cur = 0, shift = 0;
    for (int p = 0; p < ch.n_pass; p++) {
        const int bits = ch.pass_bits[p];
        if (bits <= 0) break;
        if (ch.run_route) {
            rc = sort_pass<u64>(ch, p == 0 ? (const void *)ro.key : (const void *)ch.ro_key[cur], ch.ro_key[cur ^ 1], p == 0 ? nullptr : (const u32 *)ch.ro_idx[cur],
                                ch.ro_idx[cur ^ 1], shift, bits, (const u32 *)ro.n_runs, ch.ro_tiles, ro_names);
        } else {
            const u32 *vin = p == 0 ? nullptr : (const u32 *)S.idx[cur].p;
            u32 *vout = (u32 *)S.idx[cur ^ 1].p;
            if (f.lim.dense) rc = sort_pass<u32>(ch, p == 0 ? S.jidbam.p : S.key[cur].p, S.key[cur ^ 1].p, vin, vout, shift, bits, ch.d_P, ch.rs_tiles, rs_names);
            else rc = sort_pass<u64>(ch, p == 0 ? S.okey.p : S.key[cur].p, S.key[cur ^ 1].p, vin, vout, shift, bits, ch.d_P, ch.rs_tiles, rs_names);
        }
        if (rc) return rc;
        cur ^= 1;
        shift += bits;
    }
    f.n_pass = ch.n_pass;
    if (ch.run_route) {
        // where every run's first pair goes: the counts summed in key order, written back at the run's own index; then the one pass
        // over the pairs
        const u32 *order = ch.ro_idx[cur];
        if ((rc = run_scan(c, ro_names[4], RunCountFn{(const u32 *)ro.cnt, order}, RunDestSink{ch.run_dest, order}, (u64)ch.run_cap, ch.ro_total, (const u32 *)ro.n_runs)))
            return rc;
        cur = 1;
        LAUNCH(c, ro_names[5], rs_place, dim3(ch.rs_tiles), dim3(256), (const u32 *)S.jidbam.p, ch.d_P, (const u64 *)ro.key, (const u32 *)ch.run_dest,
               (const u32 *)ro.tile_first, (const u32 *)ro.tile_n, ch.run_cap, ro.tile_bits, (u32 *)S.key[cur].p, (u32 *)S.idx[cur].p);
        f.n_pass = 1;
    }
    ch.cur = cur;
    f.sidx = (const u32 *)S.idx[cur].p;
    f.jid_sorted = f.lim.dense ? (const u32 *)S.key[cur].p : (const u32 *)S.jid.p; // junction id of every sorted pair
    STAGE_EVENT(2);
    return PJB_OK;
}

// the entropy kernels: beside what follows on the main stream (small and latency-bound, both)
static int chain_entropy(Chain &ch) {
    pjb_ctx *c = ch.c;
    CtlSlot &S = ch.S;
    LAUNCH(c, "k5_entropy_sum", k5_entropy_sum, dim3(std::max<u32>(1, (ch.JL + 15) / 16)), dim3(256), (const u32 *)S.seg.p, (const u32 *)S.runfirst.p,
           (const u32 *)S.runstart.p, ch.d_J, (double *)S.entsum.p);
    return PJB_OK;
}

#ifdef PJB_DEBUG_LAUNCH
// is the sort's output a permutation with ascending ids?  is its input what kd_assign wrote?  (waits for the device)
static void debug_sort_check(Chain &ch) {
    Flight &f = ch.f;
    CtlSlot &S = ch.S;
    const int cur = ch.cur;
    fprintf(stderr, "[k4_pairs] tid %d PL %u JL %u slots_lim %u n_slices_lim %u frag cap %zu fragj cap %zu masks cap %zu rec cap %zu idx cap %zu key cap %zu jkey cap %zu cur %d n_pass %d\n",
            f.tid, ch.PL, ch.JL, ch.slots_lim, ch.n_slices_lim, S.frag.cap, S.fragj.cap, S.masks.cap, S.rec.cap, S.idx[cur].cap, S.key[cur].cap, S.jkey.cap, cur, f.n_pass);
    ContigStats hcs;
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(&hcs, ch.d_cs, sizeof hcs, hipMemcpyDeviceToHost);
    u64 htot = 0;
    (void)hipMemcpy(&htot, S.total.p, 8, hipMemcpyDeviceToHost);
    fprintf(stderr, "[k4_pairs] cs: P %u n_pairs %llu J %u n_junc %u n_slots %u n_slices %u n_cand %u overflow %u R %u total %llu slot %d attempt %d\n", hcs.P,
            (unsigned long long)hcs.n_pairs, hcs.J, hcs.n_junc, hcs.n_slots, hcs.n_slices, hcs.n_cand, hcs.overflow, hcs.R, (unsigned long long)htot, f.slot, f.attempt);
    std::vector<u32> hs(hcs.P), hj(hcs.P), hb(hcs.P);
    (void)hipMemcpy(hs.data(), f.sidx, (size_t)hcs.P * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(hj.data(), f.jid_sorted, (size_t)hcs.P * 4, hipMemcpyDeviceToHost);
    (void)hipMemcpy(hb.data(), S.jidbam.p, (size_t)hcs.P * 4, hipMemcpyDeviceToHost);
    std::vector<char> seen(hcs.P, 0);
    size_t bad_idx = 0, dup = 0, bad_order = 0, bad_in = 0, mism = 0;
    long first_bad = -1;
    for (size_t i = 0; i < hcs.P; i++) {
        if (hb[i] >= hcs.J) bad_in++;
        if (hs[i] >= hcs.P) {
            bad_idx++;
            if (first_bad < 0) first_bad = (long)i;
            continue;
        }
        if (seen[hs[i]]) dup++;
        seen[hs[i]] = 1;
        if (hj[i] != hb[hs[i]]) mism++;
        if (i && hj[i] < hj[i - 1]) bad_order++;
    }
    fprintf(stderr, "[k4_pairs] sort check: %zu indices out of range (first at %ld), %zu duplicates, %zu order breaks, %zu key/index mismatches, %zu input ids >= J\n", bad_idx,
            first_bad, dup, bad_order, mism, bad_in);
}
#endif

// 7. runs, dense ids -- the usual chain: the sorted ids are the junction ids; K4 gathers the pairs -- one 32-byte record each -- folds them
// to fragments and leaves the junction / run boundaries as bit masks; two small kernels turn the masks into
// seg_off / run_first / run_start (no second pass over the pairs), then the entropy beside the fragment reduce
static int chain_runs_dense(Chain &ch) {
    pjb_ctx *c = ch.c;
    Flight &f = ch.f;
    CtlSlot &S = ch.S;
    const u32 n_slices_lim = ch.n_slices_lim, pair_blocks = ch.pair_blocks;
    int rc;
    u64 *head_mask = (u64 *)S.masks.p, *run_mask = head_mask + n_slices_lim;
    u32 *run_base = (u32 *)(run_mask + n_slices_lim);
    STAGE_EVENT(3);
    STAGE_EVENT(4);
    if (f.forked) HIP_TRY(c, hipStreamWaitEvent(ch.st, S.ev_join, 0)); // k4b_generic's results (side stream) are needed from here on
#ifdef PJB_DEBUG_LAUNCH
    debug_sort_check(ch);
#endif
    LAUNCH(c, "k4_pairs", k4_pairs, dim3(ch.range_blocks), dim3(256), f.sidx, f.jid_sorted, (const PairRec *)ch.pr.rec, (const u64 *)S.jkey.p, ch.kf, ch.d_P,
           (u32 *)S.frag.p, (int32_t *)S.fragj.p, head_mask, run_mask, (const ContigStats *)ch.d_cs, ch.d_err, ch.range_shift);
    if ((rc = run_scan(c, "k2_runs", Popc64Fn{(const u64 *)run_mask}, ExclusiveU32Sink{run_base}, (u64)n_slices_lim, (u64 *)S.total.p, &ch.d_cs->n_slices)))
        return rc;
    LAUNCH(c, "k2_expand", k2_expand, dim3((pair_blocks + K2E_PER - 1) / K2E_PER), dim3(256), f.jid_sorted, (const u64 *)head_mask, (const u64 *)run_mask, (const u32 *)run_base,
           (const u64 *)S.total.p, (u32 *)S.seg.p, (u32 *)S.runfirst.p, (u32 *)S.runstart.p, ch.d_cs);
    STAGE_EVENT(5);
    return chain_fork(ch, S.ev_fork2, S.ev_join2, ch.entropy_forked, chain_entropy);
}

// 8. runs, full keys -- a chain that sorted the full keys: junction ids and position runs from a scan over the sorted pairs (it fetches
// every pair's read position), the junctions' keys, anchors, ids in BAM order -- then the generic pairs and K4
static int chain_runs_keys(Chain &ch) {
    pjb_ctx *c = ch.c;
    Flight &f = ch.f;
    CtlSlot &S = ch.S;
    const u32 JL = ch.JL, pair_blocks = ch.pair_blocks;
    int rc;
    const u64 *skey = (const u64 *)S.key[ch.cur].p;
    HeadFn hf{skey, f.sidx, (const PairRec *)ch.pr.rec};
    HeadSink hs{(u32 *)S.jid.p, (u32 *)S.seg.p, (u32 *)S.runfirst.p, (u32 *)S.runstart.p, skey, (u64 *)S.jkey.p, JL};
    if ((rc = run_scan(c, "k2_heads", hf, hs, (u64)ch.PL, (u64 *)S.total.p, ch.d_P))) return rc;
    LAUNCH(c, "k2_close", k2_close, dim3(1), dim3(1), (u64 *)S.total.p, (u32 *)S.seg.p, (u32 *)S.runfirst.p,
           (u32 *)S.runstart.p, ch.d_cs, JL, (const u32 *)ch.d_gen_cnt, ch.gen_cap, ch.range_shift);
    STAGE_EVENT(3);
    if ((rc = chain_fork(ch, S.ev_fork2, S.ev_join2, ch.entropy_forked, chain_entropy))) return rc;
    LAUNCH(c, "kf_init", kf_init, dim3(std::max<u32>(1, std::min<u32>((JL * F_WORDS + 255) / 256, 4096))), dim3(256), (u32 *)S.acc.p, ch.d_J, (int32_t *)S.ancl.p,
           (int32_t *)S.ancr.p);
    LAUNCH(c, "kf_anchors", kf_anchors, dim3(pair_blocks), dim3(256), f.sidx, (const u32 *)S.jid.p, (const PairRec *)ch.pr.rec, ch.d_P, (u32 *)S.jidbam.p,
           (int32_t *)S.ancl.p, (int32_t *)S.ancr.p);
    if ((rc = chain_k4b(ch))) return rc;
    STAGE_EVENT(4);
    LAUNCH(c, "k4_pairs", k4_pairs, dim3(ch.range_blocks), dim3(256), f.sidx, f.jid_sorted, (const PairRec *)ch.pr.rec, (const u64 *)S.jkey.p, ch.kf, ch.d_P,
           (u32 *)S.frag.p, (int32_t *)S.fragj.p, (u64 *)nullptr, (u64 *)nullptr, (const ContigStats *)ch.d_cs, ch.d_err, ch.range_shift);
    STAGE_EVENT(5);
    return PJB_OK;
}

// 9. rows -- K5: fragments -> junctions -> rows; then the rows to the host (and into the caller's exchange slot), control block last: on
// the rows stream, so that the next contig's first kernels need not wait for the PCIe writes
static int chain_rows(Chain &ch) {
    pjb_ctx *c = ch.c;
    Flight &f = ch.f;
    CtlSlot &S = ch.S;
    const hipStream_t st = ch.st;
    const u32 JL = ch.JL;
    LAUNCH(c, "k5_frag_reduce", k5_frag_reduce, dim3((ch.slots_lim + 4 * FRAG_SLOTS_PER_WAVE - 1) / (4 * FRAG_SLOTS_PER_WAVE)), dim3(256),
           (const u32 *)S.frag.p, (const int32_t *)S.fragj.p, ch.d_slots, (u32 *)S.acc.p);
    if (ch.entropy_forked) HIP_TRY(c, hipStreamWaitEvent(st, S.ev_join2, 0));
    LAUNCH(c, "k5_finalize", k5_finalize, dim3(std::max<u32>(1, (JL + 255) / 256)), dim3(256), (const u64 *)S.jkey.p, (const u32 *)S.seg.p,
           (const u32 *)S.runfirst.p, (const u32 *)S.runstart.p, (const u32 *)S.acc.p,
           (const int32_t *)S.ancl.p, (const int32_t *)S.ancr.p, ch.kf, ch.GT, ch.d_J, (const double *)S.entsum.p, (pjb_junction_row *)S.rows.p, ch.d_err,
           ch.d_member_junc);
    STAGE_EVENT(6);
    u64 *mirror_table = nullptr;
    u32 mirror_room = 0; // rows the caller's slot can take (the kernel leaves the slot alone if the contig does not fit)
    if (c->mirror && c->mirror_cap >= PJB_MIRROR_HEADER_BYTES) {
        mirror_table = (u64 *)(c->mirror + PJB_MIRROR_HEADER_BYTES);
        mirror_room = (u32)std::min<size_t>((c->mirror_cap - PJB_MIRROR_HEADER_BYTES) / sizeof(pjb_junction_row), 0xffffffffu);
    }
    const hipStream_t rows_stream = c->side_stream ? c->stream3 : st;
    if (rows_stream != st) {
        HIP_TRY(c, hipEventRecord(S.ev_rows, st));
        HIP_TRY(c, hipStreamWaitEvent(rows_stream, S.ev_rows, 0));
    }
    {
        ChainScope scope{c};
        c->stream = rows_stream; // LAUNCH (and its event bracket) follow c->stream
        LAUNCH(c, "k6_rows_out", k6_rows_out, dim3(K6_BLOCKS), dim3(256), (const u64 *)S.rows.p, (const ContigStats *)ch.d_cs,
               (u64 *)c->rows_table, ch.row_base, ch.mirror_base, (RowCursor *)c->b_cursor.p, mirror_table, mirror_room, ch.d_err, ch.d_gen_cnt, S.pub_dev,
               (const MemberStats *)ch.d_members, ch.d_member_junc, ch.n_members);
    }
    S.at_rest = true;
    HIP_TRY(c, hipEventRecord(S.ev[7], rows_stream));
    HIP_TRY(c, hipEventRecord(S.ev_done, rows_stream));
    f.queued = true;
    return PJB_OK;
}
#undef STAGE_EVENT

// The device work of one contig, queued in one go.  The host does not learn a single count while the kernels run:
// buffers and grids are sized from LIMITS (pair_limit, junc_limit, the key format kf), the kernels read the actual
// counts from the control block in device memory (ContigStats) and stand still when a limit is exceeded.  Nothing
// here waits for the device: the last kernels (rows stream) write rows and control block into page-locked host memory
// and pjb_finish_contig_end waits for their event -- by which time the next contig may be queued behind this one.
static int queue_contig(pjb_ctx *c, Flight &f) {
    Chain ch{c, f, c->sl[f.slot]}; // (everything else: zero)
    int rc = chain_plan(ch);
    // the contig's chain runs on its slot's streams, beside the chain of the contig in the other slot, and its LAUNCH brackets belong
    // to its slot
    ChainScope scope{c};
    c->stream = ch.st;
    c->scan_tiles = &ch.S.scan_tiles;
    c->cur_pool = c->cur_slot = f.slot;
    ev_drop(c, f.slot);
    if (rc || (rc = chain_room(ch)) || (rc = chain_front(ch)) || (rc = chain_k1(ch)) || (rc = chain_k2d(ch)) || (rc = chain_sort(ch)) ||
        (rc = f.lim.dense ? chain_runs_dense(ch) : chain_runs_keys(ch)))
        return rc;
    return chain_rows(ch);
}
