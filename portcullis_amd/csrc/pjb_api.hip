// pjb_api.hip -- C ABI (include/portcullis_amd.h) over the HIP kernels: contexts, genomes, batches, the kernel chains (their launcher: pjb_chain.hip.h;
// a flight from begin to end: pjb_flight.hip.h, with the limits it is queued with: pjb_limits.hip.h), rows.
// One context = one HIP device + its streams + grow-only scratch.  (--extra / bamfilt: pjb_extra_api.hip; filt / train: pjb_model_api.hip; BGZF and BAM: pjb_ingest_api.hip.)
#include "pjb_host.hip.h"
#include "pjb_kernels.hip.h"
#include "pjb_chain.hip.h"
#include "pjb_flight.hip.h"

// The sort passes for a caller in another unit (pjb_bam_merge_end, pjb_bam_sort_end: the non-template rs_* kernels live in this unit
// only).  Stable LSD sort of (key of type K, index) over the low `key_bits` bits: the keys lie in key[0], the first pass hands out the
// indices 0, 1, 2, ..; returns 0 / 1: which of key[] / idx[] holds the result.  d_n: the count `n` on the device; key[] and idx[] have a
// sort tile of slack.
template <typename K>
static int sort_pairs(pjb_ctx *c, SortU32 &S, const u32 *d_n, size_t n, int key_bits, int *result) {
    // passes of equal width, at most 11 bits (rs_scatter's LDS then stays under 64 KB for 4- and 8-byte keys and needs no attribute)
    const int n_pass = (key_bits + 10) / 11, bits = (key_bits + n_pass - 1) / n_pass;
    const u32 nb = 1u << bits, tiles = (u32)((n + RS_TILE - 1) / RS_TILE), n_panels = (tiles + RSP_TILES - 1) / RSP_TILES;
    int rc;
    if ((rc = ensure(c, S.hist, (size_t)tiles * nb * 4)) || (rc = ensure(c, S.hist_scan, (size_t)tiles * nb * 4)) ||
        (rc = ensure(c, S.hist_part, (size_t)n_panels * nb * 4)) || (rc = ensure(c, S.bin_total, (size_t)nb * 4)))
        return rc;
    int cur = 0;
    for (int p = 0; p < n_pass; p++) {
        const int shift = p * bits;
        const K *kin = (const K *)S.key[cur].p;
        const u32 *vin = p == 0 ? nullptr : (const u32 *)S.idx[cur].p;
        K *kout = (K *)S.key[cur ^ 1].p;
        u32 *vout = (u32 *)S.idx[cur ^ 1].p;
        LAUNCH(c, rs_names[0], rs_hist<K>, dim3(tiles), dim3(256), kin, d_n, shift, bits, (u32 *)S.hist.p, tiles);
        LAUNCH(c, rs_names[1], rs_panel_sums, dim3(n_panels, (nb + 255) / 256), dim3(256), (const u32 *)S.hist.p, tiles, nb, (u32 *)S.hist_part.p);
        LAUNCH(c, rs_names[2], rs_panel_scan, dim3(n_panels, (nb + 255) / 256), dim3(256), (const u32 *)S.hist.p, (const u32 *)S.hist_part.p, tiles, nb,
               (u32 *)S.hist_scan.p, (u32 *)S.bin_total.p);
#define RS_SCATTER(B)                                                                                                                     \
    LAUNCH_LDS(c, rs_names[3], (rs_scatter<B, K>), dim3(tiles), dim3(256), rs_scatter_lds_bytes(bits, sizeof(K)), kin, vin, kout, vout, d_n, \
               shift, bits, (const u32 *)S.hist_scan.p, (const u32 *)S.bin_total.p, tiles)
        switch (bits) { // the usual digit widths get an unrolled match loop
        case 9: RS_SCATTER(9); break;
        case 10: RS_SCATTER(10); break;
        case 11: RS_SCATTER(11); break;
        default: RS_SCATTER(0); break;
        }
#undef RS_SCATTER
        cur ^= 1;
    }
    *result = cur;
    return PJB_OK;
}
int sort_u32_pairs(pjb_ctx *c, SortU32 &S, const u32 *d_n, size_t n, int key_bits, int *result) { return sort_pairs<u32>(c, S, d_n, n, key_bits, result); }
int sort_u64_pairs(pjb_ctx *c, SortU32 &S, const u32 *d_n, size_t n, int key_bits, int *result) { return sort_pairs<u64>(c, S, d_n, n, key_bits, result); }

extern "C" {

// Page-locked host memory.  hipHostMalloc zeroes and pins on the calling thread at ~4.6 GB/s (143 ms for the 768 MB ring of
// the end-to-end program, as much again for its genome buffers); anonymous huge-page memory touched by four threads and then
// registered is the same memory to a DMA (56.8 GB/s either way) after 23 ms (tools/debug/register_probe.hip,
// profiles/r03ap2_register_probe.txt).  Blocks below 8 MB, and anything mmap or the registration refuses, take hipHostMalloc.
namespace {
std::mutex g_host_mu;
std::map<void *, size_t> g_host_registered; // blocks of pjb_host_alloc that are mmap + hipHostRegister (value: mapped bytes)
} // namespace
void *pjb_host_alloc(size_t bytes) {
    if (bytes >= ((size_t)8 << 20)) {
        const size_t huge = (size_t)2 << 20, len = (bytes + huge - 1) & ~(huge - 1);
        void *p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p != MAP_FAILED) {
            (void)madvise(p, len, MADV_HUGEPAGE);
            const size_t nt = std::min<size_t>(4, len >> 24);
            auto touch = [&](size_t t) {
                const size_t per = ((len / std::max<size_t>(nt, 1)) + huge - 1) & ~(huge - 1), a = std::min(len, per * t), b = std::min(len, a + per);
                for (size_t o = a; o < b; o += 4096) ((volatile uint8_t *)p)[o] = 0;
            };
            if (nt <= 1) touch(0);
            else {
                std::vector<std::thread> th;
                for (size_t t = 0; t < nt; t++) th.emplace_back(touch, t);
                for (auto &x : th) x.join();
            }
            if (hipHostRegister(p, len, hipHostRegisterDefault) == hipSuccess) {
                std::lock_guard<std::mutex> lk(g_host_mu);
                g_host_registered[p] = len;
                return p;
            }
            (void)hipGetLastError();
            munmap(p, len);
        }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void pjb_host_free(void *p) {
    if (!p) return;
    size_t len = 0;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto it = g_host_registered.find(p);
        if (it != g_host_registered.end()) {
            len = it->second;
            g_host_registered.erase(it);
        }
    }
    if (len) {
        (void)hipHostUnregister(p);
        munmap(p, len);
    } else
        (void)hipHostFree(p);
}

int pjb_host_register(void *p, size_t bytes) {
    if (!p || !bytes) return PJB_ERR_ARG;
    if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        return PJB_ERR_HIP;
    }
    return PJB_OK;
}
int pjb_host_unregister(void *p) {
    if (!p) return PJB_ERR_ARG;
    if (hipHostUnregister(p) != hipSuccess) {
        (void)hipGetLastError();
        return PJB_ERR_HIP;
    }
    return PJB_OK;
}

int pjb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pjb_create(pjb_ctx **out, const pjb_config *cfg) {
    if (!out || !cfg) return fail(nullptr, PJB_ERR_ARG, "pjb_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != PJB_ABI_VERSION && cfg->abi_version != 3) // (3: the same entry points; pjb_batch ends at name_hash)
        return fail(nullptr, PJB_ERR_ARG, "pjb_create: ABI version %d, library is %d", cfg->abi_version, PJB_ABI_VERSION);
    if (cfg->orientation < PJB_OR_SE || cfg->orientation > PJB_OR_UNKNOWN)
        return fail(nullptr, PJB_ERR_ARG, "pjb_create: bad orientation %d", cfg->orientation);
    const bool ctrace = getenv("PJB_CREATE_TRACE") != nullptr; // (stderr: what the context's start is made of)
    const auto ct0 = std::chrono::steady_clock::now();
    auto cmark = [&](const char *what) {
        if (ctrace) fprintf(stderr, "[pjb_create] %7.1f ms: %s\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ct0).count(), what);
    };
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    cmark("hipGetDeviceCount");
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, PJB_ERR_NO_DEVICE,
                    "no HIP device available (%s); the junc hot path has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= n)
        return fail(nullptr, PJB_ERR_ARG, "pjb_create: device %d out of range (have %d)", cfg->device, n);
    e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail(nullptr, PJB_ERR_HIP, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, cfg->device);
    if (e != hipSuccess) return fail(nullptr, PJB_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    cmark("hipSetDevice, hipGetDeviceProperties");
    const int n_cu = prop.multiProcessorCount;
    if (prop.warpSize != 64)
        return fail(nullptr, PJB_ERR_NO_DEVICE, "device %d (%s) is not a wave64 CDNA device", cfg->device, prop.gcnArchName);
    pjb_ctx *c = new (std::nothrow) pjb_ctx();
    if (!c) return fail(nullptr, PJB_ERR_NOMEM, "out of host memory");
    // The kernels' attributes -- the first call loads the code object, 30 - 70 ms -- are set by a thread of their own while
    // this one creates the streams (PJB_CREATE_SERIAL=1: afterwards, on this thread).
    const int dev = cfg->device;
    auto attributes = [dev] {
        (void)hipSetDevice(dev);
        ingest_kernel_attributes();
        // 12-bit digits need more dynamic LDS than the 64 KB a kernel gets without asking
        (void)hipFuncSetAttribute((const void *)rs_scatter<0, u64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rs_scatter_lds_bytes(RS_MAX_BITS));
        (void)hipFuncSetAttribute((const void *)rs_scatter<0, u32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rs_scatter_lds_bytes(RS_MAX_BITS, 4));
    };
    std::thread attr_thread(attributes);
    struct JoinAttr {
        std::thread &t;
        ~JoinAttr() {
            if (t.joinable()) t.join();
        }
    } join_attr{attr_thread};
    c->cfg = *cfg;
    memset(&c->timing, 0, sizeof c->timing);
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(nullptr, PJB_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    if (!(cfg->flags & PJB_FLAG_NO_CHAINS)) aux_streams(c); // (else: with the first chain)
    (void)hipEventCreateWithFlags(&c->ev_front, hipEventDisableTiming);
    c->scan_tiles = &c->b_scan_tiles;
    // The first four control slots get their streams and events now; the others when they are first used (slot_init).  Creating
    // a stream is ~10 ms on an idle device -- and blocked for 1.9 s once when it happened in the middle of an end-to-end run
    // (the runtime creates a hardware queue behind whatever the device is doing): a caller that wants more than four chains in
    // flight on a busy device queues that deep once, early.
    // (60 ms for four slots' streams and events; from four threads at once it is 70 - 100 ms: the runtime serialises them)
    cmark("main streams");
    if (!(cfg->flags & PJB_FLAG_NO_CHAINS))
        for (int k = 0; k < 4 && k < PJB_MAX_QUEUED; k++) (void)slot_init(c, k);
    cmark("chain slots");
    c->inflate_lanes = std::max(1, n_cu) * (160 * 1024 / ingest_lds_bytes()) * 64;
    c->ktime = (cfg->flags & PJB_FLAG_KERNEL_TIMING) != 0;
    c->extra = (cfg->flags & PJB_FLAG_EXTRA) != 0;
    if (const char *s = getenv("PJB_K1_SERIAL")) c->k1_serial = atoi(s) != 0;
    if (const char *s = getenv("PJB_K1S_BLOCKS")) c->k1s_blocks_forced = std::max(0, std::min(atoi(s), (int)K1S_BLOCKS));
    if (const char *s = getenv("PJB_RADIX_BITS")) {
        int v = atoi(s);
        if (v >= 4 && v <= RS_MAX_BITS) c->radix_max_bits = v;
    }
    if (const char *s = getenv("PJB_PAIR_RANGE")) { // (A/B runs of a command that sets no options: what pjb_set_option("pair_range", n) takes)
        const int v = atoi(s);
        for (int k = 0; k <= PAIR_RANGE_SHIFT_MAX; k++)
            if (v == 1 << k) c->pair_range_shift = k;
    }
    cmark("options");
    attr_thread.join();
    cmark("kernel attributes");
    *out = c;
    return PJB_OK;
}


void pjb_destroy(pjb_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    (void)hipDeviceSynchronize(); // (contigs may still be queued)
    (void)exhume(c);
#ifdef K1E_PROF
    {
        unsigned long long h[16] = {0};
        (void)hipDeviceSynchronize();
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(pjb::g_k1e_prof), sizeof h) == hipSuccess) {
            unsigned long long tot = 0;
            for (int i = 0; i < 12; i++) tot += h[i];
            static const char *nm[12] = {"block start", "prologue", "shapes (wait ops)", "windows issue", "next records issue", "stage wait", "next ops issue", "compare+emit", "lists", "cand flush", "span of bases", "bases issue"};
            for (int i = 0; i < 12; i++) fprintf(stderr, "[k1e_prof] %-20s %6.2f %%  %llu\n", nm[i], tot ? 100.0 * (double)h[i] / (double)tot : 0.0, h[i]);
        }
    }
#endif
    while (!c->open.empty()) close_contig(c, c->open.begin()->first);
    extra_clear(c);
    for (auto &kv : c->filter_keys)
        if (kv.second.first) (void)dev_free(c, kv.second.first);
    c->filter_keys.clear();
    for (auto &g : c->contigs) free_contig(c, g);
    for (auto &b : c->genome_pool) release(c, b);
    c->genome_pool.clear();
    release_pooled_slabs(c);
    if (c->rows_pinned) (void)hipHostFree(c->rows_pinned);
    if (c->rows_table) (void)dev_free(c, c->rows_table);
    bam_stage_clear(c);
    for (int k = 0; k < PJB_MAX_QUEUED; k++) {
        CtlSlot &S = c->sl[k];
        if (S.pub) (void)hipHostFree(S.pub);
        if (S.batches_pinned) (void)hipHostFree(S.batches_pinned);
        for (auto &ev : S.ev)
            if (ev) (void)hipEventDestroy(ev);
        if (S.ev_rows) (void)hipEventDestroy(S.ev_rows);
        if (S.ev_done) (void)hipEventDestroy(S.ev_done);
        Buf *sb[] = {&S.x_q, &S.x_spos, &S.x_send, &S.x_gapoff, &S.x_zlist, &S.x_scnt, &S.x_codes, &S.cstats, &S.err, &S.gencount, &S.batches, &S.rows, &S.tile_cnt, &S.tile_stats, &S.splidx, &S.splpoff, &S.splrec, &S.tile_soff, &S.chunk_tile, &S.scan_parts, &S.members, &S.okey, &S.g,
                     &S.rec, &S.jidbam, &S.jkey, &S.total, &S.bitmap, &S.wrank, &S.pagecnt, &S.pagerank, &S.ends, &S.firstid,
                     &S.key[0], &S.key[1], &S.idx[0], &S.idx[1], &S.hist, &S.hist_scan, &S.hist_part, &S.bintotal, &S.scan_tiles, &S.jid, &S.seg, &S.runfirst,
                     &S.runstart, &S.ent, &S.entsum, &S.frag, &S.fragj, &S.masks, &S.acc, &S.ancl, &S.ancr, &S.genlist, &S.runs};
        for (Buf *b : sb) release(c, *b);
        hipEvent_t evs[] = {S.ev_k1, S.ev_xk1, S.ev_fork, S.ev_join, S.ev_fork2, S.ev_join2};
        for (hipEvent_t e : evs)
            if (e) (void)hipEventDestroy(e);
        if (S.main) (void)hipStreamDestroy(S.main);
        if (S.side) (void)hipStreamDestroy(S.side);
    }
    if (c->mirror_hdr) (void)hipHostFree(c->mirror_hdr);
    for (int k = 0; k < 2; k++) {
        if (c->stage[k]) (void)hipHostFree(c->stage[k]);
        if (c->stage_ev[k]) (void)hipEventDestroy(c->stage_ev[k]);
    }
    Buf *all[] = {&c->b_cursor, &c->b_scan_tiles, &c->b_hasx, &c->b_xtotal, &c->b_fasta_raw, &c->b_inf_comp, &c->b_inf_out, &c->b_inf_blocks, &c->b_inf_status, &c->b_inf_scratch, &c->b_inf_bitmap,
                  &c->b_bam_seg, &c->b_bam_rec, &c->b_bam_ctl, &c->f_pos, &c->f_cigoff, &c->f_cigar, &c->f_codes,
                  &c->x_pos, &c->x_endx, &c->x_q, &c->x_prefq, &c->x_ce, &c->x_bound, &c->x_de, &c->x_dropped, &c->x_zlist, &c->x_cnt,
                  &c->x_tabk, &c->x_tabc, &c->x_rs, &c->x_re, &c->x_rr, &c->x_tileoff, &c->x_xrall, &c->x_tab,
                  &c->b_dfl_in, &c->b_dfl_sym, &c->b_dfl_slots, &c->b_dfl_size, &c->b_dfl_off, &c->b_dfl_packed};
    for (Buf *b : all) release(c, *b);
    c->model.release_all(c);
    for (auto &ch : c->xarena.chunks) (void)dev_free(c, ch.p);
    if (c->xrows_pinned) (void)hipHostFree(c->xrows_pinned);
    for (auto &pool : c->pools)
        for (auto &ev : pool.ev) (void)hipEventDestroy(ev);
    if (c->ev_front) (void)hipEventDestroy(c->ev_front);
    if (c->stream3) (void)hipStreamDestroy(c->stream3);
    if (c->stream4) (void)hipStreamDestroy(c->stream4);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *pjb_last_error(const pjb_ctx *c) {
    if (!c) return g_create_error.c_str();
    return g_thread_error_ctx == c ? g_thread_error.c_str() : ""; // (this thread's last failure on THIS context; none: the empty string)
}

int pjb_set_refs(pjb_ctx *c, int32_t n_refs, const int32_t *ref_len) {
    if (!c) return PJB_ERR_ARG;
    if (n_refs < 0 || (n_refs > 0 && !ref_len)) return fail(c, PJB_ERR_ARG, "pjb_set_refs: bad arguments");
    if (!c->open.empty()) return fail(c, PJB_ERR_STATE, "pjb_set_refs: contig %d is still open", c->open.begin()->first);
    for (auto &g : c->contigs) free_contig(c, g);
    c->slab_refused_tid = -1;
    c->ref_len.assign(ref_len, ref_len + n_refs);
    c->contigs.assign((size_t)n_refs, Contig());
    return PJB_OK;
}

// fasta_flag: the upload came through k0_fasta, whose verdict -- word 3 of the flags, raised before this call -- is read with the others: a
// record that was not laid out as stated returns 1 and leaves the context as it was
static int upload_common(pjb_ctx *c, int32_t tid, uint8_t *d, int64_t len, bool owned, bool do_upper, size_t d_cap = 0, bool fasta_flag = false) {
    static const bool prof = getenv("PJB_PROFILE_HOST") != nullptr;
    const double t_up0 = wall_now();
    double t_alloc = 0;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // the kernels' three flags (an 'X' among the bases, a character outside the 16-letter alphabet, a character outside ACGT) come back in
    // ONE copy behind the last kernel: every copy to pageable memory makes this thread wait for the stream, and this is the thread that
    // serves every target (three waits a genome were 0.2 s of a human run)
    int rc = ensure(c, c->b_hasx, 4 * sizeof(int));
    if (rc) return rc;
    int *d_flags = (int *)c->b_hasx.p;
    HIP_TRY(c, hipMemsetAsync(d_flags, 0, 3 * sizeof(int), c->stream));
    if (len > 0) {
        const int64_t nthreads = (len + 15) / 16;
        const unsigned nblk = (unsigned)((nthreads + 255) / 256);
        hipLaunchKernelGGL(k0_upper, dim3(nblk), dim3(256), 0, c->stream, d, len, do_upper ? 1 : 0, d_flags + 0);
    }
    // 4-bit codes for the word-parallel compare in k4 (after upper-casing)
    u32 *codes = nullptr;
    size_t codes_cap = 0;
    const int64_t n_words = (len + 7) / 8;
    static const bool no_seq2 = getenv("PJB_NO_SEQ2") && atoi(getenv("PJB_NO_SEQ2")) != 0;
    const size_t c2_at = ((size_t)(n_words + 2) + 3) & ~(size_t)3;                       // (the 2-bit codes start on a 16-byte boundary)
    const size_t c2_words = len > 0 && !no_seq2 ? (size_t)codes2_alloc_words(len) : 0;
    if (len > 0) {
        const double ta = wall_now();
        codes = (u32 *)genome_take(c, (c2_at + c2_words) * 4, codes_cap);
        t_alloc = wall_now() - ta;
        if (!codes) return nomem(c, "genome codes", (c2_at + c2_words) * 4);
        (void)hipMemsetAsync(codes + n_words, 0, 8, c->stream);
        hipLaunchKernelGGL(k0_encode, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)d, len,
                           codes, n_words, d_flags + 1);
    }
    // 2-bit codes and their exception bitmap for k1_emit's compares (PJB_NO_SEQ2=1: not built -- A/B runs): behind the 4-bit codes, in
    // the same allocation (a hipMalloc is milliseconds on the thread that serves every target)
    u32 *codes2 = nullptr;
    if (codes && c2_words) {
        codes2 = codes + c2_at;
        const int64_t n2w = codes2_words(len), nxw = gexc_words(len);
        (void)hipMemsetAsync(codes2 + n2w, 0, (size_t)K0_CODES2_PAD * 4, c->stream);
        (void)hipMemsetAsync(codes2 + n2w + K0_CODES2_PAD + nxw, 0, (size_t)K0_GEXC_PAD * 4, c->stream);
        hipLaunchKernelGGL(k0_encode2, dim3((unsigned)(((len + 63) / 64 + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)d, len, codes2,
                           codes2 + n2w + K0_CODES2_PAD, d_flags + 2);
    }
    int flags[4] = {0, 0, 1, 0};
    HIP_TRY(c, hipMemcpyAsync(flags, d_flags, (fasta_flag ? 4 : 3) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    const double t_sync0 = wall_now();
    hipError_t se = hipStreamSynchronize(c->stream);
    if (se != hipSuccess) {
        if (codes) (void)dev_free(c, codes);
        return fail(c, PJB_ERR_HIP, "upload: %s", hipGetErrorString(se));
    }
    if (prof)
        fprintf(stderr, "[host profile] genome tid %d (%lld bases): codes allocation %.4f, launches %.4f, wait for the stream %.4f s\n", tid, (long long)len, t_alloc,
                t_sync0 - t_up0 - t_alloc, wall_now() - t_sync0);
    if (fasta_flag && flags[3]) { // (the bytes were not a FASTA record of that geometry: nothing of this upload is kept)
        if (codes) (void)dev_free(c, codes);
        return 1;
    }
    const int hx = flags[0], exotic = flags[1], any_exc = codes2 ? flags[2] : 1;
    if (exotic && codes) {
        (void)dev_free(c, codes);
        codes = nullptr;
        codes2 = nullptr;
    }
    Contig &g = c->contigs[(size_t)tid];
    free_contig(c, g, true);
    g.d = d;
    g.len = len;
    g.owned = owned;
    g.has_x = hx != 0;
    g.present = true;
    g.codes = codes;
    g.codes2 = codes2;
    g.any_exc = any_exc != 0;
    g.d_cap = owned ? d_cap : 0;
    g.codes_cap = codes ? codes_cap : 0;
    return PJB_OK;
}

int pjb_upload_contig(pjb_ctx *c, int32_t tid, const uint8_t *bases, int64_t len) {
    if (!c) return PJB_ERR_ARG;
    if (tid < 0 || (size_t)tid >= c->contigs.size() || len < 0 || (len > 0 && !bases))
        return fail(c, PJB_ERR_ARG, "pjb_upload_contig: bad arguments (tid %d)", tid);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    size_t d_cap = 0;
    uint8_t *d = (uint8_t *)genome_take(c, (size_t)std::max<int64_t>(len, 16), d_cap);
    if (!d) return nomem(c, "genome", (size_t)std::max<int64_t>(len, 16));
    hipError_t e = hipSuccess;
    // through the page-locked staging buffers in 32 MiB pieces (a pageable hipMemcpy is several times slower)
    const size_t PIECE = (size_t)32 << 20;
    for (size_t off = 0; off < (size_t)len; off += PIECE) {
        const size_t n = std::min(PIECE, (size_t)len - off);
        const unsigned si = c->stage_next++ & 1u;
        if (c->stage_busy[si]) {
            (void)hipEventSynchronize(c->stage_ev[si]);
            c->stage_busy[si] = false;
        }
        if (c->stage_cap[si] < n) {
            if (c->stage[si]) (void)hipHostFree(c->stage[si]);
            c->stage[si] = nullptr;
            c->stage_cap[si] = 0;
            if (hipHostMalloc((void **)&c->stage[si], PIECE, hipHostMallocDefault) != hipSuccess) {
                (void)dev_free(c, d);
                return fail(c, PJB_ERR_NOMEM, "upload: cannot allocate page-locked staging memory");
            }
            c->stage_cap[si] = PIECE;
        }
        if (!c->stage_ev[si]) (void)hipEventCreateWithFlags(&c->stage_ev[si], hipEventDisableTiming);
        parallel_copy(c->stage[si], bases + off, n);
        e = hipMemcpyAsync(d + off, c->stage[si], n, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) {
            (void)dev_free(c, d);
            return fail(c, PJB_ERR_HIP, "hipMemcpy(genome): %s", hipGetErrorString(e));
        }
        (void)hipEventRecord(c->stage_ev[si], c->stream);
        c->stage_busy[si] = true;
    }
    int rc = upload_common(c, tid, d, len, true, true, d_cap);
    if (rc) (void)dev_free(c, d);
    return rc;
}

int pjb_upload_contig_fasta(pjb_ctx *c, int32_t tid, const uint8_t *raw, int64_t raw_bytes, int32_t line_blen, int32_t line_len, int64_t len,
                            int *well_formed) {
    if (!c) return PJB_ERR_ARG;
    if (tid < 0 || (size_t)tid >= c->contigs.size() || len < 0 || raw_bytes < 0 || (raw_bytes > 0 && !raw) || line_blen <= 0 ||
        line_len < line_blen || !well_formed)
        return fail(c, PJB_ERR_ARG, "pjb_upload_contig_fasta: bad arguments (tid %d)", tid);
    *well_formed = 0;
    if (line_len - line_blen > 64) return PJB_OK; // (line ends are a byte or two; the kernel's check of them is a loop per line)
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc;
    if ((rc = ensure(c, c->b_fasta_raw, (size_t)std::max<int64_t>(raw_bytes, 16)))) return rc;
    if ((rc = ensure(c, c->b_hasx, 4 * sizeof(int)))) return rc;
    size_t d_cap = 0;
    const double t_a0 = wall_now();
    uint8_t *d = (uint8_t *)genome_take(c, (size_t)std::max<int64_t>(len, 16), d_cap);
    if (!d) return nomem(c, "genome", (size_t)std::max<int64_t>(len, 16));
    if (getenv("PJB_PROFILE_HOST"))
        fprintf(stderr, "[host profile] genome tid %d: bases allocation %.4f s\n", tid, wall_now() - t_a0);
    struct Guard {
        pjb_ctx *c;
        uint8_t *d;
        ~Guard() {
            if (d) (void)dev_free(c, d);
        }
    } guard{c, d};
    if (raw_bytes > 0 && (rc = upload_host(c, c->b_fasta_raw.p, raw, (size_t)raw_bytes))) return rc;
    // (k0_fasta's verdict is read with the other kernels' flags, behind the last of them: one wait a genome)
    HIP_TRY(c, hipMemsetAsync((int *)c->b_hasx.p + 3, 0, sizeof(int), c->stream));
    if (len > 0) {
        const int64_t nthreads = (len + 15) / 16;
        hipLaunchKernelGGL(k0_fasta, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)c->b_fasta_raw.p, raw_bytes, len,
                           line_blen, line_len, d, (int *)c->b_hasx.p + 3);
    }
    rc = upload_common(c, tid, d, len, true, true, d_cap, true);
    if (rc == 1) return PJB_OK; // (*well_formed stays 0: nothing was uploaded)
    if (rc) return rc;
    guard.d = nullptr;
    *well_formed = 1;
    return PJB_OK;
}

int pjb_upload_contig_device(pjb_ctx *c, int32_t tid, const uint8_t *d_bases_upper, int64_t len) {
    if (!c) return PJB_ERR_ARG;
    if (tid < 0 || (size_t)tid >= c->contigs.size() || len < 0 || (len > 0 && !d_bases_upper))
        return fail(c, PJB_ERR_ARG, "pjb_upload_contig_device: bad arguments (tid %d)", tid);
    return upload_common(c, tid, const_cast<uint8_t *>(d_bases_upper), len, false, false);
}

int pjb_release_contig(pjb_ctx *c, int32_t tid) {
    if (!c) return PJB_ERR_ARG;
    if (tid < 0 || (size_t)tid >= c->contigs.size()) return fail(c, PJB_ERR_ARG, "pjb_release_contig: bad tid %d", tid);
    Contig &g = c->contigs[(size_t)tid];
    (void)hipStreamSynchronize(c->stream);
    if (c->slab_refused_tid == tid && !c->open.count(tid)) c->slab_refused_tid = -1;
    free_contig(c, g, true);
    return PJB_OK;
}

static int add_batch(pjb_ctx *c, int32_t tid, const pjb_batch *b, bool device) {
    if (!c) return PJB_ERR_ARG;
    if (!b || b->n_reads < 0) return fail(c, PJB_ERR_ARG, "submit: bad batch");
    if (tid < 0 || (size_t)tid >= c->ref_len.size()) return fail(c, PJB_ERR_ARG, "submit: bad tid %d", tid);
    c->cur_tid = tid;
    OpenContig &oc = c->open[tid];
    if (b->n_reads == 0) return PJB_OK;
    if (!b->pos || !b->flag || !b->mapq || !b->xs || !b->l_qseq || !b->mtid || !b->mpos || !b->cig_off || !b->cigar ||
        !b->seq_off)
        return fail(c, PJB_ERR_ARG, "submit: null array in batch");
    if (c->extra && !b->name_hash) return fail(c, PJB_ERR_ARG, "submit: a PJB_FLAG_EXTRA context needs pjb_batch.name_hash");
    uint64_t total = 0;
    for (auto &x : oc.batches) total += (uint64_t)x.n;
    if (total + (uint64_t)b->n_reads >= 0xffffff00ull)
        return fail(c, PJB_ERR_ARG, "submit: more than 2^32 alignments on one target are not supported");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    DevBatch d;
    memset(&d, 0, sizeof d);
    d.n = b->n_reads;
    d.base = (uint32_t)total;
    if (device) {
        d.pos = b->pos; d.flag = b->flag; d.mapq = b->mapq; d.xs = b->xs; d.l_qseq = b->l_qseq; d.mtid = b->mtid;
        d.mpos = b->mpos; d.cig_off = b->cig_off; d.cigar = b->cigar; d.seq_off = b->seq_off; d.seq4 = b->seq4;
        d.name_hash = c->extra ? (const u64 *)b->name_hash : nullptr;
        if (c->cfg.abi_version >= 4 && b->seq2 && b->seq_exc) {
            if ((uintptr_t)b->seq2 & 3u) return fail(c, PJB_ERR_ARG, "submit: pjb_batch.seq2 must start on a 4-byte boundary");
            d.seq2 = (const uint32_t *)b->seq2;
            d.seq_exc = b->seq_exc;
        }
    } else {
        const size_t n = (size_t)b->n_reads;
        const size_t n_ops = b->cig_off[n], n_words = b->seq_off[n];
        const void *src[14] = {b->pos, b->flag, b->mapq, b->xs, b->l_qseq, b->mtid, b->mpos, b->cig_off, b->cigar, b->seq_off, b->seq4,
                               c->extra ? b->name_hash : nullptr, nullptr, nullptr};
        const bool two = c->cfg.abi_version >= 4 && b->seq2 && b->seq_exc;
        if (two) src[12] = b->seq2, src[13] = b->seq_exc;
        const size_t bytes[14] = {n * 4, n * 2, n, n, n * 4, n * 4, n * 4, (n + 1) * 4, n_ops * 4, (n + 1) * 4, n_words * 4,
                                  c->extra ? n * 8 : 0, two ? n_words * 2 : 0, two ? ((n + 31) / 32) * 4 : 0};
        // pack into a staging buffer, one DMA to a device slab region with the same packing
        size_t offs[14], total_b = 0;
        for (int k = 0; k < 14; k++) {
            offs[k] = total_b;
            total_b += (std::max<size_t>(bytes[k], 16) + 255) & ~(size_t)255;
        }
        const unsigned si = c->stage_next++ & 1u;
        if (c->stage_busy[si]) {
            HIP_TRY(c, hipEventSynchronize(c->stage_ev[si]));
            c->stage_busy[si] = false;
        }
        if (c->stage_cap[si] < total_b) {
            if (c->stage[si]) (void)hipHostFree(c->stage[si]);
            c->stage[si] = nullptr;
            c->stage_cap[si] = 0;
            const size_t want = total_b + total_b / 8;
            if (hipHostMalloc((void **)&c->stage[si], want, hipHostMallocDefault) != hipSuccess)
                return fail(c, PJB_ERR_NOMEM, "submit: cannot allocate %zu bytes of page-locked staging memory", want);
            c->stage_cap[si] = want;
        }
        if (!c->stage_ev[si]) HIP_TRY(c, hipEventCreateWithFlags(&c->stage_ev[si], hipEventDisableTiming));
        const SlabMark mark = slab_mark(c, oc);
        uint8_t *dev = (uint8_t *)slab_alloc(c, oc, total_b);
        if (!dev) { // (retryable: the target is as it was)
            slab_rollback(c, oc, mark);
            return nomem(c, "submit: a batch", total_b);
        }
        void *ptrs[14];
        for (int k = 0; k < 14; k++) {
            if (bytes[k] && src[k]) parallel_copy(c->stage[si] + offs[k], src[k], bytes[k]);
            ptrs[k] = dev + offs[k];
        }
        HIP_TRY(c, hipMemcpyAsync(dev, c->stage[si], total_b, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(c->stage_ev[si], c->stream));
        c->stage_busy[si] = true;
        d.pos = (const int32_t *)ptrs[0]; d.flag = (const uint16_t *)ptrs[1]; d.mapq = (const uint8_t *)ptrs[2];
        d.xs = (const uint8_t *)ptrs[3]; d.l_qseq = (const int32_t *)ptrs[4]; d.mtid = (const int32_t *)ptrs[5];
        d.mpos = (const int32_t *)ptrs[6]; d.cig_off = (const uint32_t *)ptrs[7]; d.cigar = (const uint32_t *)ptrs[8];
        d.seq_off = (const uint32_t *)ptrs[9]; d.seq4 = (const uint8_t *)ptrs[10];
        d.name_hash = c->extra ? (const u64 *)ptrs[11] : nullptr;
        if (two) d.seq2 = (const uint32_t *)ptrs[12], d.seq_exc = (const uint32_t *)ptrs[13];
    }
    oc.batches.push_back(d);
    if (!device) oc.on_main_stream = true;
    oc.last_known.push_back(device ? 0 : 1);
    oc.last_pos.push_back(device ? INT32_MIN : b->pos[b->n_reads - 1]);
    return PJB_OK;
}

int pjb_submit_batch(pjb_ctx *c, int32_t tid, const pjb_batch *b) { return add_batch(c, tid, b, false); }
int pjb_submit_batch_device(pjb_ctx *c, int32_t tid, const pjb_batch *b) { return add_batch(c, tid, b, true); }

int pjb_finish_contig_begin(pjb_ctx *c, int32_t tid) { return begin_flight(c, &tid, 1, "finish"); }
int pjb_finish_group_begin(pjb_ctx *c, const int32_t *tids, int32_t n_tids) { return begin_flight(c, tids, n_tids, "finish_group"); }

int pjb_finish_ready(pjb_ctx *c) {
    if (!c || c->n_fl <= 0) return 1;
    const Flight &f = c->fl[0];
    if (f.empty || !f.queued) return 1;
    const bool done = hipEventQuery(c->sl[f.slot].ev_done) == hipSuccess;
    (void)hipGetLastError(); // (hipErrorNotReady is not an error here)
    return done ? 1 : 0;
}

int pjb_finish_contig_end(pjb_ctx *c, int32_t tid, pjb_region_result *res) { return end_flight(c, &tid, 1, res, "finish"); }
int pjb_finish_group_end(pjb_ctx *c, const int32_t *tids, int32_t n_tids, pjb_region_result *results) {
    return end_flight(c, tids, n_tids, results, "finish_group");
}

int pjb_finish_contig(pjb_ctx *c, int32_t tid, pjb_region_result *res) {
    const int rc = pjb_finish_contig_begin(c, tid);
    if (rc) return rc;
    return pjb_finish_contig_end(c, tid, res);
}

int pjb_collect(pjb_ctx *c, const pjb_junction_row **rows, int64_t *n) {
    if (!c || !rows || !n) return PJB_ERR_ARG;
    int rc = rows_sync(c);
    if (rc) return rc;
    if (!c->rows_pinned && (rc = rows_pinned_reserve(c, 1))) return rc; // (a table, if an empty one: the pointer is never null)
    *rows = c->rows_pinned;
    *n = (int64_t)c->rows_n;
    return PJB_OK;
}

int pjb_collect_device(pjb_ctx *c, const pjb_junction_row **rows, int64_t *n) {
    if (!c || !rows || !n) return PJB_ERR_ARG;
    *rows = (const pjb_junction_row *)c->sl[c->last_slot].rows.p;
    *n = (int64_t)c->last_rows_n;
    return PJB_OK;
}

int pjb_set_row_mirror(pjb_ctx *c, void *device_buffer, int64_t cap_bytes) {
    if (!c) return PJB_ERR_ARG;
    if (device_buffer && cap_bytes < PJB_MIRROR_HEADER_BYTES) return fail(c, PJB_ERR_ARG, "set_row_mirror: buffer smaller than its header");
    if (c->n_fl) return fail(c, PJB_ERR_STATE, "set_row_mirror: target %d is still queued", c->fl[0].tid);
    c->mirror = (uint8_t *)device_buffer;
    c->mirror_cap = device_buffer ? (size_t)cap_bytes : 0;
    mirror_reset(c);
    if (c->mirror && !c->mirror_hdr) {
        HIP_TRY(c, hipSetDevice(c->cfg.device));
        HIP_TRY(c, hipHostMalloc((void **)&c->mirror_hdr, PJB_MIRROR_HEADER_BYTES, hipHostMallocDefault));
    }
    return PJB_OK;
}

int pjb_plan_groups(const int32_t *ref_len, const int32_t *tids, int32_t n_tids, int64_t max_bases, int32_t *group_of) {
    if (n_tids < 0 || (n_tids > 0 && (!ref_len || !tids || !group_of))) return PJB_ERR_ARG;
    if (max_bases <= 0) max_bases = (int64_t)1 << 30;
    auto span = [&](int32_t k) { return group_span(ref_len[tids[k]]); };
    auto plan = [&](int64_t cap) {
        int32_t g = 0, members = 0;
        int64_t tot = 0;
        for (int32_t k = 0; k < n_tids; k++) {
            const int64_t s = span(k);
            if (members && (tot + s > cap || members >= GROUP_MAX)) g++, members = 0, tot = 0;
            group_of[k] = g;
            members++;
            tot += s;
        }
        return n_tids ? g + 1 : 0;
    };
    for (int32_t k = 0; k < n_tids; k++)
        if (tids[k] < 0) return PJB_ERR_ARG;
    int32_t n = plan(max_bases);
    if (n == 1 && n_tids > 1) { // ONE chain of more than 0.6 Gb: two, so that the first one's tail has the second one's K1 stage beside it
        int64_t total = 0;
        for (int32_t k = 0; k < n_tids; k++) total += span(k);
        if (total > 600000000) n = plan((int64_t)((double)total * 0.55));
    }
    return n;
}

int pjb_merge_rows(const void *gathered, int32_t n_ranks, int64_t slot_stride_bytes, pjb_junction_row *rows_out, int64_t cap_rows, int64_t *n_rows,
                   pjb_region_result *totals) {
    if (n_rows) *n_rows = 0;
    if (!gathered || n_ranks < 1 || slot_stride_bytes < PJB_MIRROR_HEADER_BYTES || !n_rows || !totals || cap_rows < 0 || (cap_rows > 0 && !rows_out))
        return PJB_ERR_ARG;
    struct Run { // rows of one target in one rank's slot
        int32_t refid;
        const pjb_junction_row *first;
        int64_t n;
    };
    std::vector<Run> runs;
    pjb_region_result T;
    memset(&T, 0, sizeof T);
    T.min_len = INT32_MAX;
    int64_t total = 0;
    for (int32_t r = 0; r < n_ranks; r++) {
        const uint8_t *slot = (const uint8_t *)gathered + (size_t)r * (size_t)slot_stride_bytes;
        int64_t h[6];
        memcpy(h, slot, sizeof h); // n_rows, spliced, unspliced, sum_len, min_len, max_len
        if (h[0] < 0 || h[0] > (slot_stride_bytes - PJB_MIRROR_HEADER_BYTES) / (int64_t)sizeof(pjb_junction_row)) return PJB_ERR_ARG;
        T.spliced += (uint64_t)h[1];
        T.unspliced += (uint64_t)h[2];
        T.sum_len += (uint64_t)h[3];
        T.min_len = std::min<int32_t>(T.min_len, (int32_t)std::min<int64_t>(h[4], INT32_MAX));
        T.max_len = std::max<int32_t>(T.max_len, (int32_t)h[5]);
        const pjb_junction_row *rows = (const pjb_junction_row *)(slot + PJB_MIRROR_HEADER_BYTES);
        for (int64_t i = 0; i < h[0];) {
            int64_t j = i + 1;
            while (j < h[0] && rows[j].refid == rows[i].refid) j++;
            runs.push_back(Run{rows[i].refid, rows + i, j - i});
            i = j;
        }
        total += h[0];
    }
    T.n_reads = (int64_t)(T.spliced + T.unspliced);
    T.n_junctions = total;
    *totals = T;
    *n_rows = total;
    if (total > cap_rows) return PJB_ERR_ARG;
    std::stable_sort(runs.begin(), runs.end(), [](const Run &a, const Run &b) { return a.refid < b.refid; });
    pjb_junction_row *out = rows_out;
    for (const Run &u : runs) {
        memcpy(out, u.first, (size_t)u.n * sizeof(pjb_junction_row));
        out += u.n;
    }
    return PJB_OK;
}

int pjb_clear_rows(pjb_ctx *c) {
    if (!c) return PJB_ERR_ARG;
    if (c->n_fl) return fail(c, PJB_ERR_STATE, "clear_rows: target %d is still queued", c->fl[0].tid);
    (void)rows_sync(c);
    c->rows_n = 0;
    (void)exhume(c); // (nothing is queued: the buffers that were replaced while chains ran go back now)
    {
        std::lock_guard<std::mutex> lk(c->mem.mu);
        c->mem.peak = c->mem.held;
        c->mem.peak_slabs = c->mem.cat[MEM_SLABS_OPEN] + c->mem.cat[MEM_SLABS_POOLED];
        c->mem.largest_bytes = 0;
        c->mem.largest_tid = -1;
    }
    c->slab_refused_tid = -1;
    mirror_reset(c);
    if (c->extra) {
        (void)hipSetDevice(c->cfg.device);
        (void)hipStreamSynchronize(c->stream);
        extra_clear(c);
    }
    return PJB_OK;
}

int pjb_get_kernel_timing(const pjb_ctx *c, pjb_kernel_time *out, int32_t cap, int32_t *n) {
    if (!c || !n) return PJB_ERR_ARG;
    *n = (int32_t)c->knames.size();
    for (int32_t i = 0; out && i < cap && i < *n; i++) {
        memset(&out[i], 0, sizeof out[i]);
        strncpy(out[i].name, c->knames[(size_t)i].c_str(), sizeof(out[i].name) - 1);
        out[i].launches = c->kcount[(size_t)i];
        out[i].total_ms = c->kms[(size_t)i];
    }
    return PJB_OK;
}

int pjb_select_timed_kernels(pjb_ctx *c, const char *comma_separated_names) {
    if (!c) return PJB_ERR_ARG;
    c->ktime_only.clear();
    std::string s = comma_separated_names ? comma_separated_names : "";
    size_t a = 0;
    while (a < s.size()) {
        size_t b = s.find(',', a);
        if (b == std::string::npos) b = s.size();
        if (b > a) c->ktime_only.push_back(s.substr(a, b - a));
        a = b + 1;
    }
    return PJB_OK;
}

int pjb_reset_kernel_timing(pjb_ctx *c) {
    if (!c) return PJB_ERR_ARG;
    std::fill(c->kcount.begin(), c->kcount.end(), 0);
    std::fill(c->kms.begin(), c->kms.end(), 0.0);
    return PJB_OK;
}

int pjb_set_option(pjb_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return PJB_ERR_ARG;
    if (c->n_fl) return fail(c, PJB_ERR_STATE, "set_option: target %d is still queued", c->fl[0].tid);
    const std::string n = name;
    if (n == "overlap") c->side_stream = value != 0;
    else if (n == "dense_ids") c->dense_ids = value != 0;
    else if (n == "extra_dense") c->extra_dense_only = value != 0;
    else if (n == "sort_floor") c->sort_floor = (u32)std::max<int64_t>(1, std::min<int64_t>(value, 1 << 30));
    else if (n == "window_skip") c->window_skip = value != 0;
    else if (n == "run_sort") c->run_sort = value != 0;
    else if (n == "run_window") {
        if (value < 0 || value > (int64_t)RUN_W) return fail(c, PJB_ERR_ARG, "set_option: run_window takes 0 (the default, %u) to %u", RUN_W, RUN_W);
        c->run_window = (u32)value;
    } else if (n == "pair_range") {
        int shift = -1;
        for (int k = 0; k <= PAIR_RANGE_SHIFT_MAX; k++)
            if (value == (int64_t)1 << k) shift = k;
        if (shift < 0) return fail(c, PJB_ERR_ARG, "set_option: pair_range takes 1, 2, 4, 8, 16 or 32 slices a range (the default: %d)", 1 << PAIR_RANGE_SHIFT_DEFAULT);
        c->pair_range_shift = shift;
    } else if (n == "grow_batch") {
        if (value < 0 || value > 32768) return fail(c, PJB_ERR_ARG, "set_option: grow_batch takes 0 (the default: what the pool holds) to 32768 trees");
        c->model.grow_batch = (u32)value;
    } else if (n == "knn_chunk") {
        if (value < 0 || value > (1 << 22)) return fail(c, PJB_ERR_ARG, "set_option: knn_chunk takes 0 (the default: sized to fill the chip) to %d base rows", 1 << 22);
        c->model.knn_chunk = (u32)value;
    } else if (n == "mem_limit") {
        if (value < 0) return fail(c, PJB_ERR_ARG, "set_option: mem_limit takes 0 (the default: no limit) or a number of bytes");
        std::lock_guard<std::mutex> lk(c->mem.mu);
        c->mem.limit = (size_t)value;
    } else if (n == "list_cap") c->list_cap_forced = (u32)std::max<int64_t>(0, std::min<int64_t>(value, 1 << 30));
    else return fail(c, PJB_ERR_ARG, "set_option: unknown option '%s'", name);
    return PJB_OK;
}

int pjb_memory_info(const pjb_ctx *c, pjb_memory *out) {
    if (!c || !out) return PJB_ERR_ARG;
    memset(out, 0, sizeof *out);
    {
        std::lock_guard<std::mutex> lk(c->mem.mu);
        const MemBook &m = c->mem;
        out->genomes = m.cat[MEM_GENOMES];
        out->slabs_open = m.cat[MEM_SLABS_OPEN];
        out->slabs_pooled = m.cat[MEM_SLABS_POOLED];
        out->staging = m.cat[MEM_STAGING];
        out->scratch = m.cat[MEM_SCRATCH];
        out->rows = m.cat[MEM_ROWS];
        out->other = m.cat[MEM_OTHER];
        out->held = m.held;
        out->limit = m.limit;
        out->peak_held = m.peak;
        out->peak_records = m.peak_slabs;
        out->largest_target_bytes = m.largest_bytes;
        out->largest_target = m.largest_tid;
    }
    // (hipMemGetInfo answers for the calling thread's current device: the context's for the length of the call, the caller's again after it)
    int was = -1;
    size_t f = 0, t = 0;
    if (hipGetDevice(&was) != hipSuccess) was = -1;
    if ((was == c->cfg.device || hipSetDevice(c->cfg.device) == hipSuccess) && hipMemGetInfo(&f, &t) == hipSuccess) {
        out->hip_free = f;
        out->hip_total = t;
    }
    if (was >= 0 && was != c->cfg.device) (void)hipSetDevice(was);
    (void)hipGetLastError();
    return PJB_OK;
}

int pjb_get_timing(const pjb_ctx *c, pjb_timing *out) {
    if (!c || !out) return PJB_ERR_ARG;
    if (c->cfg.abi_version >= 4) *out = c->timing;
    else memcpy(out, &c->timing, offsetof(pjb_timing, repeats)); // (ABI 3's pjb_timing ended at checked_reads)
    return PJB_OK;
}

} // extern "C"
