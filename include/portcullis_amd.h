/*
 * portcullis_amd.h -- C ABI of the MI355X-native `junc` hot path.
 *
 * This is the drop-in boundary: everything HIP lives behind these entry
 * points; the host side (C++ JunctionBuilder / JunctionSystem mirror in
 * portcullis_amd/host/, or any other binding) only sees plain pointers and
 * sizes.  No exceptions cross the boundary: every call returns PJB_OK (0) or
 * a negative PJB_ERR_* code and pjb_last_error() gives the message.
 *
 * What each entry point replaces in the reference (paths relative to the
 * reference checkout):
 *
 *   pjb_set_refs          BamReader::createRefList           src/junction_builder.cc:103-108
 *   pjb_upload_contig     GenomeMapper::fetchBases (6 faidx fetches per junction)
 *                                                            lib/src/junction.cc:566-593,
 *                                                            lib/src/genome_mapper.cc:111-118
 *   pjb_submit_batch      the per-record body of findJuncs: BamAlignment::init,
 *                         length stats, JunctionSystem::addJunctions
 *                                                            src/junction_builder.cc:322-343,
 *                                                            lib/src/bam_alignment.cc:71-100,
 *                                                            lib/src/junction_system.cc:140-210
 *   pjb_finish_contig     junction finalisation for one target sequence:
 *                         Junction::calcMetrics + processJunctionWindow and the
 *                         RegionResult counters                src/junction_builder.cc:324-356,
 *                                                            lib/src/junction.cc:561-649,683-909
 *   pjb_collect           JunctionSystem::append of the per-contig systems
 *                                                            src/junction_builder.cc:258-269
 *   pjb_collect_device    the same rows, still in HBM (multi-GPU merge over xGMI)
 *   pjb_submit_bam        the reader loop itself: BamReader::setRegion / next and htslib's
 *                         bgzf_read_block / inflate_block / bam_read1 for one target
 *                                                            lib/src/bam_reader.cc:78-146,
 *                                                            deps/htslib-1.3/bgzf.c:292-316,421-540
 *   pjb_inflate_bgzf      inflate_block for a run of BGZF blocks
 *   pjb_deflate_bgzf      deflate_block for a stream of bytes (the BAM files the stages write)
 *                                                            deps/htslib-1.3/bgzf.c:292-316
 *
 * A context is bound to one HIP device and is not thread-safe; use one
 * context per GPU and call it from one thread.  Several contigs may be open at
 * once: the batches of one contig must arrive in BAM file order, batches of
 * different contigs may interleave, and pjb_finish_contig closes one contig.
 */
#ifndef PORTCULLIS_AMD_H
#define PORTCULLIS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PJB_ABI_VERSION 4 /* 4: pjb_batch.seq2 / .seq_exc (2-bit bases with their exception bitmap; a context created with abi_version 3 is
                           *    served as before: the two members are not read), pjb_merge_rows
                           * 2: pjb_batch.name_hash, PJB_FLAG_EXTRA, pjb_extra_finish
                           * 3: pjb_timing grew (generic_reads, position_runs, candidates, checked_reads); PJB_MAX_QUEUED 8; pjb_last_error is per calling
                           *    thread; additive since 2: PJB_FLAG_NO_CHAINS, pjb_finish_group_begin/_end, pjb_finish_ready, pjb_deflate_bgzf,
                           *    pjb_host_register/_unregister; the option "fused_k1" is gone */

/* ---- status codes ------------------------------------------------------ */
#define PJB_OK 0
/* data conditions under which the reference throws / crashes (fatal there, reported here) */
#define PJB_ERR_BAD_XS (-1)          /* strandFromChar, bam_master.hpp:60-72 */
#define PJB_ERR_NO_PRESENCE (-2)     /* bam_alignment.cc:342,406 */
#define PJB_ERR_ZERO_LEN_OP (-3)     /* bam_alignment.cc:363 */
#define PJB_ERR_QUERY_RANGE (-4)     /* bam_alignment.cc:376 */
#define PJB_ERR_GENOME_RANGE (-5)    /* bam_alignment.cc:437 */
#define PJB_ERR_QREGION (-6)         /* bam_alignment.cc:414-421 */
#define PJB_ERR_ANCHOR_MISMATCH (-7) /* junction.cc:192-223 */
#define PJB_ERR_SPLICE_SITE_LEN (-8) /* junction.cc:570-585 */
#define PJB_ERR_ANCHOR_LEN (-9)      /* junction.cc:610-623 */
#define PJB_ERR_INTRON_FLANK_LEN (-10) /* junction.cc:624-633 */
#define PJB_ERR_MIN_ANCHOR (-11)     /* intron.cc:67-83 */
#define PJB_ERR_HAMMING_LEN (-12)    /* seq_utils.hpp:62-67 */
#define PJB_ERR_CLIP_RANGE (-13)     /* substr out_of_range, bam_alignment.cc:263 */
#define PJB_ERR_UNSORTED (-14)       /* input contract: coordinate-sorted BAM */
/* API / runtime conditions */
#define PJB_ERR_NOMEM (-15)
#define PJB_ERR_ARG (-16)
#define PJB_ERR_HIP (-17)            /* a HIP runtime call failed */
#define PJB_ERR_NO_DEVICE (-18)      /* no usable gfx950 device: there is NO CPU fallback */
#define PJB_ERR_STATE (-19)          /* calls out of order */
#define PJB_ERR_DIVERGENT (-20)      /* malformed CIGAR: padded query/genome walks emit different
                                        lengths for one op (the reference would compare misaligned
                                        strings or crash; we refuse) */
#define PJB_ERR_BGZF (-22)           /* corrupt BGZF / DEFLATE data (bgzf.c:292-316 returns BGZF_ERR_ZLIB) */
#define PJB_ERR_NO_SEQ (-21)         /* a spliced read was submitted without its sequence bytes */

/* enums follow the reference's order (bam_master.hpp:50-54,92-97,133-139; junction.hpp:86-91) */
enum { PJB_STRAND_POS = 0, PJB_STRAND_NEG = 1, PJB_STRAND_UNK = 2 };
enum { PJB_CSS_CANONICAL = 0, PJB_CSS_SEMI = 1, PJB_CSS_NO = 2 };
enum { PJB_OR_SE = 0, PJB_OR_FR = 1, PJB_OR_RF = 2, PJB_OR_FF = 3, PJB_OR_UNKNOWN = 4 };
enum { PJB_SS_UNSTRANDED = 0, PJB_SS_FIRSTSTRAND = 1, PJB_SS_SECONDSTRAND = 2, PJB_SS_UNKNOWN = 3 };

typedef struct pjb_ctx pjb_ctx;

typedef struct pjb_config {
    int32_t abi_version;  /* PJB_ABI_VERSION */
    int32_t device;       /* HIP device ordinal */
    int32_t orientation;  /* PJB_OR_*  (JunctionBuilder::setOrientation, src/junction_builder.hpp:190) */
    int32_t strandedness; /* PJB_SS_*  accepted for API parity; like the reference it does not
                             change junc output (the reader's alignments carry
                             Strandedness::UNKNOWN, lib/src/bam_alignment.cc:154-165) */
    uint32_t flags;       /* PJB_FLAG_* */
} pjb_config;

/* record a HIP event pair around every kernel launch and accumulate per-kernel time
 * (pjb_get_kernel_timing); costs ~1 us per launch, off by default */
#define PJB_FLAG_KERNEL_TIMING 1u
/* `junc --extra` (JunctionBuilder::setExtra, src/junction_builder.hpp:166; calcExtraMetrics,
 * src/junction_builder.cc:293-312): every pjb_finish_contig also builds the contig's unspliced per-base depth,
 * the flanking alignment counts of its junctions and keeps the name codes of its spliced records; pjb_extra_finish
 * then yields mm_score / coverage / up_aln / down_aln for every row.  Batches must carry name_hash. */
#define PJB_FLAG_EXTRA 2u
/* a context that will not queue kernel chains (bamfilt: pjb_filter_batch, pjb_deflate_bgzf only): pjb_create leaves the chain
 * slots' streams and events (60 ms) to their first use */
#define PJB_FLAG_NO_CHAINS 4u

/* One batch of fixed-width alignment records of ONE contig, in BAM file order
 * (structure of arrays; BAM-native encodings):
 *   cigar    uint32 len<<4|op, op indexes "MIDNSHP=XB"
 *   cig_off  n_reads+1 offsets into cigar
 *   seq4     4-bit packed bases, high nibble first; each read's bytes start on a
 *            4-byte boundary
 *   seq_off  n_reads+1 offsets into seq4 in 4-byte WORDS; only reads with an N
 *            operation need sequence bytes, others may be empty
 *   xs       0 = no XS:A tag / '?' / '.', 1 = '+', 2 = '-', 3 = any other value
 */
typedef struct pjb_batch {
    int64_t n_reads;
    const int32_t *pos;
    const uint16_t *flag;
    const uint8_t *mapq;
    const uint8_t *xs;
    const int32_t *l_qseq;
    const int32_t *mtid;
    const int32_t *mpos;
    const uint32_t *cig_off;
    const uint32_t *cigar;
    const uint32_t *seq_off;
    const uint8_t *seq4;
    /* std::hash<std::string>()(BamAlignment::deriveName()) per record (lib/include/portcullis/junction.hpp:158,
     * lib/src/bam_alignment.cc:233-242: QNAME, plus "_R1" / "_R2" / "_R?" for paired reads); only read by
     * contexts created with PJB_FLAG_EXTRA, may be NULL otherwise. */
    const uint64_t *name_hash;
    /* ---- ABI 4 (read only when pjb_config.abi_version >= 4; both NULL: the compares run on seq4 as before) ----
     * seq2     the same bases in 2 bits (A 0, C 1, G 2, T 3), one uint16 per seq4 WORD: element seq_off[r] + k holds bases 8k .. 8k+7 of
     *          read r, base j at bits 2j, 2j+1 (what is stored for a base outside ACGT, or behind the read's last base, does not matter).
     *          As many elements as seq4 has words, rounded up to an even number (the device reads the array as 32-bit words); the array
     *          starts on a 4-byte boundary.
     * seq_exc  bit r (bit r & 31 of word r >> 5) set: read r is NOT to be compared in 2 bits -- one of its l_qseq bases is not A, C, G or
     *          T (BAM codes 1, 2, 4, 8), or it carries fewer than l_qseq bases.  (n_reads + 31) / 32 words.
     * Who fills them: the device ingest (pjb_submit_bam / pjb_bam_*) as it transcodes the records; a caller that decodes BAM itself
     * packs them where it copies SEQ (AlignmentInfo::calcMatchStats compares characters, lib/src/junction.cc:147-240, and a read of
     * pure ACGT against a stretch of pure ACGT compares the same in 2 bits -- k1_emit takes the 4-bit codes for everything else). */
    const uint16_t *seq2;
    const uint32_t *seq_exc;
} pjb_batch;

/* RegionResult (src/junction_builder.hpp:62-76) plus sizes of what was built */
typedef struct pjb_region_result {
    uint64_t spliced;
    uint64_t unspliced;
    uint64_t sum_len;
    int32_t min_len; /* INT32_MAX when the contig has no reads (src/junction_builder.cc:319) */
    int32_t max_len;
    int64_t n_reads;
    int64_t n_pairs;     /* (alignment, junction) pairs = N operations walked */
    int64_t n_junctions; /* distinct introns on this contig */
} pjb_region_result;

/* One junction as it stands after Junction::calcMetrics + processJunctionWindow
 * (i.e. before the cross-junction pass JunctionSystem::calcJunctionStats, which
 * is O(J) host work above this ABI).  Field names follow the .tab columns. */
typedef struct pjb_junction_row {
    int32_t refid;
    int32_t start, end;   /* intron, 0-based inclusive */
    int32_t left, right;  /* leftAncStart, rightAncEnd */
    uint8_t read_strand, ss_strand, cons_strand; /* PJB_STRAND_* */
    uint8_t canonical;                           /* PJB_CSS_* */
    uint8_t da1[2], da2[2];                      /* ss1 / ss2; may hold NUL (REVCOMP_LOOKUP quirk) */
    uint8_t suspicious;
    uint8_t _pad[3];
    uint32_t nb_raw, nb_dist, nb_ms, nb_um, nb_bpp, nb_ppp, nb_rel;
    uint32_t r1pos, r1neg, r2pos, r2neg;
    uint32_t max_min_anc, maxmmes, hamming5p, hamming3p;
    uint32_t nb_up_juncs, nb_down_juncs;
    uint32_t jad[20];
    uint32_t _pad2;
    uint64_t sum_mismatches; /* mean_mismatches = sum_mismatches / nb_raw (junction.cc:893) */
    double entropy;
} pjb_junction_row;

/* Device-side timing of the last pjb_finish_contig (HIP events on the context's stream) */
#define PJB_N_STAGES 8
typedef struct pjb_timing {
    float total_ms;               /* first kernel -> rows resident on host */
    float stage_ms[PJB_N_STAGES]; /* scan/emit, sort, group, anchors, pair stats, finalise, d2h, (spare): filled only under
                                     PJB_FLAG_KERNEL_TIMING with no kernel selection (an event between kernels costs a bubble) */
    int64_t sort_passes;
    int64_t generic_pairs; /* pairs that took the generic CIGAR walks (k4b_generic) instead of k1_emit's [S]MNM[S] fast path */
    int64_t generic_reads; /* the reads those pairs belong to */
    int64_t position_runs; /* runs of equal read position inside the junctions (the units of the entropy kernels) */
    int64_t candidates;    /* candidate keys the dense junction ids were built from (0: the chain sorted the full keys) */
    int64_t checked_reads; /* reads of the shape [S] M (N M)+ [S] with two or more introns: finished in closed form by k1_emit, their junctions'
                              anchor windows checked by k4b_generic (not counted in generic_reads unless the check failed... they never are: a
                              failed check walks the read without moving it to the other list) */
    /* ---- ABI 4 (not written for a context created with abi_version 3) ---- */
    int64_t repeats;        /* times the chain collected last was queued AGAIN because a limit it had been queued with turned out too small */
    int64_t repeat_reasons; /* which limits, OR-ed over those repeats: 1 pairs, 2 key format, 4 junctions (or the sort's digits), 8 dense ids, 16 read lists;
                               32: the chain was a group that pjb_finish_group_end took apart -- its members were finished one by one, and the
                               other fields describe the last member's chain; 64: a tile of the sort held junction ids that do not lie in a
                               window of 2 048 (or the list of the tiles' id runs was full): repeated with the radix passes, which the
                               context's later chains then plan themselves */
} pjb_timing;

/* ---- entry points ------------------------------------------------------ */

int pjb_create(pjb_ctx **out, const pjb_config *cfg);
void pjb_destroy(pjb_ctx *ctx);

/* Message of the last failing call the CALLING THREAD made on THIS context (ctx == NULL: its last failing pjb_create); the empty
 * string if that thread's last failure was on another context or it has had none.  Kept per thread: the piece calls below may run
 * beside the context's other calls, and a thread reads its own failure.  A successful call does not clear it. */
const char *pjb_last_error(const pjb_ctx *ctx);

/* Reference sequence lengths, indexed by BAM tid. */
int pjb_set_refs(pjb_ctx *ctx, int32_t n_refs, const int32_t *ref_len);

/* Bases of one contig exactly as faidx returns them (isgraph characters, any case);
 * copied to HBM and upper-cased there (junction.cc:586-587,635-638). */
int pjb_upload_contig(pjb_ctx *ctx, int32_t tid, const uint8_t *bases, int64_t len);
/* Same, for bases that are ALREADY upper-cased and resident in HBM; borrowed until
 * pjb_release_contig / pjb_destroy. */
int pjb_upload_contig_device(pjb_ctx *ctx, int32_t tid, const uint8_t *d_bases_upper, int64_t len);

/* The same upload from the FASTA file's own bytes: `raw` holds the record's sequence lines as they are in the file
 * (from the byte the .fai's OFFSET names, raw_bytes of them), line_blen / line_len are the .fai's LINEBASES / LINEWIDTH
 * and len its LENGTH.  The device takes the line terminators out (base i is byte (i / line_blen) * line_len + i % line_blen),
 * so the host neither parses nor copies the 250 MB of a human chromosome -- GenomeMapper::fetchBases's loader
 * (faidx_fetch_seq, deps/htslib-1.3/faidx.c:439-476, keeps the graphic characters) reduced to a pread.  A record that is
 * not laid out that way (a base position that holds a non-graphic byte, a graphic byte among the terminators, too few
 * bytes) is left alone: *well_formed = 0, nothing is uploaded, and the caller filters the characters itself
 * (pjb_upload_contig).  raw in page-locked memory (pjb_host_alloc) crosses in one DMA. */
int pjb_upload_contig_fasta(pjb_ctx *ctx, int32_t tid, const uint8_t *raw, int64_t raw_bytes, int32_t line_blen, int32_t line_len,
                            int64_t len, int *well_formed);
int pjb_release_contig(pjb_ctx *ctx, int32_t tid);

/* Append a batch to contig `tid` (opens it if it is not open).  The host
 * arrays are packed into one of the context's two page-locked staging buffers
 * and moved to HBM by DMA on the context's stream; the call returns as soon as
 * the arrays have been packed, so they may be reused at once while the DMA of
 * this batch overlaps the decoding of the next. */
int pjb_submit_batch(pjb_ctx *ctx, int32_t tid, const pjb_batch *host_batch);
/* Same for arrays already resident in HBM: borrowed until pjb_finish_contig (or pjb_finish_contig_end) returns. */
int pjb_submit_batch_device(pjb_ctx *ctx, int32_t tid, const pjb_batch *device_batch);

/* Run the device pipeline over everything submitted for contig `tid` and close it.  The contig's
 * genome must have been uploaded.  On return the contig's counters are in *result and its rows are appended to the
 * table pjb_collect returns (they travel to the host by DMA; pjb_collect waits for them). */
int pjb_finish_contig(pjb_ctx *ctx, int32_t tid, pjb_region_result *result);

/* The same in two halves, so that the device never waits for the host between contigs (the reference gets the
 * same effect from its thread pool: one findJuncs per target in flight per thread, src/junction_builder.cc:215-247).
 * _begin queues the whole kernel chain of the contig and returns without waiting; _end waits for the contig's rows
 * and control block, repeats the contig if a limit it was queued with turned out too small, and closes it --
 * pjb_finish_contig is _begin followed by _end.  Up to PJB_MAX_QUEUED contigs may be queued -- their kernel chains
 * run side by side on the device --; they are collected in the order they were queued and their rows land in that order.  Between the two calls the contig's batches (and device
 * arrays lent by pjb_submit_batch_device) must stay as they are; batches for OTHER targets may be submitted, genomes
 * uploaded.  pjb_collect covers collected contigs only; pjb_clear_rows / pjb_set_row_mirror need an empty queue.
 * PJB_FLAG_EXTRA contexts queue like any other -- single chains and group chains, mixed as the caller likes: the part of the
 * extra metrics that needs the records only is queued with the chain and runs beside it, the part that needs the rows when
 * the chain is collected. */
#define PJB_MAX_QUEUED 8
int pjb_finish_contig_begin(pjb_ctx *ctx, int32_t tid);
int pjb_finish_contig_end(pjb_ctx *ctx, int32_t tid, pjb_region_result *result);

/* 1 if pjb_finish_contig_end / pjb_finish_group_end for the OLDEST queued chain would not wait for the device (its kernels
 * have completed, or nothing is queued, or the chain has to be queued again first), else 0.  Never blocks: a caller that
 * serves several targets collects finished chains when they are ready and does something else meanwhile. */
int pjb_finish_ready(pjb_ctx *ctx);

/* Several targets finished as ONE kernel chain (a "group").  A chain of ~45 kernels over one human chromosome's 8 M
 * alignments leaves most of the chip idle in most of its kernels; the reference's answer to many small targets is its
 * thread pool (one findJuncs per target and thread, src/junction_builder.cc:236-247), the device's is to walk several
 * targets' records in one pass: the group's targets are laid side by side in a virtual sequence, the intron keys carry
 * the position in it -- which is what the reference's (refId, start, end) key (lib/include/portcullis/intron.hpp:44-149)
 * amounts to -- and rows come back per target, in the order of `tids`, exactly as n calls of pjb_finish_contig would have
 * produced them (same rows, same per-target results).  Every target named must have had its batches submitted and its
 * genome uploaded; targets without alignments may be named.  _begin / _end pair up like pjb_finish_contig_begin / _end
 * and share their queue (PJB_MAX_QUEUED chains, collected in order; _end names the same targets in the same order).
 * PJB_ERR_ARG from _begin means "not as a group" (more than PJB_GROUP_MAX targets, 2^31 bases or more in all, a target
 * whose genome holds characters outside the 16-letter nucleotide alphabet, a PJB_FLAG_EXTRA context with the option
 * "extra_dense" set to 1 -- it builds a depth vector per target): nothing is queued, finish the targets one by one.  A
 * member that turns out to hold alignments outside its own sequence makes _end finish the members one by one itself
 * (pjb_timing.repeat_reasons, bit 32, says so).
 *   PJB_FLAG_EXTRA contexts take groups like any other: rows, per-target results and the rows of pjb_extra_finish are what n
 * calls of pjb_finish_contig on the same context would have produced, in the order of `tids`.  The group's unspliced records
 * are kept in the coordinates of its virtual sequence, so that depth and flanking counts of all members' junctions are answered
 * in one pass; the hand-over of a target's depth to the next target's junctions (pjb_extra_finish) still goes target by target,
 * and source and junctions may lie in different chains.  A group with a member that needs the depth vector (htslib's 8000-record
 * pileup cap may bite, a record with more than 126 deletions, more deletions than the list holds) or holds an unspliced record
 * that leaves its sequence is taken apart by _end in the same way, before anything of it is committed. */
#define PJB_GROUP_MAX 32
int pjb_finish_group_begin(pjb_ctx *ctx, const int32_t *tids, int32_t n_tids);
int pjb_finish_group_end(pjb_ctx *ctx, const int32_t *tids, int32_t n_tids, pjb_region_result *results /* n_tids of them */);

/* The chain plan: which of `tids` (in the order given) go together as groups.  group_of[k] = index of the group tids[k] belongs to
 * (ascending, groups are runs of consecutive entries); returns the number of groups, a negative status on bad arguments.  No context
 * needed (host arithmetic).  The rule: a group holds consecutive targets whose sequences -- each with the gap the group's virtual
 * sequence leaves behind it, rounded up to 64 -- add up to at most max_bases (<= 0: 2^30, the measured optimum of profiles/
 * r04d_grouping_sweep.txt) and at most PJB_GROUP_MAX members; a set that would be ONE group of more than 0.6 Gb is planned again with 0.55 of its
 * bases as the limit (two chains, three when the targets do not divide that way: the first chain's tail then runs beside the second one's first kernels -- tools/rank_share.py, profiles/r06_rank_share.json).
 * The program (`portcullis_amd junc`), bench.py and the multi-GPU ranks all plan with this one function: the reference hands every target
 * to its thread pool (src/junction_builder.cc:236-247), the device gets chains that fill it. */
int pjb_plan_groups(const int32_t *ref_len, const int32_t *tids, int32_t n_tids, int64_t max_bases, int32_t *group_of);

/* Tuning switches (queue must be empty).  Results never depend on them.
 *   "overlap"    1 (default): a contig's kernels are spread over several HIP streams -- its first kernels beside the
 *                previous contig's last ones, match statistics and entropy beside the sort and the anchors; 0: one
 *                kernel at a time on one stream (clean per-kernel timings)
 *   "dense_ids"  1 (default): the sort works on ordered dense junction ids; 0: on the full intron keys
 *   "extra_dense" 0 (default): PJB_FLAG_EXTRA answers depth and flanking counts from the unspliced records themselves
 *                (a few records per junction) and builds a target's per-base depth vector only where htslib's
 *                8000-record pileup cap may bite; 1: the depth vector for every target (round 2's path; groups are
 *                then refused with PJB_ERR_ARG: the vector is per target)
 *   "sort_floor" 65536 (default): the sort's digits cover at least this many junction ids (and twice what the context's chains have
 *                had); n (test hook): a small floor, so that a chain with more junctions than planned for is repeated
 *   "list_cap"   0 (default): the kernels' read lists get the room the pair limit implies; n > 0 (test hook): the first attempt
 *                of every chain gets room for n entries per sub-list, so that the overflow-and-repeat path runs
 *   "mem_limit"  0 (default): the context holds as much device memory as the runtime gives it; n > 0: an allocation that would take
 *                pjb_memory.held beyond n bytes is treated exactly like a hipMalloc that failed (see pjb_memory_info) */
int pjb_set_option(pjb_ctx *ctx, const char *name, int64_t value);

/* The device memory this context holds, in bytes of capacity (what was allocated, not what is in use), category by category.  Every
 * allocation of the context is counted, so `held` is exact and is the sum of the seven categories before it.
 *
 * When an allocation fails -- the runtime refuses it, or it would take `held` beyond `limit` -- the context first gives back what it
 * holds without needing it: the buffers that were replaced by larger ones and wait for their release, the pooled slabs, the pooled
 * stage buffers (no chain reads any of them), in that order and no more kinds than the request needs; then it asks once more; a slab
 * or arena chunk that was asked for with room to spare is then asked for with exactly the bytes needed.  Only then does the call
 * return PJB_ERR_NOMEM; pjb_last_error names the bytes wanted, `held` and `limit`.  (A request that the limit refuses and that all
 * of the above would not make fit is refused at once, and the pools stay.)  One exception to that order: a slab of exactly the bytes
 * needed leaves a target's records in one small allocation per array, so while another open target or a queued chain holds slabs --
 * which collecting would return to the pool -- a slab request is refused BEFORE the exact size is tried.  The repeat of the refused
 * call for the same target with nothing freed in between is then given the exact size (and fails again only if that does not fit
 * either); the refusal is forgotten when the target is collected or released, by pjb_clear_rows and by pjb_set_refs.
 *
 * PJB_ERR_NOMEM from pjb_submit_batch, pjb_submit_bam, pjb_bam_begin and pjb_bam_end is RETRYABLE (pjb_bam_piece never returns it: it
 * copies into the buffer pjb_bam_begin allocated, and an early inflate that finds no memory is left to pjb_bam_end).  The call leaves the
 * target as it was before the call: no batch has been added, and what the call took from the target's slabs has gone back (bytes to the
 * target's earlier slabs, slabs to the pool they came from or to the device).  pjb_memory_info reads as before the call, with two
 * exceptions: what the release described above gave back is gone from `slabs_pooled`, `staging` and `scratch`, and a scratch buffer
 * the call had enlarged before it failed stays enlarged (the repeat needs it).  For pjb_bam_end the staged pieces and a finished
 * inflate stay: the same call can be repeated, no piece is sent again.  Free memory in between -- collect a queued chain
 * (pjb_finish_contig_end / _group_end give the chain's slabs back to the pool), raise the limit -- and repeat the call; when nothing
 * is left to free, repeat it once more: that repeat is the one that may take exact-size slabs (above), and its PJB_ERR_NOMEM is
 * final.  Any other error of pjb_bam_piece / pjb_bam_end releases the stage as before; a
 * stage that is never picked up again is released by pjb_destroy.  PJB_ERR_NOMEM from any other call (a genome upload, a chain that
 * cannot get its scratch) is final for that call's target.
 *   pjb_memory_info reads hipMemGetInfo on the context's device and leaves the calling thread's current device as it found it. */
typedef struct pjb_memory {
    uint64_t genomes;      /* bases and codes of the uploaded targets, and those kept for the next upload */
    uint64_t slabs_open;   /* the records of targets that have not been collected yet */
    uint64_t slabs_pooled; /* slabs of collected targets, kept for the next target */
    uint64_t staging;      /* pjb_bam_*: staged BGZF bytes, inflated bytes and tables, in use and pooled */
    uint64_t scratch;      /* the chains' and the ingest's working buffers, those waiting for their release included */
    uint64_t rows;         /* the row table */
    uint64_t other;        /* PJB_FLAG_EXTRA arenas and vectors, bamfilt's junction keys */
    uint64_t held;         /* the sum of the above */
    uint64_t limit;        /* pjb_set_option("mem_limit", n); 0: none */
    uint64_t peak_held;    /* the largest `held` since pjb_create or the last pjb_clear_rows */
    uint64_t peak_records; /* slabs_open + slabs_pooled at the moment peak_held was reached */
    uint64_t largest_target_bytes; /* the most slab capacity one target has held when it was collected, since pjb_create or the last */
    int64_t largest_target;        /* pjb_clear_rows, and that target (-1: none collected yet) */
    uint64_t hip_free, hip_total; /* hipMemGetInfo now: the whole device, other contexts and processes included */
} pjb_memory;
int pjb_memory_info(const pjb_ctx *ctx, pjb_memory *out);

/* All rows built so far, contig by contig in finish order, (start,end)-sorted
 * within a contig.  The pointer stays valid until the next finish/clear/destroy. */
int pjb_collect(pjb_ctx *ctx, const pjb_junction_row **rows, int64_t *n_rows);
/* The rows of the contig finished last, still in HBM (device pointer; valid until the next
 * pjb_finish_contig / pjb_destroy): what a multi-GPU merge all-gathers over xGMI without a detour
 * through host memory. */
int pjb_collect_device(pjb_ctx *ctx, const pjb_junction_row **device_rows, int64_t *n_rows);
/* A device buffer of the caller's (cap_bytes, 0 / NULL to stop) that every following pjb_finish_contig fills
 * before it returns: a 64-byte header of int64 { n_rows, spliced, unspliced, sum_len, min_len, max_len, 0, 0 }
 * followed by rows.  The buffer ACCUMULATES: the rows of every contig finished since the last
 * pjb_set_row_mirror / pjb_clear_rows are appended in finish order and the header holds the row total and the
 * folded counters (sums, min, max), so a rank that owns several contigs has ONE send slot per merge.  It is the
 * send slot of the multi-GPU merge (JunctionSystem::append + the counter sums of src/junction_builder.cc:258-269):
 * when pjb_finish_contig returns the slot can go straight into an all-gather, without a copy or a
 * synchronisation on the caller's side.  Rows that do not fit fail with PJB_ERR_ARG. */
#define PJB_MIRROR_HEADER_BYTES 64
int pjb_set_row_mirror(pjb_ctx *ctx, void *device_buffer, int64_t cap_bytes);
/* The RECEIVE side of that merge, for a caller that runs one process per GPU: `gathered` (HOST memory) holds n_ranks send slots as
 * pjb_set_row_mirror leaves them -- slot r at gathered + r * slot_stride_bytes: the 64-byte header, then its rows -- i.e. what an
 * all-gather of the ranks' slots (ncclAllGather over xGMI, MPI_Allgather, ...) followed by one copy to the host delivers.  Writes ONE
 * table to rows_out: every rank's rows, stably ordered by refid -- a target's rows are contiguous in its rank's slot and already
 * (start, end)-sorted, so this is JunctionSystem::sort's order (lib/src/junction_system.cc:322-330) over the appended systems
 * (src/junction_builder.cc:258-269) -- and folds the ranks' read-length counters into *totals (sums, min, max: src/junction_builder.cc:
 * 270-278; n_reads = spliced + unspliced, n_junctions = rows written, n_pairs = 0: the header does not carry it).  Host arithmetic
 * only: no context, no device, no collective library inside -- INTEGRATION.md section "multi-GPU" shows the lines around it.
 * PJB_ERR_ARG: a header with a negative count or more rows than the slot holds, or cap_rows too small (*n_rows then says how many). */
int pjb_merge_rows(const void *gathered, int32_t n_ranks, int64_t slot_stride_bytes, pjb_junction_row *rows_out, int64_t cap_rows,
                   int64_t *n_rows, pjb_region_result *totals);
int pjb_clear_rows(pjb_ctx *ctx);

/* The --extra columns of one junction (lib/include/portcullis/junction.hpp:240-243). */
typedef struct pjb_extra_row {
    double mm_score;  /* Junction::calcMultipleMappingScore, lib/src/junction.cc:914-921 */
    double coverage;  /* Junction::calcCoverage, lib/src/junction.cc:935-951, on DepthParser's vector
                         (lib/src/depth_parser.cc:112-164), handed out per JunctionSystem::calcCoverage
                         (lib/src/junction_system.cc:231-242) */
    uint32_t up_aln;  /* nbUpstreamFlankingAlignments, lib/src/junction.cc:651-677 */
    uint32_t down_aln;
} pjb_extra_row;
/* JunctionBuilder::calcExtraMetrics (src/junction_builder.cc:293-312) once every contig of the FILE has been
 * finished on this context (the name multiplicities and the depth hand-over between consecutive targets are
 * file-wide): one pjb_extra_row per row of pjb_collect, same order.  Needs PJB_FLAG_EXTRA.  The pointer stays
 * valid until the next pjb_clear_rows / pjb_destroy. */
int pjb_extra_finish(pjb_ctx *ctx, const pjb_extra_row **rows, int64_t *n_rows);

int pjb_get_timing(const pjb_ctx *ctx, pjb_timing *out);

/* Per-kernel device time (HIP events on the context's stream), accumulated over all
 * pjb_finish_contig calls since creation / the last reset.  Needs PJB_FLAG_KERNEL_TIMING. */
typedef struct pjb_kernel_time {
    char name[32];
    int64_t launches;
    double total_ms;
} pjb_kernel_time;
int pjb_get_kernel_timing(const pjb_ctx *ctx, pjb_kernel_time *out, int32_t cap, int32_t *n);
int pjb_reset_kernel_timing(pjb_ctx *ctx);
/* Restrict the event bracketing to the named kernels ("k4_pairs,rs_scatter"); "" or NULL = all. */
int pjb_select_timed_kernels(pjb_ctx *ctx, const char *comma_separated_names);

/* Page-locked host memory for batch arrays (hipHostMalloc); NULL if it cannot be had. */
void *pjb_host_alloc(size_t bytes);
void pjb_host_free(void *p);
/* Page-lock memory the caller already has -- e.g. a read-only mapping of the BAM file: the file's bytes then cross from the
 * page cache by DMA, without a copy by the CPU (hipHostRegister; `p` and `bytes` multiples of the page size).  The range
 * must not overlap another registered range; unregister before unmapping. */
int pjb_host_register(void *p, size_t bytes);
int pjb_host_unregister(void *p);

/* Number of visible HIP devices (0 if none); does not create a context. */
int pjb_device_count(void);

/* ---- device-side ingest -------------------------------------------------------
 * Inflate a run of whole BGZF blocks on the device: replaces the bgzf_read_block / inflate_block loop of
 * htslib (deps/htslib-1.3/bgzf.c:292-316, 421-540) that BamReader::next drives one block at a time
 * (lib/src/bam_reader.cc:134-142).  `comp` holds `comp_bytes` bytes of consecutive BGZF blocks (host
 * memory; page-locked memory from pjb_host_alloc makes the copy asynchronous); the inflated bytes of all
 * blocks are written back to `out` (capacity `out_cap`) and their count to *out_bytes.  Like
 * inflate_block, the footer CRC32 is not verified; a block whose inflated size differs from its ISIZE
 * field is an error (PJB_ERR_BGZF, message names the block).  An empty block (the BGZF EOF marker)
 * contributes nothing. */
int pjb_inflate_bgzf(pjb_ctx* ctx, const uint8_t* comp, int64_t comp_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes);

/* The other direction: BGZF-compress `n_bytes` at `in` (host memory) on the device, for the BAM files the stages write
 * (BamWriter::write -> bam_write1 -> bgzf_write -> deflate_block, lib/src/bam_writer.cc:58-60,
 * deps/htslib-1.3/bgzf.c:216-262,580-613).  The input is cut into blocks of `block_bytes` bytes (a multiple of 4, at most
 * 0xff00 = BGZF_BLOCK_SIZE; the last block may be shorter); every block becomes one complete BGZF member (gzip header with
 * the BC field, a dynamic-Huffman or stored deflate block, CRC-32, ISIZE) and the members are written back to back to `out`
 * (capacity out_cap; n_blocks * 65536 always suffices), their total to *out_bytes, and -- if member_size is not NULL -- each
 * member's length to member_size[0 .. n_blocks) (a writer needs them for virtual file offsets).  No EOF block is added.
 * Any inflater reads the result; it is not the byte stream zlib would have produced (a single hash candidate per position). */
int pjb_deflate_bgzf(pjb_ctx* ctx, const uint8_t* in, int64_t n_bytes, int32_t block_bytes, uint8_t* out, int64_t out_cap, int64_t* out_bytes,
                     uint32_t* member_size);

/* One target's alignments straight from the file bytes: inflate + BAM record parse + transcode to the
 * pjb_batch layout, all on the device; the records are appended to target `tid` exactly as a
 * pjb_submit_batch of the same alignments would be.  Replaces the reader loop of
 * JunctionBuilder::findJuncs (src/junction_builder.cc:322-343: BamReader::setRegion / next /
 * BamAlignment::init, lib/src/bam_reader.cc:78-146, lib/src/bam_alignment.cc:71-100) for the whole target.
 *   comp, comp_bytes : consecutive whole BGZF blocks (host memory; page-locked memory from pjb_host_alloc is
 *                      DMA'd directly, anything else goes through the context's staging buffers), from the
 *                      block that holds the target's
 *                      first record through (at least) the block that holds its last one;
 *   first_uoffset    : offset of that first record inside the first block's inflated bytes (the low
 *                      16 bits of the index's virtual offset).
 * Records are taken until the first one whose refID is not `tid` (or whose position is past the
 * target's end, as hts_itr would stop) or the end of the data.  Data that ends inside one of the target's
 * records (before any record of another target) is an error: PJB_ERR_BGZF.  One call per target.  *n_records (optional) receives the number of alignments added.
 * Errors: PJB_ERR_BGZF for corrupt BGZF / DEFLATE / BAM record data. */
int pjb_submit_bam(pjb_ctx* ctx, int32_t tid, const uint8_t* comp, int64_t comp_bytes, int32_t first_uoffset, int64_t* n_records);

/* The same with the target's bytes arriving in PIECES, in file order, any sizes -- for a reader that fills a small ring
 * of page-locked buffers instead of one buffer per target (page-locking memory costs ~0.15 s per GB: three 3 GB buffers
 * were 1.4 s of a 5 s run over a 33 GB file):
 *   pjb_bam_begin        announces `total_bytes` for target `tid` and reserves device memory for them;
 *   pjb_bam_piece        queues the copy of the next `bytes` to the device (asynchronous if `piece` is page-locked)
 *                        and meanwhile hops over the BGZF block headers that this piece completes; *ticket (optional)
 *                        identifies the copy;
 *   pjb_bam_pieces_done  *completed_ticket = the highest ticket whose copy has left its host buffer (copies complete
 *                        in order; never blocks): the buffers of all pieces up to it may be reused;
 *   pjb_bam_end          inflate + parse + transcode of the staged bytes: from here on exactly pjb_submit_bam
 *                        (same result, same errors; a BGZF error found while hopping is reported by the piece call;
 *                        a failing piece call drops the target's staging: begin again).
 * Several targets may be between _begin and _end at once (each has its own device buffers, taken from pools the
 * context keeps).  The call that hands over a target's LAST piece also starts its inflate (own stream, lowest priority,
 * behind the copy): see pjb_bam_inflate_done.
 * Threads: pjb_bam_begin, _piece, _pieces_done and _inflate_done may be called from other threads than the one that makes
 * the context's other calls (a thread that reads the file hands its pieces over itself); pjb_bam_end belongs to that one
 * thread, like everything else. */
int pjb_bam_begin(pjb_ctx* ctx, int32_t tid, int64_t total_bytes);
int pjb_bam_piece(pjb_ctx* ctx, int32_t tid, const uint8_t* piece, int64_t bytes, int64_t* ticket);
int pjb_bam_pieces_done(pjb_ctx* ctx, int64_t* completed_ticket);
int pjb_bam_end(pjb_ctx* ctx, int32_t tid, int32_t first_uoffset, int64_t* n_records);
/* The target's inflate (bgzf_decode + bgzf_resolve) starts by itself when its last piece has been handed over (on a stream of its own, behind the
 * copy): 1 if it has finished -- or none is in flight -- i.e. pjb_bam_end will not wait for it, else 0.  A caller that
 * serves several targets can hand over other targets' pieces meanwhile; their inflates then run side by side (a launch
 * takes ~50 ms whatever its size, and most targets do not fill the chip). */
int pjb_bam_inflate_done(pjb_ctx *ctx, int32_t tid);

/* ---- the BAM index of a coordinate-sorted file (`portcullis_amd prep`) -------------------------------------------
 * What `samtools index` does for the reference's prep (src/prepare.cc:290-332: Prepare::bamIndex shells out to it), on the
 * device: BGZF inflate, the record walk of pjb_submit_bam over every target, and the BAI arithmetic of SAM spec 5.2 / 5.3 as
 * BamWriter::indexRecord does it -- per record beg = pos, end = pos + max(1, reference span of the CIGAR) (clipped to the
 * target's end), bin = reg2bin(beg, end); chunks per (target, bin), a record joining the bin's last chunk when that chunk
 * ends where the record starts; per 16 kb window the virtual offset of the first record that overlaps it.  No metadata
 * pseudo-bin, no count of unplaced records.  Records with refID < 0 add nothing.  The targets are those of pjb_set_refs.
 *   pjb_index_begin  starts an index (drops one that was being built, and the last result);
 *   pjb_index_piece  a run of whole BGZF blocks, in file order (host memory; page-locked memory is DMA'd directly, anything
 *                    else goes through the context's staging buffers):
 *                      file_offset   : offset of the piece's first block in the file;
 *                      first_uoffset : where the first record not yet indexed starts in the piece's inflated bytes (the
 *                                      low 16 bits of the last call's *next_voffset; behind the BAM header for the first
 *                                      piece -- it may lie beyond the first block, a long header);
 *                      last          : non-zero for the piece that ends the file.
 *                    Every record that lies COMPLETELY inside the piece is indexed; *next_voffset receives the virtual
 *                    offset of the first record that was not -- one that begins in this piece and ends beyond it, or the end
 *                    of the data (then the start of the block behind the last data: the EOF block).  The next piece starts
 *                    with the block it names (next_voffset >> 16): a straddling record's block is handed over twice, no
 *                    bytes are carried.  The result does not depend on where the file was cut.
 *   pjb_index_end    closes the last chunk, orders the chunks by (target, bin, file order) and hands the result over: host
 *                    memory owned by the context until the next pjb_index_begin / pjb_destroy.
 * Errors: PJB_ERR_UNSORTED a record lies before its predecessor in (refID as unsigned, pos) -- the message names its ordinal
 * (0-based, over all alignment records); PJB_ERR_BGZF corrupt BGZF / DEFLATE / record data, a refID beyond the targets or a
 * position outside its target, data that ends inside a record when last != 0; PJB_ERR_ARG "BAI cannot index this target": a
 * record on a target of 2^29 bases or more; PJB_ERR_STATE calls out of order.  A failing piece call drops the index: begin
 * again.  The one exception: a piece whose first record is longer than the piece fails with PJB_ERR_ARG and a message that
 * says so, sets *next_voffset to that record and leaves the index as it was -- the same blocks may be handed over again with
 * more blocks behind them.
 * Threads: like pjb_bam_end, these calls belong to the thread that makes the context's other calls. */
typedef struct pjb_index_chunk {
    uint64_t vbeg, vend; /* virtual offsets: (offset of the BGZF block in the file) << 16 | offset in its inflated bytes */
    int32_t tid;
    uint32_t bin;
} pjb_index_chunk;
typedef struct pjb_index_result {
    int64_t n_records;             /* all alignment records seen, unplaced ones included */
    int64_t n_chunks;
    const pjb_index_chunk *chunks; /* ordered by (tid, bin, file order) */
    const int64_t *lin_off;        /* n_refs + 1: target t's windows are lin[lin_off[t] .. lin_off[t + 1]) */
    const uint64_t *lin;           /* per target its n_intv = (largest window touched) + 1 entries; untouched windows are 0 (a
                                      writer repeats the entry before them) */
} pjb_index_result;
int pjb_index_begin(pjb_ctx *ctx);
int pjb_index_piece(pjb_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, int64_t file_offset, int32_t first_uoffset, int32_t last,
                    uint64_t *next_voffset);
int pjb_index_end(pjb_ctx *ctx, pjb_index_result *out);

/* The same index as a CSI (`portcullis_amd prep --build_csi`): for targets of 2^29 bases or more, which reg2bin cannot bin.
 * min_shift is 14; bins are hts_reg2bin(beg, end, 14, depth) with the beg and end above, chunks as above, and instead of a
 * linear index every bin carries `loffset`: the 16 kb windows are built as above, untouched ones take the entry before them
 * (leading ones the virtual offset of the target's first record), and loffset is the entry at the bin's first window.
 *   pjb_csi_depth        host arithmetic, no context: the depth htslib chooses, the smallest n with
 *                        2^(14 + 3 n) >= (longest target) + 256 -- 5 for human, 6 from 2^29 - 255 bases up;
 *   pjb_index_begin_csi  as pjb_index_begin; depth < 0: pjb_csi_depth of the pjb_set_refs targets.  PJB_ERR_ARG for a depth
 *                        above 6 or, at a depth above 0, a target of 2^(14 + 3 depth) bases or more (the rule that keeps
 *                        targets of 2^29 bases from a BAI; at depth 0 the one bin holds whatever there is);
 *   pjb_index_piece      as above; no target is too long;
 *   pjb_index_end_csi    as pjb_index_end.  pjb_index_end after pjb_index_begin_csi, and pjb_index_end_csi after
 *                        pjb_index_begin, fail with PJB_ERR_STATE. */
typedef struct pjb_csi_result {
    int64_t n_records;
    int64_t n_chunks;
    const pjb_index_chunk *chunks; /* ordered by (tid, bin, file order) */
    const uint64_t *loffset;       /* per chunk: its bin's */
    int32_t min_shift, depth;
} pjb_csi_result;
int pjb_csi_depth(const int32_t *ref_len, int32_t n_ref);
int pjb_index_begin_csi(pjb_ctx *ctx, int32_t depth);
int pjb_index_end_csi(pjb_ctx *ctx, pjb_csi_result *out);

/* ---- several coordinate-sorted files merged into one, target by target (`portcullis_amd prep --merge`) --------------
 * What `samtools merge` does for the reference's prep (src/prepare.cc:154-195 shells out to it), for ONE target at a time and on
 * the device: every file's share of the target is inflated and walked as by pjb_submit_bam, the records of all files are put in
 * one order, gathered into one stream and deflated; only the finished BGZF members come back.
 * The order: pos ascending; records of equal pos by the index of their file, then by their order inside the file.  (samtools
 * also orders equal positions by strand; this does not, so the merge of ONE file is the identity on its record stream, and the
 * merge of a stable split of a file is sorted(concatenation, key = pos) with a stable sort.)
 *   pjb_bam_merge_begin  opens the merge of target `tid` (of pjb_set_refs) from `n_files` files; drops a merge that was open and
 *                        the last result.
 *   pjb_bam_merge_file   hands over file `file`'s share (0 <= file < n_files; each index at most once, in any order; a file
 *                        that is not handed over contributes nothing): comp / comp_bytes / first_uoffset exactly as for
 *                        pjb_submit_bam -- whole BGZF blocks from the block that holds the target's first record through (at
 *                        least) the block that holds its last one, and that first record's offset in the first block's
 *                        inflated bytes.  Records are taken until the first one whose refID is not `tid`, or the end of the
 *                        data.  *n_records (optional): how many.
 *   pjb_bam_merge_end    orders, gathers and deflates: the merged stream (per record its 4-byte block_size and its body) is cut
 *                        every `block_bytes` bytes (as for pjb_deflate_bgzf: a multiple of 4, at most 0xff00), whatever the
 *                        records' boundaries; every piece becomes one BGZF member, the last may be short, no EOF block is added.
 *                        No records: no members.
 * Errors: PJB_ERR_BGZF corrupt BGZF / DEFLATE / record data, a position outside the target (never a silent end of the run),
 * data that ends inside one of the target's records; PJB_ERR_UNSORTED a record whose pos lies below its predecessor's in the
 * same file -- the message names the file and the record's ordinal (0-based) among that file's records on the target;
 * PJB_ERR_ARG bad arguments, or more than 2^32 - 256 records on the target; PJB_ERR_STATE calls out of order, or a file index
 * handed over twice.  A failing call drops the merge: begin again.  The exception is PJB_ERR_NOMEM, which is retryable as
 * elsewhere: the merge stays as it was before the call, the call can be repeated when memory has been freed.
 * Device memory: the target's inflated bytes of all files, the merged stream and the deflate's scratch at once; the first two
 * count as `staging` in pjb_memory_info, the rest as `scratch`.  Works on a PJB_FLAG_NO_CHAINS context (after pjb_set_refs).
 * Threads: like pjb_bam_end, these calls belong to the thread that makes the context's other calls. */
typedef struct pjb_bam_merge_result {
    int64_t n_records;           /* records written for this target */
    int64_t raw_bytes;           /* their inflated bytes (4-byte block_size + body each) */
    int32_t n_members;           /* BGZF members: ceil(raw_bytes / block_bytes) */
    const uint32_t *member_size; /* n_members lengths */
    const uint8_t *members;      /* the members back to back; host memory owned by the context */
    int64_t member_bytes;        /*   until the next pjb_bam_merge_begin / pjb_destroy */
} pjb_bam_merge_result;
int pjb_bam_merge_begin(pjb_ctx *ctx, int32_t tid, int32_t n_files);
int pjb_bam_merge_file(pjb_ctx *ctx, int32_t file, const uint8_t *comp, int64_t comp_bytes, int32_t first_uoffset, int64_t *n_records);
int pjb_bam_merge_end(pjb_ctx *ctx, int32_t block_bytes, pjb_bam_merge_result *out);

/* ---- an unsorted file's records put in coordinate order, run by run (`portcullis_amd prep --sort`) --------------------
 * What `samtools sort` does for the reference's prep (src/prepare.cc: Prepare::bamSort shells out to it), for one RUN at a time
 * and on the device: a run is as much of the file, in file order, as the caller hands over between _begin and _end.  Its pieces
 * are inflated and walked as by pjb_index_piece, every record gets one key, the keys are sorted with the passes the merge uses,
 * the records are gathered into one stream and deflated; only the finished BGZF members come back.  A file that is one run is
 * sorted by that; the runs of a longer file are merged afterwards (pjb_bam_merge_*: each run is a sorted file).
 * The order: (refID as unsigned, pos) ascending, so unplaced records (refID -1) come last; records of equal key keep the order
 * they were handed over in, unplaced records among themselves too.  It is sorted(records, key = (refID & 0xffffffff, pos)) with a
 * stable sort -- the order pjb_bam_merge_* keeps.  (samtools also orders equal positions by strand; this does not.)
 *   pjb_bam_sort_begin  opens a run over the targets of pjb_set_refs; drops a run that was open and the last result.
 *   pjb_bam_sort_piece  a run of whole BGZF blocks, in file order (host memory, as for pjb_index_piece):
 *                         first_uoffset : where the first record not yet taken starts in the piece's inflated bytes (the low 16
 *                                         bits of the last call's *next_voffset; behind the BAM header for a file's first piece);
 *                         last          : non-zero for the piece that ends the file.
 *                       Every record that lies COMPLETELY inside the piece is taken.  *next_voffset receives where the first
 *                       record that was not begins -- or the end of the data --, as (offset of its BGZF block IN THE PIECE) << 16 |
 *                       offset in the block's inflated bytes: the next piece starts with that block.  *n_records (optional): how
 *                       many were taken.  The piece's inflated bytes stay on the device until pjb_bam_sort_end.
 *   pjb_bam_sort_end    orders the run's records, gathers them and deflates the stream, cut every `block_bytes` bytes as by
 *                       pjb_bam_merge_end (a multiple of 4, at most 0xff00; the last member may be short; no EOF block; no
 *                       records: no members).  A run whose records were in order already is not sorted (was_sorted = 1): its
 *                       stream is the input's.
 * Errors: PJB_ERR_BGZF corrupt BGZF / DEFLATE / record data, a refID outside [-1, n_refs), a placed record whose pos lies
 * outside its target (the message names the record's ordinal in the run, 0-based; never a silent drop), data that ends inside
 * a record when last != 0; PJB_ERR_ARG bad arguments, or 2^32 - 256 records or more in a run; PJB_ERR_STATE calls out of order.
 * A failing call drops the run: begin again.  Two exceptions leave the run as it was before the call: a piece whose first
 * record is longer than the piece fails with PJB_ERR_ARG and a message that says so and sets *next_voffset to that record -- the
 * same blocks may be handed over again with more behind them --; and PJB_ERR_NOMEM, retryable as elsewhere: the caller may close
 * the run (pjb_bam_sort_end) and hand the piece to a fresh one.
 * Device memory: the run's inflated bytes, 36 to 44 bytes a record for keys, order, sizes, addresses and offsets, the sorted stream and the deflate's scratch; the
 * inflated bytes and the stream count as `staging` in pjb_memory_info, the rest as `scratch`.  Works on a PJB_FLAG_NO_CHAINS
 * context.  Threads: like pjb_bam_end, these calls belong to the thread that makes the context's other calls. */
typedef struct pjb_bam_sort_result {
    int64_t n_records;           /* records of the run, unplaced ones included */
    int64_t raw_bytes;           /* their inflated bytes (4-byte block_size + body each) */
    int32_t n_members;           /* BGZF members: ceil(raw_bytes / block_bytes) */
    int32_t was_sorted;          /* 1: no record lay before its predecessor; the stream is the input's */
    const uint32_t *member_size; /* n_members lengths */
    const uint8_t *members;      /* the members back to back; host memory owned by the context */
    int64_t member_bytes;        /*   until the next pjb_bam_sort_begin / pjb_destroy */
    int64_t n_unplaced;          /* records with refID -1: the stream's tail */
} pjb_bam_sort_result;
int pjb_bam_sort_begin(pjb_ctx *ctx);
int pjb_bam_sort_piece(pjb_ctx *ctx, const uint8_t *comp, int64_t comp_bytes, int32_t first_uoffset, int32_t last, uint64_t *next_voffset,
                       int64_t *n_records);
int pjb_bam_sort_end(pjb_ctx *ctx, int32_t block_bytes, pjb_bam_sort_result *out);

/* ---- `portcullis filt` feature rows -------------------------------------------------------
 * ModelFeatures::setRow (lib/src/model_features.cc:161-212) for a list of junctions: the columns of VAR_NAMES +
 * JAD_NAMES (lib/include/portcullis/ml/model_features.hpp:45-60), i.e. the row getters, calcIntronScore
 * (lib/src/junction.cc:953-956), Junction::calcCodingPotential / calcSplicingScores /
 * calcJunctionAnchorDepthLogDeviation (lib/src/junction.cc:1328-1391) with the Markov scores of
 * KmerMarkovModel::getScore / PosMarkovModel::getScore (lib/src/markov_model.cc:57-78,101-115) over genome windows.
 * The models arrive as dense tables over the alphabet makeClean leaves (A C G T N -> 0..4): a k-mer model of order
 * 5 is [5^5 contexts][5 next letters] probabilities (0 = never seen), a position model [PJB_PW_LEN positions][5].
 * A NULL table is an untrained model.  *_size: the reference's model.size() (contexts / positions trained; 0 =
 * empty -> the column is 0 as isCodingPotentialModelEmpty / isPWModelEmpty make it).  The genome of every target
 * the junctions lie on must have been uploaded (pjb_upload_contig).  mean_read_length: what
 * Junction::setMeanReadLength stored (the truncated mean, lib/include/portcullis/junction.hpp:928). */
#define PJB_N_FEATURES 34
#define PJB_KMER_ORDER 5
#define PJB_KMER_TABLE (3125 * 5)
#define PJB_PW_LEN 32
typedef struct pjb_markov_models {
    const double *exon, *intron;                               /* coding potential, ModelFeatures::exonModel / intronModel */
    const double *donor_t, *donor_f, *acceptor_t, *acceptor_f; /* splicing signal: true / false models */
    const double *donor_pw, *acceptor_pw;                      /* position weights, order 1 */
    int32_t exon_size, intron_size, donor_pw_size, acceptor_pw_size;
} pjb_markov_models;
int pjb_filt_features(pjb_ctx *ctx, const pjb_junction_row *rows, int64_t n_rows, double mean_read_length, uint32_t l95,
                      const pjb_markov_models *models, double *features_out /* n_rows x PJB_N_FEATURES, host */);

/* ---- the Markov models trained on the device -----------------------------------------------------------------
 * ModelFeatures::trainCodingPotentialModel / trainSplicingModels (lib/src/model_features.cc:77-158) with KmerMarkovModel::train /
 * PosMarkovModel::train (lib/src/markov_model.cc:31-54, 80-98).  rows: host; only refid, start, end and cons_strand are read.  The three
 * lists index the rows: cp_idx trains exon ([start-202, start-2] and [end+1, end+201], each a string of its own) and intron
 * ([start, end]); pass_idx trains donor_t, acceptor_t and the two position models, fail_idx donor_f and acceptor_f, on
 * left = [start-3, start+20] and right = [end-20, end+2] (inclusive, 0-based; on the negative strand every window is read backwards
 * and complemented, `right` is the donor and `left` the acceptor).  Windows are clamped as faidx_fetch_seq clamps them.  A k-mer
 * model counts a window of n bases only if (uint16_t)n > 6 (markov_model.cc:36: the length cut to 16 bits for the gate alone), then
 * every position 5 .. n-1; a position model counts positions 1 .. min(n, PJB_PW_LEN) - 1.  An index listed twice counts twice.  Each
 * context / position whose counts sum to more than 0 is divided by that sum in f64; sizes[] counts those rows (the reference's
 * model.size() after training).  The counts are integers, so the tables are bit for bit the host's and do not depend on scheduling.
 * An empty list gives all-zero tables of size 0 (never NULL).  out: host memory owned by the context until its next pjb_markov_train /
 * pjb_destroy; out->models is what pjb_filt_features / pjb_filt_scores take.
 * PJB_ERR_ARG, found on the host before anything is launched: a negative count, an index outside the rows.  PJB_ERR_STATE: a junction
 * lies on a target whose genome was not uploaded (pjb_upload_contig), as pjb_filt_features reports it. */
typedef struct pjb_markov_tables {
    pjb_markov_models models;
    int32_t sizes[8];     /* exon, intron, donor_t, donor_f, acceptor_t, acceptor_f, donor_pw, acceptor_pw */
    uint64_t transitions; /* what the six k-mer models counted in all: the bases walked, less five a window */
} pjb_markov_tables;
int pjb_markov_train(pjb_ctx *ctx, const pjb_junction_row *rows, int64_t n_rows, const int64_t *cp_idx, int64_t n_cp,
                     const int64_t *pass_idx, int64_t n_pass, const int64_t *fail_idx, int64_t n_fail, pjb_markov_tables *out);

/* ---- `portcullis filt` forest stage: a saved ranger probability forest walked on the device -------------------
 * Tree::predict (deps/ranger-0.3.8/src/Tree.cpp:125-180) and ForestProbability::predictInternal
 * (src/ForestProbability.cpp:111-131): from node 0, value <= split value goes left, anything else (a NaN too) right; at
 * the terminal node counts[c] / n_trees is added for every class, tree after tree in file order.  The predictions are
 * bit-equal to that sequential sum.  A forest is plain arrays: the nodes of all trees one after the other. */
typedef struct pjb_forest {
    int32_t n_trees, n_classes, n_vars; /* n_vars: columns of the data matrix, the dependent one included */
    int32_t dependent_var;              /* its column: present in the matrix, never read */
    const uint8_t *is_ordered;          /* n_vars; NULL = every variable ordered */
    const int64_t *tree_off;            /* n_trees + 1: tree t owns the nodes tree_off[t] .. tree_off[t + 1] */
    const int32_t *left, *right;        /* per node: children as indices inside the tree; both -1 at a terminal node */
    const int32_t *split_var;           /* per node (read at internal nodes only) */
    const double *split_value;
    const int64_t *count_off;           /* per node: where its class counts start in `counts`; -1 = the node has none */
    const double *counts;               /* n_classes values per terminal node */
    int64_t n_counts;                   /* length of `counts` */
} pjb_forest;
/* Host arithmetic only (no context, no device).  PJB_OK: the forest can be walked by a kernel and every walk ends: n_trees >= 1,
 * 1..PJB_FOREST_MAX_CLASSES classes, 1..PJB_FOREST_MAX_VARS variables, every tree has a node, every node 0 or 2 children, both
 * inside the tree and behind their parent (ranger numbers children after parents), no node the child of two, every terminal
 * node n_classes counts inside `counts`, split variables < n_vars, ordered and not the dependent one.  Anything else is
 * PJB_ERR_ARG with the tree and the node in msg (len bytes, may be NULL). */
#define PJB_FOREST_MAX_CLASSES 16
#define PJB_FOREST_MAX_VARS 2048
int pjb_forest_check(const pjb_forest *forest, char *msg, int len);
/* Checks (a forest that fails never reaches the device), packs and uploads: one forest per context, a new one replaces the old,
 * pjb_destroy frees it. */
int pjb_forest_load(pjb_ctx *ctx, const pjb_forest *forest);
/* data: row-major n_rows x n_cols, n_cols == the forest's n_vars; pred: n_rows x n_classes.  PJB_ERR_STATE without a forest. */
int pjb_forest_predict(pjb_ctx *ctx, const double *data, int64_t n_rows, int32_t n_cols, double *pred);
/* The fused path of `filt`: the feature rows of pjb_filt_features stay on the device and are walked there.  var_feature[v] is
 * the column of the PJB_N_FEATURES row that is the forest's variable v (the dependent variable's entry is not read).
 * features_out (optional): n_rows x PJB_N_FEATURES, the rows pjb_filt_features would have returned. */
int pjb_filt_scores(pjb_ctx *ctx, const pjb_junction_row *rows, int64_t n_rows, double mean_read_length, uint32_t l95,
                    const pjb_markov_models *models, const int32_t *var_feature, double *pred, double *features_out);

/* ---- `train`: a ranger probability forest grown on the device ------------------------------------------------
 * Forest::grow with the trees of ForestProbability as ModelFeatures::trainInstance sets them up (lib/src/model_features.cc:422-440:
 * no replacement, sample fraction 1, no case weights, every variable ordered): Forest.cpp:409-416 (the trees' seeds),
 * Tree::grow / splitNode / createPossibleSplitVarSubset (deps/ranger-0.3.8/src/Tree.cpp:88-123, 232-300),
 * drawWithoutReplacementSimple (src/utility.cpp:108-131) and TreeProbability::splitNodeInternal / findBestSplit /
 * findBestSplitValueSmallQ / LargeQ / addToTerminalNodes (src/TreeProbability.cpp:57-73, 91-312).  The result, written with
 * Forest::saveToFile's layout, is byte for byte the file ranger 0.3.8 (built against libstdc++ 11) saves for the same matrix.
 * data: row-major n_rows x n_cols, host; column dependent_col holds the labels 0 / 1.
 * PJB_ERR_ARG, found on the host before anything is launched: a value that is not finite; a label other than 0 or 1;
 * n_trees < 1, n_rows < 1, n_cols < 2; mtry >= n_cols / 2 (ranger then draws by Knuth's algorithm, utility.cpp:101-105, which is
 * not built; with mtry 0 this refuses n_cols < 4); more than PJB_FOREST_MAX_VARS columns.  Works on any context
 * (PJB_FLAG_NO_CHAINS too); the forest pjb_forest_load put on the device is left alone. */
typedef struct pjb_grow_params {
    int32_t n_trees;
    uint32_t seed;         /* trainInstance: 1236456789 */
    int32_t mtry;          /* 0 = floor(sqrt(n_cols - 1)) */
    int32_t min_node_size; /* 0 = 10 */
    int32_t dependent_col;
} pjb_grow_params;
typedef struct pjb_grow_result {
    pjb_forest forest;          /* host memory, owned by the context until the next pjb_forest_grow / pjb_destroy */
    const double *class_values; /* n_classes, ascending */
} pjb_grow_result;
int pjb_forest_grow(pjb_ctx *ctx, const double *data, int64_t n_rows, int32_t n_cols, const pjb_grow_params *p, pjb_grow_result *out);

/* ---- `train --folds`: k-fold cross-validation, the folds' forests grown side by side ----------------------------
 * data, p: as pjb_forest_grow.  fold[r] in 0 .. n_folds-1: the fold that holds row r out.
 * forests (optional, n_folds entries): forests[f] is, bit for bit, the forest pjb_forest_grow returns for the sub-matrix of the rows
 * with fold[r] != f, in their original order, with the same params (every fold's tree i has the seed (i + 1) * seed).  Host memory
 * owned by the context until its next pjb_forest_cv / pjb_destroy.
 * pred: n_rows x 2, host: row r as pjb_forest_load(forests[fold[r]]) + pjb_forest_predict give it -- the quotients counts[c] / n_trees
 * made once each and added tree after tree in tree order -- without a forest leaving the device for it: the held-out rows are walked
 * through the grown nodes there.
 * One call grows n_folds * n_trees trees through one level loop (one read-back per level for every fold's trees together), in
 * batches that may cut through folds; nothing depends on where they cut ("grow_batch").  The forest pjb_forest_load put on the device
 * is left alone.  The call may invalidate the result of the context's last pjb_forest_grow: copy it first.
 * PJB_ERR_ARG, found on the host before anything is launched, the fold named in the message: n_folds < 2 or > n_rows; a fold id
 * outside 0 .. n_folds-1; a fold that holds no row; a fold whose training rows all have one label (so every forest has two
 * classes); and everything pjb_forest_grow refuses. */
int pjb_forest_cv(pjb_ctx *ctx, const double *data, int64_t n_rows, int32_t n_cols, const pjb_grow_params *p, const int32_t *fold,
                  int32_t n_folds, double *pred, pjb_grow_result *forests);

/* ---- self-training: brute-force K nearest neighbours, the search under SMOTE and ENN ---------------------------
 * KNN::doSlice (lib/src/knn.cc:46-99).  data: row-major n_rows x n_cols, host.  The distance of two rows is
 * s = sum over the columns, in ascending column order, of (base[c] - test[c])^2 in f64, the subtraction, the product and the sum
 * each rounded on their own.  A row's own index takes part (distance 0).  nn_out (n_rows x k, host) gets, per row, the indices of
 * the k rows that are smallest under the total order (s, index), in that order: the reference walks the base rows in ascending
 * order and puts a candidate behind the entries of equal distance.  k is what the caller passes; KNN's constructor rule
 * (k = rows if rows < defaultK && rows < 100) is the caller's.  The result does not depend on how the base range is cut into
 * chunks (pjb_set_option("knn_chunk", n) forces the chunk length; 0 is the default sizing).
 * PJB_ERR_ARG, found on the host before anything is launched: k < 1, k > PJB_KNN_MAX_K or k > n_rows; n_cols < 1 or
 * > PJB_KNN_MAX_COLS; n_rows < 1 or > 2^22; a value that is not finite or larger than 1e153 in magnitude (a distance could
 * overflow; the reference puts a NaN distance at the front of its list, which is not reproduced).
 * Works on any context (PJB_FLAG_NO_CHAINS too). */
#define PJB_KNN_MAX_K 8
#define PJB_KNN_MAX_COLS 32
int pjb_knn(pjb_ctx *ctx, const double *data, int64_t n_rows, int32_t n_cols, int32_t k, uint32_t *nn_out);

/* ---- `portcullis bamfilt` ----------------------------------------------------------------
 * The per-alignment decision of BamFilter::filter (src/bam_filter.cc:152-247): walk the CIGAR as
 * BamFilter::containsJunctionInSystem / clipMSR do (src/bam_filter.cc:75-150) and probe the set of junctions that
 * passed the filter.  The set of one target is uploaded as sorted keys; pjb_filter_batch then writes one code per
 * alignment of a batch of that target:
 *   0 dropped, 1 kept (not spliced), 2 kept (spliced, one of its introns is in the set),
 *   3 kept (multiply spliced read in HARD / SOFT clip mode with a good junction: the reference's "Modified" count).
 * Only pos, cig_off and cigar of the batch are read.  Kept records leave the reference unchanged in every clip
 * mode (its clipping edits a cached copy of the CIGAR that BamWriter never writes), so a code is all a writer needs.
 * Works on any context (no genome, no PJB_FLAG_*). */
enum { PJB_CLIP_HARD = 0, PJB_CLIP_SOFT = 1, PJB_CLIP_COMPLETE = 2 }; /* ClipMode, src/bam_filter.hpp:50-54 */
/* keys: (uint64)(uint32)start << 32 | (uint32)end of the target's passing junctions, ascending, host memory */
int pjb_filter_set_junctions(pjb_ctx *ctx, int32_t tid, const uint64_t *sorted_keys, int64_t n_keys);
int pjb_filter_batch(pjb_ctx *ctx, int32_t tid, const pjb_batch *host_batch, int32_t clip_mode, uint8_t *codes_out);

#ifdef __cplusplus
}
#endif
#endif
