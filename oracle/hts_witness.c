/* hts_witness: the reference's own htslib-1.3, asked directly (TEST INFRASTRUCTURE ONLY).
 *
 * The oracle, tests/util_bam.py and tests/index_model.py restate what htslib does: the pileup and its 8000-node cap,
 * the record decode (bam_endpos, bam_aux2A), the BAI, the FASTA index and faidx_fetch_seq's clamp.  This program is
 * linked against the htslib-1.3 the reference ships (oracle/Makefile builds it into oracle/_ref/) and prints what
 * that library answers, as text, so that tests can hold the restatements to it.  It is code of this project and calls
 * nothing but htslib's public API (htslib/sam.h, hts.h, bgzf.h, faidx.h).
 *
 *   hts_witness depth BAM        tid pos depth                per position the pileup reports
 *   hts_witness records BAM      one line per record, see cmd_records
 *   hts_witness index BAM OUT    sam_index_build2 (BAI)
 *   hts_witness query BAM IDX    regions "tid beg end" on stdin -> "# tid beg end", then "pos end qname" per record
 *   hts_witness faidx FA         fai_build (writes FA.fai); exit status 1 where it refuses
 *   hts_witness fetch FA         "name beg end" on stdin -> "len string" per line
 *   hts_witness eof FILE         bgzf_check_EOF
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <htslib/bgzf.h>
#include <htslib/faidx.h>
#include <htslib/hts.h>
#include <htslib/sam.h>

/* CIGAR operation k of a record.  (Not through bam_get_cigar: behind a name of any length the operations are not aligned.) */
static uint32_t cigar_op(const bam1_t *b, int k) {
    uint32_t v;
    memcpy(&v, b->data + b->core.l_qname + 4 * (size_t)k, 4);
    return v;
}

static int die(const char *what, const char *arg) {
    fprintf(stderr, "hts_witness: %s: %s\n", what, arg);
    return 2;
}

/* ---- depth: the one thin restatement left, DepthParser of the reference's lib/src/depth_parser.cc ---------------- */
typedef struct {
    BGZF *fp;
} aux_t; /* depth_parser.hpp's aux_t without iter, min_mapQ and min_len: the constructor leaves them 0 (:90-91) */

/* depth_parser.cc:60-82, read_bam_skip_gapped.  :66 reads a record (aux->iter is never set: bam_read1); :67-74 look
 * for a BAM_CREF_SKIP operation and :80 reads on while one was found.  :75-78 are the mapq and length filters, which
 * min_mapQ = 0 and min_len = 0 switch off.  One difference, on purpose: the reference's loop does not look at `ret`,
 * so at the end of a file whose last record holds an N it would test that record for ever (unspliced.bam never holds
 * one); here the end of the file ends the loop. */
static int read_bam_skip_gapped(void *data, bam1_t *b) {
    aux_t *aux = (aux_t *)data;
    int ret, skip;
    do {
        skip = 0;
        ret = bam_read1(aux->fp, b); /* :66 */
        if (ret < 0) break;
        for (int k = 0; k < b->core.n_cigar; ++k) {      /* :67-68 */
            int cop = cigar_op(b, k) & BAM_CIGAR_MASK;   /* :69 */
            if (cop == BAM_CREF_SKIP) {                  /* :70 */
                skip = 1;                                /* :71 */
                break;                                   /* :72 */
            }
        }
    } while (skip); /* :80 */
    return ret;     /* :81 */
}

static int cmd_depth(const char *fn) {
    aux_t aux, *data[1] = {&aux};
    aux.fp = bgzf_open(fn, "r"); /* :89 */
    if (!aux.fp) return die("cannot open", fn);
    bam_hdr_t *header = bam_hdr_read(aux.fp); /* :92 */
    if (!header) return die("no BAM header", fn);
    bam_mplp_t mplp = bam_mplp_init(1, read_bam_skip_gapped, (void **)data); /* :95, allowGappedAlignments false */
    int tid = -1, pos = 0, n_plp = 0, res;
    const bam_pileup1_t *plp[1]; /* :121 */
    /* :124 and :143, the two call sites of bam_mplp_auto, and :125-129 / :144-148, the count that follows each.
     * loadNextBatch stores n_plp - m at depths[pos + 1] of target tid (:131-132, :149-153); this prints pos itself. */
    while ((res = bam_mplp_auto(mplp, &tid, &pos, &n_plp, plp)) > 0) {
        int m = 0;
        for (int j = 0; j < n_plp; ++j) {
            const bam_pileup1_t *p = plp[0] + j;
            if (p->is_del || p->is_refskip) ++m;
        }
        printf("%d %d %d\n", tid, pos, n_plp - m);
    }
    bam_mplp_destroy(mplp);  /* :101 */
    bam_hdr_destroy(header); /* :102 */
    bgzf_close(aux.fp);      /* :103 */
    return res < 0 ? die("pileup failed", fn) : 0;
}

/* ---- records ----------------------------------------------------------------------------------------------------- */
/* tid pos bam_endpos flag mapq l_qseq mtid mpos CIGAR SEQ QNAME XS, tab separated.  CIGAR and SEQ are "*" when empty.
 * XS is "-" when bam_aux_get finds no XS tag, else "<type letter>:<bam_aux2A's value as a number>". */
static int cmd_records(const char *fn) {
    htsFile *fp = hts_open(fn, "r");
    if (!fp) return die("cannot open", fn);
    bam_hdr_t *h = sam_hdr_read(fp);
    if (!h) return die("no header", fn);
    printf("@ %d\n", h->n_targets);
    for (int t = 0; t < h->n_targets; t++) printf("@ %s %u\n", h->target_name[t], h->target_len[t]);
    bam1_t *b = bam_init1();
    int r;
    while ((r = sam_read1(fp, h, b)) >= 0) {
        const bam1_core_t *c = &b->core;
        printf("%d\t%d\t%d\t%u\t%u\t%d\t%d\t%d\t", c->tid, c->pos, bam_endpos(b), c->flag, c->qual, c->l_qseq, c->mtid, c->mpos);
        if (c->n_cigar == 0) putchar('*');
        for (int k = 0; k < c->n_cigar; k++) printf("%u%c", bam_cigar_oplen(cigar_op(b, k)), bam_cigar_opchr(cigar_op(b, k)));
        putchar('\t');
        const uint8_t *s = bam_get_seq(b);
        if (c->l_qseq == 0) putchar('*');
        for (int k = 0; k < c->l_qseq; k++) putchar(seq_nt16_str[bam_seqi(s, k)]);
        printf("\t%s\t", bam_get_qname(b));
        const uint8_t *xs = bam_aux_get(b, "XS");
        if (!xs) printf("-\n");
        else printf("%c:%d\n", (char)xs[0], (int)(unsigned char)bam_aux2A(xs));
    }
    bam_destroy1(b);
    bam_hdr_destroy(h);
    hts_close(fp);
    return r < -1 ? die("truncated or corrupt", fn) : 0;
}

/* ---- index / query ----------------------------------------------------------------------------------------------- */
static int cmd_index(const char *fn, const char *out) {
    int r = sam_index_build2(fn, out, 0); /* min_shift 0: BAI */
    if (r < 0) return die("sam_index_build2 failed", fn);
    return 0;
}

static int cmd_query(const char *fn, const char *fnidx) {
    htsFile *fp = hts_open(fn, "r");
    if (!fp) return die("cannot open", fn);
    bam_hdr_t *h = sam_hdr_read(fp);
    if (!h) return die("no header", fn);
    hts_idx_t *idx = sam_index_load2(fp, fn, fnidx);
    if (!idx) return die("cannot load index", fnidx);
    bam1_t *b = bam_init1();
    int tid, beg, end;
    while (scanf("%d %d %d", &tid, &beg, &end) == 3) {
        printf("# %d %d %d\n", tid, beg, end);
        hts_itr_t *it = sam_itr_queryi(idx, tid, beg, end);
        if (!it) {
            printf("! no iterator\n");
            continue;
        }
        int r;
        while ((r = sam_itr_next(fp, it, b)) >= 0) printf("%d %d %s\n", b->core.pos, bam_endpos(b), bam_get_qname(b));
        hts_itr_destroy(it);
        if (r < -1) return die("read error in a query", fn);
    }
    bam_destroy1(b);
    hts_idx_destroy(idx);
    bam_hdr_destroy(h);
    hts_close(fp);
    return 0;
}

/* ---- FASTA --------------------------------------------------------------------------------------------------------- */
static int cmd_faidx(const char *fn) { return fai_build(fn) < 0 ? 1 : 0; }

static int cmd_fetch(const char *fn) {
    faidx_t *fai = fai_load(fn);
    if (!fai) return die("cannot load", fn);
    char name[1024];
    int beg, end;
    while (scanf("%1023s %d %d", name, &beg, &end) == 3) {
        int len = 0;
        char *s = faidx_fetch_seq(fai, name, beg, end, &len);
        printf("%d %s\n", len, s ? s : "(null)");
        free(s);
    }
    fai_destroy(fai);
    return 0;
}

static int cmd_eof(const char *fn) {
    BGZF *fp = bgzf_open(fn, "r");
    if (!fp) return die("cannot open", fn);
    printf("%d\n", bgzf_check_EOF(fp));
    bgzf_close(fp);
    return 0;
}

int main(int argc, char **argv) {
    const char *c = argc > 1 ? argv[1] : "";
    if (!strcmp(c, "depth") && argc == 3) return cmd_depth(argv[2]);
    if (!strcmp(c, "records") && argc == 3) return cmd_records(argv[2]);
    if (!strcmp(c, "index") && argc == 4) return cmd_index(argv[2], argv[3]);
    if (!strcmp(c, "query") && argc == 4) return cmd_query(argv[2], argv[3]);
    if (!strcmp(c, "faidx") && argc == 3) return cmd_faidx(argv[2]);
    if (!strcmp(c, "fetch") && argc == 3) return cmd_fetch(argv[2]);
    if (!strcmp(c, "eof") && argc == 3) return cmd_eof(argv[2]);
    fprintf(stderr, "usage: hts_witness depth|records|faidx|fetch|eof FILE | index BAM OUT | query BAM IDX\n");
    return 2;
}
