/* ss.c -- `sigtk-amd ss paf2tsv [--host-decode] [--batch INT] in.paf`: the ss:Z: strings of a resquiggle PAF as one TSV
 * row per k-mer, byte for byte the rows of the reference's `sigtk ss paf2tsv` (src/ss.c) wherever the reference is
 * defined (DESIGN 3.11 lists where it is not, and what happens here instead).
 *
 * The strings are parsed and the rows written on the GPU (sgk_ss_*, csrc/ss_kernels.hip).  Records go to the device in
 * batches of --batch rows; a record with more rows than that is cut into spans over several batches.  Two batches are
 * in flight (sgk_ss_pipe_*): while one batch's text is written to stdout the next one is on the device.
 * --host-decode does the same work with ss_decode_host and the host build of text_format.h, and needs no GPU.
 *
 * The first bad record ends the run: the rows of every record in front of it are written, then one line on stderr,
 * exit status 1. */
#include <errno.h>
#include <getopt.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../csrc/text_format.h"
#include "cli.h"
#include "sigtk_gpu.h"
#include "ss.h"

/* ------------------------------------------------------------------ PAF */

static int is_sep(char c) { return c == '\t' || c == '\r' || c == '\n'; }

/* atoi where atoi is defined: 0 if the value does not fit an int */
static int paf_int(const char *s, int32_t *out) {
    errno = 0;
    const long v = strtol(s, NULL, 10);
    if (errno == ERANGE || v > INT32_MAX || v < INT32_MIN) return 0;
    *out = (int32_t)v;
    return 1;
}

int paf_parse_line(char *line, size_t len, paf_rec_t *out, int *col) {
    const size_t n = strnlen(line, len);
    char *f[12];
    int nf = 0;
    size_t pos = 0;
    memset(out, 0, sizeof *out);
    *col = 0;
    while (pos < n) {
        while (pos < n && is_sep(line[pos])) pos++;
        if (pos >= n) break;
        const size_t s0 = pos;
        while (pos < n && !is_sep(line[pos])) pos++;
        const size_t flen = pos - s0;
        if (pos < n) line[pos++] = 0; /* (line[n] is the NUL getline wrote, or the one that ended the line early) */
        if (nf < 12) {
            f[nf] = line + s0;
            if (nf == 0) out->rid_len = flen;
        } else if (flen >= 5 && memcmp(line + s0, "ss:Z:", 5) == 0) { /* the last one wins */
            out->ss = line + s0 + 5;
            out->ss_len = flen - 5;
        }
        nf++;
    }
    if (nf < 12) return PAF_FEW_FIELDS;
    out->rid = f[0];
    if (strcmp(f[4], "+") != 0 && strcmp(f[4], "-") != 0) return PAF_STRAND;
    const int cols[5] = {3, 4, 7, 8, 9};
    int32_t *dst[5] = {&out->start_raw, &out->end_raw, &out->tlen, &out->start_kmer, &out->end_kmer};
    for (int i = 0; i < 5; i++) {
        if (!paf_int(f[cols[i] - 1], dst[i])) {
            *col = cols[i];
            return PAF_NUMBER;
        }
    }
    for (int i = 0; i < 5; i++) {
        if (*dst[i] < 0 && (cols[i] == 3 || cols[i] == 8 || cols[i] == 9)) {
            *col = cols[i];
            return PAF_NEGATIVE;
        }
    }
    if (!out->ss) return PAF_NO_TAG;
    return PAF_OK;
}

/* ------------------------------------------------------------------ the grammar, one byte at a time */

#define SS_SAT 0x80000000ll /* INT32_MAX + 1: sums are clamped here, as on the device */

uint32_t ss_decode_host(const char *ss, size_t len, const sgk_ss_record_t *rec, uint32_t first, uint32_t count,
                        int32_t *pairs, int32_t ends[2]) {
    int64_t i_raw = rec->start_raw, i_k = rec->st_k;
    const int64_t base_k = (int64_t)rec->st_k + first;
    uint32_t val = 0, ndig = 0, over = 0, rng = 0;
    ends[0] = ends[1] = -1;
    for (size_t p = 0; p < len; p++) {
        const unsigned char c = (unsigned char)ss[p];
        if (c >= '0' && c <= '9') {
            const uint32_t d = c - '0';
            if (val > 214748364u || (val == 214748364u && d > 7u)) over = 1;
            val = val * 10u + d;
            if (ndig < 100u) ndig++;
        } else if (c == ',' || c == 'I' || c == 'D') {
            if (ndig == 0) return 1;
            if (ndig > 10u || over) rng = 1;
            const int64_t n = val;
            if (c == 'I') {
                i_raw += n;
            } else if (c == 'D') {
                i_k += n;
            } else {
                const int64_t j = i_k - base_k;
                if (j >= 0 && j < (int64_t)count) {
                    pairs[2 * j] = (int32_t)i_raw;
                    pairs[2 * j + 1] = (int32_t)(i_raw + n);
                }
                i_raw += n;
                i_k += 1;
            }
            if (i_raw > SS_SAT) i_raw = SS_SAT;
            if (i_k > SS_SAT) i_k = SS_SAT;
            val = 0;
            ndig = 0;
            over = 0;
        } else {
            return 2;
        }
    }
    if (rng || i_raw > INT32_MAX || i_k > INT32_MAX) return 5;
    ends[0] = (int32_t)i_raw;
    ends[1] = (int32_t)i_k;
    if (i_raw != rec->end_raw) return 3;
    if (i_k != rec->end_k) return 4;
    return 0;
}

static const char *ss_status_message(uint32_t st) {
    switch (st) {
        case 1: return "Bad ss: Preceding digit missing";
        case 2: return "Bad ss: A non-digit found when expected a digit";
        case 3: return "Bad ss: Signal end mismatch";
        case 4: return "Bad ss: Kmer end mismatch";
        case 5: return "Bad ss: Number out of range";
        default: return "Bad ss: unknown status";
    }
}

/* ------------------------------------------------------------------ ss paf2tsv */

static void *xrealloc(void *p, size_t n) {
    void *q = realloc(p, n ? n : 1);
    if (!q) {
        ERROR("ssmain", "%s", "out of memory");
        die_flushed();
    }
    return q;
}
static void out_write(const void *p, size_t n) {
    if (n && fwrite(p, 1, n, stdout) != n) {
        ERROR("ssmain", "%s", "writing to stdout failed");
        die_flushed();
    }
}

/* the records of the file in order; the line of the current record stays until all its rows are handed out */
typedef struct {
    FILE *fp;
    const char *path;
    char *line;
    size_t cap;
    long line_no;
    paf_rec_t cur;
    sgk_ss_record_t rec; /* ss_offset / id filled per batch */
    uint32_t rows, done;
    int have, fresh; /* fresh: no span of the current record was handed out yet */
    char err[512];   /* why reading stopped, "" at the end of the file */
    int stopped;
} reader_t;

/* 1 with r->cur / r->rec set, 0 at the end of the file or at a line that breaks a rule (r->err) */
static int reader_next(reader_t *r) {
    if (r->stopped) return 0;
    const ssize_t got = getline(&r->line, &r->cap, r->fp);
    if (got < 0) {
        r->stopped = 1;
        return 0;
    }
    r->line_no++;
    int col = 0;
    const int rc = paf_parse_line(r->line, (size_t)got, &r->cur, &col);
    if (rc != PAF_OK) {
        r->stopped = 1;
        if (rc == PAF_FEW_FIELDS) snprintf(r->err, sizeof r->err, "%s line %ld: fewer than 12 fields", r->path, r->line_no);
        else if (rc == PAF_STRAND) snprintf(r->err, sizeof r->err, "%s line %ld: the strand column is neither + nor -", r->path, r->line_no);
        else if (rc == PAF_NUMBER) snprintf(r->err, sizeof r->err, "%s line %ld: column %d does not fit an int", r->path, r->line_no, col);
        else if (rc == PAF_NEGATIVE) snprintf(r->err, sizeof r->err, "%s line %ld: column %d is negative", r->path, r->line_no, col);
        else snprintf(r->err, sizeof r->err, "ss:Z: tag not found in paf record for %.300s", r->cur.rid);
        return 0;
    }
    if (r->cur.ss_len > 0xffffff00ull || r->cur.rid_len > 0xffffffull) {
        r->stopped = 1;
        snprintf(r->err, sizeof r->err, "%s line %ld: the ss string or the read id is too long", r->path, r->line_no);
        return 0;
    }
    const paf_rec_t *p = &r->cur;
    memset(&r->rec, 0, sizeof r->rec);
    r->rec.ss_len = (uint32_t)p->ss_len;
    r->rec.start_raw = p->start_raw;
    r->rec.end_raw = p->end_raw;
    r->rec.rna = p->start_kmer > p->end_kmer;
    r->rec.st_k = r->rec.rna ? p->end_kmer : p->start_kmer;
    r->rec.end_k = r->rec.rna ? p->start_kmer : p->end_kmer;
    r->rec.tlen = p->tlen;
    r->rows = (uint32_t)((int64_t)r->rec.end_k - (int64_t)r->rec.st_k);
    r->done = 0;
    r->have = 1;
    r->fresh = 1;
    return 1;
}

typedef struct {
    uint8_t *ss, *ids;
    size_t ss_n, ss_cap, ids_n, ids_cap;
    sgk_ss_record_t *rec;
    sgk_ss_span_t *span;
    uint32_t *id_off;
    uint32_t n, cap;
} batch_t;

/* the next batch: one span per record, at most `budget` rows in all (a larger record continues in the next batch) */
static uint32_t next_batch(reader_t *r, uint64_t budget, batch_t *b) {
    b->n = 0;
    b->ss_n = b->ids_n = 0;
    uint64_t used = 0;
    while (used < budget && b->n < (1u << 20) && b->ss_n < (1ull << 30)) {
        if (!r->have && !reader_next(r)) break;
        if (b->n == b->cap) {
            b->cap = b->cap ? b->cap * 2 : 1024;
            b->rec = (sgk_ss_record_t *)xrealloc(b->rec, (size_t)b->cap * sizeof *b->rec);
            b->span = (sgk_ss_span_t *)xrealloc(b->span, (size_t)b->cap * sizeof *b->span);
            b->id_off = (uint32_t *)xrealloc(b->id_off, ((size_t)b->cap + 1) * sizeof *b->id_off);
        }
        if (b->ss_n + r->cur.ss_len > b->ss_cap) {
            b->ss_cap = (b->ss_n + r->cur.ss_len) * 2 + 4096;
            b->ss = (uint8_t *)xrealloc(b->ss, b->ss_cap);
        }
        if (b->ids_n + r->cur.rid_len > b->ids_cap) {
            b->ids_cap = (b->ids_n + r->cur.rid_len) * 2 + 4096;
            b->ids = (uint8_t *)xrealloc(b->ids, b->ids_cap);
        }
        const uint64_t left = (uint64_t)r->rows - r->done;
        const uint64_t take = left < budget - used ? left : budget - used;
        sgk_ss_record_t *rec = &b->rec[b->n];
        *rec = r->rec;
        rec->ss_offset = b->ss_n;
        rec->id = b->n;
        memcpy(b->ss + b->ss_n, r->cur.ss, r->cur.ss_len);
        b->ss_n += r->cur.ss_len;
        b->id_off[b->n] = (uint32_t)b->ids_n;
        memcpy(b->ids + b->ids_n, r->cur.rid, r->cur.rid_len);
        b->ids_n += r->cur.rid_len;
        sgk_ss_span_t *sp = &b->span[b->n];
        memset(sp, 0, sizeof *sp);
        sp->record = b->n;
        sp->first = r->done;
        sp->count = (uint32_t)take;
        b->n++;
        used += take;
        r->done += (uint32_t)take;
        r->fresh = 0;
        if (r->done == r->rows) r->have = 0;
    }
    if (b->n) b->id_off[b->n] = (uint32_t)b->ids_n;
    return b->n;
}

static void emit(sgk_ss_pipe_t *pipe, int slot) {
    const uint8_t *text;
    uint64_t nb;
    uint32_t bad, st;
    const int rc = sgk_ss_pipe_wait(pipe, slot, &text, &nb, &bad, &st);
    if (rc != SGK_OK) gpu_fail("ssmain", "sgk_ss_pipe_wait", rc);
    out_write(text, (size_t)nb);
    if (bad != 0xffffffffu) {
        fprintf(stderr, "%s\n", ss_status_message(st));
        die_flushed();
    }
}

static void run_gpu(reader_t *r, uint64_t budget) {
    sgk_ss_pipe_t *pipe = NULL;
    int rc = sgk_ss_pipe_create(0, &pipe);
    if (rc != SGK_OK) gpu_fail("ssmain", "sgk_ss_pipe_create", rc);
    batch_t b;
    memset(&b, 0, sizeof b);
    int slot = 0, pending = -1;
    while (next_batch(r, budget, &b)) {
        sgk_ss_stage_t st;
        rc = sgk_ss_pipe_begin(pipe, slot, b.ss_n, b.n, b.n, b.n, b.ids_n, &st);
        if (rc != SGK_OK) gpu_fail("ssmain", "sgk_ss_pipe_begin", rc);
        memcpy(st.ss, b.ss, b.ss_n);
        memcpy(st.records, b.rec, (size_t)b.n * sizeof *b.rec);
        memcpy(st.spans, b.span, (size_t)b.n * sizeof *b.span);
        memcpy(st.id_bytes, b.ids, b.ids_n);
        memcpy(st.id_offsets, b.id_off, ((size_t)b.n + 1) * sizeof *b.id_off);
        rc = sgk_ss_pipe_submit(pipe, slot);
        if (rc != SGK_OK) gpu_fail("ssmain", "sgk_ss_pipe_submit", rc);
        if (pending >= 0) emit(pipe, pending);
        pending = slot;
        slot ^= 1;
    }
    if (pending >= 0) emit(pipe, pending);
    sgk_ss_pipe_destroy(pipe);
    free(b.ss);
    free(b.ids);
    free(b.rec);
    free(b.span);
    free(b.id_off);
}

static void run_host(reader_t *r, uint64_t budget) {
    if (budget > (1u << 24)) budget = 1u << 24;
    int32_t *pairs = (int32_t *)xrealloc(NULL, (size_t)budget * 8);
    char *out = NULL;
    size_t out_cap = 0;
    while (reader_next(r)) {
        int32_t ends[2];
        uint32_t st = ss_decode_host(r->cur.ss, r->cur.ss_len, &r->rec, 0, 0, pairs, ends);
        if (st != 0) {
            fprintf(stderr, "%s\n", ss_status_message(st));
            free(pairs);
            free(out);
            free(r->line);
            fclose(r->fp);
            die_flushed();
        }
        const size_t row_max = r->cur.rid_len + 40;
        for (uint64_t first = 0; first < r->rows; first += budget) {
            const uint32_t count = (uint32_t)(r->rows - first < budget ? r->rows - first : budget);
            memset(pairs, 0xff, (size_t)count * 8);
            ss_decode_host(r->cur.ss, r->cur.ss_len, &r->rec, (uint32_t)first, count, pairs, ends);
            if ((size_t)count * row_max > out_cap) {
                out_cap = (size_t)count * row_max;
                out = (char *)xrealloc(out, out_cap);
            }
            char *p = out;
            for (uint32_t j = 0; j < count; j++) {
                const int64_t i = (int64_t)r->rec.st_k + (int64_t)first + j;
                memcpy(p, r->cur.rid, r->cur.rid_len);
                p += r->cur.rid_len;
                *p++ = '\t';
                p += sgk_tf_i64(p, r->rec.rna ? (int64_t)r->rec.tlen - i - 1 : i);
                *p++ = '\t';
                if (pairs[2 * j] == -1) {
                    *p++ = '.';
                    *p++ = '\t';
                    *p++ = '.';
                } else {
                    p += sgk_tf_i64(p, pairs[2 * j]);
                    *p++ = '\t';
                    p += sgk_tf_i64(p, pairs[2 * j + 1]);
                }
                *p++ = '\n';
            }
            out_write(out, (size_t)(p - out));
        }
    }
    free(pairs);
    free(out);
}

static void ss_usage(FILE *fp, uint64_t budget) {
    fprintf(fp, "Usage: sigtk ss paf2tsv in.paf\n");
    fprintf(fp, "   --host-decode              parse and format on the host (needs no GPU)\n");
    fprintf(fp, "   --batch INT                rows per GPU batch [%llu]\n", (unsigned long long)budget);
}

int ssmain(int argc, char *argv[]) {
    static const struct option long_options[] = {{"verbose", required_argument, 0, 'v'}, {"help", no_argument, 0, 'h'},
                                                 {"version", no_argument, 0, 'V'},       {"host-decode", no_argument, 0, OPT_HOST_DECODE},
                                                 {"batch", required_argument, 0, OPT_BATCH}, {0, 0, 0, 0}};
    int c;
    FILE *fp_help = stderr;
    int host = 0;
    uint64_t budget = 1ull << 20; /* rows per batch: 8 bytes of table and about 45 bytes of text each */
    const uint64_t budget_default = budget;
    while ((c = getopt_long(argc, argv, "hVv:", long_options, NULL)) >= 0) {
        if (c == 'V') {
            version_exit();
        } else if (c == 'h') {
            fp_help = stdout;
        } else if (c == OPT_HOST_DECODE) {
            host = 1;
        } else if (c == OPT_BATCH) {
            budget = strtoull(optarg, NULL, 10);
            if (budget < 1) budget = 1;
            if (budget > (1ull << 26)) budget = 1ull << 26;
        }
    }
    if (argc - optind != 2 || fp_help == stdout) {
        ss_usage(fp_help, budget_default);
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    if (strcmp(argv[optind], "paf2tsv") != 0) return 0; /* as the reference: nothing */
    reader_t r;
    memset(&r, 0, sizeof r);
    r.path = argv[optind + 1];
    r.fp = fopen(r.path, "r");
    if (!r.fp) {
        ERROR("ssmain", "cannot open %s", r.path);
        die_flushed();
    }
    if (!host && sgk_device_count() <= 0) {
        ERROR("ssmain", "%s", "no usable GPU: sigtk-amd has no CPU compute path (ss paf2tsv --host-decode runs on the host)");
        die_flushed();
    }
    printf("read_id\tkmer_idx\tstart_raw_idx\tend_raw_idx\n");
    if (host) run_host(&r, budget);
    else run_gpu(&r, budget);
    const int failed = r.err[0] != 0;
    if (failed) ERROR("ssmain", "%s", r.err);
    free(r.line);
    fclose(r.fp);
    if (failed) die_flushed();
    return 0;
}
