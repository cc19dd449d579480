/* sref.c -- `sigtk-amd sref [--rna] [-n] --kmer-model FILE ref.fa[.gz]`: the synthetic reference signal of every
 * sequence of a FASTA file, byte for byte the rows of the reference's `sigtk sref` (src/sref.c:100-280), with the
 * k-mer lookup and the number formatting on the GPU (sgk_sref_*, csrc/sref_kernels.hip).
 *
 * What differs by design: the pore model is an input (--kmer-model; this build carries no built-in model), and the
 * rows are not made one value at a time.  The rows are cut into spans of a fixed budget of signal positions per batch;
 * a batch's base windows go up, its text comes back and is written in order.  Two batches are in flight
 * (sgk_sref_pipe_*): while one batch's text is written to stdout the next one is on the device.
 *
 * The FASTA reader follows kseq's line rules (src/kseq.h:185-225), which decide what the reference sees as a sequence:
 * the name runs to the first whitespace of the header line; sequence lines are appended whole, only the line end
 * (and a '\r' in front of it) is stripped; a line starting with '>', '+' or '@' ends the sequence; empty lines add
 * nothing. */
#include <ctype.h>
#include <errno.h>
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include "cli.h"
#include "sigtk_gpu.h"
#include "sref.h"

uint64_t fnv1a_bytes(const void *p_, size_t n) {
    const uint8_t *p = (const uint8_t *)p_;
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) {
        h ^= p[i];
        h *= 1099511628211ull;
    }
    return h;
}

/* ------------------------------------------------------------------ FASTA */

void fasta_free(fasta_t *fa) {
    free(fa->buf);
    free(fa->rec);
    fa->buf = NULL;
    fa->rec = NULL;
    fa->n = fa->cap = 0;
    fa->size = 0;
}

static int fasta_fail(fasta_t *fa, const char *fmt, const char *arg) {
    snprintf(fa->err, sizeof fa->err, fmt, arg);
    return -1;
}

static int fasta_slurp(const char *path, fasta_t *fa) {
    gzFile fp = gzopen(path, "r"); /* plain files are passed through */
    if (!fp) return fasta_fail(fa, "cannot open %s", path);
    gzbuffer(fp, 1 << 18);
    size_t cap = 1 << 20;
    fa->buf = (uint8_t *)malloc(cap);
    if (!fa->buf) {
        gzclose(fp);
        return fasta_fail(fa, "out of memory reading %s", path);
    }
    for (;;) {
        if (fa->size == cap) {
            cap *= 2;
            uint8_t *nb = (uint8_t *)realloc(fa->buf, cap);
            if (!nb) {
                gzclose(fp);
                return fasta_fail(fa, "out of memory reading %s", path);
            }
            fa->buf = nb;
        }
        const size_t room = cap - fa->size;
        const int got = gzread(fp, fa->buf + fa->size, (unsigned)(room < (1u << 30) ? room : (1u << 30)));
        if (got < 0) {
            gzclose(fp);
            return fasta_fail(fa, "read error (damaged gzip stream?) in %s", path);
        }
        if (got == 0) break;
        fa->size += (size_t)got;
    }
    if (gzclose(fp) != Z_OK) return fasta_fail(fa, "%s ends inside its gzip stream", path); /* Z_BUF_ERROR: truncated */
    return 0;
}

int fasta_read(const char *path, fasta_t *fa) {
    memset(fa, 0, sizeof *fa);
    if (fasta_slurp(path, fa) != 0) return -1;
    uint8_t *b = fa->buf;
    const size_t n = fa->size;
    size_t pos = 0;
    while (pos < n && b[pos] != '>' && b[pos] != '@') pos++; /* kseq jumps to the first header character */
    while (pos < n) {
        if (b[pos] == '@') return fasta_fail(fa, "%s holds a FASTQ record ('@' header): FASTQ input is not supported", path);
        pos++;
        if (pos >= n) break; /* a lone '>' at the end of the file is no record */
        const size_t ns = pos;
        while (pos < n && !isspace(b[pos])) pos++;
        const size_t name_len = pos - ns;
        if (pos < n && b[pos++] != '\n') { /* the description */
            const uint8_t *e = (const uint8_t *)memchr(b + pos, '\n', n - pos);
            pos = e ? (size_t)(e - b) + 1 : n;
        }
        const size_t s0 = pos;
        size_t w = pos;
        while (pos < n) {
            const uint8_t c = b[pos];
            if (c == '>' || c == '+' || c == '@') break;
            const uint8_t *e = (const uint8_t *)memchr(b + pos, '\n', n - pos);
            const size_t end = e ? (size_t)(e - b) : n, len = end - pos;
            if (len) {
                memmove(b + w, b + pos, len);
                w += len;
                /* kseq strips one '\r' when the sequence so far is longer than one byte; a last line of one byte
                 * without a line end is appended before it sees the end of the file and keeps its byte */
                if (w - s0 > 1 && b[w - 1] == '\r' && !(len == 1 && !e)) w--;
            }
            pos = e ? end + 1 : n;
        }
        if (pos < n && b[pos] == '+')
            return fasta_fail(fa, "%s holds a FASTQ record ('+' line): FASTQ input is not supported", path);
        if (w - s0 > 0x7fffffffull) return fasta_fail(fa, "a sequence of %s is longer than 2^31 - 1 bases", path);
        if (name_len > 0xffffffull) return fasta_fail(fa, "a sequence name of %s is longer than 2^24 bytes", path);
        if (fa->n == fa->cap) {
            const uint32_t nc = fa->cap ? fa->cap * 2 : 64;
            fa_rec_t *nr = (fa_rec_t *)realloc(fa->rec, (size_t)nc * sizeof *nr);
            if (!nr) return fasta_fail(fa, "out of memory reading %s", path);
            fa->rec = nr;
            fa->cap = nc;
        }
        fa_rec_t *r = &fa->rec[fa->n++];
        r->name = (const char *)b + ns;
        r->name_len = (uint32_t)name_len;
        r->seq = b + s0;
        r->len = w - s0;
    }
    return 0;
}

int fadumpmain(int argc, char *argv[]) {
    if (argc != 2) {
        fprintf(stderr, "usage: sigtk-amd _fadump ref.fa[.gz]\n");
        return 1;
    }
    fasta_t fa;
    if (fasta_read(argv[1], &fa) != 0) {
        ERROR("_fadump", "%s", fa.err);
        fasta_free(&fa);
        return 1;
    }
    for (uint32_t i = 0; i < fa.n; i++) {
        fwrite(fa.rec[i].name, 1, fa.rec[i].name_len, stdout);
        printf("\t%llu\t%016llx\n", (unsigned long long)fa.rec[i].len,
               (unsigned long long)fnv1a_bytes(fa.rec[i].seq, (size_t)fa.rec[i].len));
    }
    fasta_free(&fa);
    return 0;
}

/* ------------------------------------------------------------------ k-mer model */

static int model_fail(char *err, size_t err_len, const char *path, long line, const char *what) {
    if (line > 0) snprintf(err, err_len, "%s line %ld: %s", path, line, what);
    else snprintf(err, err_len, "%s: %s", path, what);
    return -1;
}

int model_read(const char *path, uint32_t want_k, float *levels, uint32_t *k_out, char *err, size_t err_len) {
    FILE *fp = fopen(path, "r");
    if (!fp) return model_fail(err, err_len, path, 0, "cannot open the k-mer model file");
    uint8_t *seen = (uint8_t *)calloc(4096, 1);
    char *line = NULL;
    size_t cap = 0;
    ssize_t got;
    long line_no = 0;
    uint32_t k = 0, count = 0;
    int rc = 0;
    char msg[160];
    if (!seen) rc = model_fail(err, err_len, path, 0, "out of memory");
    while (rc == 0 && (got = getline(&line, &cap, fp)) != -1) {
        line_no++;
        while (got > 0 && (line[got - 1] == '\n' || line[got - 1] == '\r')) line[--got] = 0;
        if (got == 0) continue;
        if (line[0] == '#') {
            if (strncmp(line, "#k", 2) == 0 && (line[2] == '\t' || line[2] == ' ')) {
                char *end;
                const long v = strtol(line + 3, &end, 10);
                if (end == line + 3 || v < 1 || v > 6) {
                    rc = model_fail(err, err_len, path, line_no, "the k-mer size of the #k line must be 1..6");
                } else if (count && (uint32_t)v != k) {
                    rc = model_fail(err, err_len, path, line_no, "the #k line disagrees with the k-mers in front of it");
                } else {
                    k = (uint32_t)v;
                }
            }
            continue;
        }
        if (strncmp(line, "kmer\tlevel_mean", 15) == 0) continue;
        size_t kl = 0;
        while (line[kl] && line[kl] != '\t' && line[kl] != ' ') kl++;
        if (k == 0) k = (uint32_t)kl;
        if (kl != k || kl < 1 || kl > 6) {
            snprintf(msg, sizeof msg, "a k-mer of %zu letters where k is %u (k must be 1..6)", kl, k);
            rc = model_fail(err, err_len, path, line_no, msg);
            break;
        }
        uint32_t rank = 0;
        for (size_t i = 0; i < kl && rc == 0; i++) {
            const char c = line[i];
            const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
            if (code < 0) {
                snprintf(msg, sizeof msg, "the k-mer '%.*s' holds a letter that is not A, C, G or T", (int)kl, line);
                rc = model_fail(err, err_len, path, line_no, msg);
            }
            rank = (rank << 2) | (uint32_t)(code & 3);
        }
        if (rc) break;
        char *p = line + kl, *end;
        while (*p == '\t' || *p == ' ') p++;
        errno = 0;
        const float v = strtof(p, &end);
        if (end == p || (*end && *end != '\t' && *end != ' ')) {
            snprintf(msg, sizeof msg, "level_mean of k-mer '%.*s' is not a number", (int)kl, line);
            rc = model_fail(err, err_len, path, line_no, msg);
            break;
        }
        if (seen[rank]) {
            snprintf(msg, sizeof msg, "the k-mer '%.*s' occurs twice", (int)kl, line);
            rc = model_fail(err, err_len, path, line_no, msg);
            break;
        }
        seen[rank] = 1;
        levels[rank] = v;
        count++;
    }
    if (rc == 0 && count == 0) rc = model_fail(err, err_len, path, 0, "no k-mer lines");
    if (rc == 0 && count != (1u << (2 * k))) {
        snprintf(msg, sizeof msg, "%u of the %u %u-mers are present; every k-mer must be given exactly once", count, 1u << (2 * k), k);
        rc = model_fail(err, err_len, path, 0, msg);
    }
    if (rc == 0 && want_k && k != want_k) {
        snprintf(msg, sizeof msg, "a %u-mer model, but sref computes with a %u-mer model %s --rna", k, want_k,
                 want_k == 5 ? "with" : "without");
        rc = model_fail(err, err_len, path, 0, msg);
    }
    free(line);
    free(seen);
    fclose(fp);
    if (rc == 0) *k_out = k;
    return rc;
}

int modelcheckmain(int argc, char *argv[]) {
    const char *path = NULL;
    int rna = 0;
    for (int i = 1; i < argc; i++) {
        if (strcmp(argv[i], "--rna") == 0) rna = 1;
        else path = argv[i];
    }
    if (!path) {
        fprintf(stderr, "usage: sigtk-amd _modelcheck FILE [--rna]\n");
        return 1;
    }
    float *levels = (float *)calloc(4096, sizeof(float));
    if (!levels) return 1;
    uint32_t k = 0;
    char err[512];
    if (model_read(path, rna ? 5 : 6, levels, &k, err, sizeof err) != 0) {
        ERROR("_modelcheck", "%s", err);
        free(levels);
        return 1;
    }
    printf("k\t%u\tkmers\t%u\tfnv\t%016llx\n", k, 1u << (2 * k),
           (unsigned long long)fnv1a_bytes(levels, sizeof(float) << (2 * k)));
    free(levels);
    return 0;
}

/* ------------------------------------------------------------------ sref */

/* the rows of the file in order ('+' and, for DNA, '-' of every sequence), handed out in pieces of positions */
typedef struct {
    const fasta_t *fa;
    uint32_t k, seq;
    int rna, strand;
    uint64_t pos; /* signal positions of the current row already handed out */
} row_cursor_t;

typedef struct {
    sgk_sref_span_t *v;
    uint32_t n, cap;
} span_vec_t;

/* the next batch: spans of at most `budget` positions in all (and at most max_spans spans); 0 when the file is done */
static uint32_t next_batch(row_cursor_t *c, uint64_t budget, uint32_t max_spans, span_vec_t *out, uint64_t *n_bases,
                           uint32_t *first_seq) {
    out->n = 0;
    *first_seq = c->seq;
    *n_bases = 0;
    uint64_t used = 0;
    const uint32_t seq0 = c->seq;
    while (c->seq < c->fa->n && out->n < max_spans && used < budget) {
        const fa_rec_t *r = &c->fa->rec[c->seq];
        const int64_t ref_len = (int64_t)r->len + 1 - (int64_t)c->k;
        uint64_t count = 0;
        if (ref_len > 0) {
            count = (uint64_t)ref_len - c->pos;
            if (count > budget - used) count = budget - used;
        }
        if (out->n == out->cap) {
            const uint32_t nc = out->cap ? out->cap * 2 : 1024;
            sgk_sref_span_t *nv = (sgk_sref_span_t *)realloc(out->v, (size_t)nc * sizeof *nv);
            if (!nv) {
                ERROR("srefmain", "%s", "out of memory");
                die_flushed();
            }
            out->v = nv;
            out->cap = nc;
        }
        sgk_sref_span_t *s = &out->v[out->n++];
        memset(s, 0, sizeof *s);
        s->seq_len = (uint32_t)r->len;
        s->first = (uint32_t)c->pos;
        s->count = (uint32_t)count;
        s->seq = c->seq - seq0;
        s->strand = (uint8_t)c->strand;
        /* the forward bases the span reads: '+' [first, first + count + k - 1), '-' [l - first - count - k + 1, l - first) */
        const uint64_t nb = count ? count + c->k - 1 : 0;
        s->base_pos0 = count ? (c->strand ? r->len - c->pos - count - c->k + 1 : c->pos) : 0;
        s->base_offset = *n_bases;
        *n_bases += nb;
        used += count;
        c->pos += count;
        if (ref_len <= 0 || c->pos == (uint64_t)ref_len) {
            c->pos = 0;
            if (c->rna || c->strand == 1) {
                c->strand = 0;
                c->seq++;
            } else {
                c->strand = 1;
            }
        }
    }
    return out->n;
}

static void emit(sgk_sref_pipe_t *pipe, int slot) {
    const uint8_t *text;
    uint64_t nb;
    const int rc = sgk_sref_pipe_wait(pipe, slot, &text, &nb);
    if (rc != SGK_OK) gpu_fail("srefmain", "sgk_sref_pipe_wait", rc);
    if (nb && fwrite(text, 1, (size_t)nb, stdout) != nb) {
        ERROR("srefmain", "%s", "writing to stdout failed");
        die_flushed();
    }
}

int srefmain(int argc, char *argv[]) {
    static const struct option long_options[] = {
        {"help", no_argument, 0, 'h'},          {"version", no_argument, 0, 'V'},   {"output", required_argument, 0, 'o'},
        {"verbose", required_argument, 0, 'v'}, {"rna", no_argument, 0, OPT_RNA},   {"kmer-model", required_argument, 0, OPT_KMER_MODEL},
        {"batch", required_argument, 0, OPT_BATCH}, {0, 0, 0, 0}};
    int c;
    FILE *fp_help = stderr;
    int rna = 0, hdr = 1;
    const char *model_fn = NULL;
    uint64_t budget = 16ull << 20; /* signal positions per batch: about 11 bytes of text each, ~180 MB */
    while ((c = getopt_long(argc, argv, "o:v:hVn", long_options, NULL)) >= 0) {
        if (c == 'V') {
            version_exit();
        } else if (c == 'h') {
            fp_help = stdout;
        } else if (c == 'n') {
            hdr = 0;
        } else if (c == OPT_RNA) {
            rna = 1;
        } else if (c == OPT_KMER_MODEL) {
            model_fn = optarg;
        } else if (c == OPT_BATCH) {
            budget = strtoull(optarg, NULL, 10);
            if (budget < 1) budget = 1;
            if (budget > (1ull << 31)) budget = 1ull << 31;
        }
    }
    if (argc - optind < 1 || fp_help == stdout) {
        fprintf(fp_help, "Usage: sigtk sref --kmer-model FILE ref.fa \n");
        fprintf(fp_help, "\nbasic options:\n");
        fprintf(fp_help, "   -h                         help\n");
        fprintf(fp_help, "   -n                         suppress header\n");
        fprintf(fp_help, "   --version                  print version\n");
        fprintf(fp_help, "   --rna                      use RNA model\n");
        fprintf(fp_help, "   --kmer-model FILE          k-mer model file (6-mers; 5-mers with --rna) [required]\n");
        fprintf(fp_help, "   --batch INT                signal positions per GPU batch [%llu]\n", (unsigned long long)budget);
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    if (!model_fn) {
        ERROR("srefmain", "%s", "this build carries no built-in pore model: give one with --kmer-model FILE "
                                "(columns kmer, level_mean; 6-mers for DNA, 5-mers with --rna)");
        die_flushed();
    }
    const uint32_t k = rna ? 5 : 6;
    float *levels = (float *)calloc(4096, sizeof(float));
    if (!levels) die_flushed();
    uint32_t k_file = 0;
    char err[512];
    if (model_read(model_fn, k, levels, &k_file, err, sizeof err) != 0) {
        ERROR("srefmain", "%s", err);
        die_flushed();
    }
    fasta_t fa;
    if (fasta_read(argv[optind], &fa) != 0) {
        ERROR("srefmain", "%s", fa.err);
        die_flushed();
    }
    if (sgk_device_count() <= 0) {
        ERROR("srefmain", "%s", "no usable GPU: sigtk-amd has no CPU compute path");
        die_flushed();
    }
    sgk_sref_pipe_t *pipe = NULL;
    int rc = sgk_sref_pipe_create(0, levels, k, &pipe);
    if (rc != SGK_OK) gpu_fail("srefmain", "sgk_sref_pipe_create", rc);
    if (hdr) printf("ref_name\tref_len\tstrand\tsig_len\tsig_mean\n");

    row_cursor_t cur = {&fa, k, 0, rna, 0, 0};
    span_vec_t spans = {NULL, 0, 0};
    uint64_t n_bases = 0;
    uint32_t seq0 = 0;
    int slot = 0, pending = -1;
    while (next_batch(&cur, budget, 1u << 20, &spans, &n_bases, &seq0)) {
        /* the batch's sequences are consecutive: names are indexed from its first one */
        const uint32_t n_names = spans.v[spans.n - 1].seq + 1;
        uint64_t name_bytes = 0;
        for (uint32_t i = 0; i < n_names; i++) name_bytes += fa.rec[seq0 + i].name_len;
        if (name_bytes > 0xfffffff0ull) {
            ERROR("srefmain", "%s", "the sequence names of one batch exceed 4 GiB");
            die_flushed();
        }
        sgk_sref_stage_t st;
        rc = sgk_sref_pipe_begin(pipe, slot, n_bases, spans.n, n_names, name_bytes, &st);
        if (rc != SGK_OK) gpu_fail("srefmain", "sgk_sref_pipe_begin", rc);
        uint32_t no = 0;
        for (uint32_t i = 0; i < n_names; i++) {
            st.name_offsets[i] = no;
            memcpy(st.name_bytes + no, fa.rec[seq0 + i].name, fa.rec[seq0 + i].name_len);
            no += fa.rec[seq0 + i].name_len;
        }
        st.name_offsets[n_names] = no;
        for (uint32_t s = 0; s < spans.n; s++) {
            const sgk_sref_span_t *sp = &spans.v[s];
            if (sp->count) memcpy(st.bases + sp->base_offset, fa.rec[seq0 + sp->seq].seq + sp->base_pos0, (size_t)sp->count + k - 1);
        }
        memcpy(st.spans, spans.v, (size_t)spans.n * sizeof *spans.v);
        rc = sgk_sref_pipe_submit(pipe, slot);
        if (rc != SGK_OK) gpu_fail("srefmain", "sgk_sref_pipe_submit", rc);
        if (pending >= 0) emit(pipe, pending);
        pending = slot;
        slot ^= 1;
    }
    if (pending >= 0) emit(pipe, pending);
    sgk_sref_pipe_destroy(pipe);
    free(spans.v);
    free(levels);
    fasta_free(&fa);
    return 0;
}
