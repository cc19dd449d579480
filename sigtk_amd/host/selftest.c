/* selftest.c -- the hidden subcommands the tests drive: _dump, _zstd, _fmtcheck, _textcheck, _qtsframes.  No GPU. */
#include "blow5.h"
#include "cli.h"
#include "fmt.h"
#include "zstd_dec.h"
#include "../csrc/text_format.h"

/* _dump: id, length, scaling and a checksum of every record.  `--split` goes
 * through the pipelined reader's split API (b5_next_raw + b5_parse_raw + b5_svb_zd_decode; with --id: b5_get_raw).
 * `--aux` prints the table of the header's auxiliary columns instead (b5_aux_fields): one line, "#aux", the number of
 * columns, then every column's element size with a '*' behind it for an array -- or "#aux\tnone" without a table. */
static uint64_t fnv_i16(const int16_t *x, uint64_t n) {
    uint64_t h = 1469598103934665603ull;
    for (uint64_t i = 0; i < n; i++) {
        h ^= (uint16_t)x[i];
        h *= 1099511628211ull;
    }
    return h;
}
static void dump_view(const b5_view_t *v, const int16_t *sig) {
    printf("%.*s\t%lu\t%.17g\t%.17g\t%.17g\t%016lx\n", (int)v->id_len, v->read_id, (unsigned long)v->n_samples,
           v->digitisation, v->offset, v->range, (unsigned long)fnv_i16(sig, v->n_samples));
}
static void dump_rec(const b5_rec_t *rec) {
    printf("%s\t%lu\t%.17g\t%.17g\t%.17g\t%016lx\n", rec->read_id, (unsigned long)rec->len_raw_signal,
           rec->digitisation, rec->offset, rec->range, (unsigned long)fnv_i16(rec->raw_signal, rec->len_raw_signal));
}
/* the pipeline's read-id path: b5_get_raw (index + verification of the fetched record) + b5_parse_raw */
static int dump_id_split(b5_file_t *f, const char *want_id) {
    uint8_t *raw = NULL, *scratch = NULL;
    uint64_t len = 0, cap = 0, scap = 0, size = 0;
    int ret = b5_get_raw(f, want_id, &raw, &len, &cap, &size);
    b5_view_t v;
    if (ret == 0) ret = b5_parse_raw(f, raw, size, &scratch, &scap, &v);
    if (ret == 0) {
        int16_t *sig = (int16_t *)malloc(sizeof(int16_t) * (v.n_samples ? v.n_samples : 1));
        if (!sig) ret = -1;
        else if (f->text) ret = b5_sigtext_decode(v.signal, v.signal_bytes, sig, v.n_samples);
        else if (f->signal_press == 1) ret = b5_svb_zd_decode(v.signal, v.signal_bytes, sig, v.n_samples);
        else if (v.signal_bytes != 2 * (uint64_t)v.n_samples) ret = -1;  /* (a malformed record: the copy would overrun) */
        else memcpy(sig, v.signal, v.signal_bytes);
        if (ret == 0) dump_view(&v, sig);
        free(sig);
    }
    free(raw);
    free(scratch);
    return ret;
}
/* every record through the split API; split 2: over the mapped file (b5_map / b5_next_ref) */
static int dump_split(b5_file_t *f, int split) {
    uint8_t *raw = NULL, *scratch = NULL;
    uint64_t raw_len = 0, raw_cap = 0, scratch_cap = 0, size = 0, sig_cap = 0;
    int16_t *sig = NULL;
    int ret;
    const uint8_t *ref = NULL;
    while ((ret = split == 2 ? b5_next_ref(f, &ref, &size) : b5_next_raw(f, &raw, &raw_len, &raw_cap, &size)) >= 0) {
        b5_view_t v;
        ret = b5_parse_raw(f, split == 2 ? ref : raw + raw_len - size, size, &scratch, &scratch_cap, &v);
        if (ret < 0) break;
        raw_len = 0;
        if (v.n_samples > sig_cap) {
            GROW(sig, (size_t)v.n_samples + 1);
            sig_cap = v.n_samples;
        }
        if (f->text) {
            ret = b5_sigtext_decode(v.signal, v.signal_bytes, sig, v.n_samples);
            if (ret < 0) break;
        } else if (f->signal_press == 1) {
            ret = b5_svb_zd_decode(v.signal, v.signal_bytes, sig, v.n_samples);
            if (ret < 0) break;
        } else if (v.n_samples) {
            memcpy(sig, v.signal, v.signal_bytes);
        }
        dump_view(&v, sig);
    }
    free(raw); free(scratch); free(sig);
    return ret;
}
int dumpmain(int argc, char *argv[]) {
    int split = 0, aux = 0;
    const char *path = NULL, *want_id = NULL;
    for (int i = 1; i < argc; i++) {
        if (strcmp(argv[i], "--split") == 0) split = 1;
        else if (strcmp(argv[i], "--aux") == 0) aux = 1;
        else if (strcmp(argv[i], "--map") == 0) split = 2;  /* split API over the mapped file (b5_map / b5_next_ref) */
        else if (strcmp(argv[i], "--id") == 0 && i + 1 < argc) want_id = argv[++i]; /* one record through the index */
        else path = argv[i];
    }
    if (!path) return 1;
    b5_file_t *f = b5_open(path);
    if (!f) {
        ERROR("dumpmain", "cannot open %s. ", path);
        return 1;
    }
    int ret;
    if (aux) {
        b5_aux_field_t *tab = NULL;
        const int64_t n = b5_aux_fields(f, &tab);
        if (n < 0) printf("#aux\tnone\n");
        else {
            printf("#aux\t%ld", (long)n);
            for (int64_t k = 0; k < n; k++) printf("\t%d%s", tab[k].elem_bytes, tab[k].is_array ? "*" : "");
            printf("\n");
        }
        free(tab);
        b5_close(f);
        return 0;
    }
    if (want_id) {
        if (split) ret = dump_id_split(f, want_id);
        else {
            b5_rec_t rec;
            memset(&rec, 0, sizeof rec);
            ret = b5_get(f, want_id, &rec);
            if (ret == 0) dump_rec(&rec);
            b5_rec_free(&rec);
        }
        b5_close(f);
        return ret == 0 ? 0 : 1;
    }
    printf("#press\t%d\t%d\tgroups\t%u\n", f->record_press, f->signal_press, f->num_read_groups);
    if (split) {
        if (split == 2 && b5_map(f) != 0) {
            ERROR("dumpmain", "%s", "cannot map the file");
            return 1;
        }
        ret = dump_split(f, split);
    } else {
        b5_rec_t rec;
        memset(&rec, 0, sizeof rec);
        while ((ret = b5_next(f, &rec)) >= 0) dump_rec(&rec);
        b5_rec_free(&rec);
    }
    b5_close(f);
    return ret == B5_EOF ? 0 : 1;
}

/* _zstd FILE decodes the zstd frame in FILE with the host decoder (zstd_dec.c) and writes the
 * content to stdout; a frame that is refused: exit 1, "zstd status N: ..." on stderr.  With --head N: the frame's first
 * N bytes as zsd_decode_head gives them (what b5_parse_head uses). */
int zstdmain(int argc, char *argv[]) {
    long head = -1;
    if (argc == 4 && strcmp(argv[1], "--head") == 0) {
        head = atol(argv[2]);
        argv += 2;
        argc -= 2;
    }
    if (argc != 2 || head < -1 || head > (1l << 30)) {
        fprintf(stderr, "Usage: sigtk-amd _zstd [--head N] FILE\n");
        return 1;
    }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) {
        fprintf(stderr, "Error in opening file\n");
        return 1;
    }
    uint8_t *in = NULL;
    size_t n = 0, cap = 0;
    for (;;) {
        if (n == cap) {
            cap = cap ? cap * 2 : 1 << 16;
            GROW(in, cap);
        }
        const size_t got = fread(in + n, 1, cap - n, fp);
        if (got == 0) break;
        n += got;
    }
    fclose(fp);
    uint64_t size = 0;
    int st = zsd_content_size(in, n, &size);
    if (st == ZSD_OK && size > (1ull << 31)) st = ZSD_ERR_SIZE;
    uint8_t *out = NULL;
    size_t got = 0;
    if (st == ZSD_OK) {
        const size_t room = head >= 0 ? (size_t)head : (size_t)size;
        GROW(out, room);
        st = head >= 0 ? zsd_decode_head(in, n, out, room, &got) : zsd_decode(in, n, out, room, &got);
    }
    int ret = 0;
    if (st != ZSD_OK) {
        fprintf(stderr, "zstd status %d: %s\n", st, zsd_status_name(st));
        ret = 1;
    } else if (fwrite(out, 1, got, stdout) != got) ret = 1;
    free(in);
    free(out);
    return ret;
}

/* the cases both number checks share: every stride-th float bit pattern in [first, last] (defaults: all), then ties and
 * carries: k / 2^m around the 6th decimal, values just below integers */
typedef uint64_t (*f32_check_fn)(uint32_t w, const char *want, uint64_t *bad);
static uint64_t check_f32_sweep(int argc, char *argv[], f32_check_fn check, uint64_t *bad) {
    const uint32_t stride = argc > 1 ? (uint32_t)strtoul(argv[1], NULL, 10) : 9973u;
    const uint64_t first = argc > 3 ? strtoull(argv[2], NULL, 0) : 0, last = argc > 3 ? strtoull(argv[3], NULL, 0) : 0xffffffffull;
    uint64_t n = 0;
    for (uint64_t u = first; u <= last; u += stride ? stride : 1) n += check((uint32_t)u, NULL, bad);
    return n;
}
static uint64_t check_f32_ties(f32_check_fn check, uint64_t *bad) {
    uint64_t n = 0;
    for (int m = 1; m <= 30; m++)
        for (int k = 1; k < 4000; k += 2) {
            const float f = (float)k / (float)(1u << m);
            const float g[4] = {f, -f, f + 123456.0f, 999999.0f + f};
            for (int t = 0; t < 4; t++) {
                uint32_t w;
                memcpy(&w, &g[t], 4);
                n += check(w, NULL, bad);
            }
        }
    return n;
}

/* _fmtcheck [stride [first last]]: fmt_f6 / fmt_i64 against snprintf */
static uint64_t fmtcheck_f32(uint32_t w, const char *want, uint64_t *bad) {
    (void)want;
    char a[512], b[512];
    float f;
    memcpy(&f, &w, 4);
    *fmt_f6(a, f) = '\0';
    snprintf(b, sizeof b, "%f", f);
    if (strcmp(a, b) != 0 && (*bad)++ < 10) printf("MISMATCH %08x: %s vs %s\n", w, a, b);
    return 1;
}
int fmtcheckmain(int argc, char *argv[]) {
    uint64_t bad = 0, n = check_f32_sweep(argc, argv, fmtcheck_f32, &bad);
    char a[512], b[512];
    n += check_f32_ties(fmtcheck_f32, &bad);
    const int64_t iv[] = {0, 1, -1, 9, 10, 99, 100, 12345, -98765, 2147483647LL, -2147483648LL, 4294967295LL,
                          9223372036854775807LL, (-9223372036854775807LL - 1)};
    for (size_t i = 0; i < sizeof iv / sizeof iv[0]; i++) {
        *fmt_i64(a, iv[i]) = '\0';
        snprintf(b, sizeof b, "%ld", (long)iv[i]);
        n++;
        if (strcmp(a, b) != 0 && bad++ < 10) printf("MISMATCH int: %s vs %s\n", a, b);
    }
    printf("checked %lu values, %lu mismatches\n", (unsigned long)n, (unsigned long)bad);
    return bad ? 1 : 0;
}

/* _textcheck [stride [first last]]: csrc/text_format.h (the header the device-side writer compiles for gfx950), compiled
 * here by the host compiler, against snprintf -- the bytes and the length-only form */
static uint64_t textcheck_f32(uint32_t w, const char *want, uint64_t *bad) {
    char a[64], b[512];
    float f;
    memcpy(&f, &w, 4);
    memset(a, '#', sizeof a);
    const int n = sgk_tf_f32(a, f);
    const int m = snprintf(b, sizeof b, "%f", f);
    const int ok = n == m && n <= SGK_TF_F32_MAX_BYTES && memcmp(a, b, (size_t)m) == 0 && a[n] == '#' &&
                   sgk_tf_f32_len(f) == m && (!want || strcmp(b, want) == 0);
    if (!ok && (*bad)++ < 10) printf("MISMATCH %08x: %.*s (%d, length form %d) vs %s\n", w, n > 0 && n < 64 ? n : 0, a, n, sgk_tf_f32_len(f), b);
    return 1;
}
static uint64_t textcheck_i64(int64_t v, uint64_t *bad) {
    char a[64], b[64];
    memset(a, '#', sizeof a);
    const int n = sgk_tf_i64(a, v);
    const int m = snprintf(b, sizeof b, "%ld", (long)v);
    const int ok = n == m && memcmp(a, b, (size_t)m) == 0 && a[n] == '#' && sgk_tf_i64_len(v) == m;
    if (!ok && (*bad)++ < 10) printf("MISMATCH int %ld: length %d, length form %d vs %s\n", (long)v, n, sgk_tf_i64_len(v), b);
    if (v >= 0) {
        memset(a, '#', sizeof a);
        const int nu = sgk_tf_u64(a, (uint64_t)v);
        if ((nu != m || memcmp(a, b, (size_t)m) != 0 || a[nu] != '#' || sgk_tf_u64_len((uint64_t)v) != m) && (*bad)++ < 10)
            printf("MISMATCH unsigned %ld\n", (long)v);
    }
    return 1;
}
int textcheckmain(int argc, char *argv[]) {
    /* after the sweep, the fixed cases: powers of two and their neighbours, ties and carries, both sides of 1e15, FLT_MAX,
     * denormals, zeros, infinities, NaNs of both signs; "%ld" on 0, +-1, powers of ten +- 1 and the ends of the range */
    uint64_t bad = 0, n = check_f32_sweep(argc, argv, textcheck_f32, &bad);
    for (uint32_t e = 0; e < 256; e++)
        for (int d = -2; d <= 2; d++)
            for (uint32_t sgn = 0; sgn < 2; sgn++) n += textcheck_f32(((e << 23) + (uint32_t)d) ^ (sgn << 31), NULL, &bad);
    n += check_f32_ties(textcheck_f32, &bad);
    n += textcheck_f32(0x3c000000u, "0.007812", &bad);                 /* 2^-7 = 0.0078125: the tie goes to even */
    n += textcheck_f32(0x58635fa8u, "999999919882240.000000", &bad);
    n += textcheck_f32(0x58635fa9u, "999999986991104.000000", &bad);   /* the last float below 1e15 */
    n += textcheck_f32(0x58635faau, "1000000054099968.000000", &bad);  /* the first one above: the multi-limb path */
    n += textcheck_f32(0xd8635faau, "-1000000054099968.000000", &bad);
    n += textcheck_f32(0x7f7fffffu, "340282346638528859811704183484516925440.000000", &bad);
    n += textcheck_f32(0xff7fffffu, "-340282346638528859811704183484516925440.000000", &bad);
    n += textcheck_f32(0x00000000u, "0.000000", &bad);
    n += textcheck_f32(0x80000000u, "-0.000000", &bad);
    n += textcheck_f32(0x7f800000u, "inf", &bad);
    n += textcheck_f32(0xff800000u, "-inf", &bad);
    n += textcheck_f32(0x7fc00000u, "nan", &bad);
    n += textcheck_f32(0xffc00000u, "-nan", &bad);
    n += textcheck_f32(0x7f800001u, "nan", &bad);
    n += textcheck_f32(0xffffffffu, "-nan", &bad);
    for (uint32_t w = 0; w < 64; w++) n += textcheck_f32(w, NULL, &bad) + textcheck_f32(0x007fffffu - w, NULL, &bad) + textcheck_f32(0x80000000u | w, NULL, &bad);
    n += textcheck_i64(0, &bad);
    int64_t p10 = 1;
    for (int k = 0; k < 19; k++, p10 *= 10)
        for (int d = -1; d <= 1; d++) n += textcheck_i64(p10 + d, &bad) + textcheck_i64(-(p10 + d), &bad);
    const int64_t iv[] = {12345, -98765, 2147483647LL, -2147483648LL, 4294967295LL, 4294967296LL, 9223372036854775807LL, (-9223372036854775807LL - 1)};
    for (size_t i = 0; i < sizeof iv / sizeof iv[0]; i++) n += textcheck_i64(iv[i], &bad);
    printf("checked %lu values, %lu mismatches\n", (unsigned long)n, (unsigned long)bad);
    return bad ? 1 : 0;
}

/* _qtsframes [FILE].  For every record of the text SLOW5 file FILE, what `qts` uploads
 * around its signal column (b5_s5_qts_head and the bytes behind the column with the newline), as two lines
 * "H <bytes> <hex>" and "T <bytes> <hex>"; a record the reader refuses ends the listing as it ends the subtools.  Then the
 * int16 writer of csrc/text_format.h over all 65 536 values against snprintf("%d"), the bytes and the length-only form. */
static void qtsframes_hex(char tag, const uint8_t *p, uint64_t n) {
    printf("%c %lu ", tag, (unsigned long)n);
    for (uint64_t i = 0; i < n; i++) printf("%02x", p[i]);
    printf("\n");
}
int qtsframesmain(int argc, char *argv[]) {
    int ret = 0;
    if (argc > 1) {
        b5_file_t *f = b5_open(argv[1]);
        if (!f || !f->text) {
            fprintf(stderr, "Error in opening file\n");
            return 1;
        }
        uint8_t *raw = NULL, *head = NULL, *scratch = NULL;
        uint64_t raw_len = 0, raw_cap = 0, head_cap = 0, scratch_cap = 0, size = 0;
        int rc;
        while ((rc = b5_next_raw(f, &raw, &raw_len, &raw_cap, &size)) >= 0) {
            b5_view_t v;
            rc = b5_parse_raw(f, raw, size, &scratch, &scratch_cap, &v);
            raw_len = 0;
            if (rc < 0) break;
            const int64_t h = b5_s5_qts_head(&v, &head, &head_cap);
            if (h < 0) {
                rc = (int)h;
                break;
            }
            const uint8_t *tail = v.signal + v.signal_bytes;
            qtsframes_hex('H', head, (uint64_t)h);
            printf("T %lu ", (unsigned long)(v.rec + v.rec_len - tail) + 1);
            for (const uint8_t *q = tail; q < v.rec + v.rec_len; q++) printf("%02x", *q);
            printf("0a\n");
        }
        if (rc != B5_EOF) {
            fprintf(stderr, "Error in slow5_get_next. Error code %d\n", rc);
            ret = 1;
        }
        free(raw); free(head); free(scratch);
        b5_close(f);
    }
    uint64_t bad = 0;
    for (int32_t x = -32768; x <= 32767; x++) {
        char a[16], w[16];
        memset(a, '#', sizeof a);
        const int n = sgk_tf_i16(a, (int16_t)x), m = snprintf(w, sizeof w, "%d", x);
        if (n != m || n != sgk_tf_i16_len((int16_t)x) || memcmp(a, w, (size_t)m) != 0 || a[n] != '#') bad++;
    }
    printf("i16 checked 65536 values, %lu mismatches\n", (unsigned long)bad);
    return ret || bad ? 1 : 0;
}
