/* cli.h -- what every unit of the `sigtk-amd` host program shares: the reference's message forms, the ways out of the
 * process, wall time, a growable output buffer, the grow helper, the values of the long options, and the entry points of
 * the hidden test subcommands (selftest.c).  Needs nothing of the GPU library: pool.c links with this header alone. */
#ifndef SIGTK_AMD_CLI_H
#define SIGTK_AMD_CLI_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <unistd.h>

#define MSG(fn, tag, colour, ...)                                      \
    do {                                                                \
        fprintf(stderr, "[%s::" tag "]\033[1;" colour "m ", fn);         \
        fprintf(stderr, __VA_ARGS__);                                   \
        fprintf(stderr, "\033[0m\n");                                   \
    } while (0)
#define INFO(fn, msg) MSG(fn, "INFO", "34", "%s", msg)
#define WARNING(fn, ...) MSG(fn, "WARNING", "33", __VA_ARGS__)
#define ERROR(fn, ...) MSG(fn, "ERROR", "31", __VA_ARGS__)

/* Long options without a letter, by name: what getopt_long returns for them (cmain, qtsmain, srefmain, ssmain). */
enum {
    OPT_PRINT_STAT = 256, OPT_GPUS, OPT_BATCH_SAMPLES, OPT_HOST_DECODE, OPT_HOST_INFLATE, OPT_GPU_TEXT, OPT_AUX_SLACK,
    OPT_DETECTOR, OPT_SEGMENTER, OPT_ADAPTOR, OPT_POLYA,   /* (these four in this order: cmain's list_option) */
    OPT_GPU_DEFLATE, OPT_GPU_INFLATE, OPT_RNA, OPT_KMER_MODEL, OPT_BATCH, OPT_NORMALISE
};

/* Fatal errors can be raised on the reader, loader and writer threads while other threads still have HIP work in
 * flight: leave without running exit handlers (exit() would run the HIP runtime's concurrently with live streams). */
static inline void die_now(void) {
    fflush(stderr);
    _exit(EXIT_FAILURE);
}
/* ... of a subtool that writes its rows from one thread (sref, ss): the header line and the rows already written stay
 * in front of the error */
static inline void die_flushed(void) {
    fflush(stdout);
    die_now();
}
static inline void die_mem(void) {
    ERROR("main", "%s", "out of memory");
    die_now();
}
/* cli.c.  gpu_fail: a library call came back with rc.  tool NULL: the pipeline's form, the message under the call's own
 * name; else under the subtool's name, with its rows flushed first (sref, ss). */
void gpu_fail(const char *tool, const char *what, int rc);
void die_read_error(int code);   /* what the reference prints when slow5_get_next fails (src/cmain.c:121-124) */
void version_exit(void);         /* -V / --version */

static inline double realtime(void) {
    struct timeval tp;
    gettimeofday(&tp, NULL);
    return tp.tv_sec + tp.tv_usec * 1e-6;
}

/* make the array p hold n elements, or die */
static inline void *grow_or_die(void *p, size_t n, size_t elem) {
    const size_t bytes = n * elem;
    p = realloc(p, bytes ? bytes : 1);
    if (!p) die_mem();
    return p;
}
#define GROW(p, n) ((p) = grow_or_die((p), (size_t)(n), sizeof *(p)))

/* growable output buffer (inline: the row formatters call these per value) */
typedef struct {
    char *p;
    size_t n, cap;
} sbuf_t;

static inline char *sbuf_room(sbuf_t *b, size_t need) {
    if (b->n + need > b->cap) {
        size_t c = b->cap ? b->cap : (1u << 16);
        while (c < b->n + need) c *= 2;
        b->p = (char *)grow_or_die(b->p, c, 1);
        b->cap = c;
    }
    return b->p + b->n;
}
static inline void sbuf_str(sbuf_t *b, const char *s, size_t len) {
    memcpy(sbuf_room(b, len), s, len);
    b->n += len;
}

/* selftest.c: the hidden subcommands the tests drive (no GPU) */
int dumpmain(int argc, char *argv[]);
int zstdmain(int argc, char *argv[]);
int fmtcheckmain(int argc, char *argv[]);
int textcheckmain(int argc, char *argv[]);
int qtsframesmain(int argc, char *argv[]);

#endif
