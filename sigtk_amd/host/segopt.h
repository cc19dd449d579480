/* segopt.h -- the comma-separated lists of jnn --segmenter, prefix --adaptor and prefix --polya, parsed like event
 * --detector: an exact number of fields, none empty, no white space, nothing behind a number, integers as decimal
 * integers.  Syntax only: the domain is the library's (sgk_jnn_params_check, sgk_prefix_params_check), asked by the caller.
 * Header only, no dependency but libc: tools/segopt_check.c runs the malformed lists through it under the sanitizers. */
#ifndef SIGTK_AMD_SEGOPT_H
#define SIGTK_AMD_SEGOPT_H

#include <ctype.h>
#include <errno.h>
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#define SEGOPT_MAX_FIELDS 8

/* kinds[k]: 'i' a decimal int, 'f' a finite float, 'a' any float (NaN and infinities included).  Parses at most
 * strlen(kinds) fields into v[] and returns how many there were, or -1 with *why set.  A list with more fields than
 * kinds is "too many fields". */
static int segopt_list(const char *arg, const char *kinds, double *v, const char **why) {
    const int max = (int)strlen(kinds);
    const char *p = arg;
    for (int k = 0;; k++) {
        if (k == max) { *why = "too many fields"; return -1; }
        if (*p == '\0' || *p == ',') { *why = "an empty field"; return -1; }
        if (isspace((unsigned char)*p)) { *why = "white space in a field"; return -1; }
        char *end = NULL;
        if (kinds[k] == 'i') {
            const char *d = (*p == '-') ? p + 1 : p;
            if (*d < '0' || *d > '9') { *why = "a field that is no decimal integer"; return -1; }
            errno = 0;
            const long long u = strtoll(p, &end, 10);
            if (errno || u > 2147483647LL || u < -2147483647LL - 1) { *why = "an integer out of range"; return -1; }
            v[k] = (double)u;
        } else {
            v[k] = strtod(p, &end);
            if (end == p) { *why = "a field that is no number"; return -1; }
            /* (in double, before any cast: a double beyond float's range has no defined conversion) */
            if (kinds[k] == 'f' && !(v[k] >= -(double)FLT_MAX && v[k] <= (double)FLT_MAX)) {
                *why = "a value that is not finite";
                return -1;
            }
            if (kinds[k] == 'a' && v[k] == v[k]) {
                if (v[k] > (double)FLT_MAX) v[k] = (double)INFINITY;
                if (v[k] < -(double)FLT_MAX) v[k] = -(double)INFINITY;
            }
        }
        if (*end == '\0') return k + 1;
        if (*end != ',') { *why = "text behind a number"; return -1; }
        p = end + 1;
    }
}

/* jnn --segmenter STD_SCALE,CORRECTOR,SEG_DIST,WINDOW,STALL_LEN,ERROR[,TOP,BOT]: eight fields exactly when
 * STD_SCALE <= 0 (the fixed thresholds), six otherwise.  out[8]: the fields in that order, TOP and BOT 0 when absent. */
static int segopt_segmenter(const char *arg, double *out, const char **why) {
    memset(out, 0, 8 * sizeof *out);
    const int n = segopt_list(arg, "fiiifiaa", out, why);
    if (n < 0) return -1;
    const int want = out[0] <= 0.0 ? 8 : 6;
    if (n < want) { *why = want == 8 && n >= 6 ? "STD_SCALE <= 0 without TOP,BOT" : "too few fields"; return -1; }
    if (n > want) { *why = "TOP or BOT given with STD_SCALE > 0"; return -1; }
    return 0;
}
/* prefix --adaptor STD_SCALE,SEG_DIST,WINDOW,HI_THRESH,LO_THRESH */
static int segopt_adaptor(const char *arg, double *out, const char **why) {
    const int n = segopt_list(arg, "fiiii", out, why);
    if (n < 0) return -1;
    if (n != 5) { *why = "too few fields"; return -1; }
    return 0;
}
/* prefix --polya CORRECTOR,SEG_DIST,WINDOW,STALL_LEN,ERROR,SHIFT,BAND */
static int segopt_polya(const char *arg, double *out, const char **why) {
    const int n = segopt_list(arg, "iiififf", out, why);
    if (n < 0) return -1;
    if (n != 7) { *why = "too few fields"; return -1; }
    return 0;
}

#endif /* SIGTK_AMD_SEGOPT_H */
