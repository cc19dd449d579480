/* ss.h -- `sigtk-amd ss paf2tsv`: PAF reader (the reference's strtok field rules), the scalar ss decoder, the subcommand. */
#ifndef SIGTK_AMD_SS_H
#define SIGTK_AMD_SS_H

#include <stddef.h>
#include <stdint.h>

#include "sigtk_gpu.h"

/* ---- one PAF line (src/ss.c:40-115).  Fields are maximal runs of bytes other than '\t', '\r', '\n' (an empty field
 * vanishes); a NUL byte ends the line, as it does for strtok.  The line is cut up in place: rid and ss point into it. */
typedef struct {
    char *rid;
    size_t rid_len;
    char *ss; /* behind "ss:Z:" of the last such field */
    size_t ss_len;
    int32_t start_raw, end_raw, tlen, start_kmer, end_kmer;
} paf_rec_t;
enum { PAF_OK = 0, PAF_FEW_FIELDS, PAF_STRAND, PAF_NUMBER, PAF_NEGATIVE, PAF_NO_TAG };
/* PAF_OK or the first rule the line breaks; *col: the 1-based column of a PAF_NUMBER / PAF_NEGATIVE */
int paf_parse_line(char *line, size_t len, paf_rec_t *out, int *col);

/* ---- the grammar of sgk_ss_decode (include/sigtk_gpu.h) as a scalar loop, same statuses and ends.  Pairs of k-mers
 * st_k + first .. st_k + first + count go to pairs[2 j], pairs[2 j + 1] (filled with -1 by the caller); count may be 0. */
uint32_t ss_decode_host(const char *ss, size_t len, const sgk_ss_record_t *rec, uint32_t first, uint32_t count,
                        int32_t *pairs, int32_t ends[2]);

int ssmain(int argc, char *argv[]);

#endif
