/* sref.h -- `sigtk-amd sref`: FASTA reader (kseq's line rules), k-mer model file reader, the subcommand. */
#ifndef SIGTK_AMD_SREF_H
#define SIGTK_AMD_SREF_H

#include <stddef.h>
#include <stdint.h>

/* ---- FASTA, plain or gzip.  The whole file is inflated into one buffer and parsed in place: names and sequences
 * point into it.  Sequence bytes are kept as they are (the device ranks them). */
typedef struct {
    const char *name; /* up to the first whitespace of the header line; not NUL-terminated */
    uint32_t name_len;
    const uint8_t *seq;
    uint64_t len;
} fa_rec_t;
typedef struct {
    uint8_t *buf;
    size_t size;
    fa_rec_t *rec;
    uint32_t n, cap;
    char err[256];
} fasta_t;
int fasta_read(const char *path, fasta_t *fa); /* 0, or -1 with fa->err set; fasta_free in both cases */
void fasta_free(fasta_t *fa);

/* ---- k-mer model file (the format of the reference's read_model, src/model.c:39-140): `#` comment lines with an
 * optional "#k\t<k>", an optional header line starting "kmer\tlevel_mean", then "KMER\tlevel_mean[\t...]" lines.
 * All 4^k k-mers exactly once, in any order.  levels: 4096 floats, filled by k-mer rank.  0, or -1 with err set. */
int model_read(const char *path, uint32_t want_k, float *levels, uint32_t *k_out, char *err, size_t err_len);

uint64_t fnv1a_bytes(const void *p, size_t n);

int srefmain(int argc, char *argv[]);
int fadumpmain(int argc, char *argv[]);     /* _fadump FILE: name, length, FNV-1a of the bytes per record */
int modelcheckmain(int argc, char *argv[]); /* _modelcheck FILE [--rna]: k, number of k-mers, FNV-1a of the table */

#endif
