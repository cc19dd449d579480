/* blow5.h -- minimal BLOW5 / text SLOW5 reader of the sigtk-amd host CLI.
 *
 * Written from the on-disk layout; the reference reads the same files
 * through slow5lib (slow5_open / slow5_get_next / slow5_get, slow5lib/include/slow5/slow5.h:345-454).
 * Binary BLOW5: record compression none/zlib/zstd (the zstd frames are decoded by zstd_dec.c, written from
 * the format: no libzstd) and signal compression none/svb-zd.  Text SLOW5 (b5_file_t::text; taken from the
 * ".slow5" extension or the first bytes): one record per line, the eight main columns in order, the
 * signal column handed on as text (b5_view_t::signal) for the GPU parser or b5_sigtext_decode.
 * Auxiliary fields are skipped in both. */
#ifndef SGK_BLOW5_H
#define SGK_BLOW5_H

#include <stdint.h>
#include <stdio.h>

typedef struct {
    char *read_id;
    uint32_t read_group;
    double digitisation, offset, range, sampling_rate;
    uint64_t len_raw_signal;
    int16_t *raw_signal; /* capacity grows; reused across b5_next calls like slow5_rec_t */
    uint64_t cap_signal;
    uint8_t *buf;        /* scratch for the (de)compressed record */
    uint64_t cap_buf;
    uint8_t *zbuf;
    uint64_t cap_zbuf;
} b5_rec_t;

typedef struct {
    char *id;
    uint64_t offset; /* file offset of the u64 record size (text: of the line) */
    uint64_t size;   /* 8 + record bytes (what the reference's .idx stores; text: the line with its newline) */
} b5_idx_entry_t;

typedef struct {
    FILE *fp;
    char *path;
    uint8_t version[3];
    uint8_t record_press; /* 0 none, 1 zlib, 2 zstd */
    uint8_t signal_press; /* 0 none, 1 svb-zd */
    uint32_t num_read_groups;
    char *hdr_text;       /* header text block */
    uint32_t hdr_size;    /* its length; the file starts with 68 fixed bytes followed by it */
    uint64_t first_rec;   /* file offset of the first record */
    b5_idx_entry_t *idx;  /* built lazily by b5_index (sorted by id) */
    uint64_t n_idx;
    int idx_from_disk;    /* the index was loaded from "<file>.idx" (checked against what it points at) */
    const uint8_t *map;   /* the whole file mapped read-only (b5_map), or NULL */
    uint64_t map_len, map_pos;
    char *line;           /* text: the line read last (b5_next / b5_next_raw / b5_get*) */
    uint64_t line_cap;
    int text;             /* a text SLOW5 file: hdr_text holds its @attr, types and names lines, a record is a line */
} b5_file_t;

#define B5_EOF (-1)
#define B5_ERR_IO (-2)
#define B5_ERR_FORMAT (-3)
#define B5_ERR_PRESS (-4)
#define B5_ERR_MEM (-5)
#define B5_ERR_NOTFOUND (-6)

b5_file_t *b5_open(const char *path);
void b5_close(b5_file_t *f);
/* value of header attribute `name` for read group `rg`, or NULL (malloc'd; caller frees) */
char *b5_hdr_get(const b5_file_t *f, const char *name, uint32_t rg);
/* next record in file order: 0 ok, B5_EOF at the proper end, other negatives on error */
int b5_next(b5_file_t *f, b5_rec_t *rec);
/* the read-id index: loaded from "<file>.idx" (the reference's on-disk index, slow5lib/src/slow5_idx.c) when that
 * exists and matches the file, else built by one sequential scan and written there (best effort) */
int b5_index(b5_file_t *f);
/* random access by read id (needs b5_index) */
int b5_get(b5_file_t *f, const char *read_id, b5_rec_t *rec);
void b5_rec_free(b5_rec_t *rec);

/* ---- split API for the pipelined reader --------------------------------------
 * One thread pulls the records' bytes off the file in order (b5_next_raw / b5_get_raw); any number
 * of threads then inflate + parse them (b5_parse_raw, re-entrant) -- the split slow5lib's compiled-out
 * batch API makes between slow5_get_next_mem and slow5_rec_depress_parse (slow5_mt.c:252-317). */
typedef struct {
    const char *read_id;  /* NOT NUL-terminated: id_len bytes inside the parsed record */
    uint16_t id_len;
    uint32_t read_group;
    double digitisation, offset, range, sampling_rate;
    const uint8_t *rec;    /* the whole (inflated) record and its length: qts rewrites the signal and keeps the rest */
    uint64_t rec_len;
    const uint8_t *signal; /* svb-zd blob (signal_press 1), little-endian int16 samples, or (text) the raw_signal column */
    uint64_t signal_bytes;
    uint32_t n_samples;    /* from the blob's count word, or signal_bytes / 2; text: len_raw_signal as the record announces it */
    uint32_t signal_offset; /* of the signal inside the inflated record (b5_parse_head: `rec` / `signal` are NULL there) */
} b5_view_t;

/* appends the next record's on-disk bytes (without the u64 size; text: the line with its newline) to *buf at *len
 * (realloc'd as needed); *size receives their length.  0 ok, B5_EOF, or an error. */
int b5_next_raw(b5_file_t *f, uint8_t **buf, uint64_t *len, uint64_t *cap, uint64_t *size);
int b5_get_raw(b5_file_t *f, const char *read_id, uint8_t **buf, uint64_t *len, uint64_t *cap, uint64_t *size);
/* Zero-copy variant of b5_next_raw: maps the file once (b5_map; returns non-zero if that is not possible, the
 * caller then stays with b5_next_raw) and hands out pointers into the mapping, valid until b5_close.  The pages
 * are first touched by whoever parses the record, i.e. by the thread pool rather than by the reader. */
int b5_map(b5_file_t *f);
int b5_next_ref(b5_file_t *f, const uint8_t **ptr, uint64_t *size);
/* inflates (if the file uses zlib records) into *scratch (realloc'd as needed) and parses; the view points
 * into *scratch or into raw.  Re-entrant: touches no state of f besides its compression settings. */
int b5_parse_raw(const b5_file_t *f, const uint8_t *raw, uint64_t size, uint8_t **scratch, uint64_t *scratch_cap,
                 b5_view_t *out);
/* The HEAD of a zlib- or zstd-compressed record only: inflates just far enough (into *scratch) for the id, the scaling, the signal's
 * byte length and -- svb-zd -- its sample count; the view's read_id points into *scratch, rec / signal are NULL,
 * signal_offset tells where the signal starts in the inflated record.  A small part of the whole inflate: the record
 * itself is inflated on the GPU (sgk_job_begin_zrec).  For a zstd record that part is the first block's Huffman and FSE
 * tables, the first 512 literals and the first sequences (zsd_decode_head): some 16 us against 1 ms for the whole record
 * of a 100 000-sample read.  Files with compressed records only; rec_len is the content size a zstd
 * frame declares (the inflated length of the record, if the frame keeps its word) and 0 for a zlib record. */
int b5_parse_head(const b5_file_t *f, const uint8_t *raw, uint64_t size, uint8_t **scratch, uint64_t *scratch_cap,
                  b5_view_t *out);
/* Text files, `qts`: the line of a parsed record (b5_parse_raw's view) up to its raw_signal column as the reference
 * writes it back, into *buf (realloc'd as needed): read_id, read_group and len_raw_signal as they stand, digitisation,
 * offset, range and sampling_rate re-printed the way slow5lib prints a double ("%f" without its trailing zeros and
 * without the point when nothing follows it, "-0" as "0"; slow5_misc.c:379-406), every column with its tab.  What
 * follows the column -- v->rec + v->signal_offset + v->signal_bytes up to v->rec + v->rec_len, the auxiliary columns --
 * is written back as it stands.  Returns the byte count, or a negative error.  Re-entrant. */
int64_t b5_s5_qts_head(const b5_view_t *v, uint8_t **buf, uint64_t *cap);
/* bytes of a record's auxiliary fields when all of them are primitive (fixed size), else -1 (an array field, an unknown
 * type): with a fixed size the inflated length of a record follows from its head */
int64_t b5_aux_fixed_bytes(const b5_file_t *f);
/* The auxiliary columns of the header's type line as a table, one entry per column in header order (malloc'd into *out;
 * caller frees; NULL for none).  A type ending in '*' is an array of its element type ("char*": 1-byte elements,
 * "enum{..}*" too), an enum is 1 byte.  Returns the number of columns, or -1 for no table: no type line, fewer than the
 * eight primary columns, an unknown type name, out of memory. */
typedef struct {
    uint8_t elem_bytes; /* 1, 2, 4 or 8 */
    uint8_t is_array;
} b5_aux_field_t;
int64_t b5_aux_fields(const b5_file_t *f, b5_aux_field_t **out);
/* Room for the inflated record of a head-parsed view (b5_parse_head), for whoever inflates the record elsewhere.  A zstd
 * frame declares its content size: that is the room, exactly.  A zlib stream does not: head + signal + aux_fixed (the
 * bytes of the fixed-size columns) + for each of the n_aux_arrays array columns its u64 count and aux_slack bytes.
 * raw_size: the record's on-disk bytes.  Returns the room, or B5_ERR_FORMAT where a size does not fit 32 bits or the
 * signal ends behind the room. */
int64_t b5_zrec_room(const b5_file_t *f, const b5_view_t *v, uint64_t raw_size, uint64_t aux_fixed, uint32_t n_aux_arrays,
                     uint64_t aux_slack);
/* scalar streamvbyte + zigzag-delta decode of one blob into dst[count] (host-decode fallback path) */
int b5_svb_zd_decode(const uint8_t *blob, uint64_t nbytes, int16_t *dst, uint32_t count);
/* scalar parse of a text SLOW5 raw_signal column (nbytes of text, no tab or newline) into dst[count]: the grammar of
 * the GPU parser (sgk_sigtext_decode) -- tokens 0 | -?[1-9][0-9]{0,4} in [-32768, 32767] separated by ',', an empty
 * text exactly when count is 0.  0, or B5_ERR_PRESS for a malformed token or a token count other than `count`;
 * nothing is written behind dst[count - 1]. */
int b5_sigtext_decode(const uint8_t *text, uint64_t nbytes, int16_t *dst, uint32_t count);

#endif
