/* zrec_raw_check FILE SLACK -- what the CLI's record path does on the host for a BLOW5 file whose records are compressed
 * and whose signal is not (signal_press 0), without a GPU, for sanitizer builds: every record's head parsed
 * (b5_parse_head), its room computed (b5_zrec_room) from the header's column table, then the whole record inflated
 * (b5_parse_raw) to see what the GPU would find there -- the samples plain int16 at signal_offset, twice as many bytes as
 * samples, the length word in front of them the sample count.  Prints one line per file: records, records that fit their
 * room, samples, and a sum over all samples (so that two files with the same reads print the same line).
 * Exit status 0 when every check holds, 1 on a failed check, 2 on usage / file errors. */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "blow5.h"

#define CHECK(c)                                                                            \
    do {                                                                                    \
        if (!(c)) {                                                                         \
            fprintf(stderr, "record %" PRIu64 ": check failed: %s\n", n, #c);              \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    b5_file_t *f = b5_open(argv[1]);
    if (!f) return 2;
    const uint64_t slack = strtoull(argv[2], NULL, 10);
    b5_aux_field_t *tab = NULL;
    const int64_t n_tab = b5_aux_fields(f, &tab);
    if (n_tab < 0 || f->text || (f->record_press != 1 && f->record_press != 2) || f->signal_press != 0) {
        free(tab);
        b5_close(f);
        return 2;
    }
    uint64_t fixed = 0;
    uint32_t n_arrays = 0;
    for (int64_t k = 0; k < n_tab; k++) {
        if (tab[k].is_array) n_arrays++;
        else fixed += tab[k].elem_bytes;
    }
    uint8_t *raw = NULL, *s_head = NULL, *s_full = NULL;
    uint64_t raw_len = 0, raw_cap = 0, size = 0, head_cap = 0, full_cap = 0;
    uint64_t n = 0, n_fit = 0, n_samples = 0, sum = 0;
    int rc;
    while ((rc = b5_next_raw(f, &raw, &raw_len, &raw_cap, &size)) == 0) {
        const uint8_t *rec = raw + raw_len - size;
        b5_view_t h, v;
        memset(&h, 0, sizeof h);
        memset(&v, 0, sizeof v);
        CHECK(b5_parse_head(f, rec, size, &s_head, &head_cap, &h) == 0);
        CHECK(h.rec == NULL && h.signal == NULL);
        CHECK(h.signal_bytes == 2 * (uint64_t)h.n_samples);
        CHECK(h.signal_offset == 2u + h.id_len + 44u);
        const int64_t room = b5_zrec_room(f, &h, size, fixed, n_arrays, slack);
        CHECK(room >= 0);
        CHECK(b5_parse_raw(f, rec, size, &s_full, &full_cap, &v) == 0);
        /* the head told the truth about the record */
        CHECK(h.signal_offset == (uint64_t)(v.signal - v.rec) && h.signal_bytes == v.signal_bytes && h.n_samples == v.n_samples);
        CHECK(v.signal_bytes == 2 * (uint64_t)v.n_samples);
        CHECK(h.id_len == v.id_len && memcmp(h.read_id, v.read_id, v.id_len) == 0);
        CHECK(h.digitisation == v.digitisation && h.offset == v.offset && h.range == v.range);
        /* what the GPU moves: n_samples int16 at signal_offset, wholly inside the record and inside its room */
        CHECK((uint64_t)h.signal_offset + h.signal_bytes <= (uint64_t)room);
        CHECK((uint64_t)h.signal_offset + h.signal_bytes <= v.rec_len);
        uint64_t len_word;
        memcpy(&len_word, v.rec + h.signal_offset - 8, 8);
        CHECK(len_word == v.n_samples);
        if (f->record_press == 2) CHECK((uint64_t)room == v.rec_len);
        else if (n_arrays == 0) CHECK((uint64_t)room == v.rec_len);
        if (v.rec_len <= (uint64_t)room) n_fit++;
        for (uint32_t i = 0; i < v.n_samples; i++) {
            int16_t s;
            memcpy(&s, v.signal + 2 * (uint64_t)i, 2);
            sum += (uint64_t)(uint16_t)s * (i % 251u + 1u);
        }
        n_samples += v.n_samples;
        raw_len = 0;
        n++;
    }
    if (rc != B5_EOF) return 2;
    printf("%" PRIu64 " records, %" PRIu64 " fit their room, %" PRIu64 " samples, sum %" PRIu64 "\n", n, n_fit, n_samples, sum);
    free(raw);
    free(s_head);
    free(s_full);
    free(tab);
    b5_close(f);
    return 0;
}
