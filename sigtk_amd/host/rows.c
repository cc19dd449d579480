/* rows.c -- the subtools that go through the pipeline, one table row each, and their row formatters (src/cfunc.c):
 * byte-for-byte the reference's printf output; numbers go through fmt.h. */
#include <zlib.h>

#include "fmt.h"
#include "pipeline.h"

static inline void put_id_len(sbuf_t *o, const batch_t *b, uint32_t r) {
    char *p = sbuf_room(o, (size_t)b->recs[r].v.id_len + 32);
    memcpy(p, b->recs[r].v.read_id, b->recs[r].v.id_len);
    p += b->recs[r].v.id_len;
    *p++ = '\t';
    p = fmt_u64(p, b->lengths[r]);
    *p++ = '\t';
    o->n = (size_t)(p - o->p);
}

/* print_events, cfunc.c:16-61 */
static void row_events(sbuf_t *o, const pipe_t *P, const batch_t *b, const sgk_job_output_t *out, uint32_t r) {
    const uint64_t a = out->slots[r], n = out->counts[r];
    const uint32_t *ln = out->ev_length + a;
    if (P->opt.compact) {
        /* (the job hands back the lengths alone, SGK_JOB_EVENTS_LENGTHS: the events of a read are contiguous from
         * sample 0, events.c:491-501, so event[0].start is 0 and the last event's end the sum of the lengths) */
        put_id_len(o, b, r);
        if (n) {
            uint64_t end = 0;
            for (uint64_t j = 0; j < n; j++) end += ln[j];
            char *p = sbuf_room(o, 96 + n * 12);
            p = fmt_u64(p, 0); *p++ = '\t';
            p = fmt_u64(p, end); *p++ = '\t';
            p = fmt_u64(p, n); *p++ = '\t';
            for (uint64_t j = 0; j < n; j++) {
                const int mi = (int)ln[j];
                if (mi) {
                    p = fmt_i64(p, mi);
                    if (j < n - 1) *p++ = ',';
                }
            }
            o->n = (size_t)(p - o->p);
        } else {
            sbuf_str(o, ".\t.\t.\t.", 7);
        }
        sbuf_str(o, "\n", 1);
    } else {
        const uint32_t *st = out->ev_start + a;
        const float *mean = out->ev_mean + a, *sd = out->ev_stdv + a;
        const size_t idl = b->recs[r].v.id_len;
        char *p = sbuf_room(o, n * (idl + 160) + 8);
        for (uint64_t j = 0; j < n; j++) {
            memcpy(p, b->recs[r].v.read_id, idl);
            p += idl;
            *p++ = '\t';
            p = fmt_i64(p, (int)j); *p++ = '\t';
            p = fmt_u64(p, st[j]); *p++ = '\t';
            p = fmt_u64(p, (uint64_t)st[j] + ln[j]); *p++ = '\t';
            p = fmt_f6(p, mean[j]); *p++ = '\t';
            p = fmt_f6(p, sd[j]); *p++ = '\n';
        }
        *p++ = '\n'; /* cfunc.c:58 */
        o->n = (size_t)(p - o->p);
    }
}

/* jnn_print, jnn.c:309-350 */
static void row_jnn(sbuf_t *o, const pipe_t *P, const batch_t *b, const sgk_job_output_t *out, uint32_t r) {
    put_id_len(o, b, r);
    const uint64_t len = b->lengths[r];
    if (len > 0) {
        const uint64_t a = out->slots[r], n = out->counts[r];
        const int32_t *x = out->seg_x + a, *y = out->seg_y + a;
        char *p = sbuf_room(o, 32 + n * 48);
        p = fmt_i64(p, (int)n); *p++ = '\t';
        if (P->opt.compact) {
            uint64_t ci = 0, mi = 0;
            for (uint64_t i = 0; i < n; i++) {
                ci += (mi = (uint64_t)x[i] - ci);
                if (mi) { p = fmt_i64(p, (int)mi); *p++ = 'H'; }
                ci += (mi = (uint64_t)y[i] - ci);
                if (mi) { p = fmt_i64(p, (int)mi); *p++ = ','; }
            }
        } else {
            for (uint64_t i = 0; i < n; i++) {
                p = fmt_i64(p, x[i]); *p++ = ',';
                p = fmt_i64(p, y[i]); *p++ = ';';
            }
        }
        if (n == 0) *p++ = '.';
        o->n = (size_t)(p - o->p);
    }
    sbuf_str(o, "\n", 1);
}

/* stat_func, cfunc.c:126-159 */
static void row_stat(sbuf_t *o, const pipe_t *P, const batch_t *b, const sgk_job_output_t *out, uint32_t r) {
    (void)P;
    put_id_len(o, b, r);
    const sgk_stat_rec_t *s = &out->stat[r];
    char *p = sbuf_room(o, 6 * 52);
    p = fmt_f6(p, s->raw_mean); *p++ = '\t';
    p = fmt_f6(p, s->pa_mean); *p++ = '\t';
    p = fmt_f6(p, s->raw_std); *p++ = '\t';
    p = fmt_f6(p, s->pa_std); *p++ = '\t';
    p = fmt_i64(p, (int)(int16_t)s->raw_median); *p++ = '\t';
    p = fmt_f6(p, s->pa_median); *p++ = '\t';
    *p++ = '\n';
    o->n = (size_t)(p - o->p);
}

/* prefix_func, cfunc.c:169-234 */
static void row_prefix(sbuf_t *o, const pipe_t *P, const batch_t *b, const sgk_job_output_t *out, uint32_t r) {
    put_id_len(o, b, r);
    const sgk_prefix_rec_t *q = &out->prefix[r];
    char *p = sbuf_room(o, 512);
    if (q->adapt_y > 0) {
        p = fmt_i64(p, q->adapt_x); *p++ = '\t';
        p = fmt_i64(p, q->adapt_y); *p++ = '\t';
        if (q->polya_y > 0) {
            p = fmt_i64(p, (int64_t)q->polya_x + q->adapt_y); *p++ = '\t';
            p = fmt_i64(p, (int64_t)q->polya_y + q->adapt_y);
        } else {
            memcpy(p, ".\t.", 3); p += 3;
        }
        if (P->opt.p_stat) {
            *p++ = '\t';
            p = fmt_f6(p, q->adapt_mean); *p++ = '\t';
            p = fmt_f6(p, q->adapt_std); *p++ = '\t';
            p = fmt_f6(p, q->adapt_median); *p++ = '\t';
            if (q->polya_y > 0) {
                *p++ = '\t';
                p = fmt_f6(p, q->polya_mean); *p++ = '\t';
                p = fmt_f6(p, q->polya_std); *p++ = '\t';
                p = fmt_f6(p, q->polya_median); *p++ = '\t';
            } else {
                memcpy(p, "\t.\t.\t.", 6); p += 6;
            }
        }
    } else {
        memcpy(p, ".\t.\t.\t.", 7); p += 7;
    }
    *p++ = '\n';
    o->n = (size_t)(p - o->p);
}

/* pa_func, cfunc.c:85-102 */
static void row_pa(sbuf_t *o, const pipe_t *P, const batch_t *b, const sgk_job_output_t *out, uint32_t r) {
    (void)P;
    put_id_len(o, b, r);
    const uint64_t len = b->lengths[r];
    const float *pa = out->pa + out->offsets[r];
    char *p = sbuf_room(o, len * 50 + 8);
    for (uint64_t i = 0; i < len; i++) {
        p = fmt_f6(p, pa[i]);
        if (i != len - 1) *p++ = ',';
    }
    *p++ = '\n';
    o->n = (size_t)(p - o->p);
}

/* entmain's row, ent.c:108-163: id, then "%f" of three doubles (the histograms come from the GPU, the sum over
 * the non-empty bins is sgk_ent_finish: the reference's own arithmetic in the reference's order) */
static void row_ent(sbuf_t *o, const pipe_t *P, const batch_t *b, const sgk_job_output_t *out, uint32_t r) {
    (void)P;
    double e[3];
    const uint64_t off = out->offsets[r];
    sgk_ent_finish(&out->ent[r], out->ent_over_raw ? out->ent_over_raw + off : NULL,
                   out->ent_over_delta ? out->ent_over_delta + off : NULL, e);
    char *p = sbuf_room(o, (size_t)b->recs[r].v.id_len + 3 * 330 + 8);
    memcpy(p, b->recs[r].v.read_id, b->recs[r].v.id_len);
    p += b->recs[r].v.id_len;
    p += sprintf(p, "\t%f\t%f\t%f\n", e[0], e[1], e[2]);
    o->n = (size_t)(p - o->p);
}

/* the record around its new signal: head, u64 len_raw_signal, signal, tail */
static inline void put_record(uint8_t *dst, const uint8_t *head, size_t head_len, uint64_t len_field, const uint8_t *sig,
                              size_t sig_bytes, const uint8_t *tail, size_t tail_len) {
    memcpy(dst, head, head_len);
    memcpy(dst + head_len, &len_field, 8);
    memcpy(dst + head_len + 8, sig, sig_bytes);
    memcpy(dst + head_len + 8 + sig_bytes, tail, tail_len);
}

/* qts (src/qts.c:118-150): the record as it was read, with the signal replaced by the quantised one (and
 * len_raw_signal with it); everything else -- id, read group, scaling, auxiliary fields -- is kept byte for byte.
 * Emitted as the file stores it: u64 size, then the record (one zlib stream when the file compresses records -- a file
 * of zstd records too: the output is written with zlib records, as slow5_open(out, "w") makes it in the reference,
 * slow5lib/src/slow5.c:421-423; qtsmain sets the header byte). */
static __thread uint8_t *qts_tmp;
static __thread size_t qts_tmp_cap;
static void row_qts(sbuf_t *o, const pipe_t *P, const batch_t *b, const sgk_job_output_t *out, uint32_t r) {
    if (P->gpu_deflate) {   /* --gpu-deflate: the record came back as the zlib stream the GPU wrote around the new signal */
        if (out->qts_record_status[r] != 0) {
            fprintf(stderr, "Error writing record!\n");
            die_now();
        }
        const uint64_t z64 = out->qts_record_lengths[r];
        char *p = sbuf_room(o, 8 + (size_t)z64);
        memcpy(p, &z64, 8);
        memcpy(p + 8, out->qts_records + out->qts_record_offsets[r], (size_t)z64);
        o->n += 8 + (size_t)z64;
        return;
    }
    const b5_view_t *v = &b->recs[r].v;
    const size_t head = (size_t)(v->signal - v->rec) - 8; /* up to the u64 len_raw_signal */
    const uint8_t *tail = v->signal + v->signal_bytes;
    const size_t tail_len = (size_t)(v->rec + v->rec_len - tail);
    const int svb = P->f->signal_press == 1;
    const uint8_t *sig = svb ? out->qts_blobs + out->qts_blob_offsets[r] : (const uint8_t *)(out->qts_samples + out->offsets[r]);
    const size_t sig_bytes = svb ? (size_t)out->qts_blob_lengths[r] : (size_t)b->lengths[r] * 2;
    const uint64_t len_field = svb ? sig_bytes : b->lengths[r];
    const size_t n = head + 8 + sig_bytes + tail_len;
    if (P->f->record_press != 0) {
        if (qts_tmp_cap < n) {
            qts_tmp_cap = n + n / 4 + 64;
            GROW(qts_tmp, qts_tmp_cap);
        }
        put_record(qts_tmp, v->rec, head, len_field, sig, sig_bytes, tail, tail_len);
        uLongf zlen = compressBound((uLong)n);
        char *p = sbuf_room(o, 8 + (size_t)zlen);
        if (compress2((Bytef *)p + 8, &zlen, qts_tmp, (uLong)n, Z_DEFAULT_COMPRESSION) != Z_OK) {
            ERROR("qts", "%s", "zlib compression failed");
            die_now();
        }
        const uint64_t z64 = zlen;
        memcpy(p, &z64, 8);
        o->n += 8 + (size_t)zlen;
    } else {
        char *p = sbuf_room(o, 8 + n);
        const uint64_t n64 = n;
        memcpy(p, &n64, 8);
        put_record((uint8_t *)p + 8, v->rec, head, len_field, sig, sig_bytes, tail, tail_len);
        o->n += 8 + n;
    }
}

/* ------------------------------------------------------------------ the subtools */

static const tool_t tools[] = {
    {"event", MODE_EVENT, SGK_TOOL_EVENT, row_events, 16ull << 20, "read_id\tevent_idx\traw_start\traw_end\tevent_mean\tevent_std\n",
     "read_id\tlen_raw_signal\traw_start\traw_end\tnum_event\tevents\n"},
    {"stat", MODE_STAT, SGK_TOOL_STAT, row_stat, 16ull << 20,
     "read_id\tlen_raw_signal\traw_mean\tpa_mean\traw_std\tpa_std\traw_median\tpa_median\n", NULL},
    {"prefix", MODE_PREFIX, SGK_TOOL_PREFIX, row_prefix, 64ull << 20, "read_id\tlen_raw_signal\tadapt_start\tadapt_end\tpolya_start\tpolya_end\n",
     "read_id\tlen_raw_signal\tadapt_start\tadapt_end\tpolya_start\tpolya_end\tadapt_mean\tadapt_std\tadapt_median\tpolya_mean\tpolya_std\tpolya_median\n"},
    {"jnn", MODE_JNN, SGK_TOOL_JNN, row_jnn, 64ull << 20, "read_id\tlen_raw_signal\tnum_seg\tseg\n", NULL},
    {"pa", MODE_PA, SGK_TOOL_PA, row_pa, 16ull << 20, "read_id\tlen_raw_signal\tpa\n", "read_id\tlen_raw_signal\tnorm\n"},
    {"ent", MODE_ENT, SGK_TOOL_ENT, row_ent, 16ull << 20, "read_id\traw_ent\tdelta_ent\tbyte_ent\n", NULL},
    {"qts", MODE_QTS, -1, row_qts, 16ull << 20, NULL, NULL},
};

const tool_t *tool_by_name(const char *name) {
    for (size_t i = 0; i < sizeof tools / sizeof tools[0]; i++)
        if (strcmp(name, tools[i].name) == 0) return &tools[i];
    return NULL;
}
