/* pipeline.c -- reader, loader and writer of the per-record subtools over the jobs of the GPU library (sgk_job_*,
 * include/sigtk_gpu.h); the picture is in pipeline.h */
#include "pipeline.h"

static void batch_add_record(batch_t *b, uint64_t size, const uint8_t *ref) {
    if (b->n == b->cap) {
        const uint32_t nc = b->cap ? b->cap * 2 : 1024;
        GROW(b->recs, nc);
        GROW(b->lengths, nc);
        GROW(b->blob_bytes, nc);
        GROW(b->sig_off, nc);
        GROW(b->sig_len, nc);
        GROW(b->room, nc);
        memset(b->recs + b->cap, 0, sizeof(lrec_t) * (nc - b->cap));
        b->cap = nc;
    }
    b->recs[b->n].raw_off = b->raw_len - size;
    b->recs[b->n].raw_size = size;
    b->recs[b->n].raw_ptr = ref;
    b->bytes += size;
    b->n++;
}

/* phase 1 (parallel): inflate + parse record i */
typedef struct {
    pipe_t *P;
    batch_t *b;
    int zrec;   /* parse the head only (batch_launch of a zrec file); 0: the whole record on the host (and batch_redo_host) */
} lctx_t;
static void load_parse(void *ctx_, uint32_t i, int tid) {
    (void)tid;
    lctx_t *c = (lctx_t *)ctx_;
    const pipe_t *P = c->P;
    lrec_t *r = &c->b->recs[i];
    const uint8_t *raw = r->raw_ptr ? r->raw_ptr : c->b->raw + r->raw_off;
    if (!c->zrec) {
        r->err = b5_parse_raw(P->f, raw, r->raw_size, &r->scratch, &r->scratch_cap, &r->v);
        if (!r->err && P->q_text) {   /* the line up to its signal column, as it goes back out (the parser left scratch alone) */
            const int64_t h = b5_s5_qts_head(&r->v, &r->scratch, &r->scratch_cap);
            if (h < 0) r->err = (int)h;
            else r->head_len = (uint64_t)h;
        }
        return;
    }
    /* zrec: the head only (id, scaling, sizes: a few hundred inflated bytes); the record itself is inflated on the GPU */
    r->err = b5_parse_head(P->f, raw, r->raw_size, &r->scratch, &r->scratch_cap, &r->v);
    if (r->err) return;
    /* Room for the inflated record.  A zstd frame declares its content size: that is the room, exactly.  A zlib stream
     * does not: head + signal + the fixed-size fields + for every array column its count word and a slack (a design
     * constant: ONT's array fields are a few bytes); a record whose arrays are longer comes back 0x108 and its batch is
     * redone on the host (writer_wait).  Either way the GPU checks what the record inflated to against the columns. */
    const int64_t room = b5_zrec_room(P->f, &r->v, r->raw_size, P->aux_fixed, P->n_aux_arrays, P->aux_slack);
    if (room < 0) r->err = (int)room;
    else r->room = (uint32_t)room;
}
/* phase 2 (parallel): stage record i's signal and scaling into the job's pinned buffers */
static void load_stage(void *ctx_, uint32_t i, int tid) {
    (void)tid;
    lctx_t *c = (lctx_t *)ctx_;
    batch_t *b = c->b;
    lrec_t *r = &b->recs[i];
    b->in.digitisation[i] = r->v.digitisation;
    b->in.offset[i] = r->v.offset;
    b->in.range[i] = r->v.range;
    if (b->zrec) {
        memcpy(b->in.blobs + b->in.blob_offsets[i], r->raw_ptr ? r->raw_ptr : b->raw + r->raw_off, r->raw_size);
    } else if (b->svb || b->sigtext) {
        memcpy(b->in.blobs + b->in.blob_offsets[i], r->v.signal, r->v.signal_bytes);
    } else if (c->P->f->text) {
        r->err = b5_sigtext_decode(r->v.signal, r->v.signal_bytes, b->in.samples + b->in.offsets[i], r->v.n_samples);
    } else if (c->P->f->signal_press == 1) {
        r->err = b5_svb_zd_decode(r->v.signal, r->v.signal_bytes, b->in.samples + b->in.offsets[i], r->v.n_samples);
    } else {
        memcpy(b->in.samples + b->in.offsets[i], r->v.signal, r->v.signal_bytes);
    }
    /* qts: the record around its signal (batch_frames laid the frames out; a zrec batch has no inflated record here: its
     * frames are taken on the GPU).  A text line: the re-printed head, then what follows the column and the newline */
    if (c->P->q_text || (c->P->gpu_deflate && !b->zrec)) {
        const uint8_t *tail = r->v.signal + r->v.signal_bytes;
        const size_t tl = (size_t)(r->v.rec + r->v.rec_len - tail);
        uint8_t *fr = b->fr_blob + b->fr_offs[i];
        memcpy(fr, c->P->q_text ? r->scratch : r->v.rec, b->fr_heads[i]);
        memcpy(fr + b->fr_heads[i], tail, tl);
        if (c->P->q_text) fr[b->fr_heads[i] + tl] = '\n';
    }
}

/* qts --gpu-deflate, qts on a text file: where every record's frame goes (load_stage fills them) */
static void batch_frames(batch_t *b, int text) {
    if ((uint64_t)b->n + 1 > b->fr_offs_cap) {
        b->fr_offs_cap = (uint64_t)b->n + 1;
        GROW(b->fr_offs, b->fr_offs_cap);
        GROW(b->fr_heads, b->fr_offs_cap);
    }
    uint64_t o = 0;
    for (uint32_t i = 0; i < b->n; i++) {
        const b5_view_t *v = &b->recs[i].v;
        /* up to the u64 len_raw_signal; text: the head load_parse made, and a newline behind the tail */
        const uint64_t head = text ? b->recs[i].head_len : (uint64_t)(v->signal - v->rec) - 8;
        b->fr_offs[i] = (uint32_t)o;
        b->fr_heads[i] = (uint32_t)head;
        o += head + (uint64_t)(v->rec + v->rec_len - (v->signal + v->signal_bytes)) + (text ? 1u : 0u);
        if (o > 0xffffffffull) {
            ERROR("qts", "%s", "the records of one batch hold more than 4 GB around their signals: use a smaller --batch-samples");
            die_now();
        }
    }
    b->fr_offs[b->n] = (uint32_t)o;
    if (o + 1 > b->fr_blob_cap) {
        b->fr_blob_cap = o + o / 8 + 64;
        GROW(b->fr_blob, b->fr_blob_cap);
    }
}

/* --gpu-text: the ids travel with the batch; the job hands back the rows as the reference prints them */
static void batch_set_ids(batch_t *b) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < b->n; i++) total += b->recs[i].v.id_len;
    if (total > 0xffffffffull) {
        ERROR("cmain", "%s", "the read ids of one batch exceed 4 GB: use a smaller --batch-samples");
        die_now();
    }
    if ((uint64_t)b->n + 1 > b->id_offs_cap) GROW(b->id_offs, b->id_offs_cap = (uint64_t)b->n + 1);
    if (total + 1 > b->id_blob_cap) GROW(b->id_blob, b->id_blob_cap = total + 1);
    uint32_t o = 0;
    for (uint32_t i = 0; i < b->n; i++) {
        b->id_offs[i] = o;
        memcpy(b->id_blob + o, b->recs[i].v.read_id, b->recs[i].v.id_len);
        o += (uint32_t)b->recs[i].v.id_len;
    }
    b->id_offs[b->n] = o;
    const int rc = sgk_job_set_ids(b->job, b->id_blob, b->id_offs);
    if (rc != SGK_OK) gpu_fail(NULL, "sgk_job_set_ids", rc);
}

/* the staged batch to its subtool */
static void batch_submit(pipe_t *P, batch_t *b) {
    int flags = P->tool->mode == MODE_EVENT && P->opt.compact ? SGK_JOB_EVENTS_LENGTHS : 0, rc;
    if (P->gpu_text) {
        batch_set_ids(b);
        flags |= SGK_JOB_TEXT;
    }
    if (P->tool->mode == MODE_QTS) {
        /* --gpu-inflate (b->zrec): head and tail of every record are read where the GPU inflated it; else the frames go up */
        if (((P->gpu_deflate && !b->zrec) || P->q_text) && (rc = sgk_job_set_record_frames(b->job, b->fr_blob, b->fr_offs, b->fr_heads)) != SGK_OK)
            gpu_fail(NULL, "sgk_job_set_record_frames", rc);
        const int out_fmt = P->q_text ? SGK_SIGNAL_TEXT : (P->f->signal_press == 1 ? SGK_SIGNAL_SVBZD : SGK_SIGNAL_INT16);
        rc = sgk_job_submit_qts(b->job, P->q_bits, P->q_method, out_fmt | (P->gpu_deflate || P->q_text ? SGK_QTS_RECORDS : 0) |
                                                                   (b->zrec ? SGK_QTS_ZREC_FRAMES : 0));
    } else
        rc = sgk_job_submit(b->job, P->tool->sgk_tool, P->opt.rna, P->opt.pore, flags);
    if (rc != SGK_OK) gpu_fail(NULL, "sgk_job_submit", rc);
}

/* the parsed batch, its svb / sigtext / zrec set: begin the job, stage every record on the pool, submit */
static void batch_stage_submit(pipe_t *P, batch_t *b, pool_t *pool, lctx_t *c) {
    int rc;
    /* (signal_press 0: the inflated records hold plain samples, moved into the sample arena on the GPU) */
    if (b->zrec) rc = sgk_job_begin_zrec_signal(b->job, b->n, P->f->record_press == 2 ? SGK_RECORD_ZSTD : SGK_RECORD_ZLIB, P->f->signal_press == 1 ? SGK_SIGNAL_SVBZD : SGK_SIGNAL_INT16, b->lengths, b->blob_bytes, b->sig_off, b->sig_len, b->room, P->aux_tab, P->n_aux, &b->in);
    else rc = sgk_job_begin(b->job, b->n, b->lengths, b->sigtext ? SGK_SIGNAL_TEXT : (b->svb ? SGK_SIGNAL_SVBZD : SGK_SIGNAL_INT16), b->blob_bytes, &b->in);
    if (rc != SGK_OK) gpu_fail(NULL, "sgk_job_begin", rc);
    if ((P->gpu_deflate && !b->zrec) || P->q_text) batch_frames(b, P->q_text);
    pfor(pool, b->n, load_stage, c);
    for (uint32_t i = 0; i < b->n; i++)
        if (b->recs[i].err) die_read_error(b->recs[i].err);
    batch_submit(P, b);
}

/* parse + stage + submit the records gathered in b */
static void batch_launch(pipe_t *P, batch_t *b) {
    lctx_t c = {P, b, P->zrec};
    double t0 = realtime();
    pfor(P->load_pool, b->n, load_parse, &c);
    for (uint32_t i = 0; i < b->n; i++) {
        if (b->recs[i].err) die_read_error(b->recs[i].err);
        if (P->f->text && (b->recs[i].v.signal_bytes > 0xffffffffull || b->recs[i].v.n_samples > 0x7fffffffu))
            die_read_error(B5_ERR_FORMAT);
        b->lengths[i] = b->recs[i].v.n_samples;
        b->blob_bytes[i] = P->zrec ? (uint32_t)b->recs[i].raw_size : (uint32_t)b->recs[i].v.signal_bytes;
        if (P->zrec) {
            b->sig_off[i] = b->recs[i].v.signal_offset;
            b->sig_len[i] = (uint32_t)b->recs[i].v.signal_bytes;
            b->room[i] = b->recs[i].room;
        }
        P->n_samples += b->recs[i].v.n_samples;
    }
    P->n_reads += b->n;
    double t1 = realtime();
    P->t_parse += t1 - t0;
    b->svb = P->f->signal_press == 1 && !P->host_decode;
    b->sigtext = P->f->text && !P->host_decode;
    b->zrec = P->zrec;
    batch_stage_submit(P, b, P->load_pool, &c);
    P->t_stage += realtime() - t1;
    if (P->times->t_first_submit == 0.0) P->times->t_first_submit = realtime();
    q_push(&P->ready_q, &b->link);
}

/* A zrec batch of a zlib file with array columns came back with nothing but 0x108: records that inflate to more than
 * their room, i.e. an array longer than the slack (or a broken record, which then gets the host path's error).  The
 * batch's records are still where the reader put them: inflate and parse them on the host, stage their svb-zd blobs (or
 * their samples, when the signal is not compressed), submit and wait again -- in the writer, so the file's order is kept. */
static int batch_redo_host(pipe_t *P, batch_t *b, pool_t *pool) {
    lctx_t c = {P, b, 0};
    pfor(pool, b->n, load_parse, &c);
    for (uint32_t i = 0; i < b->n; i++) {
        if (!b->recs[i].err && b->recs[i].v.n_samples != b->lengths[i]) b->recs[i].err = B5_ERR_FORMAT;
        if (b->recs[i].err) die_read_error(b->recs[i].err);
        b->blob_bytes[i] = (uint32_t)b->recs[i].v.signal_bytes;
    }
    b->zrec = 0;
    b->svb = P->f->signal_press == 1;
    batch_stage_submit(P, b, pool, &c);   /* (qts --gpu-inflate: the frames from the host's inflated records after all) */
    P->n_redone++;
    return sgk_job_wait(b->job);
}

/* ------------------------------------------------------------------ writer */

typedef struct {
    pipe_t *P;
    batch_t *b;
    sgk_job_output_t out;
    sbuf_t *chunk;          /* one buffer per chunk of reads */
    uint32_t *chunk_lo;     /* n_chunks + 1 */
    uint32_t chunk_cap;
    int wthreads;
    pool_t *wpool;
} wctx_t;

static void write_chunk(void *ctx_, uint32_t k, int tid) {
    (void)tid;
    wctx_t *c = (wctx_t *)ctx_;
    sbuf_t *o = &c->chunk[k];
    o->n = 0;
    const row_fn row = c->P->tool->row;
    for (uint32_t r = c->chunk_lo[k]; r < c->chunk_lo[k + 1]; r++) row(o, c->P, c->b, &c->out, r);
}

static void write_or_die(const pipe_t *P, const void *p, size_t n) {
    if (n && fwrite(p, 1, n, P->out_fp) != n) {
        ERROR("writer", "%s", "write to the output failed");
        die_now();
    }
}

/* the batch's job has finished, or the program ends: a zrec batch that only ran out of room is redone on the host, a
 * record or signal the GPU could not take apart is the reference's read error */
static void writer_wait(wctx_t *c) {
    pipe_t *P = c->P;
    batch_t *b = c->b;
    int rc = sgk_job_wait(b->job);
    const int was_zrec = b->zrec;
    if (rc == SGK_ERR_FORMAT && b->zrec && P->f->record_press == 1 && P->n_aux_arrays > 0) {
        sgk_job_output_t o;
        int only_room = sgk_job_output(b->job, &o) == SGK_OK && o.decode_status != NULL;
        for (uint32_t r = 0; only_room && r < b->n; r++) only_room = o.decode_status[r] == 0 || o.decode_status[r] == 0x108u;
        if (only_room) rc = batch_redo_host(P, b, c->wpool);
    }
    /* a record that does not inflate (or not to what its head announced), a blob that does not decode, or a text
     * signal column with a malformed token or another number of tokens than the record announces: what the
     * reference reports for it (slow5_get_next's negative return, src/cmain.c:121-124) */
    if (rc == SGK_ERR_FORMAT && (was_zrec || b->sigtext)) die_read_error(B5_ERR_PRESS);
    if (rc != SGK_OK) gpu_fail(NULL, "sgk_job_wait", rc);
    if (b->zrec) P->n_zrec_reads += b->n;
    P->n_long_declined += sgk_job_long_declined(b->job);
    rc = sgk_job_output(b->job, &c->out);
    if (rc != SGK_OK) gpu_fail(NULL, "sgk_job_output", rc);
}

/* the batch's rows (qts on a text file: its lines) arrived as text: one buffered write, nothing to format */
static void writer_text(wctx_t *c, double t1) {
    pipe_t *P = c->P;
    sgk_job_text_t tx;
    const int rc = sgk_job_text(c->b->job, &tx);
    if (rc != SGK_OK) gpu_fail(NULL, "sgk_job_text", rc);
    write_or_die(P, tx.text, tx.n_bytes);
    P->text_bytes += tx.n_bytes;
    P->t_write += realtime() - t1;
}

/* rows formatted here: contiguous chunks of reads with about equal sample counts; a few per thread for balance */
static void writer_rows(wctx_t *c, double t1) {
    pipe_t *P = c->P;
    const batch_t *b = c->b;
    uint32_t nchunks = (uint32_t)c->wthreads * 4;
    if (nchunks > b->n) nchunks = b->n;
    if (nchunks > c->chunk_cap) {
        GROW(c->chunk, nchunks);
        GROW(c->chunk_lo, (size_t)nchunks + 1);
        memset(c->chunk + c->chunk_cap, 0, sizeof(sbuf_t) * (nchunks - c->chunk_cap));
        c->chunk_cap = nchunks;
    }
    uint64_t total = 0;
    for (uint32_t r = 0; r < b->n; r++) total += b->lengths[r] + 64;
    uint64_t acc = 0;
    uint32_t k = 0;
    c->chunk_lo[0] = 0;
    for (uint32_t r = 0; r < b->n && k + 1 < nchunks; r++) {
        acc += b->lengths[r] + 64;
        if (acc * nchunks >= total * (uint64_t)(k + 1)) c->chunk_lo[++k] = r + 1;
    }
    while (k < nchunks) c->chunk_lo[++k] = b->n;
    pfor(c->wpool, nchunks, write_chunk, c);
    const double t2 = realtime();
    P->t_format += t2 - t1;
    for (uint32_t i = 0; i < nchunks; i++) write_or_die(P, c->chunk[i].p, c->chunk[i].n);
    P->t_write += realtime() - t2;
}

static void batch_recycle(pipe_t *P, batch_t *b) {
    b->n = 0;
    b->raw_len = 0;
    b->bytes = 0;
    q_push(&P->free_q, &b->link);
}

static void *writer_main(void *arg) {
    pipe_t *P = (pipe_t *)arg;
    wctx_t c;
    memset(&c, 0, sizeof c);
    c.P = P;
    c.wthreads = P->nthreads > 32 ? 32 : P->nthreads;  /* formatting is light: fewer threads */
    c.wpool = pool_create(c.wthreads);
    for (;;) {
        c.b = (batch_t *)q_pop(&P->ready_q);
        if (c.b->last) break;
        const double t0 = realtime();
        writer_wait(&c);
        const double t1 = realtime();
        P->t_wait += t1 - t0;
        if (P->gpu_text || P->q_text) writer_text(&c, t1);
        else writer_rows(&c, t1);
        batch_recycle(P, c.b);
    }
    pool_destroy(c.wpool);
    for (uint32_t i = 0; i < c.chunk_cap; i++) free(c.chunk[i].p);
    free(c.chunk);
    free(c.chunk_lo);
    return NULL;
}

/* a new job takes the command line's parameters: event --detector, jnn --segmenter, prefix --adaptor / --polya,
 * pa --normalise */
static void job_create(const pipe_t *P, int k, batch_t *b) {
    int rc = sgk_job_create(k % P->n_gpus, &b->job);
    if (rc != SGK_OK) gpu_fail(NULL, "sgk_job_create", rc);
    if (P->ev_params && (rc = sgk_job_set_event_params(b->job, P->ev_params)) != SGK_OK) gpu_fail(NULL, "sgk_job_set_event_params", rc);
    if (P->jnn_params && (rc = sgk_job_set_jnn_params(b->job, P->jnn_params)) != SGK_OK) gpu_fail(NULL, "sgk_job_set_jnn_params", rc);
    if (P->prefix_params && (rc = sgk_job_set_prefix_params(b->job, P->prefix_params)) != SGK_OK)
        gpu_fail(NULL, "sgk_job_set_prefix_params", rc);
    if (P->normalise && (rc = sgk_job_set_normalise(b->job, P->normalise)) != SGK_OK) gpu_fail(NULL, "sgk_job_set_normalise", rc);
}

/* ------------------------------------------------------------------ reader thread
 * Pulls the records' bytes off the file (sequentially, or by read id) into free batches and hands each full batch
 * to the loader, so that file reads overlap with inflating / staging the previous batch. */
/* the reader's next empty batch: a free one, else a new one if the input has earned it, else wait */
static batch_t *take_free_batch(pipe_t *P) {
    batch_t *b = (batch_t *)q_try_pop(&P->free_q);
    if (!b && P->n_created < P->n_max && P->batches_read >= 4u * (uint64_t)P->n_created) {
        b = &P->pool[P->n_created];
        job_create(P, P->n_created, b);
        P->n_created++;
    }
    if (!b) b = (batch_t *)q_pop(&P->free_q);
    P->batches_read++;
    return b;
}
/* the record just read joins b; a full batch goes to the loader */
static batch_t *reader_add(pipe_t *P, batch_t *b, uint64_t size, const uint8_t *ref) {
    batch_add_record(b, size, ref);
    if (b->bytes < P->limit_bytes) return b;
    q_push(&P->filled_q, &b->link);
    return take_free_batch(P);
}

static void *reader_main(void *arg) {
    pipe_t *P = (pipe_t *)arg;
    b5_file_t *f = P->f;
    batch_t *b = take_free_batch(P);
    int ret = 0;
    if (P->n_ids == 0) {
        const int mapped = b5_map(f) == 0;  /* zero-copy: the pool touches the pages when it inflates the records */
        for (;;) {
            uint64_t size = 0;
            const uint8_t *ref = NULL;
            const double t0 = realtime();
            ret = mapped ? b5_next_ref(f, &ref, &size) : b5_next_raw(f, &b->raw, &b->raw_len, &b->raw_cap, &size);
            P->t_read += realtime() - t0;
            if (ret < 0) break;
            b = reader_add(P, b, size, ref);
        }
        if (ret != B5_EOF) die_read_error(ret);
    } else {
        if (b5_index(f) < 0) {
            ERROR("cmain", "Error loading index file for %s", f->path);
            die_now();
        }
        for (int i = 0; i < P->n_ids; i++) {
            fprintf(stderr, "Read ID %s\n", P->ids[i]);
            uint64_t size = 0;
            if (b5_get_raw(f, P->ids[i], &b->raw, &b->raw_len, &b->raw_cap, &size) < 0) {
                ERROR("cmain", "%s", "Error when fetching the read");
                die_now();
            }
            b = reader_add(P, b, size, NULL);
        }
    }
    b->last = 1;  /* the final (possibly empty) batch ends the stream */
    q_push(&P->filled_q, &b->link);
    return NULL;
}

/* ------------------------------------------------------------------ the pipeline driver */

static void report_timing(const pipe_t *P, double t_init, double t_jobs) {
    fprintf(stderr,
            "[sigtk-amd] %lu reads, %lu samples, %d threads, %d GPU(s): read %.3f s, inflate+parse %.3f s, "
            "stage+submit %.3f s | wait-for-GPU %.3f s, format %.3f s, write %.3f s | HIP init %.3f s, job create %.3f s\n",
            (unsigned long)P->n_reads, (unsigned long)P->n_samples, P->nthreads, P->n_gpus, P->t_read, P->t_parse,
            P->t_stage, P->t_wait, P->t_format, P->t_write, t_init, t_jobs);
    if (P->gpu_text)
        fprintf(stderr, "[sigtk-amd] --gpu-text: %lu bytes of rows over PCIe (formatted on the GPU; no pA floats / event arrays)\n",
                (unsigned long)P->text_bytes);
    fprintf(stderr, "[sigtk-amd] records decompressed on the GPU: %lu of %lu; batches redone on the host: %lu\n",
            (unsigned long)P->n_zrec_reads, (unsigned long)P->n_reads, (unsigned long)P->n_redone);
}

static void batch_free(batch_t *b) {
    sgk_job_destroy(b->job);
    for (uint32_t k = 0; k < b->cap; k++) free(b->recs[k].scratch);
    free(b->recs); free(b->raw); free(b->lengths); free(b->blob_bytes); free(b->sig_off); free(b->sig_len); free(b->room);
    free(b->id_blob); free(b->id_offs);
    free(b->fr_blob); free(b->fr_offs); free(b->fr_heads);
}

void run_pipeline(pipe_t *P, double t_init) {
    q_init(&P->free_q);
    q_init(&P->filled_q);
    q_init(&P->ready_q);
    /* Up to n_gpus + 3 batches (one being read, one being inflated/staged, n_gpus in flight, one being written),
     * but only two to begin with: a job's pinned and device buffers cost tens of milliseconds to set up, which a
     * small input never earns back.  The reader adds a batch when it would otherwise wait and the input has
     * already run to several batches per existing one (take_free_batch). */
    const int nbatch = P->n_gpus + 3;
    batch_t *pool = (batch_t *)calloc((size_t)nbatch + 1, sizeof(batch_t));
    if (!pool) die_mem();
    const double t_jobs0 = realtime();
    P->pool = pool;
    P->n_max = nbatch;
    P->n_created = nbatch < 2 ? nbatch : 2;
    for (int i = 0; i < P->n_created; i++) {
        job_create(P, i, &pool[i]);
        q_push(&P->free_q, &pool[i].link);
    }
    const double t_jobs = realtime() - t_jobs0;
    P->load_pool = pool_create(P->nthreads);
    pthread_t wth, rth;
    if (pthread_create(&wth, NULL, writer_main, P) != 0 || pthread_create(&rth, NULL, reader_main, P) != 0) {
        ERROR("cmain", "%s", "cannot create the pipeline threads");
        die_now();
    }
    /* loader: inflate/parse, stage and submit every filled batch */
    for (;;) {
        batch_t *b = (batch_t *)q_pop(&P->filled_q);
        const int last = b->last;
        b->last = 0;
        if (b->n) batch_launch(P, b);
        else q_push(&P->free_q, &b->link);
        if (last) break;
    }
    pthread_join(rth, NULL);
    pool[nbatch].last = 1;
    q_push(&P->ready_q, &pool[nbatch].link);
    pthread_join(wth, NULL);
    pool_destroy(P->load_pool);
    P->times->t_pipeline_end = realtime();
    if (P->n_long_declined)
        WARNING("pipeline", "%lu long read(s) were declined by the long-read path (a barrier wait timed out) and redone on one "
                "wavefront each; the output is unaffected", (unsigned long)P->n_long_declined);
    if (getenv("SGK_CLI_TIMING")) report_timing(P, t_init, t_jobs);
    /* The process is about to leave through _exit (main): the jobs' pinned and device buffers go with it.  Releasing
     * them one hipHostFree / hipFree at a time costs more than a small input's whole pipeline (SGK_CLI_TIMING shows
     * it), so they are only released when asked to (leak checkers: SGK_CLI_FREE=1). */
    if (getenv("SGK_CLI_FREE")) {
        for (int i = 0; i < P->n_created; i++) batch_free(&pool[i]);
        free(pool);
    }
    P->times->t_destroyed = realtime();
}

int pipe_zrec_setup(pipe_t *P, uint64_t aux_slack) {
    const b5_file_t *f = P->f;
    b5_aux_field_t *tab = NULL;
    const int64_t n_tab = b5_aux_fields(f, &tab);
    for (int64_t k = 0; k < n_tab; k++) {
        if (tab[k].is_array) P->n_aux_arrays++;
        else P->aux_fixed += tab[k].elem_bytes;
    }
    if (n_tab > 0) {
        GROW(P->aux_tab, n_tab);
        for (int64_t k = 0; k < n_tab; k++) {
            P->aux_tab[k].elem_bytes = tab[k].elem_bytes;
            P->aux_tab[k].is_array = tab[k].is_array;
        }
    }
    free(tab);
    P->n_aux = n_tab > 0 ? (uint32_t)n_tab : 0;
    P->aux_slack = aux_slack;
    return !f->text && (f->record_press == 1 || f->record_press == 2) && n_tab >= 0;
}
