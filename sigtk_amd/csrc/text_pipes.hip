// text_pipes.hip -- the host pipes of `sref` and `ss paf2tsv` (sgk_sref_pipe_*, sgk_ss_pipe_*; see the header) for
// callers without device memory of their own: batches in through pinned staging, their text out.  Host code only: the
// slots, the measure -> write sequence and the busy rule are text_pipe.h, the kernels sref_kernels.hip and
// ss_kernels.hip behind the library's own entry points.
#include <string.h>

#include "text_pipe.h"

using namespace sgk;

struct sgk_sref_pipe {
    int device = 0;
    uint32_t k = 0;
    Dev<float> d_levels;
    struct Slot : TextSlot {
        uint64_t n_bases = 0;
        uint32_t n_spans = 0;
        size_t off_spans = 0, off_nbytes = 0, off_noffs = 0;  // sections of the staging behind the bases
    } slot[2];
};

struct sgk_ss_pipe {
    int device = 0;
    struct Slot : TextSlot {
        uint64_t n_ss_bytes = 0;
        uint32_t n_records = 0, n_spans = 0, n_ids = 0;
        size_t off_rec = 0, off_spans = 0, off_ids = 0, off_idoffs = 0;  // sections of the staging behind the strings
        Pair<uint32_t> status;  // per record (validate), then per kept span (decode)
        Dev<int32_t> ends;
        Pair<uint64_t> offs;    // where every kept span's pairs start
        Dev<int32_t> pairs;
        uint32_t bad_record = 0xffffffffu, bad_status = 0;
    } slot[2];
};

namespace {

int sref_submit(const sgk_sref_pipe &p, sgk_sref_pipe::Slot &S) {
    const sgk_sref_span_t *hs = reinterpret_cast<const sgk_sref_span_t *>(S.in.h.p + S.off_spans);
    uint64_t n_pos = 0;
    for (uint32_t s = 0; s < S.n_spans; ++s) n_pos += hs[s].count;
    const size_t ws_bytes = sgk_sref_text_workspace_bytes(S.n_spans, n_pos);
    SGK_TRY(S.in.up(S.in_bytes, S.stream));
    const uint8_t *d_in = S.in.d.p;
    sgk_sref_batch_t b;
    memset(&b, 0, sizeof b);
    b.bases = d_in;
    b.n_bases = S.n_bases;
    b.spans = reinterpret_cast<const sgk_sref_span_t *>(d_in + S.off_spans);
    b.n_spans = S.n_spans;
    b.levels = p.d_levels.p;
    b.k = p.k;
    const sgk_text_ids_t names = {d_in + S.off_nbytes, reinterpret_cast<const uint32_t *>(d_in + S.off_noffs)};
    return text_pipe_run(
        S, ws_bytes, S.n_spans, [&] { return sgk_sref_text_measure(&b, &names, S.rows.p, S.ws.p, ws_bytes, S.stream); },
        [&] { return sgk_sref_text_write(&b, &names, S.text.d.p, S.n_bytes, S.ws.p, ws_bytes, S.stream); });
}

int ss_submit(sgk_ss_pipe::Slot &S) {
    const sgk_ss_record_t *hr = reinterpret_cast<const sgk_ss_record_t *>(S.in.h.p + S.off_rec);
    const sgk_ss_span_t *hs = reinterpret_cast<const sgk_ss_span_t *>(S.in.h.p + S.off_spans);
    // what the caller staged must be consistent with itself before anything is sized from it
    for (uint32_t r = 0; r < S.n_records; ++r) {
        if (hr[r].ss_offset > S.n_ss_bytes || hr[r].ss_len > S.n_ss_bytes - hr[r].ss_offset) return SGK_ERR_ARG;
        if (hr[r].id >= S.n_ids || hr[r].st_k > hr[r].end_k) return SGK_ERR_ARG;
    }
    for (uint32_t s = 0; s < S.n_spans; ++s) {
        if (hs[s].record >= S.n_records || (s && hs[s].record < hs[s - 1].record)) return SGK_ERR_ARG;
        const uint64_t rows = (uint64_t)((int64_t)hr[hs[s].record].end_k - (int64_t)hr[hs[s].record].st_k);
        if ((uint64_t)hs[s].first + hs[s].count > rows) return SGK_ERR_ARG;
    }
    S.bad_record = 0xffffffffu;
    S.bad_status = 0;
    if (S.n_records == 0) return SGK_OK;
    const size_t n_st = S.n_records > S.n_spans ? S.n_records : S.n_spans;
    SGK_TRY(S.status.d.ensure(n_st));
    SGK_TRY(S.ends.ensure(2 * n_st));
    SGK_TRY(S.in.up(S.in_bytes, S.stream));
    const uint8_t *d_in = S.in.d.p;
    sgk_ss_batch_t b;
    memset(&b, 0, sizeof b);
    b.ss = d_in;
    b.n_ss_bytes = S.n_ss_bytes;
    b.records = reinterpret_cast<const sgk_ss_record_t *>(d_in + S.off_rec);
    b.n_records = S.n_records;
    // 1. validate: the status of every record, nothing stored
    SGK_TRY(sgk_ss_decode(&b, nullptr, nullptr, S.status.d.p, S.ends.p, S.stream));
    SGK_TRY(S.status.down(S.n_records, S.stream));
    SGK_HIP_TRY(hipStreamSynchronize(S.stream));
    uint32_t bad = S.n_records;
    for (uint32_t r = 0; r < S.n_records; ++r) {
        if (S.status.h.p[r] != 0) {
            bad = r;
            S.bad_record = r;
            S.bad_status = S.status.h.p[r];
            break;
        }
    }
    // 2. the spans in front of the first bad record get table and text space
    uint32_t keep = 0;
    while (keep < S.n_spans && hs[keep].record < bad) ++keep;
    if (keep == 0) return SGK_OK;
    SGK_TRY(S.offs.h.ensure(keep));
    uint64_t n_rows = 0;
    for (uint32_t s = 0; s < keep; ++s) {
        S.offs.h.p[s] = n_rows;
        n_rows += hs[s].count;
    }
    const size_t ws_bytes = sgk_ss_text_workspace_bytes(keep, n_rows);
    SGK_TRY(S.pairs.ensure_bytes((size_t)n_rows * 8 + 16));
    SGK_TRY(S.offs.up(keep, S.stream));
    if (n_rows) SGK_HIP_TRY(hipMemsetAsync(S.pairs.p, 0xff, (size_t)n_rows * 8, S.stream));
    b.spans = reinterpret_cast<const sgk_ss_span_t *>(d_in + S.off_spans);
    b.n_spans = keep;
    SGK_TRY(sgk_ss_decode(&b, S.offs.d.p, S.pairs.p, S.status.d.p, S.ends.p, S.stream));
    const sgk_text_ids_t ids = {d_in + S.off_ids, reinterpret_cast<const uint32_t *>(d_in + S.off_idoffs)};
    return text_pipe_run(
        S, ws_bytes, keep,
        [&] { return sgk_ss_text_measure(&b, S.offs.d.p, S.pairs.p, &ids, S.rows.p, S.ws.p, ws_bytes, S.stream); },
        [&] { return sgk_ss_text_write(&b, S.offs.d.p, S.pairs.p, &ids, S.text.d.p, S.n_bytes, S.ws.p, ws_bytes, S.stream); });
}

}  // namespace

extern "C" {

int sgk_sref_pipe_create(int device, const float *levels, uint32_t k, sgk_sref_pipe_t **out) {
    if (!out || !levels || k < 1 || k > 6) return SGK_ERR_ARG;
    *out = nullptr;
    sgk_sref_pipe *p;
    SGK_TRY(pipe_create(device, &p));
    p->k = k;
    const size_t n_levels = (size_t)1 << (2u * k);
    int rc = p->d_levels.ensure(n_levels);
    if (rc == SGK_OK && hipMemcpy(p->d_levels.p, levels, n_levels * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        rc = SGK_ERR_HIP;
    if (rc != SGK_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return SGK_OK;
}

void sgk_sref_pipe_destroy(sgk_sref_pipe_t *p) { pipe_destroy(p); }

int sgk_sref_pipe_begin(sgk_sref_pipe_t *p, int slot, uint64_t n_bases, uint32_t n_spans, uint32_t n_names,
                        uint64_t name_bytes, sgk_sref_stage_t *out) {
    sgk_sref_pipe::Slot *S;
    if (!out) return SGK_ERR_ARG;
    SGK_TRY(pipe_slot(p, slot, false, &S));
    S->n_bases = n_bases;
    S->n_spans = n_spans;
    StageCursor c;
    c.take(n_bases, 16);
    S->off_spans = c.take((size_t)n_spans * sizeof(sgk_sref_span_t));
    S->off_nbytes = c.take(name_bytes, 16);
    S->off_noffs = c.take(((size_t)n_names + 1) * 4);
    S->in_bytes = c.pos;
    SGK_TRY(S->in.h.ensure_bytes(S->in_bytes));
    uint8_t *h = S->in.h.p;
    out->bases = h;
    out->spans = reinterpret_cast<sgk_sref_span_t *>(h + S->off_spans);
    out->name_bytes = h + S->off_nbytes;
    out->name_offsets = reinterpret_cast<uint32_t *>(h + S->off_noffs);
    return SGK_OK;
}

int sgk_sref_pipe_submit(sgk_sref_pipe_t *p, int slot) {
    return pipe_submit(p, slot, [&](sgk_sref_pipe::Slot &S) { return sref_submit(*p, S); });
}

int sgk_sref_pipe_wait(sgk_sref_pipe_t *p, int slot, const uint8_t **text, uint64_t *n_bytes) {
    sgk_sref_pipe::Slot *S;
    if (!text || !n_bytes) return SGK_ERR_ARG;
    SGK_TRY(pipe_slot(p, slot, true, &S));
    return text_pipe_finish(*S, text, n_bytes);
}

int sgk_ss_pipe_create(int device, sgk_ss_pipe_t **out) {
    if (!out) return SGK_ERR_ARG;
    return pipe_create(device, out);
}

void sgk_ss_pipe_destroy(sgk_ss_pipe_t *p) { pipe_destroy(p); }

int sgk_ss_pipe_begin(sgk_ss_pipe_t *p, int slot, uint64_t n_ss_bytes, uint32_t n_records, uint32_t n_spans, uint32_t n_ids,
                      uint64_t id_bytes, sgk_ss_stage_t *out) {
    sgk_ss_pipe::Slot *S;
    if (!out) return SGK_ERR_ARG;
    SGK_TRY(pipe_slot(p, slot, false, &S));
    S->n_ss_bytes = n_ss_bytes;
    S->n_records = n_records;
    S->n_spans = n_spans;
    S->n_ids = n_ids;
    StageCursor c;
    c.take(n_ss_bytes, 16);
    S->off_rec = c.take((size_t)n_records * sizeof(sgk_ss_record_t));
    S->off_spans = c.take((size_t)n_spans * sizeof(sgk_ss_span_t));
    S->off_ids = c.take(id_bytes, 16);
    S->off_idoffs = c.take(((size_t)n_ids + 1) * 4);
    S->in_bytes = c.pos;
    SGK_TRY(S->in.h.ensure_bytes(S->in_bytes));
    uint8_t *h = S->in.h.p;
    out->ss = h;
    out->records = reinterpret_cast<sgk_ss_record_t *>(h + S->off_rec);
    out->spans = reinterpret_cast<sgk_ss_span_t *>(h + S->off_spans);
    out->id_bytes = h + S->off_ids;
    out->id_offsets = reinterpret_cast<uint32_t *>(h + S->off_idoffs);
    return SGK_OK;
}

int sgk_ss_pipe_submit(sgk_ss_pipe_t *p, int slot) {
    return pipe_submit(p, slot, [](sgk_ss_pipe::Slot &S) { return ss_submit(S); });
}

int sgk_ss_pipe_wait(sgk_ss_pipe_t *p, int slot, const uint8_t **text, uint64_t *n_bytes, uint32_t *bad_record,
                     uint32_t *bad_status) {
    sgk_ss_pipe::Slot *S;
    if (!text || !n_bytes || !bad_record || !bad_status) return SGK_ERR_ARG;
    SGK_TRY(pipe_slot(p, slot, true, &S));
    SGK_TRY(text_pipe_finish(*S, text, n_bytes));
    *bad_record = S->bad_record;
    *bad_status = S->bad_status;
    return SGK_OK;
}

}  // extern "C"
