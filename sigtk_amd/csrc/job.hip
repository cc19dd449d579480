// job.hip -- pipelined host jobs (sgk_job_*): the host-side runtime the CLI drives.
//
// A job owns everything one batch needs on its way through a GPU: pinned host staging for the
// signal (raw int16, svb-zd blobs exactly as they sit in the BLOW5 records, or the raw_signal text of SLOW5 records), the device
// buffers, a private HIP stream, and pinned host buffers for the results.  All buffers only ever
// grow, so a job that is recycled batch after batch stops allocating after the first few batches.
//
//   sgk_job_begin   lays the batch out (64-sample aligned reads, head/tail room for the event fast
//                   path) and hands the caller the pinned staging pointers; reader threads
//                   inflate/copy records straight into them
//   sgk_job_submit  enqueues H2D -> (svb-zd decode) -> subtool kernels -> D2H on the job's stream
//                   and returns immediately (job_submit.hip; sgk_job_submit_qts: job_qts.hip)
//   sgk_job_wait    synchronises the stream and validates decode/event status
//
// Several jobs in flight (on one or several GPUs) overlap reading/inflating, PCIe transfers,
// kernels and output formatting; the reference does all of this strictly one record at a time
// (src/cmain.c:118-120).
#include <new>

#include "host_util.h"
#include "job.h"
#include "stat_args.h"

using namespace sgk;

static int job_begin(sgk_job_t *j, uint32_t n_reads, const uint32_t *lengths, int signal_format, const uint32_t *blob_bytes,
                     const uint32_t *sig_offset, const uint32_t *sig_bytes, const uint32_t *rec_room, sgk_job_input_t *in) {
    if (!j || !in || (n_reads && !lengths)) return SGK_ERR_ARG;
    if (signal_format != SGK_SIGNAL_INT16 && n_reads && !blob_bytes) return SGK_ERR_ARG;
    SGK_HIP_TRY(hipSetDevice(j->device));
    if (j->submitted) return SGK_ERR_ARG;  // previous batch still in flight: sgk_job_wait first
    const size_t nr = n_reads, nr1 = nr ? nr : 1;
    SGK_TRY(j->offsets.h.ensure(nr1));
    SGK_TRY(j->lengths.h.ensure(nr1));
    SGK_TRY(j->dig.h.ensure(nr1));
    SGK_TRY(j->off.h.ensure(nr1));
    SGK_TRY(j->rng.h.ensure(nr1));
    uint32_t mx;
    const uint64_t n_samples = layout_reads(lengths, nr, j->offsets.h.p, &mx);
    if (!n_samples) return SGK_ERR_ARG;
    if (nr) memcpy(j->lengths.h.p, lengths, nr * 4);
    j->n_reads = n_reads;
    j->max_len = mx;
    j->n_samples = n_samples;
    j->fmt = signal_format;
    j->aux = false;
    j->raw_sig = false;
    j->blob_bytes = 0;
    memset(in, 0, sizeof *in);
    if (signal_format == SGK_SIGNAL_SVBZD || signal_format == SGK_SIGNAL_ZREC || signal_format == SGK_SIGNAL_TEXT) {
        SGK_TRY(j->boffs.h.ensure(nr1));
        SGK_TRY(j->blens.h.ensure(nr1));
        uint64_t b = 0;
        for (size_t r = 0; r < nr; ++r) {
            j->boffs.h.p[r] = b;
            j->blens.h.p[r] = blob_bytes[r];
            b += round_up(blob_bytes[r], signal_format == SGK_SIGNAL_TEXT ? 16 : 8);  // (text: 16-byte words, no lead-in)
        }
        j->blob_bytes = b + 16;  // the decoders read whole aligned words
        SGK_TRY(j->blobs.h.ensure(j->blob_bytes));
        in->blobs = j->blobs.h.p;
        in->blob_offsets = j->boffs.h.p;
        if (signal_format == SGK_SIGNAL_ZREC) {
            // where every record inflates to (16-byte aligned), its room, and -- for the svb-zd decoder --
            // where its signal blob then lies and how long it is
            SGK_TRY(j->ioffs.h.ensure(nr1));
            SGK_TRY(j->icaps.h.ensure(nr1));
            SGK_TRY(j->soffs.h.ensure(nr1));     // (blob offsets inside d_inflated)
            SGK_TRY(j->slens.h.ensure(nr1));     // (blob lengths)
            uint64_t o2 = 0;
            for (size_t r = 0; r < nr; ++r) {
                if ((uint64_t)sig_offset[r] + sig_bytes[r] > rec_room[r]) return SGK_ERR_ARG;
                j->ioffs.h.p[r] = o2;
                j->icaps.h.p[r] = rec_room[r];
                j->soffs.h.p[r] = o2 + sig_offset[r];
                j->slens.h.p[r] = sig_bytes[r];
                o2 += round_up(rec_room[r], 16);
            }
            j->inflated_bytes = o2 + 16;
        }
    } else {
        SGK_TRY(j->samples.h.ensure(j->n_samples));
        in->samples = j->samples.h.p;
    }
    in->offsets = j->offsets.h.p;
    in->digitisation = j->dig.h.p;
    in->offset = j->off.h.p;
    in->range = j->rng.h.p;
    in->n_samples = j->n_samples;
    j->begun = true;
    j->have_ids = false;
    j->have_frames = false;
    j->text_bytes = 0;
    return SGK_OK;
}

extern "C" {

int sgk_job_create(int device, sgk_job_t **out) {
    if (!out) return SGK_ERR_ARG;
    *out = nullptr;
    const int nd = sgk_device_count();
    if (nd <= 0) return SGK_ERR_NODEVICE;
    if (device < 0 || device >= nd) return SGK_ERR_ARG;
    SGK_HIP_TRY(hipSetDevice(device));
    sgk_job *j = new (std::nothrow) sgk_job();
    if (!j) return SGK_ERR_NOMEM;
    j->device = device;
    const hipError_t e = hipStreamCreateWithFlags(&j->st, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_hip_error(e, "hipStreamCreateWithFlags", __FILE__, __LINE__);
        delete j;
        return SGK_ERR_HIP;
    }
    *out = j;
    return SGK_OK;
}

int sgk_job_set_options(sgk_job_t *j, const sgk_event_options_t *event_opt, const sgk_stat_options_t *stat_opt) {
    if (!j) return SGK_ERR_ARG;
    j->ev_opt = event_opt ? *event_opt : sgk_event_options_t{};
    j->st_opt = stat_opt ? *stat_opt : sgk_stat_options_t{};
    return SGK_OK;
}

int sgk_job_set_event_params(sgk_job_t *j, const sgk_event_params_t *params) {
    if (!j || (params && sgk_event_params_route(params) < 0)) return SGK_ERR_ARG;  // (the submits route by the same call)
    j->has_ev_params = params != nullptr;
    if (params) j->ev_params = *params;
    return SGK_OK;
}

int sgk_job_set_jnn_params(sgk_job_t *j, const sgk_jnn_param_t *params) {
    if (!j || (params && sgk_jnn_params_check(params) != SGK_OK)) return SGK_ERR_ARG;
    j->has_jnn_params = params != nullptr;
    if (params) j->jnn_params = *params;
    return SGK_OK;
}

int sgk_job_set_prefix_params(sgk_job_t *j, const sgk_prefix_params_t *params) {
    if (!j || (params && sgk_prefix_route(params) < 0)) return SGK_ERR_ARG;  // (the submits route by the same call)
    j->has_prefix_params = params != nullptr;
    if (params) j->prefix_params = *params;
    return SGK_OK;
}

int sgk_job_set_normalise(sgk_job_t *j, int method) {
    if (!j || (method != 0 && method != SGK_NORM_ZSCORE && method != SGK_NORM_MEDMAD)) return SGK_ERR_ARG;
    j->normalise = method;
    return SGK_OK;
}

void sgk_job_destroy(sgk_job_t *j) {
    if (!j) return;
    (void)hipSetDevice(j->device);
    if (j->st) {
        (void)hipStreamSynchronize(j->st);
        zstd_release_scratch(j->device, j->st);
        (void)hipStreamDestroy(j->st);
    }
    delete j;
}

int sgk_job_device(const sgk_job_t *j) { return j ? j->device : -1; }

int sgk_job_begin(sgk_job_t *j, uint32_t n_reads, const uint32_t *lengths, int signal_format,
                  const uint32_t *blob_bytes, sgk_job_input_t *in) {
    if (signal_format != SGK_SIGNAL_INT16 && signal_format != SGK_SIGNAL_SVBZD && signal_format != SGK_SIGNAL_TEXT) return SGK_ERR_ARG;
    return job_begin(j, n_reads, lengths, signal_format, blob_bytes, nullptr, nullptr, nullptr, in);
}

int sgk_job_begin_zrec(sgk_job_t *j, uint32_t n_reads, const uint32_t *lengths, const uint32_t *rec_bytes,
                       const uint32_t *sig_offset, const uint32_t *sig_bytes, const uint32_t *rec_room,
                       sgk_job_input_t *in) {
    return sgk_job_begin_zrec_format(j, n_reads, SGK_RECORD_ZLIB, lengths, rec_bytes, sig_offset, sig_bytes, rec_room, in);
}

int sgk_job_begin_zrec_format(sgk_job_t *j, uint32_t n_reads, int record_format, const uint32_t *lengths,
                              const uint32_t *rec_bytes, const uint32_t *sig_offset, const uint32_t *sig_bytes,
                              const uint32_t *rec_room, sgk_job_input_t *in) {
    if (record_format != SGK_RECORD_ZLIB && record_format != SGK_RECORD_ZSTD) return SGK_ERR_ARG;
    if (n_reads && (!rec_bytes || !sig_offset || !sig_bytes || !rec_room)) return SGK_ERR_ARG;
    const int rc = job_begin(j, n_reads, lengths, SGK_SIGNAL_ZREC, rec_bytes, sig_offset, sig_bytes, rec_room, in);
    if (rc == SGK_OK) j->rec_fmt = record_format;
    return rc;
}

int sgk_job_begin_zrec_aux(sgk_job_t *j, uint32_t n_reads, int record_format, const uint32_t *lengths,
                           const uint32_t *rec_bytes, const uint32_t *sig_offset, const uint32_t *sig_bytes,
                           const uint32_t *rec_room, const sgk_aux_field_t *fields, uint32_t n_fields, sgk_job_input_t *in) {
    if (!j || (n_fields && !fields)) return SGK_ERR_ARG;
    for (uint32_t c = 0; c < n_fields; ++c) {
        const uint32_t eb = fields[c].elem_bytes;
        if ((eb != 1 && eb != 2 && eb != 4 && eb != 8) || fields[c].is_array > 1) return SGK_ERR_ARG;
    }
    SGK_TRY(sgk_job_begin_zrec_format(j, n_reads, record_format, lengths, rec_bytes, sig_offset, sig_bytes, rec_room, in));
    if (n_fields > j->aux_cap) {
        sgk_aux_field_t *p = static_cast<sgk_aux_field_t *>(realloc(j->aux_fields, sizeof(sgk_aux_field_t) * n_fields));
        if (!p) return SGK_ERR_NOMEM;
        j->aux_fields = p;
        j->aux_cap = n_fields;
    }
    if (n_fields) memcpy(j->aux_fields, fields, sizeof(sgk_aux_field_t) * n_fields);
    j->n_aux = n_fields;
    SGK_TRY(j->toffs.h.ensure(n_reads ? n_reads : 1));
    for (size_t r = 0; r < n_reads; ++r) j->toffs.h.p[r] = sig_offset[r] + sig_bytes[r];   // <= rec_room[r]: job_begin checked
    j->aux = true;
    return SGK_OK;
}

int sgk_job_begin_zrec_signal(sgk_job_t *j, uint32_t n_reads, int record_format, int signal_format, const uint32_t *lengths,
                              const uint32_t *rec_bytes, const uint32_t *sig_offset, const uint32_t *sig_bytes,
                              const uint32_t *rec_room, const sgk_aux_field_t *fields, uint32_t n_fields, sgk_job_input_t *in) {
    if (signal_format == SGK_SIGNAL_SVBZD)
        return sgk_job_begin_zrec_aux(j, n_reads, record_format, lengths, rec_bytes, sig_offset, sig_bytes, rec_room, fields,
                                      n_fields, in);
    if (signal_format != SGK_SIGNAL_INT16) return SGK_ERR_ARG;
    if (n_reads && (!lengths || !sig_offset || !sig_bytes)) return SGK_ERR_ARG;
    for (size_t r = 0; r < n_reads; ++r)
        if ((uint64_t)sig_bytes[r] != 2ull * lengths[r]) return SGK_ERR_ARG;
    SGK_TRY(sgk_job_begin_zrec_aux(j, n_reads, record_format, lengths, rec_bytes, sig_offset, sig_bytes, rec_room, fields,
                                   n_fields, in));
    SGK_TRY(j->sigo.h.ensure(n_reads ? n_reads : 1));
    if (n_reads) memcpy(j->sigo.h.p, sig_offset, (size_t)n_reads * 4);
    j->raw_sig = true;
    return SGK_OK;
}

int sgk_job_set_record_frames(sgk_job_t *j, const uint8_t *bytes, const uint32_t *frame_offsets, const uint32_t *head_lengths) {
    if (!j || !j->begun || j->submitted || !frame_offsets || frame_offsets[0] != 0) return SGK_ERR_ARG;
    const size_t nr = j->n_reads;
    if (nr && !head_lengths) return SGK_ERR_ARG;
    for (size_t r = 0; r < nr; ++r)
        if (frame_offsets[r + 1] < frame_offsets[r] || head_lengths[r] > frame_offsets[r + 1] - frame_offsets[r]) return SGK_ERR_ARG;
    if (frame_offsets[nr] && !bytes) return SGK_ERR_ARG;
    SGK_HIP_TRY(hipSetDevice(j->device));
    SGK_TRY(j->fro.h.ensure(nr + 1));
    SGK_TRY(j->frh.h.ensure(nr ? nr : 1));
    SGK_TRY(j->frb.h.ensure((size_t)frame_offsets[nr] + 16));
    memcpy(j->fro.h.p, frame_offsets, (nr + 1) * 4);
    if (nr) memcpy(j->frh.h.p, head_lengths, nr * 4);
    if (frame_offsets[nr]) memcpy(j->frb.h.p, bytes, frame_offsets[nr]);
    j->frame_bytes = frame_offsets[nr];
    j->have_frames = true;
    return SGK_OK;
}

int sgk_job_set_ids(sgk_job_t *j, const uint8_t *bytes, const uint32_t *offsets) {
    if (!j || !j->begun || j->submitted || !offsets || offsets[0] != 0) return SGK_ERR_ARG;
    const size_t nr = j->n_reads;
    for (size_t r = 0; r < nr; ++r)
        if (offsets[r + 1] < offsets[r] || offsets[r + 1] - offsets[r] > 65535u) return SGK_ERR_ARG;
    if (offsets[nr] && !bytes) return SGK_ERR_ARG;
    SGK_HIP_TRY(hipSetDevice(j->device));
    SGK_TRY(j->ido.h.ensure(nr + 1));
    SGK_TRY(j->idb.h.ensure((size_t)offsets[nr] + 16));
    memcpy(j->ido.h.p, offsets, (nr + 1) * 4);
    if (offsets[nr]) memcpy(j->idb.h.p, bytes, offsets[nr]);
    j->id_bytes = offsets[nr];
    j->have_ids = true;
    return SGK_OK;
}

}  // extern "C"

namespace sgk {

// enqueue the uploads of a staged batch (and the svb-zd decode) and describe the device batch
int job_upload(sgk_job_t *j, sgk_batch_t *view) {
    const size_t nr = j->n_reads;
    hipStream_t st = j->st;
    int rc;
    SGK_TRY(j->offsets.up(nr, st));
    SGK_TRY(j->lengths.up(nr, st));
    SGK_TRY(j->dig.up(nr, st));
    SGK_TRY(j->off.up(nr, st));
    SGK_TRY(j->rng.up(nr, st));
    if (j->fmt == SGK_SIGNAL_ZREC) {
        // the records as they sit in the file -> inflated on the device -> their svb-zd blobs decoded from there
        SGK_TRY(j->samples.d.ensure(j->n_samples));
        SGK_TRY(j->blobs.up(j->blob_bytes, st));
        SGK_TRY(j->boffs.up(nr, st));
        SGK_TRY(j->blens.up(nr, st));
        SGK_TRY(j->ioffs.up(nr, st));
        SGK_TRY(j->icaps.up(nr, st));
        SGK_TRY(j->soffs.up(nr, st));
        SGK_TRY(j->slens.up(nr, st));
        SGK_TRY(j->d_inflated.ensure(j->inflated_bytes));
        SGK_TRY(j->d_ilens.ensure(nr));
        SGK_TRY(j->istat.d.ensure(nr));
        SGK_TRY(j->dstat.d.ensure(nr));
        SGK_TRY((j->rec_fmt == SGK_RECORD_ZSTD ? sgk_zstd_decompress : sgk_inflate)(
            j->blobs.d.p, j->boffs.d.p, j->blens.d.p, j->n_reads, j->d_inflated.p, j->ioffs.d.p, j->icaps.d.p, j->d_ilens.p,
            j->istat.d.p, st));
        // (a record that did not inflate leaves whatever it leaves: its blob then fails the decoder's own checks or
        // decodes to garbage nobody reads -- sgk_job_wait refuses the batch on the inflate status)
        if (j->raw_sig) {
            // plain samples: moved out of what each record inflated to (a record shorter than its signal: status 1 here
            // and from k_zrec_tail below; one that did not inflate is not read)
            SGK_TRY(j->sigo.up(nr, st));
            rc = sgk_sigraw_gather(j->d_inflated.p, j->ioffs.d.p, j->d_ilens.p, j->sigo.d.p, j->istat.d.p, j->n_reads,
                                   j->samples.d.p, j->offsets.d.p, j->lengths.d.p, j->max_len, j->n_samples, j->dstat.d.p, st);
        } else {
            rc = sgk_svbzd_decode(j->d_inflated.p, j->soffs.d.p, j->slens.d.p, j->n_reads, j->samples.d.p, j->offsets.d.p,
                                  j->lengths.d.p, j->dstat.d.p, st);
        }
        SGK_TRY(rc);
        SGK_TRY(j->dstat.down(nr, st));
        SGK_TRY(j->istat.down(nr, st));
        if (j->aux) {
            // what every record inflated to against the file's columns (a record that did not inflate is not looked at:
            // its length word may lie behind its room)
            SGK_TRY(j->toffs.up(nr, st));
            SGK_TRY(j->tstat.d.ensure(nr));
            SGK_TRY(zrec_tail_check(j->d_inflated.p, j->ioffs.d.p, j->d_ilens.p, j->toffs.d.p, j->istat.d.p, j->n_reads,
                                    j->aux_fields, j->n_aux, j->tstat.d.p, st));
            SGK_TRY(j->tstat.down(nr, st));
        }
    } else if (j->fmt == SGK_SIGNAL_SVBZD || j->fmt == SGK_SIGNAL_TEXT) {
        SGK_TRY(j->samples.d.ensure(j->n_samples));
        SGK_TRY(j->blobs.up(j->blob_bytes, st));
        SGK_TRY(j->boffs.up(nr, st));
        SGK_TRY(j->blens.up(nr, st));
        SGK_TRY(j->dstat.d.ensure(nr));
        // (text: blobs.d is 16-byte aligned and blob_bytes holds 16 bytes behind the last column)
        SGK_TRY((j->fmt == SGK_SIGNAL_TEXT ? sgk_sigtext_decode : sgk_svbzd_decode)(
            j->blobs.d.p, j->boffs.d.p, j->blens.d.p, j->n_reads, j->samples.d.p, j->offsets.d.p, j->lengths.d.p,
            j->dstat.d.p, st));
        SGK_TRY(j->dstat.down(nr, st));
    } else {
        SGK_TRY(j->samples.up(j->n_samples, st));
    }
    view->samples = j->samples.d.p;
    view->offsets = j->offsets.d.p;
    view->lengths = j->lengths.d.p;
    view->digitisation = j->dig.d.p;
    view->offset = j->off.d.p;
    view->range = j->rng.d.p;
    view->n_reads = j->n_reads;
    view->max_read_len = j->max_len;
    view->n_samples = j->n_samples;
    return SGK_OK;
}

// a batch without reads: nothing to enqueue; a text result has its one row offset
int job_submit_empty(sgk_job *j, bool text) {
    if (text) {
        SGK_TRY(j->roffs.h.ensure(1));
        j->roffs.h.p[0] = 0;
    }
    j->submitted = true;
    return SGK_OK;
}

// SGK_JOB_TEXT / qts text: the measure pass over the batch (row offsets into roffs.d), or the write pass over the
// measured batch into text.d as far as it reaches (checked on the device)
static int job_text_pass(sgk_job_t *j, bool write) {
    const sgk_batch_t &v = j->text_view;
    if (j->result == Result::QtsText) {
        const sgk_text_ids_t heads = {j->hdb.d.p, j->hdo.d.p}, tails = {j->tlb.d.p, j->tlo.d.p};
        const sgk_text_ids_t *hp = j->qts_records ? &heads : nullptr, *tp = j->qts_records ? &tails : nullptr;
        return write ? sgk_slow5_text_write(v.samples, v.offsets, v.lengths, j->n_reads, hp, tp, j->text.d.p, j->text.d.cap,
                                            j->d_tws.p, j->tws_bytes, j->st)
                     : sgk_slow5_text_measure(v.samples, v.offsets, v.lengths, j->n_reads, hp, tp, j->roffs.d.p, j->d_tws.p,
                                              j->tws_bytes, j->st);
    }
    const bool ev = j->text_kind != SGK_TEXT_PA;
    const sgk_text_ids_t ids = {j->idb.d.p, j->ido.d.p};
    const uint64_t *slots = ev ? j->slots.d.p : nullptr;
    const sgk_event_rec_t *recs = ev ? j->d_out[0].as<sgk_event_rec_t>() : nullptr;
    const uint32_t *cnt = ev ? j->cnt.d.p : nullptr;
    return write ? sgk_text_write(j->text_kind, &v, &ids, slots, recs, cnt, j->text.d.p, j->text.d.cap, j->d_tws.p,
                                  j->tws_bytes, j->st)
                 : sgk_text_measure(j->text_kind, &v, &ids, slots, recs, cnt, j->roffs.d.p, j->d_tws.p, j->tws_bytes, j->st);
}

// (sgk_job_wait learns the total, grows the buffer and writes again if that one was too small -- the first batches of a job)
int job_text_rows(sgk_job *j, size_t tws_bytes, const sgk_batch_t &view) {
    const size_t nr = j->n_reads;
    j->tws_bytes = tws_bytes;
    SGK_TRY(j->d_tws.ensure(tws_bytes));
    SGK_TRY(j->roffs.d.ensure(nr + 1));
    j->text_view = view;
    SGK_TRY(job_text_pass(j, false));
    SGK_TRY(j->roffs.down(nr + 1, j->st));
    j->text_written = false;
    if (j->text.d.cap) {
        SGK_TRY(job_text_pass(j, true));
        j->text_written = true;
    }
    return SGK_OK;
}

}  // namespace sgk

// after the stream has drained: the total is known -- write (again) if the rows are not in text.d yet, fetch them
static int job_text_fetch(sgk_job_t *j) {
    const uint64_t total = j->roffs.h.p[j->n_reads];
    if (!j->text_written || total > j->text.d.cap) {
        SGK_TRY(j->text.d.ensure((size_t)total));
        SGK_HIP_TRY(hipMemsetAsync(j->d_tws.p, 0, 4, j->st));  // the overflow flag of the attempt at submit
        SGK_TRY(job_text_pass(j, true));
    }
    SGK_TRY(j->text.down((size_t)total, j->st));
    SGK_HIP_TRY(hipStreamSynchronize(j->st));
    sgk_text_status_t ts;
    SGK_TRY(sgk_text_status(j->d_tws.p, &ts));
    j->text_bytes = total;
    return SGK_OK;
}

// the total of a result is known now: `bytes` of each of the n buffers d[] into h[], and wait for them
template <typename H, typename D>
static int fetch_now(sgk_job_t *j, H *h, const D *d, int n, size_t bytes) {
    for (int k = 0; k < n; ++k) SGK_TRY(fetch(h[k], d[k].p, bytes, j->st));
    SGK_HIP_TRY(hipStreamSynchronize(j->st));
    return SGK_OK;
}

extern "C" {

int sgk_job_wait(sgk_job_t *j) {
    if (!j || !j->submitted) return SGK_ERR_ARG;
    SGK_HIP_TRY(hipSetDevice(j->device));
    j->submitted = false;  // the staged batch stays valid: it may be submitted again (e.g. with another tool)
    memset(&j->ev_status, 0, sizeof j->ev_status);
    SGK_HIP_TRY(hipStreamSynchronize(j->st));
    j->long_declined = 0u;
    const uint32_t n = j->n_reads;
    if (n == 0) return SGK_OK;
    if (j->long_fetched) {
        // n_timeouts of sgk_long_status_t: long reads whose workgroups gave up at a barrier; they were redone on one
        // wavefront, the records are right -- a caller that wants to know (the CLI warns) asks sgk_job_long_declined
        j->long_declined = j->h_long.as<LongHdr>()->n_declined;
        j->long_fetched = false;
    }
    if (j->fmt == SGK_SIGNAL_ZREC) {
        // a record that did not inflate (malformed stream, check value, more bytes than its head announced): as the
        // reference's slow5_get_next error.  decode_status carries 0x100 | the inflate status for such a read (zstd
        // records: 0x200 | sgk_zstd_decompress's status).
        uint32_t *ds = j->dstat.h.p;
        const uint32_t *is = j->istat.h.p;
        const uint32_t *ts = j->aux ? j->tstat.h.p : nullptr;   // (sgk_job_begin_zrec_aux: 0x400 | k_zrec_tail's)
        bool bad = false;
        for (uint32_t r = 0; r < n; ++r) {
            if (is[r] != 0) ds[r] = (j->rec_fmt == SGK_RECORD_ZSTD ? 0x200u : 0x100u) | is[r];
            else if (ts && ts[r] != 0) ds[r] = 0x400u | ts[r];
            bad = bad || ds[r] != 0;
        }
        // the sound records of the batch were assembled and deflated all the same (the others: qts_record_status 2)
        if (bad && j->result == Result::QtsRecords && j->zrec_frames)
            SGK_TRY(fetch_now(j, &j->zdense.h, &j->zdense.d, 1, (size_t)j->zdoffs.h.p[n]));
        if (bad) return SGK_ERR_FORMAT;
    }
    if (j->fmt == SGK_SIGNAL_SVBZD || j->fmt == SGK_SIGNAL_TEXT) {
        for (uint32_t r = 0; r < n; ++r)
            if (j->dstat.h.p[r] != 0) return SGK_ERR_FORMAT;
    }
    switch (j->result) {
        case Result::TextRows:
        case Result::QtsText:
            SGK_TRY(job_text_fetch(j));
            break;
        case Result::Events:
        case Result::Segments:
            SGK_TRY(fetch_now(j, j->h_out, j->d_dense, j->n_dense, (size_t)j->doffs.h.p[n] * 4));
            if (j->result == Result::Segments && *j->h_err.as<uint32_t>()) return SGK_ERR_CAPACITY;
            break;
        case Result::QtsBlobs:
            SGK_TRY(fetch_now(j, j->h_out, j->d_out, 1, (size_t)j->h_out[1].as<uint64_t>()[n]));
            break;
        case Result::QtsRecords:
            SGK_TRY(fetch_now(j, &j->zdense.h, &j->zdense.d, 1, (size_t)j->zdoffs.h.p[n]));
            break;
        case Result::Ent: {
            const sgk_ent_hist_t *rec = j->h_out[0].as<sgk_ent_hist_t>();
            j->ent_over = false;
            for (uint32_t r = 0; r < n && !j->ent_over; ++r) j->ent_over = rec[r].n_over_raw || rec[r].n_over_delta;
            if (j->ent_over) SGK_TRY(fetch_now(j, j->h_out + 1, j->d_out + 1, 2, j->n_samples * sizeof(uint16_t)));
            break;
        }
        default:   // pa, stat, prefix, qts samples: all of it was fetched at submit
            break;
    }
    if (j->tool == SGK_TOOL_EVENT) return sgk_event_status(j->d_ws.p, &j->ev_status, j->st);   // (also for event text)
    return SGK_OK;
}

uint32_t sgk_job_long_declined(const sgk_job_t *j) { return j ? j->long_declined : 0u; }

int sgk_job_text(const sgk_job_t *j, sgk_job_text_t *out) {
    if (!j || !out) return SGK_ERR_ARG;
    if (j->result != Result::TextRows && j->result != Result::QtsText) return SGK_ERR_ARG;
    out->text = j->text.h.p;
    out->row_offsets = j->roffs.h.p;
    out->n_bytes = j->n_reads ? j->text_bytes : 0;
    return SGK_OK;
}

int sgk_job_output(const sgk_job_t *j, sgk_job_output_t *out) {
    if (!j || !out) return SGK_ERR_ARG;
    memset(out, 0, sizeof *out);
    out->n_reads = j->n_reads;
    out->offsets = j->offsets.h.p;
    out->lengths = j->lengths.h.p;
    out->decode_status = (j->fmt == SGK_SIGNAL_SVBZD || j->fmt == SGK_SIGNAL_ZREC || j->fmt == SGK_SIGNAL_TEXT) ? j->dstat.h.p : nullptr;
    switch (j->result) {
        case Result::None:
            return SGK_ERR_ARG;
        case Result::TextRows:
            out->event_status = j->ev_status;  // the results are the rows: sgk_job_text
            break;
        case Result::QtsText:  // the results are the rows: sgk_job_text
            break;
        case Result::Pa:
            out->pa = j->h_out[0].as<float>();
            break;
        case Result::Events:
            out->slots = j->doffs.h.p;
            out->counts = j->cnt.h.p;
            out->event_status = j->ev_status;
            if (j->flags & SGK_JOB_EVENTS_LENGTHS) {
                out->ev_length = j->h_out[0].as<uint32_t>();
                break;
            }
            out->ev_start = j->h_out[0].as<uint32_t>();
            out->ev_length = j->h_out[1].as<uint32_t>();
            if (!(j->flags & SGK_JOB_EVENTS_COMPACT)) {
                out->ev_mean = j->h_out[2].as<float>();
                out->ev_stdv = j->h_out[3].as<float>();
            }
            break;
        case Result::Segments:
            out->slots = j->doffs.h.p;
            out->counts = j->cnt.h.p;
            out->seg_x = j->h_out[0].as<int32_t>();
            out->seg_y = j->h_out[1].as<int32_t>();
            break;
        case Result::Stat:
            out->stat = j->h_out[0].as<sgk_stat_rec_t>();
            break;
        case Result::Prefix:
            out->prefix = j->h_out[0].as<sgk_prefix_rec_t>();
            break;
        case Result::QtsRecords:
            out->qts_records = j->zdense.h.p;
            out->qts_record_offsets = j->zdoffs.h.p;
            out->qts_record_lengths = j->zlen.h.p;
            out->qts_record_status = j->zstat.h.p;
            break;
        case Result::QtsBlobs:
            out->qts_blobs = j->h_out[0].as<uint8_t>();
            out->qts_blob_offsets = j->h_out[1].as<uint64_t>();
            out->qts_blob_lengths = j->cnt.h.p;
            break;
        case Result::QtsSamples:
            out->qts_samples = j->h_out[0].as<int16_t>();
            break;
        case Result::Ent:
            out->ent = j->h_out[0].as<sgk_ent_hist_t>();
            out->ent_over_raw = j->ent_over ? j->h_out[1].as<uint16_t>() : nullptr;
            out->ent_over_delta = j->ent_over ? j->h_out[2].as<uint16_t>() : nullptr;
            break;
    }
    return SGK_OK;
}

}  // extern "C"
