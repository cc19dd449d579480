// job.h -- what the job units (job.hip, job_submit.hip, job_qts.hip) share: struct sgk_job on the growing buffers of
// grow_buf.h, the kind of result a submit leaves behind, and the internal functions one unit calls in another.
#pragma once
#include <stdlib.h>
#include <string.h>

#include "grow_buf.h"
#include "job_launch.h"
#include "sgk_common.h"

namespace sgk {

// what the last submit leaves behind: sgk_job_wait, sgk_job_output and sgk_job_text fetch and expose by this alone
enum class Result { None, Pa, Events, Segments, Stat, Prefix, Ent, TextRows, QtsSamples, QtsBlobs, QtsRecords, QtsText };

}  // namespace sgk

struct sgk_job {
    int device = 0;
    hipStream_t st = nullptr;
    // batch geometry
    uint32_t n_reads = 0, max_len = 0;
    uint64_t n_samples = 0, blob_bytes = 0;
    int fmt = SGK_SIGNAL_INT16;
    // input staging (pinned) and device mirrors
    sgk::Pair<int16_t> samples;
    sgk::Pair<uint8_t> blobs;
    sgk::Pair<uint64_t> offsets, boffs, slots;
    sgk::Pair<uint32_t> lengths, blens, dstat;
    sgk::Pair<double> dig, off, rng;
    // d_ws: the tool's workspace -- words, LongHdr behind the dispatch order (stat / jnn / prefix), the event status
    sgk::Bytes<sgk::Mem::Dev> d_ws;
    // d_out: pa float (+ sgk_norm_rec_t with sgk_job_set_normalise) | events sgk_event_rec_t | seg x, y int32 | stat, prefix, ent records (+ ent overflow uint16 x 2) |
    //        qts blobs uint8, their offsets uint64;  h_out: the same fetched, or the dense arrays | qts samples int16
    sgk::Bytes<sgk::Mem::Dev> d_out[4];
    sgk::Bytes<sgk::Mem::Pin> h_out[4];
    // d_dense: events uint32 start, length, float mean, stdv | seg int32 x, y, gathered to dense per-read ranges (doffs)
    sgk::Bytes<sgk::Mem::Dev> d_dense[4];
    sgk::Pair<uint32_t> cnt;          // per-read counts (events, segments); qts: blob lengths
    sgk::Pair<uint64_t> doffs;
    sgk::Bytes<sgk::Mem::Pin> h_err;  // jnn: uint32, the reads whose segments overflowed their slots
    sgk::Bytes<sgk::Mem::Pin> h_long; // stat / jnn / prefix: LongHdr
    // SGK_SIGNAL_ZREC: the records as they sit in the file (blobs), inflated on the device into d_inflated;
    // per record: where it goes there, how much room it has, where its signal blob starts (all relative to d_inflated)
    sgk::Pair<uint64_t> ioffs, soffs;
    sgk::Pair<uint32_t> icaps, istat, slens;
    sgk::Dev<uint8_t> d_inflated;
    sgk::Dev<uint32_t> d_ilens;
    uint64_t inflated_bytes = 0;
    int rec_fmt = SGK_RECORD_ZLIB;   // SGK_SIGNAL_ZREC: what the records are compressed with
    // sgk_job_begin_zrec_aux: the file's auxiliary columns; what every record inflated to (d_ilens) is then checked against
    // them from the end of its signal (toffs, relative to the record) by k_zrec_tail
    bool aux = false;
    sgk_aux_field_t *aux_fields = nullptr;
    uint32_t n_aux = 0, aux_cap = 0;
    sgk::Pair<uint32_t> toffs, tstat;
    // sgk_job_begin_zrec_signal with SGK_SIGNAL_INT16: the signal of the inflated records is plain samples, moved into
    // samples.d by k_sigraw_gather from sig_offset[r] of every record (sigo)
    bool raw_sig = false;
    sgk::Pair<uint32_t> sigo;
    ~sgk_job() { free(aux_fields); }
    bool long_fetched = false;        // stat / jnn / prefix: the long-read header of the call is on its way to h_long
    uint32_t long_declined = 0;       // ... long reads the long path declined (n_timeouts of sgk_long_status_t), after wait
    int n_dense = 0;                  // arrays to fetch in sgk_job_wait once the dense total is known
    // SGK_JOB_TEXT: the read ids (sgk_job_set_ids), the rows and their offsets
    sgk::Pair<uint8_t> idb, text;
    sgk::Pair<uint32_t> ido;
    sgk::Pair<uint64_t> roffs;
    sgk::Bytes<sgk::Mem::Dev> d_tws;  // the text workspace: its overflow flag (uint32), then what the passes keep per tile
    bool have_ids = false;
    // qts record mode (sgk_job_set_record_frames + SGK_QTS_RECORDS): the frames; the assembled records (d_rec*), their
    // zlib streams where k_deflate writes them (d_z*: worst-case room each) and gathered densely for the download
    sgk::Pair<uint8_t> frb, zdense;
    sgk::Pair<uint32_t> fro, frh, zlen, zstat;
    sgk::Pair<uint64_t> zdoffs;
    sgk::Dev<uint32_t> d_reclen, d_zcap;
    sgk::Dev<uint64_t> d_recoffs, d_zoffs;
    sgk::Dev<uint8_t> d_rec, d_z;
    bool have_frames = false;
    size_t frame_bytes = 0;
    // ... where k_qts_assemble finds every record's head and tail (the frames, or with SGK_QTS_ZREC_FRAMES the records in
    // d_inflated: d_ahl the head lengths there, d_abad the records whose inflated length nobody vouches for)
    sgk::Dev<uint64_t> d_aho, d_ato;
    sgk::Dev<uint32_t> d_atl, d_ahl, d_abad;
    // qts with SGK_SIGNAL_TEXT out: the frames again as the heads and the tails of the rows (sgk_slow5_text_*)
    sgk::Pair<uint8_t> hdb, tlb;
    sgk::Pair<uint32_t> hdo, tlo;
    bool text_written = false;        // the write pass was enqueued at submit, into the buffer earlier batches grew
    int text_kind = 0;
    size_t tws_bytes = 0, id_bytes = 0;
    uint64_t text_bytes = 0;          // after wait: row_offsets[n_reads]
    sgk_batch_t text_view;
    size_t ws_bytes = 0;
    // the submit in flight / waited for last
    sgk::Result result = sgk::Result::None;
    int tool = -1;
    int flags = 0;                    // events: SGK_JOB_EVENTS_COMPACT / SGK_JOB_EVENTS_LENGTHS
    int qts_fmt = SGK_SIGNAL_INT16;   // qts: the output format (SGK_SIGNAL_*), and the two bits or'ed into it:
    bool qts_records = false, zrec_frames = false;   // SGK_QTS_RECORDS, SGK_QTS_ZREC_FRAMES
    bool begun = false, submitted = false, ent_over = false;
    sgk_event_status_t ev_status = {};
    sgk_event_options_t ev_opt = {};    // sgk_job_set_options (all zero: the defaults)
    sgk_stat_options_t st_opt = {};
    sgk_event_params_t ev_params;       // sgk_job_set_event_params, ..._jnn_params, ..._prefix_params
    sgk_jnn_param_t jnn_params;
    sgk_prefix_params_t prefix_params;
    bool has_ev_params = false, has_jnn_params = false, has_prefix_params = false;
    int normalise = 0;                  // sgk_job_set_normalise: SGK_TOOL_PA hands out sgk_normalise of the batch (0: pA)
};

namespace sgk {
#pragma GCC visibility push(hidden)

// job.hip
int job_upload(sgk_job *j, sgk_batch_t *view);   // the uploads of the staged batch (and its decode), the device batch
int job_submit_empty(sgk_job *j, bool text);     // a batch without reads: nothing to enqueue
// workspace, measure pass, row offsets home; the write pass too when the job already owns a text buffer
int job_text_rows(sgk_job *j, size_t tws_bytes, const sgk_batch_t &view);

#pragma GCC visibility pop
}  // namespace sgk
