// job_qts.hip -- sgk_job_submit_qts: the staged batch quantised, then handed back as samples, svb-zd blobs, whole
// deflated records or text SLOW5 rows.
#include "job.h"

using namespace sgk;

// qts record mode: the records assembled around the quantised signal (blobs at d_out[0] / d_out[1] / cnt, or the
// samples), deflated, gathered densely; lengths, statuses and dense offsets on their way home -- the streams themselves
// follow in sgk_job_wait once their total is known
static int job_qts_records(sgk_job_t *j, const sgk_batch_t &view) {
    const uint32_t n = j->n_reads;
    const size_t nr = n;
    hipStream_t st = j->st;
    const bool svb = j->qts_fmt == SGK_SIGNAL_SVBZD, zrec = j->zrec_frames;
    const uint32_t *lens = j->lengths.h.p, *fro = j->fro.h.p, *icaps = j->icaps.h.p, *slens = j->slens.h.p;
    const uint64_t *ioffs = j->ioffs.h.p, *soffs = j->soffs.h.p;
    size_t rec_bound = 0, z_bound = 0;
    for (size_t r = 0; r < nr; ++r) {
        const size_t sig = svb ? 4 + ((size_t)lens[r] + 3) / 4 + 3 * (size_t)lens[r] : 2 * (size_t)lens[r];
        // zrec: the host does not know the tail: whatever the record's room leaves around its old blob (the u64 included)
        if (zrec && soffs[r] - ioffs[r] < 8) return SGK_ERR_ARG;   // (no len_raw_signal in front of the blob)
        const size_t rec = zrec ? (size_t)(icaps[r] - slens[r]) + sig : (size_t)(fro[r + 1] - fro[r]) + 8 + sig;
        if (rec >= ((size_t)1 << 29)) return SGK_ERR_ARG;   // (sgk_deflate's limit)
        rec_bound += round_up(rec, 16);
        z_bound += round_up(sgk_deflate_bound(rec), 16);
    }
    if (!zrec) {
        SGK_TRY(j->frb.up(j->frame_bytes, st));
        SGK_TRY(j->fro.up(nr + 1, st));
        SGK_TRY(j->frh.up(nr, st));
    } else {
        SGK_TRY(j->d_ahl.ensure(nr));
        SGK_TRY(j->d_abad.ensure(nr));
    }
    SGK_TRY(j->d_aho.ensure(nr));
    SGK_TRY(j->d_ato.ensure(nr));
    SGK_TRY(j->d_atl.ensure(nr));
    SGK_TRY(j->d_reclen.ensure(nr));
    SGK_TRY(j->d_zcap.ensure(nr));
    SGK_TRY(j->zlen.d.ensure(nr));
    SGK_TRY(j->zstat.d.ensure(nr));
    SGK_TRY(j->d_recoffs.ensure(nr + 1));
    SGK_TRY(j->d_zoffs.ensure(nr + 1));
    SGK_TRY(j->zdoffs.d.ensure(nr + 1));
    SGK_TRY(j->d_rec.ensure(rec_bound + 16));
    SGK_TRY(j->d_z.ensure(z_bound + 16));
    SGK_TRY(j->zdense.d.ensure(z_bound + 16));
    const uint32_t *counts = svb ? j->cnt.d.p : view.lengths;
    const uint64_t *sig_offs = svb ? j->d_out[1].as<uint64_t>() : view.offsets;
    const uint8_t *signal = svb ? j->d_out[0].as<uint8_t>() : reinterpret_cast<const uint8_t *>(view.samples);
    const uint32_t unit = svb ? 1u : 2u;
    if (zrec)   // (tstat: only a batch with a column table has had its tails checked)
        SGK_TRY(launch_qts_zrec_sizes(j->ioffs.d.p, j->icaps.d.p, j->d_ilens.p, j->soffs.d.p, j->slens.d.p, j->istat.d.p,
                                      j->aux ? j->tstat.d.p : nullptr, counts, n, j->d_aho.p, j->d_ahl.p, j->d_ato.p,
                                      j->d_atl.p, j->d_reclen.p, j->d_zcap.p, j->d_abad.p, st));
    else
        SGK_TRY(launch_qts_record_sizes(j->fro.d.p, j->frh.d.p, counts, unit, n, j->d_aho.p, j->d_ato.p, j->d_atl.p,
                                        j->d_reclen.p, j->d_zcap.p, st));
    SGK_TRY(launch_layout(j->d_reclen.p, nullptr, n, 16u, j->d_recoffs.p, st));
    SGK_TRY(launch_layout(j->d_zcap.p, nullptr, n, 16u, j->d_zoffs.p, st));
    const uint8_t *src = zrec ? j->d_inflated.p : j->frb.d.p;
    SGK_TRY(launch_qts_assemble(src, j->d_aho.p, zrec ? j->d_ahl.p : j->frh.d.p, src, j->d_ato.p, j->d_atl.p,
                                zrec ? j->d_abad.p : nullptr, signal, sig_offs, counts, unit, j->d_rec.p, j->d_recoffs.p, n, st));
    SGK_TRY(launch_deflate_unchecked(j->d_rec.p, j->d_recoffs.p, j->d_reclen.p, n, j->d_z.p, j->d_zoffs.p, j->d_zcap.p,
                                     j->zlen.d.p, j->zstat.d.p, st));
    if (zrec) SGK_TRY(launch_qts_zrec_mark(j->d_abad.p, n, j->zlen.d.p, j->zstat.d.p, st));
    SGK_TRY(launch_layout(j->zlen.d.p, nullptr, n, 16u, j->zdoffs.d.p, st));
    SGK_TRY(launch_bytes_gather(j->d_z.p, j->d_zoffs.p, j->zlen.d.p, n, j->zdense.d.p, j->zdoffs.d.p, st));
    SGK_TRY(j->zlen.down(nr, st));
    SGK_TRY(j->zstat.down(nr, st));
    return j->zdoffs.down(nr + 1, st);
}

// qts with SGK_SIGNAL_TEXT out: the quantised samples as the rows' columns; with frames, head r and tail r around them.
// The frames are split into a blob of heads and one of tails here (a few hundred bytes per read), then the rows.
static int job_qts_text_submit(sgk_job_t *j, const sgk_batch_t &view) {
    const size_t nr = j->n_reads;
    hipStream_t st = j->st;
    if (j->qts_records) {
        const uint32_t *fro = j->fro.h.p, *frh = j->frh.h.p;
        const uint8_t *frb = j->frb.h.p;
        size_t hb = 0;
        for (size_t r = 0; r < nr; ++r) hb += frh[r];
        const size_t tb = j->frame_bytes - hb;
        SGK_TRY(j->hdb.h.ensure(hb + 16));
        SGK_TRY(j->tlb.h.ensure(tb + 16));
        SGK_TRY(j->hdo.h.ensure(nr + 1));
        SGK_TRY(j->tlo.h.ensure(nr + 1));
        uint32_t *ho = j->hdo.h.p, *to = j->tlo.h.p;
        uint32_t h = 0, t = 0;
        for (size_t r = 0; r < nr; ++r) {
            const uint32_t hl = frh[r], tl = fro[r + 1] - fro[r] - hl;
            ho[r] = h;
            to[r] = t;
            if (hl) memcpy(j->hdb.h.p + h, frb + fro[r], hl);
            if (tl) memcpy(j->tlb.h.p + t, frb + fro[r] + hl, tl);
            h += hl;
            t += tl;
        }
        ho[nr] = h;
        to[nr] = t;
        SGK_TRY(j->hdb.up(hb, st));
        SGK_TRY(j->tlb.up(tb, st));
        SGK_TRY(j->hdo.up(nr + 1, st));
        SGK_TRY(j->tlo.up(nr + 1, st));
    }
    return job_text_rows(j, sgk_slow5_text_workspace_bytes(j->n_reads, j->n_samples), view);
}

extern "C" int sgk_job_submit_qts(sgk_job_t *j, int bits, int method, int out_fmt_flags) {
    if (!j || !j->begun || j->submitted) return SGK_ERR_ARG;
    const bool records = (out_fmt_flags & SGK_QTS_RECORDS) != 0;
    // SGK_QTS_ZREC_FRAMES: the frames are the records where they were inflated -- records of a ZREC batch with an svb-zd
    // signal only (one begun with SGK_SIGNAL_INT16 by sgk_job_begin_zrec_signal is refused: its len_raw_signal is a
    // sample count)
    const bool zrec_frames = (out_fmt_flags & SGK_QTS_ZREC_FRAMES) != 0;
    const int out_fmt = out_fmt_flags & ~(SGK_QTS_RECORDS | SGK_QTS_ZREC_FRAMES);
    if (zrec_frames && (!records || j->fmt != SGK_SIGNAL_ZREC || j->raw_sig || out_fmt != SGK_SIGNAL_SVBZD)) return SGK_ERR_ARG;
    if (out_fmt != SGK_SIGNAL_INT16 && out_fmt != SGK_SIGNAL_SVBZD && out_fmt != SGK_SIGNAL_TEXT) return SGK_ERR_ARG;
    // text in, bare int16 samples out stays refused (tests/test_gpu_slow5_cli.py pins it): that is the decoder alone,
    // and no record of either container holds uncompressed samples next to text ones
    if (j->fmt == SGK_SIGNAL_TEXT && out_fmt == SGK_SIGNAL_INT16 && !records) return SGK_ERR_ARG;
    if (records && !zrec_frames && !j->have_frames) return SGK_ERR_ARG;
    if (bits < 1 || bits > 15 || method < SGK_QTS_FLOOR || method > SGK_QTS_FILL_ONES) return SGK_ERR_ARG;
    SGK_HIP_TRY(hipSetDevice(j->device));
    const bool text = out_fmt == SGK_SIGNAL_TEXT, svb = out_fmt == SGK_SIGNAL_SVBZD;
    j->tool = SGK_TOOL_QTS;
    j->result = text ? Result::QtsText : records ? Result::QtsRecords : svb ? Result::QtsBlobs : Result::QtsSamples;
    j->qts_fmt = out_fmt;
    j->qts_records = records;
    j->zrec_frames = zrec_frames;
    if (j->n_reads == 0) return job_submit_empty(j, text);
    const size_t nr = j->n_reads;
    hipStream_t st = j->st;
    sgk_batch_t view;
    SGK_TRY(job_upload(j, &view));
    int16_t *smp = j->samples.d.p;
    SGK_TRY(sgk_qts(smp, view.offsets, view.lengths, j->n_reads, j->max_len, bits, method, st));
    if (svb) {
        // d_out[0] blobs (worst-case sized), d_out[1] blob offsets, cnt blob lengths
        const uint32_t *lens = j->lengths.h.p;
        size_t bound = 0;
        for (size_t r = 0; r < nr; ++r) bound += round_up(4 + ((size_t)lens[r] + 3) / 4 + 3 * (size_t)lens[r], 8);
        SGK_TRY(j->d_out[0].ensure(bound + 16));
        SGK_TRY(j->d_out[1].ensure((nr + 1) * 8));
        SGK_TRY(j->cnt.d.ensure(nr));
        SGK_TRY(sgk_svbzd_size(smp, view.offsets, view.lengths, j->n_reads, j->cnt.d.p, st));
        SGK_TRY(launch_layout(j->cnt.d.p, nullptr, j->n_reads, 8u, j->d_out[1].as<uint64_t>(), st));
        SGK_TRY(sgk_svbzd_encode(smp, view.offsets, view.lengths, j->n_reads, j->d_out[0].as<uint8_t>(),
                                 j->d_out[1].as<uint64_t>(), j->cnt.d.p, st));
    }
    switch (j->result) {
        case Result::QtsText:
            SGK_TRY(job_qts_text_submit(j, view));
            break;
        case Result::QtsRecords:
            SGK_TRY(job_qts_records(j, view));
            break;
        case Result::QtsBlobs:
            SGK_TRY(j->cnt.down(nr, st));
            SGK_TRY(fetch(j->h_out[1], j->d_out[1].p, (nr + 1) * 8, st));
            break;  // the blobs themselves are fetched by sgk_job_wait once their total size is known
        default:   // Result::QtsSamples
            SGK_TRY(fetch(j->h_out[0], j->samples.d.p, j->n_samples * sizeof(int16_t), st));
    }
    j->submitted = true;
    return SGK_OK;
}
