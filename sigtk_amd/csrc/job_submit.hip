// job_submit.hip -- sgk_job_submit: the staged batch through one subtool, results on their way home.
#include "host_util.h"
#include "job.h"
#include "stat_args.h"

using namespace sgk;

// stat / jnn / prefix: the long-read path's header (64 bytes behind the dispatch order in the workspace) rides home with
// the results, so that sgk_job_wait can tell how many long reads were declined and redone (n_timeouts of
// sgk_long_status_t; the results are right either way)
static int fetch_long_hdr(sgk_job *j) {
    j->long_fetched = false;
    const size_t off = order_workspace_bytes(j->n_reads);
    if (!j->d_ws.p || j->d_ws.cap < off + long_workspace_bytes(0, 0)) return SGK_OK;
    SGK_TRY(j->h_long.ensure(sizeof(LongHdr)));
    SGK_HIP_TRY(hipMemcpyAsync(j->h_long.p, j->d_ws.p + off, sizeof(LongHdr), hipMemcpyDeviceToHost, j->st));
    j->long_fetched = true;
    return SGK_OK;
}

// ids up, then the rows of the batch (job_text_rows)
static int job_text_submit(sgk_job_t *j, int kind, const sgk_batch_t &view, uint64_t n_items) {
    SGK_TRY(j->idb.up(j->id_bytes, j->st));
    SGK_TRY(j->ido.up((size_t)j->n_reads + 1, j->st));
    j->text_kind = kind;
    return job_text_rows(j, sgk_text_workspace_bytes(kind, j->n_reads, n_items), view);
}

// event / jnn: items into a capacity-sized arena (sgk_event_slots_for(n) / sgk_jnn_slots_for(n) slots per read); what was
// produced is gathered into dense ranges on the device and only that comes home (sgk_job_wait fetches the arrays once the
// total is known).  Event text: rows straight from the arena: no counts, no dense arrays over PCIe
static int job_items(sgk_job_t *j, const sgk_batch_t &view, bool ev, int rna, int flags) {
    const size_t nr = j->n_reads;
    hipStream_t st = j->st;
    SGK_TRY(j->slots.h.ensure(nr + 1));
    const uint64_t s = make_slots(j->lengths.h.p, nr, j->slots.h.p,
                                  [ev](uint32_t len) { return ev ? sgk_event_slots_for(len) : sgk_jnn_slots_for(len); });
    SGK_TRY(j->slots.up(nr + 1, st));
    const int narr = ev ? 4 : 2;
    if (ev) {
        SGK_TRY(j->d_out[0].ensure(s * sizeof(sgk_event_rec_t)));
    } else {
        for (int k = 0; k < narr; ++k) SGK_TRY(j->d_out[k].ensure(s * 4));
    }
    SGK_TRY(j->cnt.d.ensure(nr));
    const bool evp = ev && j->has_ev_params;
    j->ws_bytes = evp ? sgk_event_workspace_bytes_param(j->n_reads, j->n_samples, j->max_len, &j->ev_opt, &j->ev_params)
                  : ev ? sgk_event_workspace_bytes_opt(j->n_reads, j->n_samples, j->max_len, &j->ev_opt)
                       : sgk_jnn_workspace_bytes(j->n_reads, j->n_samples, j->max_len);
    SGK_TRY(j->d_ws.ensure(j->ws_bytes));
    sgk_event_rec_t *recs = j->d_out[0].as<sgk_event_rec_t>();
    int32_t *x = j->d_out[0].as<int32_t>(), *y = j->d_out[1].as<int32_t>();
    if (evp)
        SGK_TRY(sgk_event_param(&view, &j->ev_params, j->slots.d.p, recs, j->cnt.d.p, j->d_ws.p, j->d_ws.cap, st, &j->ev_opt));
    else if (ev)
        SGK_TRY(sgk_event_opt(&view, rna, j->slots.d.p, recs, j->cnt.d.p, j->d_ws.p, j->d_ws.cap, st, &j->ev_opt));
    else if (j->has_jnn_params)
        SGK_TRY(sgk_jnn_param(&view, &j->jnn_params, j->slots.d.p, x, y, j->cnt.d.p, j->d_ws.p, j->d_ws.cap, st, &j->st_opt));
    else
        SGK_TRY(sgk_jnn_opt(&view, rna, j->slots.d.p, x, y, j->cnt.d.p, j->d_ws.p, j->d_ws.cap, st, &j->st_opt));
    if (!ev) SGK_TRY(fetch_long_hdr(j));
    j->n_dense = 0;
    if (flags & SGK_JOB_TEXT) {
        const bool compact = flags & (SGK_JOB_EVENTS_COMPACT | SGK_JOB_EVENTS_LENGTHS);
        return job_text_submit(j, compact ? SGK_TEXT_EVENT_COMPACT : SGK_TEXT_EVENT, view, s);
    }
    SGK_TRY(j->cnt.down(nr, st));
    const int ncopy = (ev && (flags & SGK_JOB_EVENTS_LENGTHS)) ? 1 : ((ev && (flags & SGK_JOB_EVENTS_COMPACT)) ? 2 : narr);
    SGK_TRY(j->doffs.d.ensure(nr + 1));
    SGK_TRY(launch_layout(j->cnt.d.p, j->slots.d.p, j->n_reads, 1u, j->doffs.d.p, st));
    GatherArgs g = {};
    for (int k = 0; k < ncopy; ++k) {
        SGK_TRY(j->d_dense[k].ensure(s * 4));
        g.src[k] = ev ? nullptr : j->d_out[k].as<uint32_t>();
        g.dst[k] = j->d_dense[k].as<uint32_t>();
    }
    if (ev)
        SGK_TRY(launch_gather_events(recs, g, ncopy, j->slots.d.p, j->cnt.d.p, j->doffs.d.p, j->n_reads, st));
    else
        SGK_TRY(launch_gather(g, ncopy, j->slots.d.p, j->cnt.d.p, j->doffs.d.p, j->n_reads, st));
    SGK_TRY(j->doffs.down(nr + 1, st));
    if (!ev) {  // sgk_jnn counts the reads whose segments overflowed their slots in the workspace's first word
        SGK_TRY(j->h_err.ensure(64));
        SGK_HIP_TRY(hipMemcpyAsync(j->h_err.p, j->d_ws.p, 4, hipMemcpyDeviceToHost, st));
    }
    j->n_dense = ncopy;
    return SGK_OK;
}

extern "C" int sgk_job_submit(sgk_job_t *j, int tool, int rna, int pore, int flags) {
    if (!j || !j->begun || j->submitted) return SGK_ERR_ARG;
    if (tool < SGK_TOOL_PA || tool > SGK_TOOL_ENT) return SGK_ERR_ARG;
    const bool text = (flags & SGK_JOB_TEXT) != 0;
    if (text && ((tool != SGK_TOOL_PA && tool != SGK_TOOL_EVENT) || !j->have_ids)) return SGK_ERR_ARG;
    if (text && tool == SGK_TOOL_PA && j->normalise) return SGK_ERR_ARG;  // the device formatter writes pA rows
    SGK_HIP_TRY(hipSetDevice(j->device));
    static const Result kinds[] = {Result::Pa, Result::Events, Result::Stat, Result::Segments, Result::Prefix, Result::Ent};
    static_assert(SGK_TOOL_PA == 0 && SGK_TOOL_EVENT == 1 && SGK_TOOL_STAT == 2 && SGK_TOOL_JNN == 3 && SGK_TOOL_PREFIX == 4 &&
                  SGK_TOOL_ENT == 5, "kinds[] is indexed by tool");
    j->tool = tool;
    j->result = text ? Result::TextRows : kinds[tool];
    j->flags = flags & (SGK_JOB_EVENTS_COMPACT | SGK_JOB_EVENTS_LENGTHS);
    if (j->n_reads == 0) return job_submit_empty(j, text);
    const size_t nr = j->n_reads;
    hipStream_t st = j->st;
    sgk_batch_t view;
    SGK_TRY(job_upload(j, &view));
    switch (tool) {
        case SGK_TOOL_PA: {
            if (text) {  // the rows are made from the int16 samples: no float array, on the device or over PCIe
                SGK_TRY(job_text_submit(j, SGK_TEXT_PA, view, j->n_samples));
                break;
            }
            const size_t bytes = j->n_samples * sizeof(float);
            SGK_TRY(j->d_out[0].ensure(bytes));
            if (j->normalise) {  // the float array that goes home is the normalised one; the records stay on the device
                SGK_TRY(j->d_out[1].ensure(nr * sizeof(sgk_norm_rec_t)));
                j->ws_bytes = sgk_normalise_workspace_bytes(j->n_reads, j->n_samples, j->max_len);
                SGK_TRY(j->d_ws.ensure(j->ws_bytes));
                SGK_TRY(sgk_normalise(&view, j->normalise, j->d_out[0].as<float>(), j->d_out[1].as<sgk_norm_rec_t>(), j->d_ws.p,
                                      j->d_ws.cap, st));
            } else
                SGK_TRY(sgk_pa(&view, j->d_out[0].as<float>(), st));
            SGK_TRY(fetch(j->h_out[0], j->d_out[0].p, bytes, st));
            break;
        }
        case SGK_TOOL_EVENT:
        case SGK_TOOL_JNN:
            SGK_TRY(job_items(j, view, tool == SGK_TOOL_EVENT, rna, flags));
            break;
        case SGK_TOOL_STAT: {
            const size_t bytes = nr * sizeof(sgk_stat_rec_t);
            SGK_TRY(j->d_out[0].ensure(bytes));
            j->ws_bytes = sgk_stat_workspace_bytes(j->n_reads, j->n_samples, j->max_len);
            SGK_TRY(j->d_ws.ensure(j->ws_bytes));
            SGK_TRY(sgk_stat_opt(&view, j->d_out[0].as<sgk_stat_rec_t>(), j->d_ws.p, j->d_ws.cap, st, &j->st_opt));
            SGK_TRY(fetch_long_hdr(j));
            SGK_TRY(fetch(j->h_out[0], j->d_out[0].p, bytes, st));
            break;
        }
        case SGK_TOOL_ENT: {
            const size_t ob = j->n_samples * sizeof(uint16_t);
            SGK_TRY(j->d_out[0].ensure(nr * sizeof(sgk_ent_hist_t)));
            SGK_TRY(j->d_out[1].ensure(ob));
            SGK_TRY(j->d_out[2].ensure(ob));
            SGK_TRY(sgk_ent(&view, j->d_out[0].as<sgk_ent_hist_t>(), j->d_out[1].as<uint16_t>(), j->d_out[2].as<uint16_t>(), st));
            SGK_TRY(fetch(j->h_out[0], j->d_out[0].p, nr * sizeof(sgk_ent_hist_t), st));
            break;  // the overflow lists are fetched by sgk_job_wait only when some read has entries
        }
        case SGK_TOOL_PREFIX: {
            const size_t bytes = nr * sizeof(sgk_prefix_rec_t);
            SGK_TRY(j->d_out[0].ensure(bytes));
            j->ws_bytes = sgk_prefix_workspace_bytes(j->n_reads, j->n_samples, j->max_len);
            SGK_TRY(j->d_ws.ensure(j->ws_bytes));
            sgk_prefix_rec_t *out = j->d_out[0].as<sgk_prefix_rec_t>();
            if (j->has_prefix_params)
                SGK_TRY(sgk_prefix_param(&view, rna, &j->prefix_params, out, j->d_ws.p, j->d_ws.cap, st, &j->st_opt));
            else
                SGK_TRY(sgk_prefix_opt(&view, rna, pore, out, j->d_ws.p, j->d_ws.cap, st, &j->st_opt));
            SGK_TRY(fetch_long_hdr(j));
            SGK_TRY(fetch(j->h_out[0], j->d_out[0].p, bytes, st));
            break;
        }
    }
    j->submitted = true;
    return SGK_OK;
}
