// api.hip -- C ABI of libsigtk_gpu.so (include/sigtk_gpu.h): error plumbing, per-kernel timing, the side-stream pool,
// the pa / event / synth entry points and their host-pointer layer.  (stat / jnn / prefix entry points live in
// api_stat.hip; what an event call plans, lays out and launches is event_plan.hip's.)
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

#include "event_args.h"
#include "host_util.h"
#include "sgk_common.h"
#include "side_stream.h"
#include "synth.h"

namespace sgk {

// ---------------------------------------------------------------- errors
static thread_local char g_hip_err[512] = "";

void set_hip_error(hipError_t e, const char *what, const char *file, int line) {
    snprintf(g_hip_err, sizeof g_hip_err, "%s: %s (%s:%d)", hipGetErrorName(e), what, file, line);
}

// ---------------------------------------------------------------- profiling
struct ProfRec {
    const char *name;
    hipEvent_t t0, t1;
    int device;  // the events belong to this device: it is made current again to read / destroy them
};
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;

ProfScope::ProfScope(const char *n, hipStream_t s) : name(n), stream(s), slot(-1) {
    if (!g_prof_on) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ProfRec r;
    r.name = n;
    r.device = 0;
    (void)hipGetDevice(&r.device);
    if (hipEventCreate(&r.t0) != hipSuccess) return;
    if (hipEventCreate(&r.t1) != hipSuccess) {
        (void)hipEventDestroy(r.t0);
        return;
    }
    (void)hipEventRecord(r.t0, s);
    g_prof.push_back(r);
    slot = (int)g_prof.size() - 1;
}
ProfScope::~ProfScope() {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lk(g_prof_mu);
    (void)hipEventRecord(g_prof[slot].t1, stream);
}

// ---------------------------------------------------------------- side streams (side_stream.h)
constexpr int SIDE_POOL = 4;
constexpr int SIDE_DEVICES = 64;
static SideSlot g_side[SIDE_DEVICES][SIDE_POOL];
static std::once_flag g_side_made[SIDE_DEVICES];
static std::atomic<unsigned> g_side_next[SIDE_DEVICES];

// Stream i of every slot is made before stream i + 1 of any: the runtime shares a few hardware queues among the
// streams in the order they are made, and the first streams are the ones every fork uses (made slot by slot, stat / jnn /
// prefix took 3 - 5 % longer on ragged batches with a 3 000 000-sample read).
static void side_make(SideSlot (&pool)[SIDE_POOL]) {
    for (int i = 0; i < SideSlot::N; ++i)
        for (SideSlot &x : pool)
            if (hipStreamCreateWithFlags(&x.s[i], hipStreamNonBlocking) != hipSuccess) x.s[i] = nullptr;
    for (SideSlot &x : pool) {
        bool ok = hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < SideSlot::N; ++i)
            ok = ok && x.s[i] && hipEventCreateWithFlags(&x.join[i], hipEventDisableTiming) == hipSuccess;
        x.ok = ok;
        if (ok) continue;
        for (int i = 0; i < SideSlot::N; ++i) {
            if (x.s[i]) (void)hipStreamDestroy(x.s[i]);
            if (x.join[i]) (void)hipEventDestroy(x.join[i]);
        }
        if (x.fork) (void)hipEventDestroy(x.fork);
    }
}

SideSlot *side_acquire() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SIDE_DEVICES) return nullptr;
    // the whole pool of a device is made by the first call that needs one (stream creation takes milliseconds: made
    // one by one, the first SIDE_POOL launches each paid for one -- a two-step warm-up was not enough)
    std::call_once(g_side_made[dev], [dev] { side_make(g_side[dev]); });
    // round-robin; a busy slot is passed over, and only when every slot is busy does the thread wait for one
    const unsigned first = g_side_next[dev].fetch_add(1u);
    SideSlot *wait_for = nullptr;
    for (unsigned k = 0; k < SIDE_POOL; ++k) {
        SideSlot &x = g_side[dev][(first + k) % SIDE_POOL];
        if (!x.ok) continue;
        if (x.mu.try_lock()) return &x;
        if (!wait_for) wait_for = &x;
    }
    if (wait_for) wait_for->mu.lock();
    return wait_for;
}

int launch_pa(const sgk_batch_t *b, float *out, hipStream_t st);
int launch_synth(int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, double *dig, double *off,
                 double *rng, uint32_t n_reads, uint32_t max_read_len, uint64_t first_read, uint64_t seed, int kind,
                 hipStream_t st);

int check_batch(const sgk_batch_t *b) {
    if (!b) return SGK_ERR_ARG;
    if (b->n_reads == 0) return SGK_OK;
    if (!b->samples || !b->offsets || !b->lengths || !b->digitisation || !b->offset || !b->range) return SGK_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(b->samples) & 15u) return SGK_ERR_ALIGN;
    if (b->n_samples & 7u) return SGK_ERR_ARG;
    return SGK_OK;
}

}  // namespace sgk

using namespace sgk;

// ====================================================================== C ABI

extern "C" {

const char *sgk_strerror(int code) {
    switch (code) {
        case SGK_OK: return "ok";
        case SGK_ERR_ARG: return "invalid argument";
        case SGK_ERR_HIP: return "HIP runtime error";
        case SGK_ERR_NODEVICE: return "no usable GPU";
        case SGK_ERR_WORKSPACE: return "workspace too small";
        case SGK_ERR_CAPACITY: return "output arena slot range too small";
        case SGK_ERR_ALIGN: return "buffer not sufficiently aligned";
        case SGK_ERR_NOMEM: return "host allocation failed";
        case SGK_ERR_FORMAT: return "malformed compressed signal";
        default: return "unknown sgk error";
    }
}

const char *sgk_version(void) { return SGK_VERSION_STRING; }
const char *sgk_last_hip_error(void) { return g_hip_err; }

int sgk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sgk_set_device(int ordinal) {
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    SGK_HIP_TRY(hipSetDevice(ordinal));
    return SGK_OK;
}

void sgk_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
}

void sgk_profile_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto &r : g_prof) {
        (void)hipSetDevice(r.device);
        (void)hipEventSynchronize(r.t1);
        (void)hipEventDestroy(r.t0);
        (void)hipEventDestroy(r.t1);
    }
    (void)hipSetDevice(cur);
    g_prof.clear();
}

int sgk_profile_read(const char **names, double *ms, uint32_t *calls, int cap) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    int k = 0;
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto &r : g_prof) {
        (void)hipSetDevice(r.device);  // records of several devices (sigtk-amd --gpus N) share the list
        if (hipEventSynchronize(r.t1) != hipSuccess) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, r.t0, r.t1) != hipSuccess) continue;
        int j = 0;
        for (; j < k; ++j)
            if (strcmp(names[j], r.name) == 0) break;
        if (j == k) {
            if (k >= cap) continue;
            names[k] = r.name;
            ms[k] = 0.0;
            calls[k] = 0;
            ++k;
        }
        ms[j] += (double)t;
        calls[j] += 1;
    }
    (void)hipSetDevice(cur);
    return k;
}

// ---------------------------------------------------------------- pa
int sgk_pa(const sgk_batch_t *batch, float *pa_out, void *stream) {
    const int rc = check_batch(batch);
    if (rc != SGK_OK) return rc;
    if (batch->n_reads == 0) return SGK_OK;
    if (!pa_out) return SGK_ERR_ARG;
    return launch_pa(batch, pa_out, static_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------- event
size_t sgk_event_workspace_bytes_opt(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len,
                                     const sgk_event_options_t *opt) {
    return event_workspace_layout(event_config(opt), n_reads, n_samples, max_read_len, 0).total;
}
size_t sgk_event_workspace_bytes(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len) {
    return sgk_event_workspace_bytes_opt(n_reads, n_samples, max_read_len, nullptr);
}

int sgk_event_opt(const sgk_batch_t *b, int rna, const uint64_t *ev_slots, sgk_event_rec_t *events, uint32_t *n_events,
                  void *ws, size_t ws_bytes, void *stream, const sgk_event_options_t *opt) {
    const int rc = check_batch(b);
    if (rc != SGK_OK) return rc;
    return run_event(event_batch(*b), {ev_slots, events, n_events, ws, ws_bytes, stream}, rna, nullptr, opt);
}
int sgk_event(const sgk_batch_t *b, int rna, const uint64_t *ev_slots, sgk_event_rec_t *events, uint32_t *n_events,
              void *ws, size_t ws_bytes, void *stream) {
    return sgk_event_opt(b, rna, ev_slots, events, n_events, ws, ws_bytes, stream, nullptr);
}

int sgk_event_pa_opt(const float *pa, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                     uint32_t max_read_len, uint64_t n_samples, int rna, const uint64_t *ev_slots,
                     sgk_event_rec_t *events, uint32_t *n_events, void *ws, size_t ws_bytes, void *stream,
                     const sgk_event_options_t *opt) {
    return run_event({pa, true, offsets, lengths, nullptr, nullptr, nullptr, n_reads, max_read_len, n_samples},
                     {ev_slots, events, n_events, ws, ws_bytes, stream}, rna, nullptr, opt);
}
int sgk_event_pa(const float *pa, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                 uint32_t max_read_len, uint64_t n_samples, int rna, const uint64_t *ev_slots,
                 sgk_event_rec_t *events, uint32_t *n_events, void *ws, size_t ws_bytes, void *stream) {
    return sgk_event_pa_opt(pa, offsets, lengths, n_reads, max_read_len, n_samples, rna, ev_slots, events, n_events, ws,
                            ws_bytes, stream, nullptr);
}

// pa -> event -> stat over one resident batch (BASELINE config 5): the fused stat + pA pass (per-read statistics and the pA
// array: two reads of the samples, one write), then event on the raw samples (it scales on the fly).
// (Round 5 also had the event BUILDER write the pA -- it converts every sample on its walk anyway -- with stat on the lane
// path: bit-identical, and not faster: 62.4 ms against 63.1 at 125 000 x 100 000; k_event went from 39 to 52 ms, 15.8 GB
// of traffic per 1e9 samples make it HBM-bound where it is issue-bound without.  profiles/r05_event_experiments.md.)
int sgk_pipeline(const sgk_batch_t *b, int rna, const uint64_t *ev_slots, sgk_event_rec_t *events, uint32_t *n_events,
                 float *pa_out, sgk_stat_rec_t *stat_out, void *event_ws, size_t event_ws_bytes, void *stat_ws,
                 size_t stat_ws_bytes, void *stream, const sgk_event_options_t *event_opt, const sgk_stat_options_t *stat_opt) {
    int rc = check_batch(b);
    if (rc != SGK_OK) return rc;
    if (!pa_out || !stat_out) return SGK_ERR_ARG;
    rc = sgk_stat_pa_opt(b, stat_out, pa_out, stat_ws, stat_ws_bytes, stream, stat_opt);
    if (rc != SGK_OK) return rc;
    return run_event(event_batch(*b), {ev_slots, events, n_events, event_ws, event_ws_bytes, stream}, rna, nullptr, event_opt);
}

// ---------------------------------------------------------------- event with caller-supplied parameters
int sgk_event_params_preset(int rna, sgk_event_params_t *out) {
    if (!out) return SGK_ERR_ARG;
    memset(out, 0, sizeof *out);
    out->window_length1 = rna ? 7u : 3u;
    out->window_length2 = rna ? 14u : 6u;
    out->threshold1 = rna ? 2.5f : 1.4f;
    out->threshold2 = 9.0f;
    out->peak_height = rna ? 1.0f : 0.2f;
    return SGK_OK;
}
int sgk_event_params_check(const sgk_event_params_t *p) {
    if (!p) return SGK_ERR_ARG;
    if (p->window_length1 < 2 || p->window_length1 > SGK_EVENT_W_MAX) return SGK_ERR_ARG;
    if (p->window_length2 < 2 || p->window_length2 > SGK_EVENT_W_MAX) return SGK_ERR_ARG;
    // a long window under 4 lets the long detector emit a peak two samples in front of a short peak that opens at the
    // emitting index (i - pos > w2 / 2 = 1): peaks 2 apart, which sgk_event_slots_for does not cover.  Equal windows
    // see the same statistic and cannot do that.
    if (p->window_length2 < 4 && p->window_length2 != p->window_length1) return SGK_ERR_ARG;
    const float f[3] = {p->threshold1, p->threshold2, p->peak_height};
    for (int k = 0; k < 3; ++k)
        if (!(f[k] >= 0.0f) || !(f[k] <= FLT_MAX)) return SGK_ERR_ARG;  // NaN fails both comparisons
    if (p->flags & ~(SGK_EVENT_PARAMS_GENERIC | SGK_EVENT_PARAMS_PRESET_KERNELS)) return SGK_ERR_ARG;
    return SGK_OK;
}
int sgk_event_params_route(const sgk_event_params_t *p) {
    if (sgk_event_params_check(p) != SGK_OK) return SGK_ERR_ARG;
    return event_params_route(p);
}
size_t sgk_event_workspace_bytes_param(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len,
                                       const sgk_event_options_t *opt, const sgk_event_params_t *p) {
    if (sgk_event_params_check(p) != SGK_OK) return 0;
    if (sgk_event_params_route(p) != SGK_EVENT_ROUTE_GENERIC) return sgk_event_workspace_bytes_opt(n_reads, n_samples, max_read_len, opt);
    return event_param_workspace_layout(n_reads, max_read_len).total;
}
int sgk_event_param(const sgk_batch_t *b, const sgk_event_params_t *p, const uint64_t *ev_slots, sgk_event_rec_t *events,
                    uint32_t *n_events, void *ws, size_t ws_bytes, void *stream, const sgk_event_options_t *opt) {
    if (sgk_event_params_check(p) != SGK_OK) return SGK_ERR_ARG;
    const int rc = check_batch(b);
    if (rc != SGK_OK) return rc;
    return run_event(event_batch(*b), {ev_slots, events, n_events, ws, ws_bytes, stream}, 0, p, opt);
}
int sgk_event_pa_param(const float *pa, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                       uint32_t max_read_len, uint64_t n_samples, const sgk_event_params_t *p, const uint64_t *ev_slots,
                       sgk_event_rec_t *events, uint32_t *n_events, void *ws, size_t ws_bytes, void *stream,
                       const sgk_event_options_t *opt) {
    if (!p) return SGK_ERR_ARG;   // (run_event checks the rest of them)
    return run_event({pa, true, offsets, lengths, nullptr, nullptr, nullptr, n_reads, max_read_len, n_samples},
                     {ev_slots, events, n_events, ws, ws_bytes, stream}, 0, p, opt);
}

int sgk_event_status(const void *ws, sgk_event_status_t *out, void *stream) {
    if (!ws || !out) return SGK_ERR_ARG;
    EvHeader h;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SGK_HIP_TRY(hipMemcpyAsync(&h, ws, sizeof h, hipMemcpyDeviceToHost, st));
    SGK_HIP_TRY(hipStreamSynchronize(st));
    out->n_fallback_reads = h.n_flagged;
    out->n_rerun_passes = h.n_rerun;
    out->n_capacity_overflow = h.n_overflow;
    out->n_long_replays = h.n_hot_runs;
    out->n_events_total = h.n_events_total;
    out->n_split_reads = h.n_long;   // (reads k_seg_plan could not place count here and under n_fallback_reads)
    out->n_segments = h.n_segs;
    out->n_seam_reruns = h.n_seam_rerun;
    out->reserved = 0;
    out->n_replay_indices = h.n_replay_idx;
    return h.n_overflow ? SGK_ERR_CAPACITY : SGK_OK;
}

int sgk_event_plan_opt(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len, int rna, const sgk_event_options_t *opt,
                       sgk_event_plan_t *out) {
    if (!out) return SGK_ERR_ARG;
    const EvPlan p = event_plan(event_config(opt), {n_reads, n_samples, max_read_len, rna});
    memset(out, 0, sizeof *out);
    out->segment_len = p.seg_len;
    out->long_min = p.long_min;
    out->max_segments = p.max_segs;   // (this preset's own: the workspace holds the larger of both presets')
    out->max_long_reads = p.max_long;
    out->short_max = p.multi_max;
    out->lanes_per_short_read = p.multi_lanes;
    out->warmup_override = (uint32_t)p.lead_override;
    out->tail_split_from = p.split_from;
    out->tail_segment_len = p.split_seg;
    return SGK_OK;
}
// the 0.1.0 form under its 0.1.0 name (0.2.0 / 0.2.1 had put the six-argument form under this symbol: a caller compiled
// against 0.1.0 then passed its `out` in the options' slot): the defaults, and only the 32 bytes that struct had
int sgk_event_plan(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len, int rna, void *out32) {
    if (!out32) return SGK_ERR_ARG;
    sgk_event_plan_t p;
    const int rc = sgk_event_plan_opt(n_reads, n_samples, max_read_len, rna, nullptr, &p);
    if (rc == SGK_OK) memcpy(out32, &p, 32);
    return rc;
}

// ---------------------------------------------------------------- synthetic reads
int sgk_synth_reads(int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, double *dig, double *off,
                    double *rng, uint32_t n_reads, uint32_t max_read_len, uint64_t first_read, uint64_t seed,
                    int kind, void *stream) {
    if (n_reads == 0) return SGK_OK;
    if (!samples || !offsets || !lengths || !dig || !off || !rng) return SGK_ERR_ARG;
    return launch_synth(samples, offsets, lengths, dig, off, rng, n_reads, max_read_len, first_read, seed, kind,
                        static_cast<hipStream_t>(stream));
}

void sgk_synth_reads_host(int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, double *dig,
                          double *off, double *rng, uint32_t n_reads, uint64_t first_read, uint64_t seed, int kind) {
    for (uint32_t r = 0; r < n_reads; ++r) {
        const int64_t n = (int64_t)lengths[r];
        const sgk_synth_read_t R = sgk_synth_read_init(seed, first_read + r, n, kind);
        dig[r] = SGK_SYNTH_DIGITISATION;
        off[r] = (double)R.offset;
        rng[r] = SGK_SYNTH_RANGE;
        for (int64_t i = 0; i < n; ++i) samples[offsets[r] + i] = sgk_synth_sample(R, i);
    }
}

// ====================================================================== Host API

int sgk_pa_host(const sgk_host_batch_t *hb, float *pa_out) {
    DeviceBatch db;
    int rc = db.upload(hb);
    if (rc != SGK_OK) return rc;
    if (hb->n_reads == 0) return SGK_OK;
    if (!pa_out) return SGK_ERR_ARG;
    DevBuf d_out;
    SGK_TRY(d_out.alloc((size_t)db.n_samples * sizeof(float)));
    SGK_TRY(sgk_pa(&db.view, d_out.as<float>(), nullptr));
    SGK_HIP_TRY(hipDeviceSynchronize());
    for (uint32_t r = 0; r < hb->n_reads; ++r) {
        if (!db.lengths[r]) continue;
        SGK_HIP_TRY(hipMemcpy(pa_out + hb->offsets[r], d_out.as<float>() + db.offsets[r],
                              (size_t)db.lengths[r] * sizeof(float), hipMemcpyDeviceToHost));
    }
    return SGK_OK;
}

// shared tail of sgk_event_host / sgk_getevents: run on an uploaded batch view (raw or pA input)
static int event_collect(const void *d_samples, bool float_input, const DeviceBatch &db, const sgk_batch_t *view,
                         int rna, sgk_events_host_t *out, const sgk_event_options_t *opt = nullptr,
                         const sgk_event_params_t *params = nullptr) {
    const uint32_t nr = (uint32_t)db.lengths.size();
    memset(out, 0, sizeof *out);
    out->n_reads = nr;
    out->ev_offsets = (uint64_t *)calloc((size_t)nr + 1, sizeof(uint64_t));
    if (!out->ev_offsets) return SGK_ERR_NOMEM;
    if (nr == 0) return SGK_OK;
    const std::vector<uint64_t> slots = make_slots(db.lengths, [](uint32_t n) { return sgk_event_slots_for(n); });
    const uint64_t nslots = slots[nr];
    DevBuf d_slots, d_ev, d_nev, d_ws;
    int rc;
    SGK_TRY(d_slots.alloc((nr + 1) * sizeof(uint64_t)));
    SGK_TRY(d_ev.alloc(nslots * sizeof(sgk_event_rec_t)));
    SGK_TRY(d_nev.alloc((size_t)nr * 4));
    const size_t wsb = params ? sgk_event_workspace_bytes_param(nr, db.n_samples, db.max_len, opt, params)
                              : sgk_event_workspace_bytes_opt(nr, db.n_samples, db.max_len, opt);
    SGK_TRY(d_ws.alloc(wsb));
    SGK_HIP_TRY(hipMemcpy(d_slots.p, slots.data(), (nr + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    // (an uploaded view is a valid batch; the view of pA input has no scaling arrays)
    const EvBatch b = {d_samples, float_input, view->offsets, view->lengths, view->digitisation, view->offset, view->range,
                       nr, db.max_len, db.n_samples};
    rc = run_event(b, {d_slots.as<uint64_t>(), d_ev.as<sgk_event_rec_t>(), d_nev.as<uint32_t>(), d_ws.p, wsb, nullptr}, rna,
                   params, opt);
    if (rc != SGK_OK) return rc;
    rc = sgk_event_status(d_ws.p, &out->status, nullptr);
    if (rc != SGK_OK) return rc;
    std::vector<uint32_t> nev(nr);
    SGK_HIP_TRY(hipMemcpy(nev.data(), d_nev.p, (size_t)nr * 4, hipMemcpyDeviceToHost));
    uint64_t tot = 0;
    for (uint32_t r = 0; r < nr; ++r) {
        out->ev_offsets[r] = tot;
        tot += nev[r];
    }
    out->ev_offsets[nr] = tot;
    out->start = (uint32_t *)malloc((tot ? tot : 1) * 4);
    out->length = (uint32_t *)malloc((tot ? tot : 1) * 4);
    out->mean = (float *)malloc((tot ? tot : 1) * 4);
    out->stdv = (float *)malloc((tot ? tot : 1) * 4);
    if (!out->start || !out->length || !out->mean || !out->stdv) return SGK_ERR_NOMEM;
    // one bulk copy of the records (capacity layout), compacted and split into the four arrays on the host
    std::vector<sgk_event_rec_t> tmp((size_t)nslots ? (size_t)nslots : 1);
    SGK_HIP_TRY(hipMemcpy(tmp.data(), d_ev.p, (size_t)nslots * sizeof(sgk_event_rec_t), hipMemcpyDeviceToHost));
    for (uint32_t r = 0; r < nr; ++r) {
        // an overflowing read keeps what fitted
        const uint64_t cap = slots[r + 1] - slots[r];
        const uint64_t k = nev[r] < cap ? nev[r] : cap;
        const sgk_event_rec_t *src = tmp.data() + slots[r];
        const uint64_t o = out->ev_offsets[r];
        for (uint64_t i = 0; i < k; ++i) {
            out->start[o + i] = src[i].start;
            out->length[o + i] = src[i].length;
            out->mean[o + i] = src[i].mean;
            out->stdv[o + i] = src[i].stdv;
        }
    }
    return SGK_OK;
}

int sgk_event_host_opt(const sgk_host_batch_t *hb, int rna, sgk_events_host_t *out, const sgk_event_options_t *opt) {
    if (!out) return SGK_ERR_ARG;
    memset(out, 0, sizeof *out);
    DeviceBatch db;
    int rc = db.upload(hb);
    if (rc != SGK_OK) return rc;
    rc = event_collect(db.view.samples, false, db, &db.view, rna, out, opt);
    if (rc != SGK_OK) sgk_events_host_free(out);
    return rc;
}
int sgk_event_host(const sgk_host_batch_t *hb, int rna, sgk_events_host_t *out) {
    return sgk_event_host_opt(hb, rna, out, nullptr);
}

void sgk_events_host_free(sgk_events_host_t *ev) {
    if (!ev) return;
    free(ev->ev_offsets);
    free(ev->start);
    free(ev->length);
    free(ev->mean);
    free(ev->stdv);
    memset(ev, 0, sizeof *ev);
}

// ---------------------------------------------------------------- per-read shims
float *sgk_signal_in_picoamps(const int16_t *raw, uint64_t n, double digitisation, double offset, double range) {
    float *out = (float *)malloc(sizeof(float) * (n ? n : 1));
    if (!out) return nullptr;
    const uint64_t offs[2] = {0, n};
    sgk_host_batch_t hb = {raw, offs, &digitisation, &offset, &range, 1};
    if (sgk_pa_host(&hb, out) != SGK_OK) {
        free(out);
        return nullptr;
    }
    return out;
}

static sgk_event_table getevents_impl(size_t nsample, float *rawptr, int rna, const sgk_event_params_t *params) {
    sgk_event_table et;
    memset(&et, 0, sizeof et);
    if (params && sgk_event_params_check(params) != SGK_OK) return et;
    if (!rawptr || nsample == 0 || nsample > 0x7fffffffull || sgk_device_count() <= 0) return et;
    DeviceBatch db;  // only offsets/lengths bookkeeping is used here
    db.offsets.assign(1, 256);  // head/tail room for the event fast path
    db.lengths.assign(1, (uint32_t)nsample);
    db.max_len = (uint32_t)nsample;
    db.n_samples = round_up(nsample, 64) + 320;
    DevBuf d_pa, d_o, d_l;
    if (d_pa.alloc((size_t)db.n_samples * sizeof(float)) != SGK_OK) return et;
    if (d_o.alloc(8) != SGK_OK || d_l.alloc(4) != SGK_OK) return et;
    if (hipMemset(d_pa.p, 0, (size_t)db.n_samples * sizeof(float)) != hipSuccess) return et;
    if (hipMemcpy(d_pa.as<float>() + 256, rawptr, nsample * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return et;
    if (hipMemcpy(d_o.p, db.offsets.data(), 8, hipMemcpyHostToDevice) != hipSuccess) return et;
    if (hipMemcpy(d_l.p, db.lengths.data(), 4, hipMemcpyHostToDevice) != hipSuccess) return et;
    sgk_batch_t view;
    memset(&view, 0, sizeof view);
    view.offsets = d_o.as<uint64_t>();
    view.lengths = d_l.as<uint32_t>();
    sgk_events_host_t ev;
    if (event_collect(d_pa.p, true, db, &view, rna, &ev, nullptr, params) != SGK_OK) {
        sgk_events_host_free(&ev);
        return et;
    }
    const size_t k = (size_t)ev.ev_offsets[1];
    et.event = (sgk_event_t *)calloc(k ? k : 1, sizeof(sgk_event_t));
    if (et.event) {
        et.n = k;
        et.start = 0;
        et.end = k;
        for (size_t i = 0; i < k; ++i) {
            et.event[i].start = ev.start[i];
            et.event[i].length = (float)ev.length[i];
            et.event[i].mean = ev.mean[i];
            et.event[i].stdv = ev.stdv[i];
        }
    }
    sgk_events_host_free(&ev);
    return et;
}
sgk_event_table sgk_getevents(size_t nsample, float *rawptr, int8_t rna) {
    return getevents_impl(nsample, rawptr, rna, nullptr);
}
sgk_event_table sgk_getevents_param(size_t nsample, float *rawptr, const sgk_event_params_t *params) {
    sgk_event_table et;
    memset(&et, 0, sizeof et);
    if (!params) return et;
    return getevents_impl(nsample, rawptr, 0, params);
}

}  // extern "C"
