// event_plan.hip -- host side of `event`, in front of the launches: how a batch is laid out and what its kernels get.
// The caller's options become a configuration (event_config), the batch's totals a plan (event_plan: long-read geometry,
// dispatch order, short-read packing, tail split, segment capacities), both presets' plans a workspace layout; run_event
// fills the kernels' arguments from them.  It holds no kernel and includes no device header (unit map: event_device.h).
#include <string.h>

#include <mutex>

#include "event_args.h"
#include "stat_args.h"

namespace sgk {

// ---------------------------------------------------------------- event options -> configuration
// (no process-wide state: every entry point derives its configuration from the caller's options)
EvSegConfig event_config(const sgk_event_options_t *o) {
    EvSegConfig c;
    c.dev = 0;
    c.seg_len = 131072;    // one wavefront's share of a long read: ~0.6 ms of detector + builder
    c.long_min = 262144;   // reads at least this long are cut into segments
    c.lead_override = 0;
    c.multi = 0;
    c.multi_max = 0;
    c.tail_split = 0;
    c.auto_geometry = !o || (o->segment_len == 0 && o->long_min == 0);
    if (!o) return c;
#ifdef SGK_DEV
    c.dev = o->reserved[0];
#endif
    if (o->segment_len >= 1024 && o->segment_len <= (1u << 30)) c.seg_len = o->segment_len / 1024 * 1024;
    if (o->long_min >= 1) c.long_min = o->long_min;
    if (c.long_min <= c.seg_len) c.long_min = c.seg_len + 1;  // a long read has at least two segments
    if (o->warmup >= 16 && o->warmup <= 512) c.lead_override = o->warmup / 16 * 16;
    if (o->lanes_per_short_read < 0) c.multi = -1;
    else if (o->lanes_per_short_read > 0) {
        int p = 1;
        while (p * 2 <= o->lanes_per_short_read && p < 32) p *= 2;
        c.multi = p;
    }
    if (o->short_max >= 1024) {
        uint32_t p2 = 1024;
        while (p2 < (1u << 30) && (uint64_t)p2 * 2 <= o->short_max) p2 *= 2;
        c.multi_max = p2;
    }
    c.tail_split = o->tail_split < 0 ? -1 : o->tail_split;   // (> 0: that many reads are cut, whatever the batch)
    return c;
}

// Resident wavefront slots of the current device for the event kernels (CUs x 4 SIMDs x waves per SIMD: 3 with the
// DNA preset, 2 with RNA parameters)
static uint32_t event_wave_slots(int rna) {
    static std::mutex mu;
    static int cus[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (cus[dev] == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        cus[dev] = v;
    }
    return (uint32_t)cus[dev] * 4u * (rna ? 2u : 3u);
}

// From what length on a read is shared by several wavefronts, per batch (round 5).  A read should be cut when its one
// wavefront would outlast the rest of the batch -- which depends on the batch: at 10 000 x 100 000 samples (a third of
// a millisecond per 100 000 samples and wave, 3.6 ms per batch) reads up to 262 144 samples finish inside it and cutting
// them only costs (log-normal lengths around 100 000, 10^9 samples: 3.59 ms with 131 072-sample segments from 262 144 on,
// 3.72 with 65 536 from 131 072 on); at 3 000 such reads the same geometry leaves the GPU waiting for a few 200 000-sample
// reads (1.85 ms against 1.49; 3 000 x 100 000 + 16 x 250 000: 1.65 against 1.15).  The batch's samples per wave slot are
// what a wave's share of it is: long_min = 0.9 of that, between 131 072 and 262 144; segments of half of it.
// tests/test_gpu_event_long.py::test_long_read_threshold_is_no_cliff times both ends of the range on both kinds of batch.
static EvSegConfig event_config_for(const EvSegConfig &c0, uint64_t n_samples, int rna) {
    EvSegConfig c = c0;
    if (!c.auto_geometry) return c;
    uint64_t lm = n_samples / event_wave_slots(rna) * 9u / 10u;
    lm = (lm + 2047u) / 2048u * 2048u;
    lm = lm < 131072u ? 131072u : (lm > 262144u ? 262144u : lm);
    c.long_min = (uint32_t)lm;
    c.seg_len = (uint32_t)(lm / 2u);
    return c;
}

// Short reads.  On all 64 lanes a 5 000-sample read spends more steps on warm-ups (lead per lane) than on its samples;
// k_event_multi gives a read fewer lanes and a wave several reads.  Worth it when the batch has enough reads to fill
// the GPU that way (>= 4 rounds of waves) -- a small batch wants every lane it can get.  `sorted`: the batch gets a
// dispatch order (its short reads are the order's tail); without one the batch must be short as a whole.
static void event_multi_plan(const EvSegConfig &sc, const EvTotals &t, EvPlan &p) {
    p.multi_lanes = 0;
    // (RNA parameters: warm-ups of 128 / 256 samples make the 64-lane layout 1.3 x its samples' worth up to ~64 k
    // samples: 33 333 x 30 000 samples 6.15 -> 5.13 ms; DNA parameters: 32 / 64, 20 000-sample reads already cost what
    // 100 000-sample reads cost.  Above that the packed kernel's per-lane read parameters cost more than they save:
    // two 100 000-sample reads per wave are 6-9 % slower than one.)
    p.multi_max = sc.multi_max ? sc.multi_max : (t.rna ? 65536u : 16384u);
    if (t.n_reads == 0) return;
    const uint64_t mean = t.n_samples / t.n_reads;
    if (sc.multi >= 0 && mean < p.multi_max && (p.sorted || t.max_read_len < p.multi_max)) {
        const uint32_t lead = sc.lead_override > 0 ? (uint32_t)sc.lead_override : (t.rna ? 128u : 32u);
        uint32_t lanes = 1;
        while (lanes < 64 && (uint64_t)lanes * 2 * 8 * lead <= mean) lanes *= 2;       // chunks of >= 8 warm-ups
        while (lanes < 64 && (uint64_t)t.n_reads * lanes < 64ull * 4 * 3072) lanes *= 2;  // >= 4 rounds of waves
        if (sc.multi > 0) lanes = (uint32_t)sc.multi;
        if (lanes < 64) p.multi_lanes = lanes;
    }
}

// The tail split (event_device.h: seg_len_of).  A batch of fewer than 8 rounds of waves whose last round is a SMALL
// fraction of one: the reads of that round (the last dispatch positions) are cut into segments, as many per read as fill
// a round (up to 8), never shorter than 16 384 samples.  Not in a batch with packed short reads (they balance by
// themselves), not for reads under 32 768 samples on average.
// A cut read costs ~1.5 x a whole one (every lane of every segment warms up, the chain waits for the segment in front,
// the builder starts from the last boundary in front of it), so cutting pays only where FEW reads would otherwise keep
// the whole GPU waiting.  The rule is fitted to whole-call times of the shipped kernels with the split forced on / off
// over 50 batch sizes per preset (tools/tail_sweep.py -> profiles/r05_tail_split_sweep.txt, 100 000-sample reads), and
// tests/test_gpu_event_long.py::test_tail_split_rule_is_no_cliff times both either side of every cut of it:
//   a batch of less than one round of waves: DNA preset up to 0.55 of a round (1 536 reads 0.88 -> 0.65 ms; a tie from
//     0.58 on), RNA preset up to 7 / 8 of one (1 024 reads 1.12 -> 0.78 ms, 1 877 reads 1.31 -> 1.25);
//   a longer batch, DNA preset: the last round at most a quarter of a round behind ONE full round (3 840 reads 1.54 ->
//     1.48 ms), a sixth behind more (9 728 reads 3.56 -> 3.42; 9 984 reads 3.54 -> 3.60);
//   a longer batch, RNA preset: never -- at two waves per SIMD the first waves of a round are done at half time and a
//     small surplus runs in their slots (2 218 reads 1.55 ms whole, 1.72 split); the best case gains 6 %, most lose.
// (Round 4's rule -- any last round under 7 / 8 full -- was tuned on a kernel whose whole reads were 6 % slower; the
// first rule of round 5, a sixth / a third, came from a sweep of an instrumented build and left 25 % on the table for
// batches of 1 100 - 1 600 reads: the guard test's first run found that.)
static void event_tail_plan(const EvSegConfig &sc, const EvTotals &t, EvPlan &p) {
    const uint32_t n_reads = t.n_reads;
    p.split_from = n_reads;
    p.split_seg = 0;
    if (n_reads == 0 || p.multi_lanes != 0 || sc.tail_split < 0) return;
    const uint32_t slots = event_wave_slots(t.rna);
    const uint64_t mean = t.n_samples / n_reads;
    if (mean < 32768 || (sc.tail_split == 0 && n_reads >= 8ull * slots)) return;
    uint32_t rem = n_reads % slots;
    if (sc.tail_split > 0) rem = (uint32_t)sc.tail_split < n_reads ? (uint32_t)sc.tail_split : n_reads;   // the caller's number
    else if (n_reads < slots) {
        if (t.rna ? (uint64_t)n_reads * 8u > (uint64_t)slots * 7u : (uint64_t)n_reads * 20u > (uint64_t)slots * 11u) return;
    } else if (rem == 0 || t.rna || rem * (n_reads < 2u * slots ? 4u : 6u) > slots) return;
    // (the number of segments per read hardly matters: 2 .. 16 per read, one or two rounds of them: 3.77 - 3.89 ms)
    uint32_t G = (slots - slots / 16 + rem - 1) / rem;   // units of the split reads ~ one round
    if (G < 2) G = 2;
    if (G > 8) G = 8;
    uint64_t seg = (mean + G - 1) / G;
    seg = (seg + 1023) / 1024 * 1024;
    if (seg < 16384) seg = 16384;
    if (seg >= sc.long_min) return;   // (reads that long are cut anyway)
    p.split_from = n_reads - rem;
    p.split_seg = (uint32_t)seg;
}

static void event_seg_capacity(const EvSegConfig &c, const EvTotals &t, EvPlan &p) {
    uint64_t ns = 0, ml = 0;
    if (t.max_read_len >= c.long_min) {
        uint64_t nl = t.n_samples / c.long_min;
        if (nl > t.n_reads) nl = t.n_reads;
        if (nl < 1) nl = 1;
        ns = t.n_samples / c.seg_len + nl;  // sum of ceil(n_r / seg_len) over at most nl reads
        // every long read has at least two segments; k_seg_plan admits long reads while their segments fit
        ml = ns / 2;
        if (ml < nl) ml = nl;
    }
    if (p.split_seg) {
        // the split reads: at most n_reads - split_from of them, each under long_min samples
        const uint64_t nsplit = t.n_reads - p.split_from;
        ns += nsplit * (((uint64_t)c.long_min + p.split_seg - 1) / p.split_seg);
        ml += nsplit;
    }
    if (ml > t.n_reads) ml = t.n_reads;
    p.max_segs = ns > 0x7fffffffull ? 0x7fffffffu : (uint32_t)ns;
    p.max_long = (uint32_t)ml;
}

// longest-first dispatch only pays when lengths differ: a batch of equal-length reads is launched in batch order
static bool batch_ragged(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len) {
    return (uint64_t)max_read_len * n_reads > n_samples + n_samples / 4;
}

EvPlan event_plan(const EvSegConfig &c0, const EvTotals &t) {
    const EvSegConfig c = event_config_for(c0, t.n_samples, t.rna);
    EvPlan p;
    p.seg_len = c.seg_len;
    p.long_min = c.long_min;
    p.lead_override = c.lead_override;
    p.dev = c.dev;
    p.ragged = batch_ragged(t.n_reads, t.n_samples, t.max_read_len);
    p.sorted = p.ragged && t.n_reads >= ORDER_MIN_READS;   // (launch_event sorts from ORDER_MIN_READS reads on)
    event_multi_plan(c, t, p);
    event_tail_plan(c, t, p);      // (whether the short reads are packed decides)
    event_seg_capacity(c, t, p);   // (the long reads' segments and the tail split's)
    p.has_long = t.max_read_len >= c.long_min;
    return p;
}

// ---------------------------------------------------------------- workspace layouts
EvWorkspace event_workspace_layout(const EvSegConfig &c, uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len,
                                   size_t available) {
    EvWorkspace w;
    const uint64_t nr = n_reads ? n_reads : 1;
    size_t o = 0;
    w.off_hdr = o;     o += sizeof(EvHeader);
    w.off_flags = o;   o += round_up(nr, 64);
    w.off_list = o;    o += round_up(nr * 4, 64);
    w.off_order = o;   o += round_up(nr * 4 + 128 * 4, 64);
    w.off_bitmap = o;  o += round_up((n_samples / 64 + nr + 2) * 8, 64);
    // (the layout does not know the preset: the larger of the two presets' capacities)
    const EvPlan p0 = event_plan(c, {n_reads, n_samples, max_read_len, 0}), p1 = event_plan(c, {n_reads, n_samples, max_read_len, 1});
    w.max_segs = p0.max_segs > p1.max_segs ? p0.max_segs : p1.max_segs;
    w.max_long = p0.max_long > p1.max_long ? p0.max_long : p1.max_long;
    w.off_segs = o;       o += round_up((size_t)w.max_segs * sizeof(SegDesc), 64);
    w.off_seg_state = o;  o += round_up((size_t)w.max_segs * sizeof(SegState), 64);
    w.off_longs = o;      o += round_up((size_t)w.max_long * sizeof(LongRead), 64);
    w.off_scratch = o;
    w.scratch_stride = round_up(2ull * ((uint64_t)max_read_len + 1), 2);
    const size_t per_block = (size_t)w.scratch_stride * sizeof(double);
    uint64_t nb = nr < 256 ? nr : 256;  // persistent fallback blocks (each owns a scratch region)
    // default sizing: keep the scratch under 2 GiB even for multi-million-sample reads (fewer, still >= 1, blocks)
    const uint64_t budget = (2ull << 30) / per_block;
    if (nb > budget) nb = budget ? budget : 1;
    if (available) {
        const size_t room = available > o ? available - o : 0;
        uint64_t fit = room / per_block;
        if (fit > 256) fit = 256;
        if (fit > nr) fit = nr;
        nb = fit;
    }
    w.n_fb_blocks = (uint32_t)nb;
    w.total = o + (size_t)nb * per_block;
    return w;
}

// Workspace of k_event_param: header, dispatch order, and per persistent workgroup the prefix arrays and the bitmap of
// the longest read.  Nothing here depends on the batch's total samples.
EvParamWorkspace event_param_workspace_layout(uint32_t n_reads, uint32_t max_read_len) {
    EvParamWorkspace w;
    const uint64_t nr = n_reads ? n_reads : 1;
    size_t o = 0;
    w.off_hdr = o;    o += sizeof(EvHeader);
    w.off_order = o;  o += round_up(nr * 4 + 128 * 4, 64);
    w.off_scratch = o;
    const uint64_t L = max_read_len;
    w.scratch_stride = round_up(2 * (L + 1) + (L / 64 + 2), 8);  // in doubles: 64-byte multiples
    const size_t per_block = (size_t)w.scratch_stride * sizeof(double);
    uint64_t nb = nr < PARAM_MAX_BLOCKS ? nr : PARAM_MAX_BLOCKS;
    const uint64_t budget = PARAM_SCRATCH_BUDGET / per_block;
    if (nb > budget) nb = budget ? budget : 1;
    w.n_blocks = (uint32_t)nb;
    w.total = o + (size_t)nb * per_block;
    return w;
}

// ---------------------------------------------------------------- caller-supplied detector parameters: the route
static bool params_equal_preset(const sgk_event_params_t *p, int rna) {
    sgk_event_params_t q;
    sgk_event_params_preset(rna, &q);
    return p->window_length1 == q.window_length1 && p->window_length2 == q.window_length2 &&
           memcmp(&p->threshold1, &q.threshold1, 4) == 0 && memcmp(&p->threshold2, &q.threshold2, 4) == 0 &&
           memcmp(&p->peak_height, &q.peak_height, 4) == 0;
}
// The presets' windows with the caller's thresholds on the presets' kernels (<.., RT = true>): the fast pass skips the
// long detector where it proves the statistic <= 9 (sgk_long_cold), which says "not > threshold2" from 9.0f on.
static bool params_preset_windows(const sgk_event_params_t *p) {
    const bool win = (p->window_length1 == 3 && p->window_length2 == 6) || (p->window_length1 == 7 && p->window_length2 == 14);
    return win && p->threshold2 >= 9.0f;
}
// the one routing decision (sgk_event_params_route); `p` has passed sgk_event_params_check
int event_params_route(const sgk_event_params_t *p) {
    if (p->flags & SGK_EVENT_PARAMS_GENERIC) return SGK_EVENT_ROUTE_GENERIC;
    if (params_equal_preset(p, 0) || params_equal_preset(p, 1)) return SGK_EVENT_ROUTE_PRESET;
    if ((p->flags & SGK_EVENT_PARAMS_PRESET_KERNELS) && params_preset_windows(p)) return SGK_EVENT_ROUTE_PRESET_WINDOWS;
    return SGK_EVENT_ROUTE_GENERIC;
}

// ---------------------------------------------------------------- batch + plan + layout -> kernel arguments
static int check_event_io(const EvBatch &b, const EvArena &o) {
    if (!b.samples || !b.offsets || !b.lengths || !o.ev_slots || !o.events || !o.n_events || !o.ws) return SGK_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(b.samples) & 15u) return SGK_ERR_ALIGN;
    if (reinterpret_cast<uintptr_t>(o.events) & 15u) return SGK_ERR_ALIGN;
    if (reinterpret_cast<uintptr_t>(o.ws) & 63u) return SGK_ERR_ALIGN;
    return SGK_OK;
}

// the batch and the arena, which EvArgs begins with in this order; everything behind them zero
static EvArgs event_args(const EvBatch &b, const EvArena &o) {
    return {b.samples, b.offsets, b.lengths, b.dig, b.off, b.rng, b.n_reads, b.n_samples, o.ev_slots, o.events, o.n_events};
}

// the presets' kernels.  rt: the thresholds of the <.., RT = true> instances (SGK_EVENT_ROUTE_PRESET_WINDOWS; rna says
// which windows)
static int run_event_preset(EvArgs a, const EvBatch &b, const EvArena &o, int rna, const sgk_event_params_t *rt,
                            const sgk_event_options_t *opt) {
    const EvSegConfig sc = event_config(opt);
    const EvPlan p = event_plan(sc, {b.n_reads, b.n_samples, b.max_read_len, rna});
    const EvWorkspace w = event_workspace_layout(sc, b.n_reads, b.n_samples, b.max_read_len, o.ws_bytes);
    if (w.n_fb_blocks == 0 || w.total > o.ws_bytes) return SGK_ERR_WORKSPACE;
    char *base = static_cast<char *>(o.ws);
    a.hdr = reinterpret_cast<EvHeader *>(base + w.off_hdr);
    a.flags = reinterpret_cast<uint8_t *>(base + w.off_flags);
    a.flag_list = reinterpret_cast<uint32_t *>(base + w.off_list);
    a.order = p.ragged ? reinterpret_cast<uint32_t *>(base + w.off_order) : nullptr;
    a.bitmap = reinterpret_cast<unsigned long long *>(base + w.off_bitmap);
    a.scratch = reinterpret_cast<double *>(base + w.off_scratch);
    a.scratch_stride = w.scratch_stride;
    // (the layout's capacities, the larger over both presets: max_segs is k_event_seg's grid)
    a.max_segs = w.max_segs;
    a.max_long = w.max_long;
    a.seg_len = p.seg_len;
    a.long_min = p.long_min;
    a.lead_override = p.lead_override;
    a.dev = p.dev;
    a.segs = reinterpret_cast<SegDesc *>(base + w.off_segs);
    a.seg_state = reinterpret_cast<SegState *>(base + w.off_seg_state);
    a.longs = reinterpret_cast<LongRead *>(base + w.off_longs);
    a.multi_lanes = p.multi_lanes;
    a.multi_max = p.multi_max;
    a.split_from = p.split_from;
    a.split_seg = p.split_seg;
    a.has_long = p.has_long ? 1u : 0u;
    a.thr1 = rt ? rt->threshold1 : 0.0f;
    a.thr2 = rt ? rt->threshold2 : 0.0f;
    a.ph = rt ? rt->peak_height : 0.0f;
    return launch_event(a, rna, b.float_input, w.n_fb_blocks, static_cast<hipStream_t>(o.stream), rt != nullptr);
}

// the generic kernel (k_event_param)
static int run_event_generic(EvArgs a, const EvBatch &b, const EvArena &o, const sgk_event_params_t *p, int lead_override) {
    const EvParamWorkspace w = event_param_workspace_layout(b.n_reads, b.max_read_len);
    if (w.total > o.ws_bytes) return SGK_ERR_WORKSPACE;
    char *base = static_cast<char *>(o.ws);
    a.hdr = reinterpret_cast<EvHeader *>(base + w.off_hdr);
    a.order = batch_ragged(b.n_reads, b.n_samples, b.max_read_len) ? reinterpret_cast<uint32_t *>(base + w.off_order) : nullptr;
    a.scratch = reinterpret_cast<double *>(base + w.off_scratch);
    a.scratch_stride = w.scratch_stride;
    // the warm-up scales with the windows (a statistic looks w samples back); results do not depend on it
    const uint32_t wmax = p->window_length1 > p->window_length2 ? p->window_length1 : p->window_length2;
    const int lead = lead_override > 0 ? lead_override : (int)(4 * wmax < 64 ? 64 : 4 * wmax);
    const EvParamArgs pa = {p->window_length1, p->window_length2, p->threshold1, p->threshold2, p->peak_height, lead, b.max_read_len};
    return launch_event_param(a, pa, b.float_input, w.n_blocks, static_cast<hipStream_t>(o.stream));
}

int run_event(const EvBatch &b, const EvArena &o, int rna, const sgk_event_params_t *params, const sgk_event_options_t *opt) {
    int route = SGK_EVENT_ROUTE_PRESET;
    if (params) {
        if (sgk_event_params_check(params) != SGK_OK) return SGK_ERR_ARG;
        route = event_params_route(params);
        rna = params->window_length1 == 7 ? 1 : 0;   // (both presets' kernels: the plan follows the windows)
    }
    if (b.n_reads == 0) return SGK_OK;
    const int rc = check_event_io(b, o);
    if (rc != SGK_OK) return rc;
    if (route == SGK_EVENT_ROUTE_GENERIC) return run_event_generic(event_args(b, o), b, o, params, event_config(opt).lead_override);
    return run_event_preset(event_args(b, o), b, o, rna, route == SGK_EVENT_ROUTE_PRESET_WINDOWS ? params : nullptr, opt);
}

}  // namespace sgk

#ifdef SGK_DEV
// development builds only: where in the workspace the fallback scratch -- SGK_DEV_TRACE's records -- begins
extern "C" size_t sgk_debug_scratch_offset(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len,
                                           const sgk_event_options_t *opt, size_t ws_bytes) {
    return sgk::event_workspace_layout(sgk::event_config(opt), n_reads, n_samples, max_read_len, ws_bytes).off_scratch;
}
#endif
