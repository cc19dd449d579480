/* sigtk_gpu.h -- C ABI of libsigtk_gpu.so: sigtk's per-read raw-signal hot path
 * (pa / event / stat / jnn / prefix) as batched HIP kernels for AMD MI355X (gfx950).
 *
 * The reference (hasindu2008/sigtk, C99, single-threaded) has no FFI layer: its seam is
 * the per-record function-pointer slot `void (*func)(slow5_rec_t*, opt_t)` in
 * src/cmain.c:95-120 and, below it, the compute entry points declared in
 * src/sigtk.h:124-134 and src/jnn.h:104-109.  This header is what a sigtk maintainer
 * would bind instead of those entry points (see INTEGRATION.md for the stub):
 *
 *   reference (file:line)                         replaced by
 *   --------------------------------------------  -------------------------------------
 *   signal_in_picoamps   src/misc.c:15            sgk_pa            / sgk_signal_in_picoamps
 *   getevents            src/events.c:553         sgk_event         / sgk_getevents
 *   meanf..mediani16     src/stat.h:17-73         sgk_stat
 *   jnn_raw/jnn_print    src/jnn.c:282,309        sgk_jnn
 *   find_adaptor/jnnv2   src/jnn.c:99,181         sgk_prefix
 *   find_polya/jnn_pa    src/jnn.c:295,352        sgk_prefix
 *   prefix_func compute  src/cfunc.c:169-216      sgk_prefix
 *   entropy (ent)        src/ent.c:25-50,107-164  sgk_ent + sgk_ent_finish
 *   qts quantisers       src/qts.c:27-43,126-142  sgk_qts
 *   svb-zd decode/encode slow5_press.c:1063-1146  sgk_svbzd_decode / sgk_svbzd_size + sgk_svbzd_encode
 *   the record loop      src/cmain.c:118-120      sgk_job_* (pipelined batches: staging, stream, results)
 *
 * Conventions
 *   - Plain C: pointers and sizes only.  No exceptions, no exit(): every function returns
 *     SGK_OK (0) or a negative sgk error code; sgk_strerror() names it.
 *   - "Device API" functions take DEVICE pointers and a hipStream_t passed as void*
 *     (NULL = default stream) and only enqueue work; nothing is synchronised.
 *   - "Jobs" (sgk_job_*) are the throughput path for host callers: pinned staging the caller fills, asynchronous
 *     upload / kernels / download on a private stream, results in pinned buffers; several can be in flight.
 *   - "Host API" functions (suffix _host and the per-read shims) take HOST pointers,
 *     stage through the GPU and synchronise before returning.  Results they allocate are
 *     released with the matching *_free function.
 *   - The library never falls back to a CPU implementation: without a usable GPU every
 *     compute entry point returns SGK_ERR_NODEVICE / SGK_ERR_HIP.
 *
 * Batch layout (structure of arrays, one batch = many reads):
 *   samples  int16 raw samples of all reads in one buffer; 16-byte aligned; n_samples is the
 *            readable length of the buffer in samples and must be a multiple of 8;
 *   offsets  n_reads sample indices, lengths n_reads sample counts: read r is
 *            samples[offsets[r] .. offsets[r]+lengths[r]).  Reads must be stored in
 *            increasing, non-overlapping order; gaps between reads are allowed (and ignored),
 *            which lets a packer start every read on an aligned boundary.  Any offsets are
 *            accepted; reads starting on a multiple of 8 samples (16 bytes) take the
 *            vectorised load paths (the host packer aligns to 64 samples = 128 bytes).  The
 *            event fast path additionally wants >= 64 (DNA) / 256 (RNA parameters) readable samples in front of
 *            a read and >= 16 behind it (neighbouring reads or padding, any content); reads without that room, or
 *            starting on an odd sample, are processed by the slower exact fallback kernel;
 *   digitisation/offset/range  the three per-read doubles of slow5_rec_t
 *            (slow5lib/include/slow5/slow5_defs.h:84-92), narrowed to float on the device
 *            exactly as src/misc.c:17-19 does.
 */
#ifndef SIGTK_GPU_H
#define SIGTK_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 0.2.0: per-call options (sgk_event_options_t, sgk_stat_options_t) replace the process-wide sgk_event_configure* and
 * the environment variables of 0.1.0; sgk_event_plan takes the options; sgk_event_plan_t / sgk_event_status_t as below.
 * Bindings should compare sgk_version() with the header they were written against.
 * 0.2.1: sgk_stat_options_t::long_min (was reserved), sgk_stat_long_status, sgk_stat_plan; sgk_stat / sgk_jnn / sgk_prefix_workspace_bytes
 *        ask for the long reads' records as well (an older, smaller workspace still works: long reads then run on one
 *        wavefront).
 * 0.2.2: the long-read path of stat / jnn / prefix declines a read whose workgroups time out at a barrier and the wave
 *        kernel redoes it (no result depends on the long path having worked; sgk_long_status_t::n_timeouts counts those
 *        reads); sgk_stat_options_t::debug_fault (was reserved[0]); sgk_job_long_declined; sgk_inflate, SGK_SIGNAL_ZREC / sgk_job_begin_zrec;
 *        the six-argument plan call is sgk_event_plan_opt; sgk_event_plan is the 0.1.0 five-argument form again (deprecated).
 * 0.2.3: SGK_JOB_EVENTS_LENGTHS (additive submit flag).  Additive to 0.2.3 (no version change): sgk_sigtext_decode;
 *        SGK_SIGNAL_TEXT for sgk_job_begin; sgk_ss_* (`ss paf2tsv`: decode, text, host pipe); sgk_zstd_decompress,
 *        SGK_RECORD_ZLIB / SGK_RECORD_ZSTD and sgk_job_begin_zrec_format (BLOW5 files with zstd records);
 *        sgk_aux_field_t, sgk_zrec_tail_check and sgk_job_begin_zrec_aux (records with variable-length auxiliary fields);
 *        sgk_deflate, sgk_deflate_bound, sgk_deflate_block_bytes, sgk_job_set_record_frames and SGK_QTS_RECORDS with the
 *        qts_record* fields at the end of sgk_job_output_t (`qts --gpu-deflate`: records deflated on the GPU);
 *        sgk_slow5_text_* and SGK_SIGNAL_TEXT as input and output format of sgk_job_submit_qts (`qts` on text SLOW5);
 *        SGK_QTS_ZREC_FRAMES (`qts --gpu-inflate`: the frames of the record mode taken from the records inflated on the GPU);
 *        sgk_sigraw_unit_samples, sgk_sigraw_gather and sgk_job_begin_zrec_signal (compressed records around an uncompressed signal).
 *        The literal medians (additive to 0.2.3, no version change: every 0.2.3 caller keeps working): pA medians that are a
 *        pick among equal-comparing or unordered values (a zero; a unit or offset that is not finite) are the element the
 *        reference's selection leaves at n / 2.  sgk_stat / sgk_stat_pa / sgk_prefix redo them on scratch rows that
 *        sgk_stat_workspace_bytes / sgk_prefix_workspace_bytes now ask for: min(n_reads, 1024) rows of 2 max_read_len bytes,
 *        fewer rows where that would pass SGK_LITERAL_MAX_BYTES (256 MiB), never less than one.  A smaller workspace, down
 *        to the 0.2.3 size, still works: with fewer rows fewer workgroups share the work; with none such a median is
 *        pA(raw order statistic) as before, its record keeps SGK_MEDIAN_INEXACT / SGK_MEDIAN_INEXACT_POLYA in `reserved`, and
 *        sgk_stat_literal_status counts it. */
#define SGK_VERSION_STRING "0.2.3"

/* ---- error codes --------------------------------------------------------------- */
#define SGK_OK 0
#define SGK_ERR_ARG (-1)        /* NULL / inconsistent argument                         */
#define SGK_ERR_HIP (-2)        /* a HIP runtime call failed (sgk_last_hip_error())      */
#define SGK_ERR_NODEVICE (-3)   /* no usable GPU                                        */
#define SGK_ERR_WORKSPACE (-4)  /* workspace too small (see *_workspace_bytes)          */
#define SGK_ERR_CAPACITY (-5)   /* an output arena slot range was too small             */
#define SGK_ERR_ALIGN (-6)      /* samples buffer not 16-byte aligned                   */
#define SGK_ERR_NOMEM (-7)      /* host allocation failed                               */
#define SGK_ERR_FORMAT (-8)     /* malformed compressed signal (svb-zd blob)            */

const char *sgk_strerror(int code);
const char *sgk_version(void);
/* text of the last failing HIP call on this thread ("" if none) */
const char *sgk_last_hip_error(void);
/* number of visible GPUs (0 if none / HIP unusable); never fails */
int sgk_device_count(void);
/* bind the calling thread to a GPU ordinal */
int sgk_set_device(int ordinal);

/* pore ids, as OPT_PORE_* in src/sigtk.h:50-52 */
#define SGK_PORE_R9 0
#define SGK_PORE_R10 1
#define SGK_PORE_RNA004 2

/* ---- batch view (device pointers) ---------------------------------------------- */
typedef struct sgk_batch {
    const int16_t *samples;
    const uint64_t *offsets;   /* n_reads: first sample of each read */
    const uint32_t *lengths;   /* n_reads: samples in each read (len_raw_signal) */
    const double *digitisation;
    const double *offset;
    const double *range;
    uint32_t n_reads;
    uint32_t max_read_len; /* max over reads of lengths[r]; host-known */
    uint64_t n_samples;    /* readable length of `samples` (multiple of 8; all reads lie inside) */
} sgk_batch_t;

/* ---- pa: int16 -> picoamps (src/misc.c:15-32) ----------------------------------- */
/* pa_out[offsets[r]+i] for every sample i of every read r (same layout as `samples`;
 * gap samples are not written). */
int sgk_pa(const sgk_batch_t *batch, float *pa_out, void *stream);

/* ---- event: Scrappie-derived event detection (src/events.c:553) ------------------ */
/* One event = event_t of src/sigtk.h:55-62 with integer start / length (16 bytes). */
typedef struct sgk_event_rec {
    uint32_t start;   /* first raw sample of the event                       */
    uint32_t length;  /* samples (event_t.length is this number as a float)  */
    float mean;       /* pA                                                  */
    float stdv;       /* pA                                                  */
} sgk_event_rec_t;
/* Events of read r are written to events[ev_slots[r] .. ev_slots[r]+n_events[r]-1] (16-byte aligned array of
 * records).  ev_slots (device, n_reads+1, increasing) is an INPUT describing the arena: read r may use at most
 * ev_slots[r+1]-ev_slots[r] slots.  sgk_event_slots_for() gives a capacity that can never overflow (peaks are at
 * least 3 samples apart).  If a read would overflow, its surplus events are dropped, n_events[r] still holds the
 * true count and the status word reports it (sgk_event_status -> SGK_ERR_CAPACITY).
 * Where the reference aborts or is undefined the library defines: a read with no peak
 * (incl. reads shorter than 2*window) yields one event [0,n); empty reads yield none. */
static inline uint64_t sgk_event_slots_for(uint64_t n_samples_of_read) { return n_samples_of_read / 3 + 2; }

/* (the tail split is planned from the CURRENT device's compute units -- 256 without one: size a workspace with the
 * device the launch will use current, sgk_set_device; a workspace sized for another device makes the launch return
 * SGK_ERR_WORKSPACE, never write out of bounds) */
size_t sgk_event_workspace_bytes(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len);

int sgk_event(const sgk_batch_t *batch, int rna, const uint64_t *ev_slots, sgk_event_rec_t *events,
              uint32_t *n_events, void *workspace, size_t workspace_bytes, void *stream);

/* Same path fed with pA floats instead of raw int16 (drop-in for getevents(), whose input
 * is the pA array): pa is packed like `samples` (float per sample, 16-byte aligned). */
int sgk_event_pa(const float *pa, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                 uint32_t max_read_len, uint64_t n_samples, int rna, const uint64_t *ev_slots,
                 sgk_event_rec_t *events, uint32_t *n_events, void *workspace, size_t workspace_bytes, void *stream);

typedef struct sgk_event_status {
    uint32_t n_fallback_reads;   /* reads re-done by the sequential-prefix exact path (no room around the read,
                                  * the exactness guard on the sample magnitudes failed, inf/nan samples, or
                                  * more than 512 event boundaries within 2048 samples): same results, slower */
    uint32_t n_rerun_passes;     /* speculative chunk boundaries that needed a re-run     */
    uint32_t n_capacity_overflow;/* reads whose events did not fit their slot range       */
    uint32_t n_long_replays;     /* lanes (chunks) in which a run of the lazily evaluated long detector could not be
                                  * proven silent and was re-played exactly (diagnostic)  */
    uint64_t n_events_total;
    uint32_t n_split_reads;      /* reads taken by several wavefronts: long reads (from long_min samples on, in
                                  * segments of segment_len) and the reads of the tail split */
    uint32_t n_segments;         /* their segments                                         */
    uint32_t n_seam_reruns;      /* segments whose speculative start was wrong and that were run again */
    uint32_t reserved;
    uint64_t n_replay_indices;   /* indices the exact replay of the long detector walked (diagnostic: one lane each) */
} sgk_event_status_t;
/* Per-call options of the event path.  All zero (or a null pointer) = the defaults.  The library keeps no mutable
 * process-wide configuration and reads no environment variable: two callers in one process may use different options
 * at the same time; size a workspace with the options the call will use.  Results do not depend on any of them.
 *   segment_len / long_min   a read of at least long_min samples is cut into segments of segment_len samples (a multiple
 *                            of 1024), one wavefront each      (both 0: chosen per batch -- long_min = 0.9 x the
 *                            batch's samples per wavefront slot, between 131 072 and 262 144, segments of half of it;
 *                            sgk_event_plan_opt tells)
 *   warmup                   speculative warm-up in samples, a multiple of 16, <= 512  (0: the presets' own; tests use
 *                            16 to make speculation fail at every few chunk boundaries)
 *   lanes_per_short_read     short reads (< short_max samples) in large batches: a wavefront takes 64 / lanes reads,
 *                            lanes lanes each (a power of two, 1 .. 32)           (0: chosen per batch, -1: off)
 *   short_max                (0: 16 384, 65 536 with RNA parameters; a power of two >= 1024)
 *   tail_split               a batch of fewer than 8 rounds of wavefronts: the reads of its last, partial round are cut
 *                            into segments so that the GPU drains on small units  (0: chosen per batch -- where it
 *                            was measured to pay: a small batch, a small last round, DESIGN.md 3.1 --, -1: off,
 *                            n > 0: the last n reads are cut whatever the batch -- tuning / tests) */
typedef struct sgk_event_options {
    uint32_t segment_len, long_min;
    int32_t warmup;
    int32_t lanes_per_short_read;
    uint32_t short_max;
    int32_t tail_split;
    uint32_t reserved[2];
} sgk_event_options_t; /* 32 bytes */
size_t sgk_event_workspace_bytes_opt(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len,
                                     const sgk_event_options_t *opt);
int sgk_event_opt(const sgk_batch_t *batch, int rna, const uint64_t *ev_slots, sgk_event_rec_t *events,
                  uint32_t *n_events, void *workspace, size_t workspace_bytes, void *stream,
                  const sgk_event_options_t *opt);
int sgk_event_pa_opt(const float *pa, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                     uint32_t max_read_len, uint64_t n_samples, int rna, const uint64_t *ev_slots,
                     sgk_event_rec_t *events, uint32_t *n_events, void *workspace, size_t workspace_bytes, void *stream,
                     const sgk_event_options_t *opt);

/* How sgk_event_opt would take a batch with these totals under `opt` (host only, no GPU work; the tail split assumes
 * the current device's CU count, 256 without a device): the segment geometry and list capacities of the long reads, the
 * threshold and the lanes per read of the short ones (0: every read has a wavefront of its own), the tail split.
 * Run it with the device the launch will use current (sgk_set_device): so must sgk_event_workspace_bytes(_opt). */
typedef struct sgk_event_plan {
    uint32_t segment_len, long_min;         /* long reads: >= long_min samples, cut into segments of segment_len */
    uint32_t max_segments, max_long_reads;  /* capacities reserved in the workspace (0: no read is cut)           */
    uint32_t short_max;                     /* reads under this many samples are short ...                      */
    uint32_t lanes_per_short_read;          /* ... and get this many lanes each (0: packing is off for the batch) */
    uint32_t warmup_override;               /* 0: the presets' warm-ups                                          */
    uint32_t tail_split_from;               /* tail split: reads at dispatch positions >= this (n_reads: none) ... */
    uint32_t tail_segment_len;              /* ... are cut into segments of this many samples (0: none)           */
    uint32_t reserved[3];
} sgk_event_plan_t;
int sgk_event_plan_opt(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len, int rna,
                       const sgk_event_options_t *opt, sgk_event_plan_t *out);
/* Deprecated: the 0.1.0 call under its 0.1.0 name and signature -- the defaults, and only the first 32 bytes of the
 * struct (what sgk_event_plan_t was then: up to warmup_override + one reserved word).  0.2.0 / 0.2.1 had the
 * six-argument form under this symbol; it is sgk_event_plan_opt now, so that no caller can bind the wrong one. */
int sgk_event_plan(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len, int rna, void *out32);

/* Synchronises `stream`, copies the status block of the last sgk_event on this workspace.
 * Returns SGK_ERR_CAPACITY if any read overflowed its slots. */
int sgk_event_status(const void *workspace, sgk_event_status_t *out, void *stream);

/* ---- event with caller-supplied detector parameters (additive to 0.2.3) --------------------------------------------
 * The five numbers of detector_param (src/events.c:35-41) that sgk_event fixes to one of two presets by `rna`.  For a
 * read of n samples the events are, bit for bit, those of the reference's own steps with these numbers: pA, the
 * sequential double prefix sums (events.c:293-303), compute_tstat with window_length1 and with window_length2
 * (:315-364), short_long_peak_detector (:371-443), create_event between consecutive peaks (:457-504).  Where the
 * reference is undefined sgk_event's definitions hold: no peak gives one event [0,n), an empty read none, a window with
 * n < 2w an all-zero statistic.  pA input with NaN or infinite samples (sgk_event_pa_param): the bits of NaN fields are
 * undefined.
 *   Domain: 2 <= window_length1, window_length2 <= SGK_EVENT_W_MAX, in any relation to each other -- except that a
 *   window_length2 of 2 or 3 must equal window_length1 (see Capacity); threshold1, threshold2, peak_height finite and
 *   >= 0 (FLT_MAX: "never"); flags holds known bits only.  Anything else is SGK_ERR_ARG and nothing is launched.
 *   Capacity: over this domain peak positions are strictly increasing and at least 3 apart, so sgk_event_slots_for(n)
 *   bounds the events of a read as it does for the presets (DESIGN.md 3.16 has the argument, tests/
 *   test_event_params_cpu.py checks it).  The excluded corner is where that fails: with window_length2 < 4 the long
 *   detector emits as soon as i - pos > 1, which can be the index at which a short peak opens -- two peaks 2 apart.
 *   A slot range smaller than a read's events behaves as in sgk_event: the surplus is dropped, n_events[r] holds the
 *   true count and sgk_event_status returns SGK_ERR_CAPACITY.
 *   Routing (sgk_event_params_route is the one decision every entry point uses):
 *     SGK_EVENT_ROUTE_PRESET          parameters that equal a preset bit for bit, without SGK_EVENT_PARAMS_GENERIC, whatever
 *                                     else flags holds: sgk_event_opt's kernels through sgk_event_opt's launch (same results,
 *                                     same time, same status fields, workspace as sgk_event_workspace_bytes_opt).
 *     SGK_EVENT_ROUTE_PRESET_WINDOWS  opt-in by SGK_EVENT_PARAMS_PRESET_KERNELS, without SGK_EVENT_PARAMS_GENERIC: windows
 *                                     3 / 6 or 7 / 14 and threshold2 >= 9.0f, any threshold1 and peak_height of the domain.
 *                                     The presets' kernels compiled with the three thresholds as run-time arguments, planned
 *                                     and launched like sgk_event_opt with rna = (window_length1 == 7): every field of `opt`
 *                                     applies, the status is filled as for sgk_event_opt, the workspace is
 *                                     sgk_event_workspace_bytes_opt's (and, as there, a smaller one is accepted while
 *                                     the scratch of at least one fallback workgroup fits).  Why 9: the fast kernels
 *                                     skip the long detector wherever they prove its statistic <= 9, which is then not
 *                                     > threshold2 either; where the proof fails the long detector is replayed exactly
 *                                     with the caller's threshold2 and peak_height (DESIGN.md 3.16 goes through every
 *                                     site and lists the kernels' registers, spills, scratch and LDS).
 *     SGK_EVENT_ROUTE_GENERIC         everything else, and everything with SGK_EVENT_PARAMS_GENERIC (both flags: generic).
 *   The generic route takes the kernel k_event_param: one wavefront per read of any length, reads dispatched
 *   longest first; of `opt` only `warmup` applies there (results do not depend on it); of the status it fills
 *   n_rerun_passes, n_capacity_overflow and n_events_total, the rest are zero.
 *   Workspace of the generic kernel: 64 + 4 n_reads + 512 bytes (rounded up to 64) + B x S, where
 *   B = min(n_reads, 1024) persistent workgroups and S = 16 (max_read_len + 1) + 8 (max_read_len / 64 + 2) bytes rounded
 *   up to 64 (two prefix arrays and a peak bitmap for the longest read); B is lowered (never below 1) to keep B x S under
 *   2 GiB.  It does not grow with n_samples.  sgk_event_workspace_bytes_param is the single source of truth; a smaller
 *   workspace gives SGK_ERR_WORKSPACE and nothing is written. */
#define SGK_EVENT_W_MAX 64
#define SGK_EVENT_PARAMS_GENERIC 1u /* flags: take the generic kernel even for a preset (tests, measurements) */
#define SGK_EVENT_PARAMS_PRESET_KERNELS 4u /* flags: the presets' kernels with run-time thresholds where the domain allows
                                             (bit 2u is not assigned: like every unknown bit it is SGK_ERR_ARG) */
#define SGK_EVENT_ROUTE_PRESET 0
#define SGK_EVENT_ROUTE_PRESET_WINDOWS 1
#define SGK_EVENT_ROUTE_GENERIC 2
typedef struct sgk_event_params {
    uint32_t window_length1, window_length2;
    float threshold1, threshold2, peak_height;
    uint32_t flags, reserved[2];
} sgk_event_params_t; /* 32 bytes */
/* host only: the preset sgk_event uses for `rna` (0: 3 / 6 / 1.4 / 9.0 / 0.2, else 7 / 14 / 2.5 / 9.0 / 1.0), flags 0 */
int sgk_event_params_preset(int rna, sgk_event_params_t *out);
/* host only: SGK_OK when `p` lies in the domain above, else SGK_ERR_ARG */
int sgk_event_params_check(const sgk_event_params_t *p);
/* host only: the route these parameters take, SGK_EVENT_ROUTE_*; SGK_ERR_ARG when sgk_event_params_check refuses them */
int sgk_event_params_route(const sgk_event_params_t *p);
size_t sgk_event_workspace_bytes_param(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len,
                                       const sgk_event_options_t *opt, const sgk_event_params_t *p);
int sgk_event_param(const sgk_batch_t *batch, const sgk_event_params_t *p, const uint64_t *ev_slots,
                    sgk_event_rec_t *events, uint32_t *n_events, void *workspace, size_t workspace_bytes, void *stream,
                    const sgk_event_options_t *opt);
int sgk_event_pa_param(const float *pa, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                       uint32_t max_read_len, uint64_t n_samples, const sgk_event_params_t *p, const uint64_t *ev_slots,
                       sgk_event_rec_t *events, uint32_t *n_events, void *workspace, size_t workspace_bytes, void *stream,
                       const sgk_event_options_t *opt);

/* ---- stat: per-read mean/std/median of raw and pA (src/stat.h, src/cfunc.c:126-159) */
typedef struct sgk_stat_rec {
    float raw_mean, pa_mean, raw_std, pa_std;
    int32_t raw_median;
    float pa_median;
    uint32_t n;
    uint32_t reserved;   /* 0, or SGK_MEDIAN_INEXACT: see below */
} sgk_stat_rec_t; /* 32 bytes per read */
/* `reserved` of a stat / prefix record after the call: pa_median / adapt_median (SGK_MEDIAN_INEXACT) or polya_median
 * (SGK_MEDIAN_INEXACT_POLYA) is a zero, or the read's unit or offset is not finite, and the workspace had no scratch row
 * to redo it with the reference's selection: the value is pA(raw order statistic), which can differ from the reference's
 * in the sign of a zero, or in inf against NaN.  Never set with a workspace of sgk_*_workspace_bytes. */
#define SGK_MEDIAN_INEXACT 4u
#define SGK_MEDIAN_INEXACT_POLYA 8u

size_t sgk_stat_workspace_bytes(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len);
int sgk_stat(const sgk_batch_t *batch, sgk_stat_rec_t *out, void *workspace, size_t workspace_bytes,
             void *stream);
/* fused stat + pa (BASELINE config 4): one launch sequence producing both outputs */
int sgk_stat_pa(const sgk_batch_t *batch, sgk_stat_rec_t *out, float *pa_out, void *workspace,
                size_t workspace_bytes, void *stream);

/* ---- jnn: state-machine segmenter on raw signal (src/jnn.c:190-350) --------------- */
/* Segments of read r go to slots seg_slots[r].. (same arena convention as events);
 * seg_x/seg_y are jnn_pair_t (src/jnn.h:13-16) as SoA with 32-bit members. */
/* sgk_jnn may use ALL slots of a read as scratch (the wave-per-read kernel stages kept segments in the upper half
 * before merging them into the lower half): only the first n_segs[r] entries are results afterwards. */
static inline uint64_t sgk_jnn_slots_for(uint64_t n_samples_of_read) { return n_samples_of_read / 32 + 2; }
size_t sgk_jnn_workspace_bytes(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len);
int sgk_jnn(const sgk_batch_t *batch, int rna, const uint64_t *seg_slots, int32_t *seg_x, int32_t *seg_y,
            uint32_t *n_segs, void *workspace, size_t workspace_bytes, void *stream);

/* ---- prefix: adaptor / polyA finder (src/cfunc.c:169-216, src/jnn.c:99-188,352-374) */
typedef struct sgk_prefix_rec {
    int32_t adapt_x, adapt_y;  /* find_adaptor(): -1/-1 read too short, 0/0 none found  */
    int32_t polya_x, polya_y;  /* find_polya(), RELATIVE to adapt_y; -1/-1 if none      */
    float adapt_mean, adapt_std, adapt_median;
    float polya_mean, polya_std, polya_median;
    uint32_t n;
    uint32_t reserved;   /* 0, or SGK_MEDIAN_INEXACT | SGK_MEDIAN_INEXACT_POLYA */
} sgk_prefix_rec_t; /* 48 bytes per read */

size_t sgk_prefix_workspace_bytes(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len);
int sgk_prefix(const sgk_batch_t *batch, int rna, int pore, sgk_prefix_rec_t *out, void *workspace,
               size_t workspace_bytes, void *stream);

/* Per-call options of stat / jnn / prefix (null = defaults).  The library has two implementations of these subtools:
 * one read per wavefront (round 2; any batch) and one read per lane (round 1; wins on large batches of short reads of
 * similar length: stat >= 49 152 reads of <= 32 768 samples or >= 16 384 reads of <= 16 384 (without the pA output also
 * >= 81 920 reads of <= 131 072), jnn >= 65 536 reads of <= 12 288 samples,
 * the longest <= 1.5 x the mean; prefix: the wave finders, and the lane kernels for the statistics of the regions they find
 * when the batch has >= 49 152 reads; sgk_stat_plan tells).  kernels: 0 chosen per batch,
 * 1 one read per lane, 2 one read per wavefront.  Results do not depend on it (the tests compare the two bit for bit). */
typedef struct sgk_stat_options {
    int32_t kernels;
    int32_t long_min;   /* reads of at least this many samples get 16 workgroups (64 wavefronts) of their own before
                         * the wave-per-read kernel runs (sequential float sums composed from tile summaries, stat's
                         * histogram and pA output, jnn's automaton): 0 = chosen per batch and tool, max(n_samples / 2048 (jnn: / 3072),
                         * a floor between 131 072 and 262 144 by the size of the batch; sgk_stat_plan tells)
                         * -- the reads one wavefront would still be busy with when the rest of the batch is done (and
                         * none if that still lists more than 128 reads: a batch of similar long reads balances itself);
                         * -1 = never; else the threshold (>= 8 192).  Results do not depend on it.  Needs the workspace
                         * sgk_*_workspace_bytes asks for (with less, such reads run on one wavefront). */
    uint32_t debug_fault; /* 0.  Tests only: fault injection into the long-read path's barriers (a withheld workgroup /
                           * a tiny spin bound, see lc_barrier in csrc/stat_long.hip) to exercise the decline-and-redo path */
    uint32_t reserved;
} sgk_stat_options_t;
int sgk_stat_opt(const sgk_batch_t *batch, sgk_stat_rec_t *out, void *workspace, size_t workspace_bytes, void *stream,
                 const sgk_stat_options_t *opt);
int sgk_stat_pa_opt(const sgk_batch_t *batch, sgk_stat_rec_t *out, float *pa_out, void *workspace,
                    size_t workspace_bytes, void *stream, const sgk_stat_options_t *opt);
int sgk_jnn_opt(const sgk_batch_t *batch, int rna, const uint64_t *seg_slots, int32_t *seg_x, int32_t *seg_y,
                uint32_t *n_segs, void *workspace, size_t workspace_bytes, void *stream, const sgk_stat_options_t *opt);
int sgk_prefix_opt(const sgk_batch_t *batch, int rna, int pore, sgk_prefix_rec_t *out, void *workspace,
                   size_t workspace_bytes, void *stream, const sgk_stat_options_t *opt);
/* ---- the pa -> event -> stat pipeline over one batch (BASELINE config 5; src/cfunc.c:72-83, 85-102, 126-159) -------- */
/* One call for what `pa`, `event` and `stat` print of the same reads: pa_out as sgk_pa, events as sgk_event_opt, stat_out as
 * sgk_stat_opt -- the fused stat + pA pass, then event on the raw samples; workspaces as for sgk_event_opt and
 * sgk_stat_pa_opt.  0.2.2. */
int sgk_pipeline(const sgk_batch_t *batch, int rna, const uint64_t *ev_slots, sgk_event_rec_t *events, uint32_t *n_events,
                 float *pa_out, sgk_stat_rec_t *stat_out, void *event_workspace, size_t event_workspace_bytes,
                 void *stat_workspace, size_t stat_workspace_bytes, void *stream, const sgk_event_options_t *event_opt,
                 const sgk_stat_options_t *stat_opt);

/* What the long-read path of the last stat / jnn / prefix call on `workspace` did (copied from the device: call it when
 * the stream has drained).  A long read's sequential float sums (src/stat.h:17-54, src/jnn.c:106-124, 195-199) are
 * composed from per-tile summaries; n_true_tiles of the n_tiles tile sums had to be evaluated from the true accumulator
 * instead (binade crossings, mispredicted binades).  All zero when the call had no long read or no room for them. */
/* What a stat (tool 0) / jnn (1) / prefix (2) / stat_pa (3) call would do with a batch of these totals (host arithmetic only, no GPU):
 * which implementation kernels = 0 resolves to, the long-read threshold it uses (0: no read of the batch can be long)
 * and how many long reads it accepts (under the per-batch threshold more than that many and none is treated as long;
 * under an explicit one the surplus runs on one wavefront each), the workspace sgk_*_workspace_bytes asks for. */
typedef struct sgk_stat_plan {
    uint32_t kernels;         /* 1: one read per lane, 2: one read per wavefront */
    uint32_t long_min;
    uint32_t long_max_reads;
    uint32_t reserved;
    uint64_t workspace_bytes;
} sgk_stat_plan_t;
int sgk_stat_plan(int tool, uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len, const sgk_stat_options_t *opt,
                  sgk_stat_plan_t *out);
/* The table behind kernels = 0, one row per tool (0 stat, 1 jnn, 3 stat + pA, 4 the region statistics of prefix): a batch
 * of similar read lengths takes the lane-per-read kernels iff n_reads >= min_reads and its longest read has at most
 * min(cap, slope_x1024 * n_reads / 1024 + intercept) samples.  Returns the number of rows; fills at most cap of them.
 * (0.2.2; the guard test times both implementations either side of that line.) */
typedef struct sgk_stat_lane_rule {
    uint32_t tool, min_reads, slope_x1024;
    int32_t intercept;
    uint32_t cap, reserved;
} sgk_stat_lane_rule_t;
int sgk_stat_lane_rules(sgk_stat_lane_rule_t *out, int cap);
typedef struct sgk_long_status {
    uint32_t n_long_reads, n_tiles, n_true_tiles;
    uint32_t n_timeouts;  /* long reads DECLINED by the long path: a workgroup of the read gave up at a barrier (after
                           * seconds: never on a GPU of its own) or was told that another one had.  Nothing of such a read
                           * is written by the long path; the wave-per-read kernel redoes it on one wavefront behind the
                           * join, so the results are right either way (0.2.1 left them wrong and only counted here);
                           * jobs report the count through sgk_job_long_declined() */
} sgk_long_status_t;
int sgk_stat_long_status(const void *workspace, size_t workspace_bytes, uint32_t n_reads, sgk_long_status_t *out);
/* the last sgk_stat / sgk_stat_pa / sgk_prefix call on this workspace (synchronises): medians redone with the reference's
 * own selection, and medians that would have been but for the workspace (their records keep SGK_MEDIAN_INEXACT*) */
#define SGK_LITERAL_MAX_BYTES (256u << 20) /* what the scratch rows add to sgk_stat / sgk_prefix_workspace_bytes at most
                                            * (one row, 2 max_read_len bytes, if a single read is longer than that) */
typedef struct sgk_literal_status {
    uint32_t n_literal, n_inexact;
} sgk_literal_status_t;
int sgk_stat_literal_status(const void *workspace, size_t workspace_bytes, uint32_t n_reads, sgk_literal_status_t *out);

/* ---- ent: the histograms behind `sigtk ent` (src/ent.c) ----------------- */
/* The counting runs on the GPU, the sum of -p*log2(p) over the (few thousand) non-empty bins on the host
 * with the reference's own operations and order (sgk_ent_finish), so the printed entropies are identical.
 * Values below the windows are counted in the record; the rare others (raw < 0 or >= 8192, zigzag delta
 * >= 4096) are listed, unordered, in over_raw / over_delta at [offsets[r], offsets[r] + n_over_*). */
#define SGK_ENT_RAW_WINDOW 8192
#define SGK_ENT_DELTA_WINDOW 4096
typedef struct sgk_ent_hist {
    uint32_t n;            /* samples of the read */
    uint32_t n_over_raw;   /* entries of this read in over_raw */
    uint32_t n_over_delta; /* entries of this read in over_delta */
    uint32_t reserved;
    uint32_t raw[SGK_ENT_RAW_WINDOW];     /* count of samples with (uint16)raw == v, all n samples */
    uint32_t delta[SGK_ENT_DELTA_WINDOW]; /* count of (uint16)zigzag(raw[i]-raw[i-1]) == v, i = 0..n-2, raw[-1] = 0 */
    uint32_t hi[256], lo[256];            /* byte planes of those n-1 values */
} sgk_ent_hist_t;
/* over_raw / over_delta: device arrays of batch->n_samples uint16 each (same layout as the samples) */
int sgk_ent(const sgk_batch_t *batch, sgk_ent_hist_t *out, uint16_t *over_raw, uint16_t *over_delta, void *stream);
/* HOST function: out[0..2] = raw, delta, byte entropy of one read from host copies of its record and of its
 * two overflow lists (which it sorts in place; may be NULL when the counts are 0) */
void sgk_ent_finish(const sgk_ent_hist_t *hist, uint16_t *over_raw, uint16_t *over_delta, double *out);

/* ---- svb-zd signal decode on the device ------------------------------- */
/* Expands BLOW5 svb-zd signal blobs (slow5lib/src/slow5_press.c:1116-1146: u32 count, streamvbyte
 * keys + data of the zigzag deltas) into int16 samples, one wavefront per read.  The record layer
 * (zlib) stays on the host; files written with signal compression svb-zd hand the blob over as it
 * sits in the record.  blobs: device buffer, readable up to its size rounded up to a multiple of 4
 * bytes (the kernel uses aligned 4-byte loads); blob_offsets/blob_lengths: byte offset and byte length
 * of each read's blob (the length INCLUDES the 4-byte count); samples/offsets/lengths as in
 * sgk_batch_t (lengths[r] must equal the blob's count); status[r]: 0 ok, 1 count mismatch (or fewer
 * than 4 bytes: no count word), 2 truncated / inconsistent blob: fewer bytes than 4 + ceil(count / 4),
 * data shorter than the keys promise, or data bytes left over (the read's samples are then undefined;
 * where 1 and 2 both apply either may be reported). */
int sgk_svbzd_decode(const uint8_t *blobs, const uint64_t *blob_offsets, const uint32_t *blob_lengths,
                     uint32_t n_reads, int16_t *samples, const uint64_t *offsets, const uint32_t *lengths,
                     uint32_t *status, void *stream);

/* ---- text SLOW5: the raw_signal column parsed on the device ------------------------------------------ */
/* Turns the raw_signal column of text SLOW5 records (slow5lib/src/slow5.c:2754-2778: decimal int16 tokens separated by
 * ',') into int16 samples, one wavefront per read.  text: 16-byte aligned device buffer; text + text_offsets[r] holds
 * text_lengths[r] bytes, exactly the column of record r (no tab, no newline), at any byte alignment.  The kernel loads
 * aligned 16-byte words and never reads outside [text_offsets[r] rounded down to 16, text_offsets[r] + text_lengths[r]
 * rounded up to 16): pad the buffer by 16 bytes at both ends.  samples/offsets/lengths as in sgk_batch_t; lengths[r] is
 * what the record announces and is not trusted: nothing is stored at a sample index >= lengths[r].
 * Accepted tokens, and nothing else: 0 | -?[1-9][0-9]{0,4} with the value in [-32768, 32767]; an empty text is valid
 * exactly when lengths[r] == 0.  status[r]: 2 when any token is malformed (empty token, leading zero, "-0", a lone or
 * interior '-', more than five digits, out of range, any other byte), else 1 when the number of tokens is not
 * lengths[r], else 0.  With a non-zero status the read's own sample range is undefined; nothing outside it is touched.
 * (slow5lib's slow5_int_check lets '-' appear anywhere in a token, "1-2" parses as 1 there: no writer produces that.) */
int sgk_sigtext_decode(const uint8_t *text, const uint64_t *text_offsets, const uint32_t *text_lengths,
                       uint32_t n_reads, int16_t *samples, const uint64_t *offsets, const uint32_t *lengths,
                       uint32_t *status, void *stream);

/* ---- zlib record inflate on the device (round 5; SURVEY 8f-1 / 8f-2 taken to the record layer) ------------------ */
/* BLOW5 files compress every record as one zlib stream (slow5lib/src/slow5.c:2583-2598); the reference inflates them one
 * at a time on its one thread, and a pool of host threads is what bounded the drop-in CLI's rate.  sgk_inflate inflates n
 * zlib streams (RFC 1950: header, DEFLATE blocks of every type, Adler-32), one wavefront per stream.  in: device buffer
 * readable up to its size rounded up to a multiple of 4 bytes; in_offsets / in_lengths: byte offset and length of every
 * stream; out: 16-byte aligned device buffer, stream r's bytes go to out + out_offsets[r] (offsets multiples of 16), which
 * must have room for out_caps[r] bytes >= what the stream inflates to (matches that reach far back read the stream's own
 * earlier bytes from there); out_lengths[r]: what the stream inflated to; status[r]: 0 ok, 1 bad zlib header / preset
 * dictionary, 2 bad block type / stored length, 3 bad code lengths (an invalid, over-subscribed or incomplete set),
 * 4 invalid code, 5 distance in front of the stream, 6 truncated input, 7 Adler-32 mismatch, 8 the stream inflates to
 * more than out_caps[r] (1 - 8: the bytes are undefined). */
int sgk_inflate(const uint8_t *in, const uint64_t *in_offsets, const uint32_t *in_lengths, uint32_t n, uint8_t *out,
                const uint64_t *out_offsets, const uint32_t *out_caps, uint32_t *out_lengths, uint32_t *status,
                void *stream);

/* ---- zstd record decompression on the device (additive to 0.2.3) -------------------------------------------------- */
/* BLOW5 files written with record compression 2 hold one zstd frame (RFC 8878) per record, as ZSTD_compress makes it
 * (slow5lib/src/slow5_press.c:1156-1200).  sgk_zstd_decompress decodes n frames, one wavefront per frame, with the buffer
 * contract of sgk_inflate: in readable up to its size rounded up to a multiple of 4 bytes, out 16-byte aligned, frame r's
 * bytes at out + out_offsets[r] (multiples of 16) with room for out_caps[r] bytes; out_lengths[r]: the bytes written.
 * Taken: every frame header layout that declares the content size, Raw / RLE / Compressed blocks, all literals types and
 * sequence modes, the content checksum (verified when present).  Refused: no content size, a dictionary id other than 0,
 * skippable frames, anything behind the frame.  status[r]:
 *   0 ok                          1 frame header refused (magic, reserved bit, dictionary, skippable, no content size,
 *   2 bad block header              bytes behind the frame)
 *   3 bad table description       4 bad literals or sequences section
 *   5 offset 0 or in front of the frame                              6 truncated input
 *   7 checksum mismatch           8 size differs from the declaration or exceeds out_caps[r]
 * (1 - 8: the bytes are undefined; nothing is written at or behind out_caps[r]).  The library keeps the literals scratch
 * (128 KB per resident wavefront, at most ten per compute unit) per device and stream: a job's is freed by
 * sgk_job_destroy, that of a stream the caller owns stays allocated until the process ends. */
int sgk_zstd_decompress(const uint8_t *in, const uint64_t *in_offsets, const uint32_t *in_lengths, uint32_t n, uint8_t *out,
                        const uint64_t *out_offsets, const uint32_t *out_caps, uint32_t *out_lengths, uint32_t *status,
                        void *stream);

/* ---- zlib record deflate on the device (additive to 0.2.3) ---------------------------------------------------------- */
/* The counterpart of sgk_inflate: n byte strings become n complete zlib streams (RFC 1950 / 1951: header 78 9C, DEFLATE
 * blocks over sgk_deflate_block_bytes() input bytes each, big-endian Adler-32), one wavefront per stream.  The tokens are
 * literals and matches of distance 1 (runs), every block dynamic-Huffman or stored, whichever is shorter -- what zlib's
 * Z_RLE strategy writes, and all that svb-zd bytes reward.  tools/proto/deflate_proto.py writes the same bytes on the CPU.
 * Buffers as sgk_inflate with the directions swapped, all device memory: stream r's in_lengths[r] bytes at
 * in + in_offsets[r] (any alignment; 16-byte aligned reads faster); its zlib stream goes to out + out_offsets[r] (out and
 * every out_offsets[r] 16-byte aligned), out_lengths[r] bytes.  Nothing is written at or behind out_caps[r]:
 * status[r] is 1 for a stream that needs more (out_lengths[r] is then undefined), else 0.  sgk_deflate_bound(n) bytes
 * are always enough for n input bytes.  Positions are 32-bit: SGK_ERR_ARG if an in_lengths[r] is 2^29 or more (nothing
 * is written then; the call waits for the lengths to be looked at on `stream`). */
uint32_t sgk_deflate_block_bytes(void);
/* n + 5 * max(1, ceil(n / min(sgk_deflate_block_bytes(), 65535))) + 6: every block stored.  Host arithmetic, no GPU. */
uint64_t sgk_deflate_bound(uint64_t n);
int sgk_deflate(const uint8_t *in, const uint64_t *in_offsets, const uint32_t *in_lengths, uint32_t n, uint8_t *out,
                const uint64_t *out_offsets, const uint32_t *out_caps, uint32_t *out_lengths, uint32_t *status, void *stream);

/* ---- the auxiliary fields of an inflated BLOW5 record, checked on the device (additive to 0.2.3) ----------------------- */
/* Behind its signal a record carries one field per auxiliary column of the file's header, in header order: a primitive
 * column elem_bytes bytes, an array column (`char*`, `double*`, `enum{..}*`) a u64 element count and then count x
 * elem_bytes bytes (slow5lib/src/slow5.c:3088-3165).  With an array column the inflated length of a record does not
 * follow from its head; sgk_zrec_tail_check walks the fields of n records, one lane per record, and tells whether they
 * fill the record exactly.  inflated: device buffer, record r's rec_lengths[r] bytes at inflated + rec_offsets[r] (any
 * byte alignment); tail_offsets[r]: where the record's signal ends, relative to the record.  fields is a HOST table of
 * n_fields columns (elem_bytes 1, 2, 4 or 8; any number of columns -- up to 256 the table travels with the launch and the
 * call only enqueues work, with more it goes through a temporary device buffer and the call waits for the stream).
 * Nothing at or behind rec_offsets[r] + rec_lengths[r] is read; only status is written.  status[r]:
 *   0 ok (with n_fields == 0: the record ends exactly at its signal)
 *   1 the record is shorter than tail_offsets[r]: it ended inside or in front of its signal
 *   2 a field is missing or cut: no byte left where a field must start, or a count word or data that would end behind
 *     the record (where the reference reads past its buffer)
 *   3 bytes are left behind the last field (with n_fields == 0: any byte behind the signal)
 *   4 an array's count x elem_bytes does not fit in 32 bits */
typedef struct sgk_aux_field {
    uint8_t elem_bytes;
    uint8_t is_array;
} sgk_aux_field_t;
int sgk_zrec_tail_check(const uint8_t *inflated, const uint64_t *rec_offsets, const uint32_t *rec_lengths,
                        const uint32_t *tail_offsets, uint32_t n, const sgk_aux_field_t *fields /* host */,
                        uint32_t n_fields, uint32_t *status, void *stream);

/* ---- the uncompressed signal of an inflated BLOW5 record, moved into the sample arena (additive to 0.2.3) -- */
/* A record of a file with signal_press 0 holds its samples as plain little-endian int16 behind its head.
 * sgk_sigraw_gather moves them, for n_reads records, to where sgk_batch_t wants them.  records: 16-byte aligned device
 * buffer (else SGK_ERR_ALIGN, as for samples); record r is rec_lengths[r] bytes at records + rec_offsets[r], at any byte alignment; its signal is lengths[r]
 * samples at sig_offsets[r] inside the record, at any residue of 16.  The kernel loads aligned 16-byte words and never
 * reads outside [rec_offsets[r] rounded down to 16, rec_offsets[r] + rec_lengths[r] rounded up to 16): pad the buffer by
 * 16 bytes at both ends.  samples (16-byte aligned) / offsets / lengths as in sgk_batch_t; offsets[r] must be a multiple
 * of 8 samples, as sgk_job_begin lays them out.  Exactly samples[offsets[r] .. offsets[r] + lengths[r]) is written: the
 * arena's padding keeps its bytes.  max_read_len (>= every lengths[r]) and n_samples (the arena's size, or 0 when not
 * known) size the launch as in sgk_batch_t; a wrong value costs time only.  Work is dealt out in units of
 * sgk_sigraw_unit_samples() samples over all reads, so one long read spreads over the device.  The call only enqueues.
 * status[r]: 0 moved; 1 when sig_offsets[r] + 2 * lengths[r] > rec_lengths[r] (the read's own range is then undefined,
 * nothing else is touched); 2 when rec_status is given and rec_status[r] != 0 -- that record did not inflate, its
 * rec_lengths[r] may be garbage, nothing of it is read and nothing is written. */
uint32_t sgk_sigraw_unit_samples(void); /* host arithmetic, no GPU */
int sgk_sigraw_gather(const uint8_t *records, const uint64_t *rec_offsets, const uint32_t *rec_lengths,
                      const uint32_t *sig_offsets, const uint32_t *rec_status /* may be NULL */, uint32_t n_reads,
                      int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, uint32_t max_read_len,
                      uint64_t n_samples, uint32_t *status, void *stream);

/* ---- qts: quantise the raw signal (src/qts.c:27-43, :126-142) and re-encode it ------ */
#define SGK_QTS_FLOOR 0     /* (raw >> b) << b                                       */
#define SGK_QTS_ROUND 1     /* round_to_power_of_2(raw, b): the reference's default   */
#define SGK_QTS_FILL_ONES 2 /* raw | ((1 << b) - 1)                                   */
/* in place on the samples of every read; bits in [1, 15] */
int sgk_qts(int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
            uint32_t max_read_len, int bits, int method, void *stream);
/* svb-zd ENCODE (slow5lib/src/slow5_press.c:1063-1089): canonical streamvbyte, so the blobs equal slow5lib's byte
 * for byte.  Two steps: sgk_svbzd_size fills blob_lengths[r] (4 + key bytes + data bytes); the caller lays the blobs
 * out (blob_offsets[r], 4-byte aligned) and sgk_svbzd_encode writes them. */
int sgk_svbzd_size(const int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                   uint32_t *blob_lengths, void *stream);
int sgk_svbzd_encode(const int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                     uint8_t *blobs, const uint64_t *blob_offsets, const uint32_t *blob_lengths, void *stream);

/* ---- text: the TSV rows of pa / event / event -c written on the device (csrc/text_kernels.hip) -------------------- */
/* The batch's whole stdout body (header line excluded) as one dense byte range in file order, byte for byte what the
 * reference's printf calls give (src/cfunc.c:16-61, 85-102: ids and len_raw_signal included, the empty line after every
 * read of the long event form, zero-length events skipped in the compact form, ".\t.\t.\t." for a read without events).
 * Two calls, because a byte's position depends on every byte in front of it:
 *   sgk_text_measure   counts: row_offsets[r] = byte offset of read r's rows, row_offsets[n_reads] = the total
 *   sgk_text_write     the characters: text[0 .. row_offsets[n_reads])
 * both asynchronous on `stream`, with the same inputs and the same workspace (which carries the layout from the first
 * call to the second).  pa text is made from the int16 samples (the float array is never written); event text from the
 * arena sgk_event left on the device (ev_slots / events / n_events as there: a read whose events overflowed its slots is
 * written with what fitted).  ids: the read ids, device pointers -- id r is bytes[offsets[r] .. offsets[r + 1]).
 * n_items_capacity: the samples of the batch (pa: the sum of the lengths or more) or the slots of the arena
 * (ev_slots[n_reads]); text may start at any byte address. */
#define SGK_TEXT_PA 0
#define SGK_TEXT_EVENT 1
#define SGK_TEXT_EVENT_COMPACT 2
typedef struct sgk_text_ids {
    const uint8_t *bytes;
    const uint32_t *offsets; /* n_reads + 1 */
} sgk_text_ids_t;
typedef struct sgk_text_status {
    uint32_t overflow; /* 1: the text needed more than text_capacity bytes; nothing was written behind it */
    uint32_t n_tiles;  /* tiles of 256 items the batch was cut into (diagnostic) */
    uint64_t n_bytes;  /* row_offsets[n_reads] */
} sgk_text_status_t;
size_t sgk_text_workspace_bytes(int kind, uint32_t n_reads, uint64_t n_items_capacity);
int sgk_text_measure(int kind, const sgk_batch_t *batch, const sgk_text_ids_t *ids, const uint64_t *ev_slots,
                     const sgk_event_rec_t *events, const uint32_t *n_events, uint64_t *row_offsets, void *workspace,
                     size_t workspace_bytes, void *stream);
/* text_capacity is checked ON THE DEVICE (the total is not known on the host when the call is made): a tile of rows that
 * would end behind it is not written and the workspace's status word says so. */
int sgk_text_write(int kind, const sgk_batch_t *batch, const sgk_text_ids_t *ids, const uint64_t *ev_slots,
                   const sgk_event_rec_t *events, const uint32_t *n_events, uint8_t *text, uint64_t text_capacity,
                   void *workspace, size_t workspace_bytes, void *stream);
/* after the caller has synchronised the stream: SGK_ERR_CAPACITY if the text did not fit, SGK_ERR_WORKSPACE if the
 * workspace was sized for fewer items than the batch has (nothing was written then) */
int sgk_text_status(const void *workspace, sgk_text_status_t *out);
/* test entries: printf("%f") / "%ld" of n values, value i into slots48[48 * i ..), its byte count into lengths[i]
 * (255 if the writer and its length-only form disagree); device pointers */
int sgk_text_numbers_f32(const float *v, uint64_t n, uint8_t *slots48, uint8_t *lengths, void *stream);
int sgk_text_numbers_i64(const int64_t *v, uint64_t n, uint8_t *slots48, uint8_t *lengths, void *stream);

/* ---- text SLOW5: the raw_signal column written on the device (csrc/slow5_text_kernels.hip; additive to 0.2.3) ------ */
/* The inverse of sgk_sigtext_decode, for `qts` on text files.  Row r of the batch is head_r | v0,v1,...,v(n-1) | tail_r
 * with n = lengths[r] and every sample as printf("%d") (slow5lib/src/slow5.c:3826-3860); a read of 0 samples has an
 * empty column.  heads / tails (device pointers, as sgk_text_ids_t: entry r is bytes[offsets[r] .. offsets[r + 1]))
 * hold arbitrary bytes of any length; NULL means all empty.  The kernels add no tab and no newline: for whole lines
 * the head ends with the tab in front of the column and the tail with the newline.  samples / offsets / lengths as in
 * sgk_batch_t (device pointers).  measure / write / status work as for sgk_text_*: both calls asynchronous on `stream`
 * with the same inputs and the same workspace (16-byte aligned; n_samples_capacity: the sum of the lengths or more),
 * row_offsets[r] the byte offset of row r and row_offsets[n_reads] the total, `text` at any byte address, no byte
 * outside [text, text + row_offsets[n_reads]) written, text_capacity checked on the device, sgk_text_status afterwards
 * (SGK_ERR_CAPACITY / SGK_ERR_WORKSPACE).  Tiles of 256 samples are staged in an LDS image of
 * SGK_SLOW5_TEXT_STAGE_BYTES and leave as 16-byte stores; a tile that carries a head or a tail and does not fit the
 * image writes its bytes straight to global memory.  A tile of 4 GiB or more reports SGK_ERR_CAPACITY. */
#define SGK_SLOW5_TEXT_STAGE_BYTES 8192
size_t sgk_slow5_text_workspace_bytes(uint32_t n_reads, uint64_t n_samples_capacity);
int sgk_slow5_text_measure(const int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                           const sgk_text_ids_t *heads, const sgk_text_ids_t *tails, uint64_t *row_offsets /* n_reads + 1 */,
                           void *workspace, size_t workspace_bytes, void *stream);
int sgk_slow5_text_write(const int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                         const sgk_text_ids_t *heads, const sgk_text_ids_t *tails, uint8_t *text, uint64_t text_capacity,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- sref: the synthetic reference signal of a sequence (csrc/sref_kernels.hip) -------------------------------------- */
/* `sigtk sref` (src/sref.c:100-210): position j of a strand's row is level_mean[rank(bases j .. j + k)], rank with the
 * first base most significant, A/a 0, C/c 1, G/g 2, T/t 3 and every other byte 0; the '-' strand is the reverse
 * complement, where the complement of a non-ACGT byte is T.  The pore model is an argument: `levels` holds level_mean by
 * k-mer rank, 4^k floats.  The library carries no model.
 * The unit of work is a span: signal positions [first, first + count) of one strand of one sequence of l = seq_len
 * bases, whose row has ref_len = l + 1 - k values.  The caller uploads only the forward bases a span needs: forward base
 * f sits at bases[base_offset + (f - base_pos0)].  A '+' span needs forward bases [first, first + count + k - 1), a '-'
 * span [l - first - count - k + 1, l - first).  A base in front of a span's window or outside `bases` reads as 'A' (never
 * out of bounds); behind a window that is too small the kernel reads what follows it in `bases`.
 * Text of a span: the row head "name \t l \t strand \t ref_len \t" if first == 0, then every value as printf("%f")
 * followed by ',' -- position ref_len - 1, the row's last, by '\n'.  A row with ref_len <= 0 is one span with count 0:
 * its head and no line end, as the reference prints it.  The spans of a row, in order, concatenate to the reference's row.
 * measure / write / status work as for sgk_text_* (same workspace in both calls, capacity checked on the device,
 * sgk_text_status afterwards); names: the sequence names, indexed by span.seq. */
typedef struct sgk_sref_span {
    uint64_t base_offset; /* where forward base base_pos0 of this span's sequence sits in `bases` */
    uint64_t base_pos0;
    uint32_t seq_len;      /* l, as printed */
    uint32_t first, count; /* signal positions [first, first + count) of this strand's row */
    uint32_t seq;          /* index into the names */
    uint8_t strand;        /* 0 '+', 1 '-' */
    uint8_t reserved[7];
} sgk_sref_span_t;
typedef struct sgk_sref_batch {
    const uint8_t *bases; /* device, ASCII as read from the file */
    uint64_t n_bases;
    const sgk_sref_span_t *spans; /* device */
    uint32_t n_spans;
    uint32_t k;          /* 1..6 */
    const float *levels; /* device, 4^k floats: level_mean by k-mer rank */
    uint32_t table_in_lds; /* EXPERIMENTAL, leave 0: text only, identical output.  0 the per-call table of the levels' text
                            * is read from global memory through L2; 1 every workgroup keeps a copy in LDS.  Kept until the
                            * two are timed (profiles/sref.md); the slower one and this field then go */
    uint32_t reserved;
} sgk_sref_batch_t;
/* out[out_offsets[s] + i] = the level of position first + i of span s (device pointers) */
int sgk_sref_levels(const sgk_sref_batch_t *batch, const uint64_t *out_offsets, float *out, void *stream);
size_t sgk_sref_text_workspace_bytes(uint32_t n_spans, uint64_t n_positions_capacity);
int sgk_sref_text_measure(const sgk_sref_batch_t *batch, const sgk_text_ids_t *names, uint64_t *row_offsets /* n_spans + 1 */,
                          void *workspace, size_t workspace_bytes, void *stream);
int sgk_sref_text_write(const sgk_sref_batch_t *batch, const sgk_text_ids_t *names, uint8_t *text, uint64_t text_capacity,
                        void *workspace, size_t workspace_bytes, void *stream);
/* Host pipe for callers without device memory of their own (the CLI): batches of spans in, their text out.  Two slots;
 * a slot goes begin -> (the caller fills the pinned staging) -> submit -> wait.  submit uploads, measures, sizes the
 * text buffers, writes and starts the download; it returns once the size is known.  wait returns the slot's text in
 * pinned host memory, valid until the slot's next begin.  `levels` is a host pointer here, 4^k floats. */
typedef struct sgk_sref_pipe sgk_sref_pipe_t;
typedef struct sgk_sref_stage {
    uint8_t *bases;          /* n_bases bytes */
    sgk_sref_span_t *spans;  /* n_spans; base_offset relative to `bases` */
    uint8_t *name_bytes;     /* name i is name_bytes[name_offsets[i] .. name_offsets[i + 1]) */
    uint32_t *name_offsets;  /* n_names + 1 */
} sgk_sref_stage_t;
int sgk_sref_pipe_create(int device, const float *levels, uint32_t k, sgk_sref_pipe_t **out);
void sgk_sref_pipe_destroy(sgk_sref_pipe_t *pipe);
int sgk_sref_pipe_begin(sgk_sref_pipe_t *pipe, int slot, uint64_t n_bases, uint32_t n_spans, uint32_t n_names,
                        uint64_t name_bytes, sgk_sref_stage_t *out);
int sgk_sref_pipe_submit(sgk_sref_pipe_t *pipe, int slot);
int sgk_sref_pipe_wait(sgk_sref_pipe_t *pipe, int slot, const uint8_t **text, uint64_t *n_bytes);

/* ---- ss: signal-alignment strings to k-mer rows (csrc/ss_kernels.hip) --------------------------------- */
/* `sigtk ss paf2tsv` (src/ss.c:124-197).  A record is one PAF line: its ss:Z: string and the columns start_raw, end_raw,
 * start_kmer, end_kmer and tlen.  st_k = min(start_kmer, end_kmer), end_k = max, rna = start_kmer > end_kmer.
 * Grammar: tokens <digits><op>, op one of ',' 'I' 'D'.  With i_k = st_k and i_raw = start_raw at the start,
 *   nI: i_raw += n     nD: i_k += n     n,: k-mer i_k gets the pair (i_raw, i_raw + n); i_raw += n; i_k += 1
 * Leading zeros are allowed, "0," is an empty mapping, digits behind the last op are ignored.
 * status, the first that applies:
 *   1  an op with no digit in front of it          }  of these two the one at the lower byte position
 *   2  a byte that is neither a digit nor an op    }
 *   5  a run of more than 10 digits in front of an op, a number above INT32_MAX, or i_raw / i_k above INT32_MAX
 *      (undefined in the reference: buff[11] and int overflow)
 *   3  i_raw != end_raw at the end
 *   4  i_k != end_k at the end
 *   0  ok
 * ends: the final (i_raw, i_k), or (-1, -1) with status 1, 2 or 5.
 * The unit of work is a span: k-mers st_k + first .. st_k + first + count of one record; one wavefront parses the
 * record's whole string for every span of it (a record may expand 8 bytes into 10^6 rows, so rows are budgeted by span,
 * never by what a line claims).  A span's pairs go to pairs[2 * (out_offsets[s] + j)], j < count, (start, end) of k-mer
 * st_k + first + j; the caller fills the table with -1 beforehand and a k-mer no ',' reached keeps (-1, -1).  A pair is
 * stored only at j < count, whatever the string says.  With a non-zero status the span's own table range is undefined;
 * nothing outside it is touched.  status and ends are indexed by SPAN (status[s], ends[2 s], ends[2 s + 1]); with
 * spans == NULL every record is one span of count 0 (n_spans is ignored): validation, nothing is stored.
 * start_raw and st_k must not be negative (a pair of -1 reads as "not mapped"); the kernel is memory-safe regardless.
 * ss: 16-byte aligned device buffer, readable up to n_ss_bytes rounded up to a multiple of 16.  A record's string is
 * ss[ss_offset .. ss_offset + ss_len), at any byte alignment, without the "ss:Z:" prefix.  The kernel loads aligned
 * 16-byte words below round_up(n_ss_bytes, 16) only; bytes of a string that lie behind n_ss_bytes read as invalid
 * bytes (status 2).  ss_len < 2^32 - 16.
 * Rows of a span's text: "id \t idx \t start \t end \n" per k-mer i, ascending, idx = rna ? tlen - i - 1 : i (computed in
 * 64 bits, may be negative), start and end "." for a k-mer that is not mapped; id = ids[record.id].  Text is made from
 * the pair table; measure / write / sgk_text_status work as for sgk_sref_text_* (n_rows_capacity: the sum of the spans'
 * counts or more).  Only spans of records whose status is 0 may be given to the text calls. */
typedef struct sgk_ss_record {
    uint64_t ss_offset;
    uint32_t ss_len;
    int32_t start_raw, end_raw;
    int32_t st_k, end_k; /* st_k <= end_k */
    int32_t tlen;
    uint32_t rna; /* 0 / 1 */
    uint32_t id;  /* index into the ids */
} sgk_ss_record_t;
typedef struct sgk_ss_span {
    uint32_t record;
    uint32_t first, count; /* k-mers st_k + first .. st_k + first + count */
    uint32_t reserved;
} sgk_ss_span_t;
typedef struct sgk_ss_batch {
    const uint8_t *ss; /* device */
    uint64_t n_ss_bytes;
    const sgk_ss_record_t *records; /* device */
    const sgk_ss_span_t *spans;     /* device; NULL (decode only): one span of count 0 per record */
    uint32_t n_records, n_spans;
} sgk_ss_batch_t;
int sgk_ss_decode(const sgk_ss_batch_t *batch, const uint64_t *out_offsets /* n_spans, in pairs */, int32_t *pairs,
                  uint32_t *status, int32_t *ends, void *stream);
size_t sgk_ss_text_workspace_bytes(uint32_t n_spans, uint64_t n_rows_capacity);
int sgk_ss_text_measure(const sgk_ss_batch_t *batch, const uint64_t *out_offsets, const int32_t *pairs,
                        const sgk_text_ids_t *ids, uint64_t *row_offsets /* n_spans + 1 */, void *workspace,
                        size_t workspace_bytes, void *stream);
int sgk_ss_text_write(const sgk_ss_batch_t *batch, const uint64_t *out_offsets, const int32_t *pairs,
                      const sgk_text_ids_t *ids, uint8_t *text, uint64_t text_capacity, void *workspace,
                      size_t workspace_bytes, void *stream);
/* Host pipe for the CLI, in the manner of sgk_sref_pipe_*: two slots, begin -> (fill the pinned staging) -> submit ->
 * wait.  The caller cuts the records into spans of at most its row budget per batch; a record larger than the budget is
 * given again, with its next span, in the next batch.  submit uploads, validates every record (status), keeps the spans
 * in front of the first record whose status is not 0, and only then sizes the pair table and the text for them: device
 * memory follows the caller's budget and the strings' verdict, not the columns of a line.  It then decodes, measures,
 * writes and starts the download.  wait returns the text of the kept spans (pinned, valid until the slot's next begin)
 * and the first bad record of the batch with its status (bad_record = UINT32_MAX: none).
 * id i is id_bytes[id_offsets[i] .. id_offsets[i + 1]); records[r].ss_offset is relative to `ss`. */
typedef struct sgk_ss_pipe sgk_ss_pipe_t;
typedef struct sgk_ss_stage {
    uint8_t *ss;              /* n_ss_bytes */
    sgk_ss_record_t *records; /* n_records */
    sgk_ss_span_t *spans;     /* n_spans, ascending record */
    uint8_t *id_bytes;
    uint32_t *id_offsets; /* n_ids + 1 */
} sgk_ss_stage_t;
int sgk_ss_pipe_create(int device, sgk_ss_pipe_t **out);
void sgk_ss_pipe_destroy(sgk_ss_pipe_t *pipe);
int sgk_ss_pipe_begin(sgk_ss_pipe_t *pipe, int slot, uint64_t n_ss_bytes, uint32_t n_records, uint32_t n_spans,
                      uint32_t n_ids, uint64_t id_bytes, sgk_ss_stage_t *out);
int sgk_ss_pipe_submit(sgk_ss_pipe_t *pipe, int slot);
int sgk_ss_pipe_wait(sgk_ss_pipe_t *pipe, int slot, const uint8_t **text, uint64_t *n_bytes, uint32_t *bad_record,
                     uint32_t *bad_status);

/* ---- synthetic reads (BASELINE configs 2-5) ---------------------------- */
/* Deterministic counter-based generator, identical on host and device (integer only).
 * kind 0: DNA-like (mean dwell 9 samples); kind 1: RNA-like (mean dwell 36, adaptor +
 * polyA prefix structure).  Read r of the batch is global read index first_read + r. */
int sgk_synth_reads(int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, double *digitisation,
                    double *offset, double *range, uint32_t n_reads, uint32_t max_read_len,
                    uint64_t first_read, uint64_t seed, int kind, void *stream); /* device pointers */
void sgk_synth_reads_host(int16_t *samples, const uint64_t *offsets, const uint32_t *lengths,
                          double *digitisation, double *offset, double *range, uint32_t n_reads,
                          uint64_t first_read, uint64_t seed, int kind);

/* ---- per-launch timing (HIP events on the caller's stream) ------------------------ */
/* When enabled, every device-API call records hipEvents around each kernel it launches;
 * sgk_profile_read() synchronises and returns the accumulated milliseconds per kernel
 * name since the last reset.  Used by bench.py for the roofline figure. */
void sgk_profile_enable(int on);
void sgk_profile_reset(void);
/* names/ms/calls: caller arrays of length cap; returns the number of distinct kernels */
int sgk_profile_read(const char **names, double *ms, uint32_t *calls, int cap);

/* ================================ Host API ======================================== */

typedef struct sgk_host_batch {
    const int16_t *samples;   /* host, packed; no alignment/padding requirement */
    const uint64_t *offsets;  /* host, n_reads+1 */
    const double *digitisation, *offset, *range; /* host, n_reads */
    uint32_t n_reads;
} sgk_host_batch_t;

typedef struct sgk_events_host {
    uint32_t n_reads;
    uint64_t *ev_offsets; /* n_reads+1, compact CSR: events of read r are [ev_offsets[r], ev_offsets[r+1]) */
    uint32_t *start, *length;
    float *mean, *stdv;
    sgk_event_status_t status;
} sgk_events_host_t;
int sgk_event_host(const sgk_host_batch_t *batch, int rna, sgk_events_host_t *out);
int sgk_event_host_opt(const sgk_host_batch_t *batch, int rna, sgk_events_host_t *out, const sgk_event_options_t *opt);
void sgk_events_host_free(sgk_events_host_t *ev);

int sgk_pa_host(const sgk_host_batch_t *batch, float *pa_out /* host, n_samples */);
int sgk_stat_host(const sgk_host_batch_t *batch, sgk_stat_rec_t *out /* host, n_reads */);
int sgk_stat_host_opt(const sgk_host_batch_t *batch, sgk_stat_rec_t *out, const sgk_stat_options_t *opt);

typedef struct sgk_segs_host {
    uint32_t n_reads;
    uint64_t *seg_offsets; /* n_reads+1, compact CSR */
    int32_t *x, *y;
} sgk_segs_host_t;
int sgk_jnn_host(const sgk_host_batch_t *batch, int rna, sgk_segs_host_t *out);
int sgk_jnn_host_opt(const sgk_host_batch_t *batch, int rna, sgk_segs_host_t *out, const sgk_stat_options_t *opt);
void sgk_segs_host_free(sgk_segs_host_t *s);

int sgk_prefix_host(const sgk_host_batch_t *batch, int rna, int pore, sgk_prefix_rec_t *out /* host, n_reads */);
int sgk_prefix_host_opt(const sgk_host_batch_t *batch, int rna, int pore, sgk_prefix_rec_t *out,
                        const sgk_stat_options_t *opt);

/* ---- pipelined host jobs (the batched, overlapped replacement of the ------
 *      reference's one-record-at-a-time loop, src/cmain.c:118-120) ---------------------
 * A job owns pinned host staging, device buffers, a private stream and pinned result buffers
 * for one batch; all of them only grow, so recycled jobs stop allocating.  Typical use, with
 * several jobs in flight so that reading/inflating, PCIe, kernels and formatting overlap:
 *     sgk_job_begin(job, n, lengths, SGK_SIGNAL_SVBZD, blob_bytes, &in);
 *     ... reader threads copy blob r to in.blobs + in.blob_offsets[r], fill in.digitisation[r] ...
 *     sgk_job_submit(job, SGK_TOOL_EVENT, rna, pore, 0);       // returns at once
 *     ... (another thread) sgk_job_wait(job); sgk_job_output(job, &out); format rows ...
 * begin/submit/wait may be called from different threads, one at a time per job.  After a call on a job has
 * returned an error other than SGK_ERR_FORMAT / SGK_ERR_CAPACITY (which describe the data, the job stays usable),
 * destroy the job: work may still be queued on its stream. */
typedef struct sgk_job sgk_job_t;

#define SGK_TOOL_PA 0
#define SGK_TOOL_EVENT 1
#define SGK_TOOL_STAT 2
#define SGK_TOOL_JNN 3
#define SGK_TOOL_PREFIX 4
#define SGK_TOOL_ENT 5
#define SGK_TOOL_QTS 6 /* submitted with sgk_job_submit_qts */

#define SGK_SIGNAL_INT16 0 /* caller stages decoded int16 samples                        */
#define SGK_SIGNAL_SVBZD 1 /* caller stages svb-zd blobs; decoded on the GPU (8f-1)      */
#define SGK_SIGNAL_ZREC 2  /* caller stages whole zlib-compressed BLOW5 records (svb-zd signal): inflated and decoded on the
                            * GPU (sgk_job_begin_zrec) */
#define SGK_SIGNAL_TEXT 3  /* caller stages the raw_signal column of text SLOW5 records (blob_bytes[r] = its byte length) at
                            * in.blobs + in.blob_offsets[r]; parsed on the GPU (sgk_sigtext_decode; additive to 0.2.3).
                            * Every sgk_job_submit kind and sgk_job_submit_qts take it.  As the OUTPUT format of
                            * sgk_job_submit_qts: the quantised signal written as text on the device (sgk_slow5_text_*) */

#define SGK_JOB_EVENTS_COMPACT 1 /* submit flag: only event start/length are copied back (event -c) */
#define SGK_JOB_EVENTS_LENGTHS 2 /* submit flag (0.2.3): only the event lengths are copied back -- ev_start, ev_mean and
                                  * ev_stdv are NULL.  The events of a read are contiguous from sample 0
                                  * (src/events.c:491-501), so start_i is the sum of the lengths in front of event i: half
                                  * of SGK_JOB_EVENTS_COMPACT's bytes over PCIe, which is what `event -c` waits for */

#define SGK_JOB_TEXT 4           /* submit flag, SGK_TOOL_PA and SGK_TOOL_EVENT (additive; sgk_job_set_ids first): the rows are
                                  * written on the device (sgk_text_*; with _COMPACT or _LENGTHS the compact event grammar,
                                  * else the long form) and the job downloads row_offsets and the text and nothing else --
                                  * no pA floats, no event arrays.  sgk_job_text hands them out after sgk_job_wait, which
                                  * returns SGK_ERR_CAPACITY for a read whose events overflowed its slots, as without the flag */

typedef struct sgk_job_input {
    int16_t *samples;             /* pinned host (SGK_SIGNAL_INT16): read r at samples + offsets[r] */
    uint8_t *blobs;               /* pinned host (SGK_SIGNAL_SVBZD): blob r at blobs + blob_offsets[r] */
    const uint64_t *offsets;      /* n_reads: sample offset of every read (also indexes the pa output) */
    const uint64_t *blob_offsets; /* n_reads */
    double *digitisation, *offset, *range; /* pinned host, n_reads: filled by the caller */
    uint64_t n_samples;           /* length of the sample arena */
} sgk_job_input_t;

typedef struct sgk_job_output {
    uint32_t n_reads;
    const uint64_t *offsets;        /* as in sgk_job_input_t */
    const uint32_t *lengths;
    const uint32_t *decode_status;  /* svb-zd / text input: per-read status of sgk_svbzd_decode / sgk_sigtext_decode, else NULL */
    const float *pa;                /* pa: pa[offsets[r] + i] */
    const uint64_t *slots;          /* event / jnn: arena slot of read r's first item (n_reads+1) */
    const uint32_t *counts;         /* event / jnn: items of read r */
    const uint32_t *ev_start, *ev_length;
    const float *ev_mean, *ev_stdv; /* NULL with SGK_JOB_EVENTS_COMPACT / _LENGTHS (_LENGTHS: ev_start as well) */
    const int32_t *seg_x, *seg_y;
    const sgk_stat_rec_t *stat;
    const sgk_prefix_rec_t *prefix;
    sgk_event_status_t event_status;
    /* qts: the quantised signal, as svb-zd blobs (blob r at qts_blobs + qts_blob_offsets[r], qts_blob_lengths[r]
     * bytes) or, for files without signal compression, as int16 samples at qts_samples + offsets[r] */
    const uint8_t *qts_blobs;
    const uint64_t *qts_blob_offsets;
    const uint32_t *qts_blob_lengths;
    const int16_t *qts_samples;
    const sgk_ent_hist_t *ent;            /* ent: one record per read */
    uint16_t *ent_over_raw, *ent_over_delta; /* ent: host copies of the overflow lists (NULL if all empty) */
    /* qts with SGK_QTS_RECORDS: the rewritten records as zlib streams (record r at qts_records + qts_record_offsets[r],
     * qts_record_lengths[r] bytes; qts_record_status[r]: sgk_deflate's status, or with SGK_QTS_ZREC_FRAMES 2 and length 0
     * for a record that did not inflate or fill its fields), else NULL.  The blobs / samples above
     * are NULL then: the signal is not downloaded uncompressed */
    const uint8_t *qts_records;
    const uint64_t *qts_record_offsets;
    const uint32_t *qts_record_lengths;
    const uint32_t *qts_record_status;
} sgk_job_output_t;

int sgk_job_create(int device, sgk_job_t **out);
/* the options the job's submits use from now on (copied; null = defaults) */
int sgk_job_set_options(sgk_job_t *job, const sgk_event_options_t *event_opt, const sgk_stat_options_t *stat_opt);
/* Detector parameters of the job's SGK_TOOL_EVENT submits (copied; every submit flag and input format; `rna` is then
 * ignored by them).  NULL: back to the presets by `rna`.  SGK_ERR_ARG when sgk_event_params_check refuses them. */
int sgk_job_set_event_params(sgk_job_t *job, const sgk_event_params_t *params);
void sgk_job_destroy(sgk_job_t *job);
int sgk_job_device(const sgk_job_t *job);
/* lengths[r]: samples of read r; blob_bytes[r] (SGK_SIGNAL_SVBZD, SGK_SIGNAL_TEXT): byte length of its blob / text column */
int sgk_job_begin(sgk_job_t *job, uint32_t n_reads, const uint32_t *lengths, int signal_format,
                  const uint32_t *blob_bytes, sgk_job_input_t *in);
/* The records as they sit in a BLOW5 file with zlib records and svb-zd signal (0.2.2): the caller stages record r's
 * rec_bytes[r] on-disk bytes at in->blobs + in->blob_offsets[r] and fills the scaling; the job inflates them on the GPU
 * (sgk_inflate) and decodes the signal blobs from there.  What the caller must know of a record it knows from its head
 * (a few hundred inflated bytes): lengths[r] samples, the signal blob at sig_offset[r] of the inflated record and
 * sig_bytes[r] long, the inflated record rec_room[r] bytes at most (head + signal + auxiliary fields; a record that
 * inflates to more fails with status 0x108).  sgk_job_wait returns SGK_ERR_FORMAT if a record did not inflate or decode
 * (decode_status[r]: 0x100 | sgk_inflate's status, or sgk_svbzd_decode's). */
int sgk_job_begin_zrec(sgk_job_t *job, uint32_t n_reads, const uint32_t *lengths, const uint32_t *rec_bytes,
                       const uint32_t *sig_offset, const uint32_t *sig_bytes, const uint32_t *rec_room,
                       sgk_job_input_t *in);
/* The same for either record compression of a BLOW5 file (additive to 0.2.3): SGK_RECORD_ZLIB is sgk_job_begin_zrec,
 * SGK_RECORD_ZSTD decodes the records with sgk_zstd_decompress -- rec_room[r] is then at least the content size the
 * frame declares, and decode_status[r] of a record that did not decode is 0x200 | sgk_zstd_decompress's status. */
#define SGK_RECORD_ZLIB 1
#define SGK_RECORD_ZSTD 2
int sgk_job_begin_zrec_format(sgk_job_t *job, uint32_t n_reads, int record_format, const uint32_t *lengths,
                              const uint32_t *rec_bytes, const uint32_t *sig_offset, const uint32_t *sig_bytes,
                              const uint32_t *rec_room, sgk_job_input_t *in);
/* sgk_job_begin_zrec_format for a file whose records carry auxiliary fields of the given columns (host table, copied;
 * n_fields 0: none), arrays included (additive to 0.2.3).  rec_room[r] is then an upper bound -- for zstd records the
 * content size the frame declares, for zlib records head + signal + the fixed fields + room for every array -- and what a
 * record inflated to is checked with sgk_zrec_tail_check against the end of its signal (sig_offset[r] + sig_bytes[r]).
 * decode_status[r] of a record that inflated but whose fields do not fill it exactly is 0x400 | that status; the inflate
 * statuses (0x100 |, 0x200 |) come first, as before.  A zlib record that inflates to more than its room reports 0x108:
 * with an array column that may be a sound record with a long array, which the caller can inflate on the host instead. */
int sgk_job_begin_zrec_aux(sgk_job_t *job, uint32_t n_reads, int record_format, const uint32_t *lengths,
                           const uint32_t *rec_bytes, const uint32_t *sig_offset, const uint32_t *sig_bytes,
                           const uint32_t *rec_room, const sgk_aux_field_t *fields, uint32_t n_fields, sgk_job_input_t *in);
/* sgk_job_begin_zrec_aux with the signal's own format named (additive to 0.2.3).  SGK_SIGNAL_SVBZD is exactly
 * sgk_job_begin_zrec_aux.  SGK_SIGNAL_INT16: the records' signal is not compressed (signal_press 0: what slow5tools
 * wrote before svb-zd, every `-s none` file) -- lengths[r] little-endian int16 samples at sig_offset[r] of the inflated
 * record; SGK_ERR_ARG unless sig_bytes[r] == 2 * lengths[r] for every r.  The job inflates the records and moves the
 * samples with sgk_sigraw_gather; what every record inflated to is always checked with sgk_zrec_tail_check (n_fields 0:
 * the record must end exactly at its signal), so a record that inflates cleanly but is shorter than its signal is
 * reported.  decode_status[r]: 0x100 | / 0x200 | the inflate status first, then 0x400 | the tail status, else
 * sgk_sigraw_gather's.  Any other signal_format: SGK_ERR_ARG.  Every sgk_job_submit tool and sgk_job_submit_qts work on
 * such a batch as on any staged one; SGK_QTS_ZREC_FRAMES stays SGK_ERR_ARG for it. */
int sgk_job_begin_zrec_signal(sgk_job_t *job, uint32_t n_reads, int record_format, int signal_format,
                              const uint32_t *lengths, const uint32_t *rec_bytes, const uint32_t *sig_offset,
                              const uint32_t *sig_bytes, const uint32_t *rec_room, const sgk_aux_field_t *fields,
                              uint32_t n_fields, sgk_job_input_t *in);
/* may be called again after sgk_job_wait to run another tool over the same staged batch */
int sgk_job_submit(sgk_job_t *job, int tool, int rna, int pore, int flags);
/* qts over the staged batch (any input format; text input with bare SGK_SIGNAL_INT16 samples out, without
 * SGK_QTS_RECORDS, is SGK_ERR_ARG as it always was): quantise (bits in [1,15], method SGK_QTS_*), then hand the signal back
 * as svb-zd blobs (out_signal_format SGK_SIGNAL_SVBZD), int16 samples (SGK_SIGNAL_INT16) or -- additive to 0.2.3 --
 * as the raw_signal columns of text SLOW5 records (SGK_SIGNAL_TEXT): row r is the column of read r, fetched with
 * sgk_job_text after sgk_job_wait.  With SGK_QTS_RECORDS (below) the rows are whole lines: frame r's first
 * head_lengths[r] bytes, the column, the rest of the frame; nothing is inserted between them and nothing is deflated. */
int sgk_job_submit_qts(sgk_job_t *job, int bits, int method, int out_signal_format);
/* qts record mode (additive to 0.2.3).  Between sgk_job_begin* and sgk_job_submit_qts: what a BLOW5 record holds around
 * its signal.  Frame r is bytes[frame_offsets[r] .. frame_offsets[r + 1]) (frame_offsets[0] = 0): first the record's
 * head_lengths[r] bytes in front of len_raw_signal, then its bytes behind the signal (the auxiliary fields).  Copied into
 * the job's pinned staging.  With SGK_QTS_RECORDS or'ed into out_signal_format, sgk_job_submit_qts then assembles
 * head | u64 len_raw_signal | signal | tail for every read on the device (k_qts_assemble; len_raw_signal is the blob
 * length for SGK_SIGNAL_SVBZD, the sample count for SGK_SIGNAL_INT16), deflates the records there (sgk_deflate) and
 * downloads only the zlib streams: sgk_job_output_t::qts_records.  SGK_ERR_ARG without frames. */
#define SGK_QTS_RECORDS 0x100
int sgk_job_set_record_frames(sgk_job_t *job, const uint8_t *bytes, const uint32_t *frame_offsets /* n + 1 */,
                              const uint32_t *head_lengths /* n */);
/* Record mode without staged frames (additive to 0.2.3): or'ed into out_signal_format together with SGK_QTS_RECORDS, for a
 * batch begun with sgk_job_begin_zrec / _format / _aux and SGK_SIGNAL_SVBZD out (anything else: SGK_ERR_ARG, as is a
 * sig_offset below 8, and a batch begun with sgk_job_begin_zrec_signal and SGK_SIGNAL_INT16). Record r's frame is read where the record was inflated on the device: its head is bytes
 * [0, sig_offset[r] - 8), its tail bytes [sig_offset[r] + sig_bytes[r], what the record inflated to); no
 * sgk_job_set_record_frames is needed and the records never leave the device between the file's bytes and the new zlib
 * streams.  A record that did not inflate, or whose auxiliary fields do not fill it, is not read from: its
 * qts_record_status is 2 and its qts_record_lengths 0 (1 stays sgk_deflate's "no room"); sgk_job_wait returns
 * SGK_ERR_FORMAT with decode_status as for every SGK_SIGNAL_ZREC batch, and the other records' streams are valid. */
#define SGK_QTS_ZREC_FRAMES 0x200
/* SGK_ERR_FORMAT if a blob (a text column) did not decode, SGK_ERR_CAPACITY on event-slot overflow */
int sgk_job_wait(sgk_job_t *job);
/* valid after sgk_job_wait until the job's next sgk_job_begin */
int sgk_job_output(const sgk_job_t *job, sgk_job_output_t *out);
/* stat / jnn / prefix jobs, after sgk_job_wait: long reads the 16-workgroup path declined (a barrier wait timed out) and
 * the wave-per-read kernel redid -- sgk_long_status_t::n_timeouts of the job's last submit.  The records are right
 * either way; non-zero means the GPU did not dispatch a grid's workgroups the way the long path assumes (0.2.2). */
uint32_t sgk_job_long_declined(const sgk_job_t *job);
/* The read ids of the staged batch, between sgk_job_begin* and sgk_job_submit (arbitrary bytes, 0 - 65 535 per id; id r
 * is bytes[offsets[r] .. offsets[r + 1]), offsets[0] = 0): copied into the job's pinned staging, uploaded with the batch. */
int sgk_job_set_ids(sgk_job_t *job, const uint8_t *bytes, const uint32_t *offsets);
typedef struct sgk_job_text {
    const uint8_t *text;         /* pinned host: the rows of read r are text[row_offsets[r] .. row_offsets[r + 1]) */
    const uint64_t *row_offsets; /* n_reads + 1 */
    uint64_t n_bytes;            /* row_offsets[n_reads] */
} sgk_job_text_t;
/* after sgk_job_wait of a submit with SGK_JOB_TEXT, or of sgk_job_submit_qts with SGK_SIGNAL_TEXT as the output format;
 * valid until the job's next sgk_job_begin */
int sgk_job_text(const sgk_job_t *job, sgk_job_text_t *out);

/* ---- per-read shims with the reference's own signatures (batch of one) ------------- */
/* event_t / event_table exactly as src/sigtk.h:55-70 */
typedef struct {
    uint64_t start;
    float length;
    float mean;
    float stdv;
} sgk_event_t;
typedef struct {
    size_t n;
    size_t start;
    size_t end;
    sgk_event_t *event; /* malloc'd; caller frees, as with getevents() (src/cfunc.c:82) */
} sgk_event_table;
/* float *signal_in_picoamps(slow5_rec_t*) (src/misc.c:15): malloc'd, caller frees */
float *sgk_signal_in_picoamps(const int16_t *raw, uint64_t len_raw_signal, double digitisation,
                              double offset, double range);
/* event_table getevents(size_t nsample, float *rawptr, int8_t rna) (src/events.c:553) */
sgk_event_table sgk_getevents(size_t nsample, float *rawptr, int8_t rna);
/* ... with the caller's own detector_param in place of the two presets (an empty table when they are out of domain) */
sgk_event_table sgk_getevents_param(size_t nsample, float *rawptr, const sgk_event_params_t *params);

/* jnn_pair_t, jnn_param_t, jnnv2_param_t exactly as src/jnn.h:13-16, 18-27, 74-81 */
typedef struct {
    int64_t x;
    int64_t y;
} sgk_jnn_pair_t;
typedef struct {
    float std_scale;
    int corrector;
    int seg_dist;
    int window;
    float stall_len;
    int error;
    float top;
    float bot;
} sgk_jnn_param_t;
typedef struct {
    float std_scale;
    int seg_dist;
    int window; /* must be 2000 (both presets of the reference): the rolling mean divides by it exactly */
    float stall_len;
    int hi_thresh;
    int lo_thresh;
} sgk_jnnv2_param_t;
/* jnn_pair_t *jnn_raw(const int16_t*, int64_t, jnn_param_t, int *n) (src/jnn.c:282): malloc'd, caller frees; NULL with
 * *n = 0 for an empty read, as the reference */
sgk_jnn_pair_t *sgk_jnn_raw(const int16_t *raw, int64_t nsample, sgk_jnn_param_t param, int *n);
/* jnn_pair_t *jnn_pa(const float*, int64_t, jnn_param_t, int *n) (src/jnn.c:295) */
sgk_jnn_pair_t *sgk_jnn_pa(const float *raw, int64_t nsample, sgk_jnn_param_t param, int *n);
/* jnn_pair_t jnnv2(const int16_t*, int64_t, jnnv2_param_t) (src/jnn.c:99): {-1,-1} when nsample <= window */
sgk_jnn_pair_t sgk_jnnv2(const int16_t *sig, int64_t nsample, sgk_jnnv2_param_t param);
/* jnn_pair_t find_adaptor(slow5_rec_t*, int8_t pore) (src/jnn.c:181): the record's raw signal and its length */
sgk_jnn_pair_t sgk_find_adaptor(const int16_t *raw, int64_t nsample, int8_t pore);
/* jnn_pair_t find_polya(const float*, int64_t, float top, float bot, int8_t pore) (src/jnn.c:352) */
sgk_jnn_pair_t sgk_find_polya(const float *raw, int64_t nsample, float top, float bot, int8_t pore);
/* the six inlines of src/stat.h:17-73 (sequential float sums in sample order; medians = rank n/2) */
float sgk_meanf(const float *x, int n);
float sgk_meani16(const int16_t *x, int n);
float sgk_stdvf(const float *x, int n);
float sgk_stdvi16(const int16_t *x, int n);
float sgk_medianf(const float *x, int n);
int16_t sgk_mediani16(const int16_t *x, int n);
/* SGK_OK, or why the last shim call of this thread returned NULL / {-1,-1} / NaN */
int sgk_shim_status(void);

/* ---- jnn and prefix with caller-supplied segmenter parameters (additive to 0.2.3) ------------------------------------
 * The compiled-in constants of the reference's segmenters (src/jnn.h) as arguments: jnn_param_t for jnn, jnnv2_param_t
 * for the adaptor finder, and for find_polya its jnn_param_t plus the band of src/cfunc.c:191,
 * top = (m_a + shift) + band, bot = (m_a + shift) - band (presets 30 and 20; one float rounding per operator).  The
 * results are, bit for bit, those of the reference's own steps with these numbers.  Outside the domain every entry
 * returns SGK_ERR_ARG and launches nothing (DESIGN.md 3.17 has each bound's reason):
 *   jnn      32 <= window <= 2^24 (from 32 up sgk_jnn_slots_for bounds a read's segments), corrector >= 1, error >= 0,
 *            seg_dist >= 0, stall_len finite and >= 0, std_scale finite; std_scale <= 0 means the fixed top / bot,
 *            which may be anything, NaN included.
 *   adaptor  2 <= window <= 13 981 (below 2 the reference reads current[-1]; 13 981 is the largest window whose float
 *            running total 1200 * window <= 2^24 is an exact integer), lo_thresh >= 1, hi_thresh >= lo_thresh,
 *            seg_dist >= 0, std_scale finite; stall_len is ignored, as the reference ignores it.
 *   polyA    corrector, seg_dist, window, stall_len, error as for jnn; shift and band finite, band >= 0.
 * Routes (sgk_prefix_route): an adaptor set equal to a preset (JNNV2_RNA_R9_ADAPTOR or JNNV2_RNA_RNA004_ADAPTOR) takes
 * sgk_prefix's kernels; anything else, and everything with SGK_PREFIX_PARAMS_GENERIC, takes k_adaptor_param: one
 * wavefront per read, any window of the domain, any read length, no long-read split -- a read of 10^6 samples is slow
 * and right.  A polyA set equal to the preset takes sgk_prefix's kernels; any other set with stall_len == 1 and error <
 * corrector the same wave kernel with the set as an argument, the rest the lane-per-read kernel with the set as an
 * argument.  sgk_jnn_param routes as sgk_jnn_raw does: the wave kernel where error < corrector, error <= 31 and
 * window >= 128, else the lane-per-read kernel. */
#define SGK_PREFIX_PARAMS_GENERIC 1u       /* flags: k_adaptor_param even for a preset (tests, measurements) */
#define SGK_PREFIX_ROUTE_ADAPTOR_PARAM 1   /* sgk_prefix_route, bit set: k_adaptor_param */
#define SGK_PREFIX_ROUTE_POLYA_WAVE_PARAM 2 /* the parametrised k_polya_wave */
#define SGK_PREFIX_ROUTE_POLYA_LANE_PARAM 4 /* the parametrised k_polya */
#define SGK_ADAPTOR_WINDOW_MAX 13981
typedef struct sgk_prefix_params {
    sgk_jnnv2_param_t adaptor; /* 24 bytes */
    sgk_jnn_param_t polya;     /* 32 bytes; std_scale, top, bot are not used: the thresholds come from shift / band */
    float shift, band;
    uint32_t flags, reserved;
} sgk_prefix_params_t; /* 72 bytes */
/* host only: the sets sgk_prefix(rna, pore) uses, flags 0 */
int sgk_prefix_params_preset(int rna, int pore, sgk_prefix_params_t *out);
/* host only: SGK_OK inside the domain above, else SGK_ERR_ARG */
int sgk_jnn_params_check(const sgk_jnn_param_t *p);
int sgk_prefix_params_check(const sgk_prefix_params_t *p);
/* host only: the SGK_PREFIX_ROUTE_* bits these parameters take (0: sgk_prefix's kernels); SGK_ERR_ARG outside the domain */
int sgk_prefix_route(const sgk_prefix_params_t *p);
/* sgk_jnn_opt / sgk_prefix_opt with the caller's parameters; workspaces as sgk_jnn / sgk_prefix_workspace_bytes */
int sgk_jnn_param(const sgk_batch_t *batch, const sgk_jnn_param_t *p, const uint64_t *seg_slots, int32_t *seg_x,
                  int32_t *seg_y, uint32_t *n_segs, void *workspace, size_t workspace_bytes, void *stream,
                  const sgk_stat_options_t *opt);
int sgk_prefix_param(const sgk_batch_t *batch, int rna, const sgk_prefix_params_t *p, sgk_prefix_rec_t *out,
                     void *workspace, size_t workspace_bytes, void *stream, const sgk_stat_options_t *opt);
/* per read: jnnv2 with any window of the domain (sgk_jnnv2 keeps refusing all but 2000), on k_adaptor_param;
 * find_polya on pA samples with the caller's set, top and bot as given */
sgk_jnn_pair_t sgk_jnnv2_param(const int16_t *sig, int64_t nsample, sgk_jnnv2_param_t param);
sgk_jnn_pair_t sgk_find_polya_param(const float *raw, int64_t nsample, float top, float bot, sgk_jnn_param_t param);
/* Segmenter parameters of the job's SGK_TOOL_JNN / SGK_TOOL_PREFIX submits (copied).  NULL: back to the presets. */
int sgk_job_set_jnn_params(sgk_job_t *job, const sgk_jnn_param_t *params);
int sgk_job_set_prefix_params(sgk_job_t *job, const sgk_prefix_params_t *params);
/* tests: out[i] = the quotient k_adaptor_param forms for the rolling total i, 0 <= i < n (device pointer) */
int sgk_debug_roll_means(int window, uint32_t n, float *out, void *stream);

/* ---- stat and jnn on batches of float (pA) signals (additive to 0.2.3) -----------------------------------------------
 * The batched counterparts of meanf / stdvf / medianf (src/stat.h:17-63), jnn_pa (src/jnn.c:295-306) and find_polya
 * (src/jnn.c:352-374) for signals that are floats already: normalised or rescaled signals, pA kept from sgk_pa /
 * sgk_stat_pa, the levels of sgk_sref_levels.  (The per-read shims above take one array per call and launch.)
 * A float batch is x, offsets, lengths, n_reads, max_read_len, n_values, all device pointers: read r is
 * x[offsets[r] .. offsets[r] + lengths[r]).  x is 4-byte aligned and offsets[r] is ANY element index: no alignment, head
 * room or tail room is asked of the caller.  Reads may touch but not overlap, in any order; lengths[r] <= max_read_len <
 * 2^31 (the reference's n is an int: a larger max_read_len is SGK_ERR_ARG); n_values is the readable length of x.
 * Memory contract: no byte outside [x, x + n_values) is read -- in fact none outside the reads --, no result depends on
 * a value outside the read's own range, and nothing but the documented outputs and the workspace is written.
 * One wavefront per read, longest reads first; a read is never split over workgroups: a read of 10^6 values is slow and
 * right, like k_adaptor_param's.  Both calls are asynchronous on `stream`, allocate nothing and make no host round trip.
 * The workspace is 16-byte aligned; one smaller than *_workspace_bytes is SGK_ERR_WORKSPACE with nothing written.
 * Without a GPU they return SGK_ERR_NODEVICE, after the argument checks; n_reads == 0 is SGK_OK.  DESIGN.md 3.18.
 *
 * sgk_stat_f32: mean, std, median are bit for bit meanf, stdvf, medianf of the read (sequential float sums in sample
 * order; the order statistic of rank n / 2; a median that is a zero, and any array holding a NaN, redone with the
 * reference's own selection; mean and std of an array holding a NaN or an infinity redone with x86's NaN rules).  flags
 * is 0, or SGK_MEDIAN_INEXACT where such a median found no scratch row (see sgk_stat): never with a workspace of
 * sgk_stat_f32_workspace_bytes while the read fits SGK_LITERAL_MAX_BYTES.  A read of no values has NaN in all three. */
typedef struct sgk_statf_rec {
    float mean, std, median;
    uint32_t flags;
} sgk_statf_rec_t; /* 16 bytes */
size_t sgk_stat_f32_workspace_bytes(uint32_t n_reads, uint64_t n_values, uint32_t max_read_len);
int sgk_stat_f32(const float *x, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads, uint32_t max_read_len,
                 uint64_t n_values, sgk_statf_rec_t *out, void *workspace, size_t workspace_bytes, void *stream);
/* sgk_jnn_f32: the segments of read r are bit for bit jnn_pa(x_r, n, *p, &n_segs): rm_outlierf clamps to [0, 1200] (a
 * NaN passes the clamp and is then out of range), with p->std_scale > 0 the thresholds come from meanf / stdvf of the
 * clamped values, else they are p->top, p->bot; then jnn_core, every compare in float.  p is checked with
 * sgk_jnn_params_check (refused: SGK_ERR_ARG before any device work).  top / bot (device, n_reads each, or both NULL;
 * one of them NULL is SGK_ERR_ARG) give each read its own fixed thresholds and are allowed only with p->std_scale <= 0:
 * with the polyA preset of a pore the first segment of read r is then find_polya(x_r, n, top[r], bot[r], pore).
 * The slot arena, sgk_jnn_slots_for, the use of a read's upper slots as scratch and the report of a read that overflowed
 * its slots (n_segs[r] the true count, the surplus dropped, the uint32 at the start of the workspace the number of such
 * reads) are those of sgk_jnn_param.  Sets with error < corrector, error <= 31 and window >= 128 run in chunks, a lane
 * per chunk; the others, and reads whose staging overflowed, take the literal loop, one read per lane. */
size_t sgk_jnn_f32_workspace_bytes(uint32_t n_reads, uint64_t n_values, uint32_t max_read_len);
int sgk_jnn_f32(const float *x, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads, uint32_t max_read_len,
                uint64_t n_values, const sgk_jnn_param_t *p, const float *top, const float *bot, const uint64_t *seg_slots,
                int32_t *seg_x, int32_t *seg_y, uint32_t *n_segs, void *workspace, size_t workspace_bytes, void *stream);

/* ---- normalised signals (additive to 0.2.3) ---------------------------------------------------------------------------
 * y[i] = (x[i] - shift) / scale for every value of every read, in float32: one float subtraction and one correctly
 * rounded float division, no contraction, no reciprocal, subnormal quotients kept.  With meanf / stdvf / medianf as
 * sgk_stat_f32 delivers them (bit for bit the reference's, src/stat.h):
 *   SGK_NORM_ZSCORE  shift = meanf(x),   scale = stdvf(x)
 *   SGK_NORM_MEDMAD  shift = medianf(x), scale = medianf(d) * 1.4826f (one float multiply), d[i] = fabsf(x[i] - shift),
 *                    medianf(d) the order statistic of rank n / 2, as everywhere
 * What IEEE makes of the formula is the result: a constant read has scale == 0 and every y = 0 / 0 = NaN, a read with
 * mad == 0 that is not constant gets +-inf and NaN; the record of such a read carries SGK_NORM_ZERO_SCALE.  A read holding
 * a NaN or an infinity (no reference function says what its normalisation is): SGK_NORM_NONFINITE, shift and scale NaN,
 * every y of the read NaN.  A read of no values: nothing of y is written, shift and scale NaN, flags 0.  Where
 * sgk_stat_f32 would leave SGK_MEDIAN_INEXACT on the read's median the record keeps that bit (never with a workspace of
 * the size function's while the read fits SGK_LITERAL_MAX_BYTES).
 * sgk_normalise_f32 takes a float batch under the contract above (x 4-byte aligned, offsets any element index, reads may
 * touch but not overlap, no byte outside the reads is read, asynchronous, no allocation, no host round trip).  y has x's
 * layout, y[offsets[r] + i], and is 4-byte aligned; y may be x itself (in place), otherwise [y, y + n_values) must not
 * overlap [x, x + n_values) (SGK_ERR_ARG).  No byte of y outside the reads is written: not a gap, not a neighbour, not
 * the slack in front of an unaligned first value.  rec: n_reads records.  A method other than the two, or a null pointer
 * with n_reads > 0, is SGK_ERR_ARG; a short workspace SGK_ERR_WORKSPACE with nothing written; SGK_ERR_NODEVICE comes
 * after the argument checks; n_reads == 0 is SGK_OK.
 * sgk_normalise is the same for an int16 batch: x is sgk_pa of the batch, written into y and normalised there.
 * DESIGN.md 3.19. */
#define SGK_NORM_ZSCORE 1
#define SGK_NORM_MEDMAD 2
#define SGK_NORM_ZERO_SCALE 1u /* sgk_norm_rec_t::flags: scale == 0 */
#define SGK_NORM_NONFINITE 2u  /* ... the read holds a NaN or an infinity (SGK_MEDIAN_INEXACT, 4u, is the third bit) */
typedef struct sgk_norm_rec {
    float shift, scale;
    uint32_t n, flags;
} sgk_norm_rec_t; /* 16 bytes */
size_t sgk_normalise_f32_workspace_bytes(uint32_t n_reads, uint64_t n_values, uint32_t max_read_len);
int sgk_normalise_f32(const float *x, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads, uint32_t max_read_len,
                      uint64_t n_values, int method, float *y, sgk_norm_rec_t *rec, void *workspace, size_t workspace_bytes,
                      void *stream);
size_t sgk_normalise_workspace_bytes(uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len);
int sgk_normalise(const sgk_batch_t *batch, int method, float *y, sgk_norm_rec_t *rec, void *workspace, size_t workspace_bytes,
                  void *stream);
/* The job's SGK_TOOL_PA submits from now on: 0 the pA values (the default), SGK_NORM_* the normalised signal in their
 * place (sgk_job_output_t::pa; every input format).  Any other method is SGK_ERR_ARG.  No other tool looks at it; a
 * SGK_TOOL_PA submit with SGK_JOB_TEXT is SGK_ERR_ARG while it is set.  The job keeps the sgk_norm_rec_t records on the
 * device and hands none of them out: shift, scale, SGK_NORM_ZERO_SCALE and SGK_NORM_NONFINITE of a read are to be had
 * from sgk_normalise / sgk_normalise_f32 alone. */
int sgk_job_set_normalise(sgk_job_t *job, int method);

/* ---- subsequence DTW of float query batches against float target batches (additive to 0.2.3) --------------------------
 * What the rows of sgk_sref_levels are for: every query (a read's normalised event means, say) is aligned whole against
 * every target (a strand's normalised levels), with a free start and a free end in the target.  No reference function
 * defines this; the definition is the library's, and the results are bit for bit what it gives (tools/proto/
 * sdtw_proto.py is its numpy model).  Query q[0..m), target t[0..n), every operation float32 with one rounding per
 * operation and no contraction:
 *   c(i,j) = fabsf(q[i] - t[j])
 *   D(0,j) = c(0,j)                   S(0,j) = j
 *   D(i,0) = D(i-1,0) + c(i,0)        S(i,0) = S(i-1,0)          (= 0)
 *   D(i,j) = c(i,j) + best            S(i,j) = S(best's cell)
 *            best = D(i-1,j-1);  if (D(i-1,j) < best) best = D(i-1,j);  if (D(i,j-1) < best) best = D(i,j-1);
 *   score = min_j D(m-1,j);  end = the smallest j with that value;  start = S(m-1,end)
 * On a tie the diagonal wins over "up" and both win over "left": the order of the two strict compares is part of the
 * contract.  The query's values q[0 .. m) lie along target values t[start .. end], both inclusive.  score is not divided
 * by anything.  Sums of finite values that overflow give what IEEE gives (inf < inf is false: the earlier candidate
 * stays).  A pair whose query or target holds a NaN or an infinity: score NaN, end = start = -1, SGK_SDTW_NONFINITE (a
 * sweep over the reads decides this first; the recurrence never sees such a value).  A pair with m == 0 or n == 0: the
 * same outputs and SGK_SDTW_EMPTY (both bits where both hold).  With SGK_SDTW_NO_START in `options` start is -1
 * everywhere, score, end and flags are unchanged, and the call is faster.
 * The call is all against all, out[qi * n_targets + ti]; targets are few (the two strands of each contig).  Both batches
 * are float batches under the contract above: q and t are 4-byte aligned, offsets are any element index, reads may touch
 * but not overlap, no byte outside the reads is read, nothing but `out` and the workspace is written; the call is
 * asynchronous on `stream`, allocates nothing and makes no host round trip.  n_queries == 0 or n_targets == 0 is SGK_OK
 * with nothing written.  Unknown option bits, a null pointer with a non-zero count, max_query_len or max_target_len >=
 * 2^31 are SGK_ERR_ARG; the workspace is 16-byte aligned, and one smaller than sgk_sdtw_f32_workspace_bytes is
 * SGK_ERR_WORKSPACE with nothing written; SGK_ERR_NODEVICE comes after the argument checks.  lengths[r] <= max_*_len is
 * the caller's word, as in every float batch (the lengths are device memory and the call makes no round trip, so the host
 * cannot answer SGK_ERR_ARG); here the device checks it, since the band rows below are sized by max_target_len: every
 * pair of a read longer than its max gets score NaN, end = start = -1 and SGK_SDTW_TOO_LONG, and the read is not looked at.
 * One wavefront per pair, the pairs of the longest queries first; a pair is never split over wavefronts or workgroups: a
 * target of 10^8 values is slow and right.  A query of up to 1 024 values lives in the wavefront's registers and needs no
 * workspace beyond a flag word per read and the dispatch order; a longer one runs in passes of 1 024 rows and keeps one
 * row of D and S per pass in one of a fixed number of slots (at most 2 048, fewer above 1 GB, never less than one) that
 * the wavefronts in flight take: the workspace does not grow with n_queries x max_target_len.  DESIGN.md 3.20. */
#define SGK_SDTW_NO_START 1u  /* options: start is -1 everywhere, score and end unchanged */
#define SGK_SDTW_EMPTY 1u     /* sgk_sdtw_rec_t::flags: m == 0 or n == 0 */
#define SGK_SDTW_NONFINITE 2u /* ... the query or the target holds a NaN or an infinity */
#define SGK_SDTW_TOO_LONG 4u  /* ... the query or the target is longer than its batch's max_*_len */
typedef struct sgk_sdtw_rec {
    float score;
    int32_t end, start;
    uint32_t flags;
} sgk_sdtw_rec_t; /* 16 bytes */
size_t sgk_sdtw_f32_workspace_bytes(uint32_t n_queries, uint32_t max_query_len, uint32_t n_targets, uint32_t max_target_len);
int sgk_sdtw_f32(const float *q, const uint64_t *q_offsets, const uint32_t *q_lengths, uint32_t n_queries,
                 uint32_t max_query_len, uint64_t n_q_values, const float *t, const uint64_t *t_offsets,
                 const uint32_t *t_lengths, uint32_t n_targets, uint32_t max_target_len, uint64_t n_t_values, uint32_t options,
                 sgk_sdtw_rec_t *out /* n_queries * n_targets records */, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGTK_GPU_H */
