// stat_launch.hip -- host side of stat / jnn / prefix: the presets, when a batch gets a dispatch order, the rule that
// picks the lane-per-read or the wave-per-read implementation for a batch, and the launchers.  It holds no kernel and
// includes no device header: every kernel is launched through the launch_k_* function its own unit exports
// (stat_args.h).  The map of the stat units is in stat_device.h.
#include "sgk_common.h"
#include "side_stream.h"
#include "stat_args.h"

namespace sgk {

JnnP jnn_preset(int rna) {  // JNNV1_DRNA_R9_PARAM / JNNV1_CDNA_R9_PARAM, src/jnn.h:29-49
    JnnP p;
    p.std_scale = 0.75f; p.corrector = 50; p.seg_dist = 50; p.error = 5; p.top = 0.0f; p.bot = 0.0f;
    if (rna) { p.window = 1000; p.stall_len = 1.0f; }
    else { p.window = 150; p.stall_len = 0.25f; }
    return p;
}
JnnP jnn_polya_preset() {  // src/jnn.h:52-72
    JnnP p;
    p.std_scale = -1.0f; p.corrector = 50; p.seg_dist = 200; p.window = 250; p.stall_len = 1.0f; p.error = 30;
    p.top = 0.0f; p.bot = 0.0f;
    return p;
}
AdaptP adaptor_preset(int pore) {  // JNNV2_RNA_R9_ADAPTOR / JNNV2_RNA_RNA004_ADAPTOR, src/jnn.h:84-98
    AdaptP p;
    p.std_scale = (pore == SGK_PORE_RNA004) ? 0.7f : 0.5f;
    p.seg_dist = 1500;
    p.lo_thresh = (pore == SGK_PORE_RNA004) ? 500 : 2000;
    p.hi_thresh = 200000;
    return p;
}

// ---------------------------------------------------------------- dispatch order of the wave-per-read kernels:
// its place in the workspace and which batches get one (the sort itself, launch_order, is in stat_wave.hip)
size_t order_workspace_bytes(uint32_t n_reads) { return 64 + ((size_t)n_reads * 4 + 128 * 4 + 63) / 64 * 64; }
int prepare_order(StatArgs &a, void *ws, size_t ws_bytes, hipStream_t st) {
    a.order = nullptr;
    const uint32_t nr = a.b.n_reads;
    if (!ws || nr < ORDER_MIN_READS || ws_bytes < order_workspace_bytes(nr) || (reinterpret_cast<uintptr_t>(ws) & 3u)) return SGK_OK;
    // (a batch of near-equal lengths -- the longest read at most 1.25 x the mean -- is taken in batch order)
    if ((uint64_t)a.b.max_read_len * nr <= a.b.n_samples + a.b.n_samples / 4) return SGK_OK;
    uint32_t *order = reinterpret_cast<uint32_t *>(static_cast<char *>(ws) + 64), *hist = order + nr;
    const int rc = launch_order(a.b.lengths, nr, order, hist, st);
    if (rc != SGK_OK) return rc;
    a.order = order;
    return SGK_OK;
}

// ---------------------------------------------------------------- launchers
// Two implementations (sgk_stat_options_t::kernels): the lane-per-read kernels of round 1 (1; kept as an independent
// second implementation: tests compare the two, tools/bench_subtools.py times both) and the wave-per-read kernels (2).
// By default (0) a batch takes the wave kernels unless it is a LARGE batch of SHORT reads of SIMILAR length (stat:
// >= 49 152 reads of at most 32 768 samples or >= 16 384 of at most 16 384; jnn: >= 65 536 reads of at most 12 288; the
// longest at most 1.5 x the mean; prefix: see launch_prefix): there the lane-per-read kernels have 64 reads per wavefront, nothing to gain from intra-read parallelism and
// no per-read costs (native heads, binade crossings, chunk start-up), and are up to 2 x faster (400 000 x 5 000 samples:
// jnn 3.7 ms against 7.7 ms); everywhere else -- ragged, small or long-read batches -- the wave kernels win by 1.5 - 40 x.
// Per subtool (profiles/r04_z_subtools_wave_vs_lane_short_reads.txt, 2e9 samples per batch): stat's lane kernels win up to
// 32 768 samples per read (2.67 against 3.05 ms; at 65 536 the wave kernel wins), jnn's and prefix' only up to ~12 000
// (8 192: 3.5 / 7.0 against 5.4 / 7.6 ms; 16 384: 4.0 / 7.3 against 3.5 / 5.6).  stat's also win on smaller batches of
// short reads (20 000 x 5 000: 0.28 against 0.49 ms; 40 000 x 10 000: 0.61 against 1.13; 20 000 x 20 000: a tie), jnn's and
// prefix' need the 65 536 reads (40 000 x 5 000: 0.74 / 1.48 against 0.85 / 0.85).
bool stat_lane_per_read(int tool, int kernels, uint32_t n_reads, uint64_t n_samples, uint32_t max_read_len) {
    if (kernels == 1) return true;
    if (kernels == 2) return false;
    if (tool != 4 && (uint64_t)max_read_len * n_reads > n_samples + n_samples / 2) return false;  // not of similar length
    for (int k = 0; k < N_LANE_RULES; ++k) {
        const LaneRule &q = LANE_RULES[k];
        if (q.tool == tool && n_reads >= q.min_reads && max_read_len <= lane_rule_max_len(q, n_reads)) return true;
    }
    return false;   // (prefix' finders, tool 2: the wave kernels win at every shape)
}
static bool lane_per_read(int tool, const StatArgs &a) {
    return stat_lane_per_read(tool, a.kernels, a.b.n_reads, a.b.n_samples, a.b.max_read_len);
}

// The wave kernel (wave_launch(stream, args, grid) -> int) beside k_long_chains<kind>.  The long reads' few workgroups
// go to the caller's stream and the wave kernel to a side stream that first waits for the fork event: launched the other
// way round the long workgroups found every slot taken by the wave kernel's -- whose first workgroups hold the batch's
// longest reads -- and started 2 ms late.  Behind the join the wave kernel is launched once more over the long list
// (redo args: LC_CAP waves) for the reads k_long_chains declined -- a barrier of theirs timed out, lc_barrier; usually
// none, the launch costs a few microseconds: no read's result depends on the long path having worked.
template <typename WL>
static int launch_beside_long(int kind, const StatArgs &a, const JnnP &p, const AdaptP &ap, const char *name, hipStream_t st,
                              WL wave_launch) {
    if (!a.longs) return wave_launch(st, a, (a.b.n_reads + 3) / 4);
    {
        SideFork side;  // (joins at the end of this block)
        side.open(st, 1);
        int rc = launch_k_long_chains(name, kind, st, a, p, ap);
        if (rc == SGK_OK) rc = wave_launch(side.stream(0), a, (a.b.n_reads + 3) / 4);
        if (rc != SGK_OK) return rc;
    }
    StatArgs redo = a;
    redo.long_redo = 1u;
    redo.order = nullptr;
    return wave_launch(st, redo, LC_CAP / 4);
}

static int launch_stat_medians(const StatArgs &a, hipStream_t st);
// ... and behind whichever implementation ran, the pA medians that are a pick among equal-comparing values (a zero, a
// scale that is not finite) are redone with the reference's own selection (stat_literal.hip): one look per record
int launch_stat(const StatArgs &a, hipStream_t st) {
    if (a.b.n_reads == 0) return SGK_OK;
    const int rc = launch_stat_medians(a, st);
    return rc != SGK_OK ? rc : launch_k_median_literal("k_median_literal", REG_WHOLE, st, a);
}
static int launch_stat_medians(const StatArgs &a, hipStream_t st) {
    const uint32_t nr = a.b.n_reads;
    int rc;
    if (lane_per_read(a.pa_out ? 3 : 0, a)) {
        if (a.pa_out) {
            rc = launch_k_moments("k_moments", REG_WHOLE, false, st, a);
            if (rc == SGK_OK) rc = launch_k_median("k_median_pa", REG_WHOLE, true, false, st, a);
        } else if (nr >= STAT_MOMENTS_MEDIAN_MIN_READS) {
            // the medians come out of the moments' second pass; k_median only for the reads it flagged.  (With fewer reads
            // k_moments has too few wavefronts -- 64 reads each -- to hide what the counting adds, and k_median, a
            // workgroup per read, fills the GPU: 61 035 x 32 768 fused 2.70, apart 2.33 ms; 100 000 x 20 000 2.00 / 2.24.)
            rc = launch_k_moments("k_moments_median", REG_WHOLE, true, st, a);
            if (rc == SGK_OK) rc = launch_k_median("k_median_flagged", REG_WHOLE, false, true, st, a);
        } else {
            rc = launch_k_moments("k_moments", REG_WHOLE, false, st, a);
            if (rc == SGK_OK) rc = launch_k_median("k_median", REG_WHOLE, false, false, st, a);
        }
        return rc;
    }
    // the long reads' workgroups run beside the wave kernel (which skips those reads) when a side stream is to be had
    rc = launch_beside_long(LC_STAT, a, JnnP{}, AdaptP{}, "k_long_chains_stat", st, [&](hipStream_t st, const StatArgs &aw, uint32_t grid) {
        if (aw.pa_out) return launch_k_stat_wave(aw.long_redo ? "k_stat_wave_pa_redo" : "k_stat_wave_pa", REG_WHOLE, true, grid, st, aw);
        return launch_k_stat_wave(aw.long_redo ? "k_stat_wave_redo" : "k_stat_wave", REG_WHOLE, false, grid, st, aw);
    });
    if (rc != SGK_OK) return rc;
    return launch_k_median("k_median_flagged", REG_WHOLE, false, true, st, a);
}

int launch_jnn(const StatArgs &a, const JnnP &p, hipStream_t st) {
    const uint32_t nr = a.b.n_reads;
    if (nr == 0) return SGK_OK;
    SGK_HIP_TRY(hipMemsetAsync(a.err_count, 0, 4, st));
    const bool wave_ok = p.error >= 0 && p.error < p.corrector && p.error <= 31 && p.window >= 128;
    if (lane_per_read(1, a) || !wave_ok) return launch_k_jnn("k_jnn", st, a, p);
    StatArgs aw = a;
    if (!(p.std_scale > 0.0f)) aw.longs = nullptr;  // (fixed thresholds: no sums, k_jnn_wave does every read)
    const int rc = launch_beside_long(LC_JNN, aw, p, AdaptP{}, "k_long_chains_jnn", st, [&](hipStream_t st, const StatArgs &ax, uint32_t grid) {
        return launch_k_jnn_wave(ax.long_redo ? "k_jnn_wave_redo" : "k_jnn_wave", grid, st, ax, p);
    });
    if (rc != SGK_OK) return rc;
    StatArgs redo = a;
    redo.jnn_redo = 1u;  // the reads the wave kernel gave up on (none, usually: its wavefronts return at once)
    return launch_k_jnn("k_jnn_redo", st, redo, p);
}

int launch_adaptor(const StatArgs &a, const AdaptP &p, hipStream_t st) {
    const uint32_t nr = a.b.n_reads;
    if (nr == 0) return SGK_OK;
    if (lane_per_read(2, a)) return launch_k_adaptor(st, a, p);
    return launch_beside_long(LC_ADAPT, a, JnnP{}, p, "k_long_chains_adapt", st, [&](hipStream_t st, const StatArgs &ax, uint32_t grid) {
        return launch_k_adaptor_wave(ax.long_redo ? "k_adaptor_wave_redo" : "k_adaptor_wave", grid, st, ax, p);
    });
}

// The statistics of one region the prefix finders found (REG_ADAPT / REG_POLYA), under the region's profile names.
// lane_regions && !lanes: the medians out of the moments' second pass, k_median for the regions it flags.
static int launch_region_stats(int region, const StatArgs &a, bool lanes, bool lane_regions, hipStream_t st) {
    struct Names { const char *moments_median, *median_flagged, *moments, *median, *stat_wave; };
    static constexpr Names NAMES[2] = {
        {"k_moments_median_adapt", "k_median_adapt_flagged", "k_moments_adapt", "k_median_adapt", "k_stat_wave_adapt"},
        {"k_moments_median_polya", "k_median_polya_flagged", "k_moments_polya", "k_median_polya", "k_stat_wave_polya"}};
    static constexpr const char *LITERAL[2] = {"k_median_literal_adapt", "k_median_literal_polya"};
    if (region != REG_ADAPT && region != REG_POLYA) return SGK_ERR_ARG;  // a prefix region
    const Names &n = NAMES[region == REG_POLYA];
    int rc;
    if (lane_regions && !lanes) {
        rc = launch_k_moments(n.moments_median, region, true, st, a);
        if (rc == SGK_OK) rc = launch_k_median(n.median_flagged, region, false, true, st, a);
    } else if (lane_regions) {
        rc = launch_k_moments(n.moments, region, false, st, a);
        if (rc == SGK_OK) rc = launch_k_median(n.median, region, false, false, st, a);
    } else {
        rc = launch_k_stat_wave(n.stat_wave, region, false, (a.b.n_reads + 3) / 4, st, a);
        if (rc == SGK_OK) rc = launch_k_median(n.median_flagged, region, false, true, st, a);
    }
    if (rc == SGK_OK) rc = launch_k_median_literal(LITERAL[region == REG_POLYA], region, st, a);  // (see launch_stat)
    return rc;
}

int launch_prefix(const StatArgs &a, int rna, int pore, hipStream_t st) {
    return launch_prefix_param(a, rna, adaptor_preset(pore), 2000, false, nullptr, st);
}

// generic: k_adaptor_param whatever the window (it has no long-read split: a.longs is not looked at); poly: the
// parametrised polyA kernels -- one read per wavefront where polya_wave_ok holds, else (and where the caller forces the
// lane kernels) one read per lane
int launch_prefix_param(const StatArgs &a, int rna, const AdaptP &ap, int window, bool generic, const PolyP *poly, hipStream_t st) {
    const uint32_t nr = a.b.n_reads;
    if (nr == 0) return SGK_OK;
    // The adaptor and polyA finders: one read per wavefront unless the caller forces the lane kernels (k_adaptor_wave 4.3
    // against k_adaptor 5.5 ms on 400 000 x 5 000, 13.4 against 29 on 125 000 x 100 000; k_polya_wave 0.2 against 1.2 - 5.9).
    // The statistics of the regions they find are a few thousand samples per read whatever the read's length: with enough
    // reads to fill the lanes (64 per wavefront) the lane kernels do them in 1.0 ms where k_stat_wave takes 2.4 (400 000 x
    // 5 000), 0.9 + 1.2 against 1.1 + 1.4 (50 000 x 100 000 RNA, adaptor + polyA), a tie at 125 000 x 100 000.
    const bool lanes = lane_per_read(2, a);
    const bool lane_regions = lanes || lane_per_read(4, a);
    // (launch_adaptor joins its side stream inside: the kernels behind read every read's adapt_x / adapt_y)
    int rc = (generic || window != 2000) ? launch_k_adaptor_param(st, a, ap, window) : launch_adaptor(a, ap, st);
    if (rc == SGK_OK) rc = launch_region_stats(REG_ADAPT, a, lanes, lane_regions, st);
    if (rc != SGK_OK || !rna) return rc;
    if (!poly) rc = lanes ? launch_k_polya(st, a) : launch_k_polya_wave(st, a);
    else rc = (lanes || !polya_wave_ok(*poly)) ? launch_k_polya_param(st, a, *poly) : launch_k_polya_wave_param(st, a, *poly);
    if (rc != SGK_OK) return rc;
    return launch_region_stats(REG_POLYA, a, lanes, lane_regions, st);
}

}  // namespace sgk
