/* cmain.c -- the front ends of the subtools that go through the pipeline: option parsing and set-up only.
 *   cmain    pa / event / stat / jnn / prefix / ent (src/cmain.c:40-156, src/ent.c:63-105)
 *   qtsmain  qts (src/qts.c:46-165)
 * Options beyond the reference's: --gpus N, --batch-samples M, -t/--threads T, --host-decode, --host-inflate, --gpu-text,
 * event --detector, jnn --segmenter, prefix --adaptor / --polya, pa --normalise; qts --gpu-deflate, --gpu-inflate. */
#include <ctype.h>
#include <errno.h>
#include <float.h>
#include <getopt.h>
#include <sched.h>

#include "pipeline.h"
#include "segopt.h"

/* ------------------------------------------------------------------ what cmain and qtsmain share */

typedef struct {
    int n_gpus, nthreads, batch_set;
    uint64_t batch_samples;
    uint64_t aux_slack;   /* bytes of room per array column of a zlib record sent to the GPU (load_parse) */
} run_opts_t;

/* --gpus, --batch-samples, -t, --aux-slack; returns whether c was one of them */
static int run_option(int c, run_opts_t *o) {
    switch (c) {
        case OPT_GPUS: o->n_gpus = atoi(optarg); return 1;
        case 't': o->nthreads = atoi(optarg); return 1;
        case OPT_BATCH_SAMPLES:
            o->batch_samples = strtoull(optarg, NULL, 10);
            o->batch_set = 1;
            return 1;
        case OPT_AUX_SLACK:
            o->aux_slack = strtoull(optarg, NULL, 10);
            if (o->aux_slack > (1ull << 20)) o->aux_slack = 1ull << 20;
            return 1;
        default: return 0;
    }
}

/* host threads worth starting: half the online CPUs, but no more than the affinity mask or a cgroup CPU quota allow
 * (a GPU box may show 256 CPUs and grant a job 16: 64 threads then only throttle each other -- 1e10 samples of `stat`
 * took 3.7 s with 64 threads and 3.1 s with 16, profiles/r05_k_cli_steady_before.json) */
static int host_thread_budget(void) {
    long nc = sysconf(_SC_NPROCESSORS_ONLN);
    int n = nc > 1 ? (int)(nc / 2) : 1;
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) {
        const int a = CPU_COUNT(&set);
        if (a > 0 && a < n) n = a;
    }
    FILE *fp = fopen("/sys/fs/cgroup/cpu.max", "r");
    if (fp) {
        char q[64];
        long period = 0;
        if (fscanf(fp, "%63s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const long quota = atol(q);
            const int c = (int)((quota + period - 1) / period);
            if (c > 0 && c < n) n = c;
        }
        fclose(fp);
    }
    if (n > 64) n = 64;  /* inflate scales to ~64 threads; beyond that thread start-up dominates */
    return n < 1 ? 1 : n;
}

/* the devices and threads of a run; returns what initialising HIP took.  cmain says when it uses fewer GPUs than asked
 * for, qtsmain does not. */
static double devices_and_threads(run_opts_t *o, const char *who, int warn) {
    const double t_init0 = realtime();
    const int ndev = sgk_device_count();
    const double t_init = realtime() - t_init0;
    if (ndev <= 0) {
        ERROR(who, "%s", "no usable GPU: sigtk-amd has no CPU compute path");
        die_now();
    }
    if (o->n_gpus < 1) o->n_gpus = 1;
    if (o->n_gpus > ndev) {
        if (warn) WARNING(who, "--gpus %d requested but %d visible; using %d", o->n_gpus, ndev, ndev);
        o->n_gpus = ndev;
    }
    if (o->nthreads <= 0) o->nthreads = host_thread_budget();
    return t_init;
}

static void pipe_init(pipe_t *P, b5_file_t *f, const tool_t *tool, cli_times_t *times, const run_opts_t *o, FILE *out) {
    memset(P, 0, sizeof *P);
    P->f = f;
    P->tool = tool;
    P->times = times;
    P->nthreads = o->nthreads;
    P->n_gpus = o->n_gpus;
    P->out_fp = out;
}
/* the batch limit, once P->zrec is known: files whose records go to the GPU as they are take larger batches unless
 * --batch-samples says otherwise (the limit counts on-disk bytes: about one per sample in a BLOW5, four to five in a
 * text file) */
static void pipe_batch_limit(pipe_t *P, const run_opts_t *o, uint64_t zrec_samples) {
    const uint64_t samples = P->zrec && !o->batch_set ? zrec_samples : o->batch_samples;
    P->limit_bytes = P->f->text ? samples * 4 : samples;
}

/* ------------------------------------------------------------------ header-derived options */

/* the read groups beyond the first are only compared with it */
static void warn_other_groups(const b5_file_t *f, const char *fn, const char *key, const char *what, const char *first) {
    for (uint32_t i = 1; i < f->num_read_groups; i++) {
        char *cur = b5_hdr_get(f, key, i);
        if (cur && strcmp(cur, first))
            WARNING(fn, "%s mismatch: %s != %s in read group %d. Defaulted to %s", what, cur, first, (int)i, first);
        free(cur);
    }
}

/* src/misc.c:34-60 */
static int8_t drna_detect(const b5_file_t *f) {
    char *exp = b5_hdr_get(f, "experiment_type", 0);
    int8_t rna = 0;
    if (!exp) {
        WARNING("drna_detect", "%s", "experiment_type not found in SLOW5 header. Assuming genomic_dna");
        return 0;
    }
    if (strcmp(exp, "genomic_dna") == 0) {
        INFO("drna_detect", "DNA data detected.");
    } else if (strcmp(exp, "rna") == 0) {
        rna = 1;
        INFO("drna_detect", "RNA data detected.");
    } else {
        WARNING("drna_detect", "Unknown experiment type: %s. Assuming genomic_dna", exp);
    }
    warn_other_groups(f, "drna_detect", "experiment_type", "Experiment type", exp);
    free(exp);
    return rna;
}

/* src/misc.c:74-101 */
static int8_t pore_detect(const b5_file_t *f) {
    char *kit = b5_hdr_get(f, "sequencing_kit", 0);
    int8_t pore = SGK_PORE_R9;
    if (!kit) {
        WARNING("pore_detect", "%s", "sequencing_kit not found in SLOW5 header. Assuming R9.4.1");
        return 0;
    }
    if (strstr(kit, "114")) {
        pore = SGK_PORE_R10;
        INFO("pore_detect", "R10 data detected.");
    } else if (strstr(kit, "rna004")) {
        pore = SGK_PORE_RNA004;
        INFO("pore_detect", "RNA004 data detected.");
    } else {
        INFO("pore_detect", "R9 data detected.");
    }
    warn_other_groups(f, "pore_detect", "sequencing_kit", "sequencing_kit type", kit);
    free(kit);
    return pore;
}

/* ------------------------------------------------------------------ cmain: options */

typedef struct {
    run_opts_t run;
    opt_t opt;
    FILE *fp_help;
    int hdr, host_decode, host_inflate, gpu_text;
    int verbosity;   /* -v / --verbose: 4 and up names the routes the given parameters take */
    int have_det, have_seg, have_ad, have_pl;
    int normalise;   /* pa --normalise: SGK_NORM_* */
    sgk_event_params_t det;                /* event --detector */
    double seg_v[8], ad_v[5], pl_v[7];     /* jnn --segmenter, prefix --adaptor, prefix --polya */
} copts_t;

static struct option long_options[] = {
    {"verbose", required_argument, 0, 'v'}, {"help", no_argument, 0, 'h'}, {"version", no_argument, 0, 'V'},
    {"output", required_argument, 0, 'o'}, {"print-stat", no_argument, 0, OPT_PRINT_STAT}, {"no-header", no_argument, 0, 'n'},
    {"compact", no_argument, 0, 'c'}, {"gpus", required_argument, 0, OPT_GPUS}, {"batch-samples", required_argument, 0, OPT_BATCH_SAMPLES},
    {"threads", required_argument, 0, 't'}, {"host-decode", no_argument, 0, OPT_HOST_DECODE}, {"host-inflate", no_argument, 0, OPT_HOST_INFLATE},
    {"gpu-text", no_argument, 0, OPT_GPU_TEXT}, {"aux-slack", required_argument, 0, OPT_AUX_SLACK}, {"detector", required_argument, 0, OPT_DETECTOR},
    {"segmenter", required_argument, 0, OPT_SEGMENTER}, {"adaptor", required_argument, 0, OPT_ADAPTOR}, {"polya", required_argument, 0, OPT_POLYA},
    {"normalise", required_argument, 0, OPT_NORMALISE}, {0, 0, 0, 0}};

/* event --detector W1,W2,THR1,THR2,PEAK_HEIGHT: exactly five fields, none empty, nothing behind a number, windows as
 * decimal integers; the domain is the library's (sgk_event_params_check, a host-only call).  Returns 0, or -1 with *why
 * set to what is wrong. */
static int parse_detector(const char *arg, sgk_event_params_t *out, const char **why) {
    double v[5];
    const char *p = arg;
    memset(out, 0, sizeof *out);
    for (int k = 0; k < 5; k++) {
        if (*p == '\0' || *p == ',') { *why = "an empty field"; return -1; }
        if (isspace((unsigned char)*p)) { *why = "white space in a field"; return -1; }
        char *end = NULL;
        if (k < 2) {
            if (*p < '0' || *p > '9') { *why = "a window length that is no unsigned integer"; return -1; }
            errno = 0;
            const unsigned long long u = strtoull(p, &end, 10);
            if (errno || u > 0xffffffffull) { *why = "a window length out of range"; return -1; }
            v[k] = (double)u;
        } else {
            v[k] = strtod(p, &end);
            if (end == p) { *why = "a field that is no number"; return -1; }
            /* (in double, before the cast: a double beyond float's range has no defined conversion; NaN fails too) */
            if (!(v[k] >= 0.0 && v[k] <= (double)FLT_MAX)) { *why = "a threshold or peak height that is not finite and >= 0"; return -1; }
        }
        if (k < 4) {
            if (*end == '\0') { *why = "fewer than five fields"; return -1; }
            if (*end != ',') { *why = "text behind a number"; return -1; }
            p = end + 1;
        } else if (*end == ',') { *why = "more than five fields"; return -1; }
        else if (*end != '\0') { *why = "text behind a number"; return -1; }
    }
    out->window_length1 = (uint32_t)v[0];
    out->window_length2 = (uint32_t)v[1];
    out->threshold1 = (float)v[2];
    out->threshold2 = (float)v[3];
    out->peak_height = (float)v[4];
    if (sgk_event_params_check(out) != SGK_OK) {
        *why = "values out of domain (windows 2 .. 64, W2 of 2 or 3 only with W1 = W2; thresholds and peak height finite and >= 0)";
        return -1;
    }
    return 0;
}

/* --detector, --segmenter, --adaptor, --polya: each an option of one subtool, each a list of a fixed form */
static void list_option(int c, const tool_t *tool, copts_t *o) {
    static const char *const name[4] = {"--detector", "--segmenter", "--adaptor", "--polya"};
    static const char *const owner[4] = {"event", "jnn", "prefix", "prefix"};
    static const char *const form[4] = {"W1,W2,THR1,THR2,PEAK_HEIGHT",
                                        "STD_SCALE,CORRECTOR,SEG_DIST,WINDOW,STALL_LEN,ERROR[,TOP,BOT] (TOP,BOT exactly when STD_SCALE <= 0)",
                                        "STD_SCALE,SEG_DIST,WINDOW,HI_THRESH,LO_THRESH", "CORRECTOR,SEG_DIST,WINDOW,STALL_LEN,ERROR,SHIFT,BAND"};
    const int k = c - OPT_DETECTOR;
    const char *why = "";
    if (strcmp(tool->name, owner[k]) != 0) {
        ERROR("cmain", "%s is an option of the %s subtool", name[k], owner[k]);
        exit(EXIT_FAILURE);
    }
    const int rc = k == 0 ? parse_detector(optarg, &o->det, &why) : k == 1 ? segopt_segmenter(optarg, o->seg_v, &why) :
                   k == 2 ? segopt_adaptor(optarg, o->ad_v, &why) : segopt_polya(optarg, o->pl_v, &why);
    if (rc != 0) {
        ERROR("cmain", "%s wants %s; '%s' has %s", name[k], form[k], optarg, why);
        exit(EXIT_FAILURE);
    }
    if (k == 0) o->have_det = 1; else if (k == 1) o->have_seg = 1; else if (k == 2) o->have_ad = 1; else o->have_pl = 1;
}

/* pa --normalise zscore|medmad */
static void normalise_option(const tool_t *tool, copts_t *o) {
    if (tool->mode != MODE_PA) {
        ERROR("cmain", "%s", "--normalise is an option of the pa subtool");
        exit(EXIT_FAILURE);
    }
    if (strcmp(optarg, "zscore") == 0) o->normalise = SGK_NORM_ZSCORE;
    else if (strcmp(optarg, "medmad") == 0) o->normalise = SGK_NORM_MEDMAD;
    else {
        ERROR("cmain", "--normalise wants zscore or medmad; '%s' is neither", optarg);
        exit(EXIT_FAILURE);
    }
}

static void cmain_parse(int argc, char *argv[], const tool_t *tool, copts_t *o) {
    /* `ent` has its own front end in the reference (src/ent.c:63-105): only -h/-V (and --no-header) are options,
     * exactly one file argument, no DNA/RNA or pore detection */
    const char *optstring = tool->mode == MODE_ENT ? "hVt:" : "o:hVnct:v:";
    int c;
    memset(o, 0, sizeof *o);
    o->fp_help = stderr;
    o->hdr = 1;
    o->run.n_gpus = 1;
    o->run.aux_slack = 256;
    o->run.batch_samples = tool->batch_samples;
    while ((c = getopt_long(argc, argv, optstring, long_options, NULL)) >= 0) {
        if (run_option(c, &o->run)) continue;
        switch (c) {
            case 'V': version_exit(); break;
            case 'h': o->fp_help = stdout; break;
            case 'n': o->hdr = 0; break;
            case 'c': o->opt.compact = 1; break;
            case 'v': o->verbosity = atoi(optarg); break;
            case OPT_PRINT_STAT: o->opt.p_stat = 1; break;
            case OPT_HOST_DECODE: o->host_decode = 1; break;
            case OPT_HOST_INFLATE: o->host_inflate = 1; break;
            case OPT_GPU_TEXT: o->gpu_text = 1; break;
            case OPT_DETECTOR: case OPT_SEGMENTER: case OPT_ADAPTOR: case OPT_POLYA: list_option(c, tool, o); break;
            case OPT_NORMALISE: normalise_option(tool, o); break;
            default: break;   /* -o, and what getopt has already complained about: ignored, as in the reference */
        }
    }
    if (o->normalise && o->gpu_text) {   /* the device formatter writes pA rows from the int16 samples */
        ERROR("cmain", "%s", "--normalise cannot be combined with --gpu-text");
        exit(EXIT_FAILURE);
    }
}

/* ------------------------------------------------------------------ cmain: segmenter, adaptor and polyA parameters */

static void fill_adaptor(sgk_prefix_params_t *p, const double *v) {
    p->adaptor.std_scale = (float)v[0]; p->adaptor.seg_dist = (int)v[1]; p->adaptor.window = (int)v[2];
    p->adaptor.hi_thresh = (int)v[3]; p->adaptor.lo_thresh = (int)v[4];
}
static void fill_polya(sgk_prefix_params_t *p, const double *v) {
    memset(&p->polya, 0, sizeof p->polya);
    p->polya.std_scale = -1.0f; p->polya.corrector = (int)v[0]; p->polya.seg_dist = (int)v[1]; p->polya.window = (int)v[2];
    p->polya.stall_len = (float)v[3]; p->polya.error = (int)v[4];
    p->shift = (float)v[5];
    p->band = (float)v[6];
}
static void domain_error(const char *msg) {
    ERROR("cmain", "%s", msg);
    exit(EXIT_FAILURE);
}
/* the domain is the library's (host-only calls): refused before any file is opened.  Leaves the segmenter's set in *seg. */
static void check_params(const copts_t *o, sgk_jnn_param_t *seg) {
    const double *v = o->seg_v;
    memset(seg, 0, sizeof *seg);
    if (o->have_seg) {
        seg->std_scale = (float)v[0]; seg->corrector = (int)v[1]; seg->seg_dist = (int)v[2]; seg->window = (int)v[3];
        seg->stall_len = (float)v[4]; seg->error = (int)v[5]; seg->top = (float)v[6]; seg->bot = (float)v[7];
        if (sgk_jnn_params_check(seg) != SGK_OK)
            domain_error("--segmenter: values out of domain (WINDOW 32 .. 16777216, CORRECTOR >= 1, ERROR >= 0, SEG_DIST >= 0, STALL_LEN >= 0)");
    }
    if (!o->have_ad && !o->have_pl) return;
    /* one definition of the domain, the library's: the given sets over a preset (the file's pore, known once it is
     * open, picks the preset of the set that is not given) */
    sgk_prefix_params_t chk;
    if (sgk_prefix_params_preset(1, SGK_PORE_R9, &chk) != SGK_OK) exit(EXIT_FAILURE);
    if (o->have_ad) {
        fill_adaptor(&chk, o->ad_v);
        if (sgk_prefix_params_check(&chk) != SGK_OK)
            domain_error("--adaptor: values out of domain (WINDOW 2 .. 13981, LO_THRESH >= 1, HI_THRESH >= LO_THRESH, SEG_DIST >= 0)");
    }
    if (o->have_pl) {
        fill_polya(&chk, o->pl_v);
        if (sgk_prefix_params_check(&chk) != SGK_OK)
            domain_error("--polya: values out of domain (WINDOW 32 .. 16777216, CORRECTOR >= 1, ERROR >= 0, SEG_DIST >= 0, STALL_LEN >= 0, BAND >= 0)");
    }
}

/* the parameters the jobs of this run take in place of the presets (P->opt is set: the file is open) */
static void run_params(pipe_t *P, copts_t *o, const sgk_jnn_param_t *seg, sgk_prefix_params_t *pre) {
    if (o->have_det) {   /* the read kind no longer selects the detector */
        /* the presets' kernels with these thresholds wherever the library's domain allows (windows 3/6 or 7/14,
         * THR2 >= 9); elsewhere the flag is ignored and the generic kernel runs.  The rows do not depend on the route. */
        o->det.flags |= SGK_EVENT_PARAMS_PRESET_KERNELS;
        if (o->verbosity >= 4) {
            const int route = sgk_event_params_route(&o->det);
            fprintf(stderr, "[event] detector route: %s\n", route == SGK_EVENT_ROUTE_PRESET ? "preset" :
                    route == SGK_EVENT_ROUTE_PRESET_WINDOWS ? "preset windows" : "generic");
        }
        P->ev_params = &o->det;
    }
    if (o->have_seg) P->jnn_params = seg;
    if (o->have_ad || o->have_pl) {
        /* the set that is not given stays the preset of the file's pore */
        const int rc = sgk_prefix_params_preset(P->opt.rna, P->opt.pore, pre);
        if (rc != SGK_OK) gpu_fail(NULL, "sgk_prefix_params_preset", rc);
        if (o->have_ad) fill_adaptor(pre, o->ad_v);
        if (o->have_pl) fill_polya(pre, o->pl_v);
        const int route = sgk_prefix_route(pre);
        if (route < 0) gpu_fail(NULL, "sgk_prefix_route", route);
        if (o->verbosity >= 4)
            fprintf(stderr, "[prefix] adaptor route: %s; polyA route: %s\n", (route & SGK_PREFIX_ROUTE_ADAPTOR_PARAM) ? "generic" : "preset",
                    (route & SGK_PREFIX_ROUTE_POLYA_WAVE_PARAM) ? "wave, parameters" :
                    (route & SGK_PREFIX_ROUTE_POLYA_LANE_PARAM) ? "lane, parameters" : "preset");
        P->prefix_params = pre;
    }
}

/* ------------------------------------------------------------------ cmain */

static void cmain_usage(FILE *fp, const tool_t *tool) {
    const int is_ent = tool->mode == MODE_ENT;
    if (is_ent) fprintf(fp, "Usage: sigtk ent a.blow5\n");
    else fprintf(fp, "Usage: sigtk %s reads.blow5 read_id1 read_id2 .. \n       sigtk %s reads.blow5\n", tool->name, tool->name);
    fprintf(fp, "\nbasic options:\n");
    fprintf(fp, "   -h                         help\n");
    fprintf(fp, "   -n                         suppress header\n");
    if (!is_ent) fprintf(fp, "   -c                         compact output\n");
    fprintf(fp, "   --version                  print version\n");
    if (is_ent) exit(fp == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    fprintf(fp, "   --gpus INT                 number of GPUs; whole batches go round-robin [1]\n");
    fprintf(fp, "   --batch-samples INT        approximate raw samples per batch [134217728; with --host-inflate 16777216, jnn / prefix 67108864]\n");
    fprintf(fp, "   -t, --threads INT          host threads for inflating records / formatting rows [auto]\n");
    fprintf(fp, "   --host-decode              decode svb-zd signals (parse text SLOW5 signals) on the host instead of the GPU\n");
    fprintf(fp, "   --host-inflate             decompress zlib / zstd records on the host threads instead of the GPU\n");
    fprintf(fp, "   --gpu-text                 pa / event, whole-file mode: format the rows on the GPU and fetch them as text\n");
    fprintf(fp, "   --aux-slack INT            test option\n");
    if (tool->mode == MODE_PA) {
        fprintf(fp, "   --normalise zscore|medmad  print the normalised signal, (pA - shift) / scale in float, in place of pA:\n");
        fprintf(fp, "                              zscore: mean and standard deviation; medmad: median and 1.4826 * MAD\n");
    }
    if (tool->mode == MODE_JNN) {
        fprintf(fp, "   --segmenter STD_SCALE,CORRECTOR,SEG_DIST,WINDOW,STALL_LEN,ERROR[,TOP,BOT]\n");
        fprintf(fp, "                              the segmenter's parameters in place of the presets (WINDOW 32 .. 16777216;\n");
        fprintf(fp, "                              TOP,BOT: the fixed thresholds, given exactly when STD_SCALE <= 0)\n");
    }
    if (tool->mode == MODE_PREFIX) {
        fprintf(fp, "   --adaptor STD_SCALE,SEG_DIST,WINDOW,HI_THRESH,LO_THRESH\n");
        fprintf(fp, "                              the adaptor finder's parameters in place of the presets (WINDOW 2 .. 13981)\n");
        fprintf(fp, "   --polya CORRECTOR,SEG_DIST,WINDOW,STALL_LEN,ERROR,SHIFT,BAND\n");
        fprintf(fp, "                              the polyA finder's parameters in place of the presets; its thresholds are\n");
        fprintf(fp, "                              (adaptor mean + SHIFT) +- BAND [30, 20]\n");
        fprintf(fp, "   -v, --verbose INT          4 and up: name the kernels these parameters take\n");
    }
    exit(fp == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
}

int cmain(int argc, char *argv[], const tool_t *tool, cli_times_t *times) {
    const int is_ent = tool->mode == MODE_ENT;
    copts_t o;
    sgk_jnn_param_t seg_p;
    sgk_prefix_params_t pre_p;
    cmain_parse(argc, argv, tool, &o);
    check_params(&o, &seg_p);
    if ((is_ent ? argc - optind != 1 : argc - optind < 1) || o.fp_help == stdout) cmain_usage(o.fp_help, tool);

    b5_file_t *f = b5_open(argv[optind]);
    if (!f) {
        if (is_ent) fprintf(stderr, "Error in opening file\n"); /* ent.c:97-100 */
        else ERROR("cmain", "cannot open %s. ", argv[optind]);
        die_now();
    }
    if (!is_ent) {
        o.opt.rna = drna_detect(f);
        o.opt.pore = pore_detect(f);
    }
    if (o.hdr) fputs((tool->mode == MODE_EVENT && o.opt.compact) || (tool->mode == MODE_PREFIX && o.opt.p_stat) ||
                   (tool->mode == MODE_PA && o.normalise) ? tool->header_alt : tool->header, stdout);
    const double t_init = devices_and_threads(&o.run, "cmain", 1);

    pipe_t P;
    pipe_init(&P, f, tool, times, &o.run, stdout);
    P.host_decode = o.host_decode;
    P.opt = o.opt;
    P.ids = argv + optind + 1;
    P.n_ids = argc - optind - 1;
    /* Records go to the GPU as they sit in the file when they are zlib streams or zstd frames around an svb-zd or an
     * uncompressed signal (signal_press 1 or 0: sgk_job_begin_zrec_signal) and the header's type line names only types
     * this reader knows, arrays included (the GPU then checks every record's auxiliary fields against that table);
     * everything else -- and --host-inflate / --host-decode, and reads fetched by id from a file with array columns -- is
     * inflated by the host threads as before. */
    P.zrec = pipe_zrec_setup(&P, o.run.aux_slack) && (f->signal_press == 0 || f->signal_press == 1) && !o.host_inflate && !o.host_decode && (P.n_ids == 0 || P.n_aux_arrays == 0);
    /* ... in batches of 128 M samples: the inflate kernel is a wavefront per record and takes ~35 ms however many records
     * it has (up to the ~4 800 the GPU holds at once), so a batch should bring a thousand of them (1e10 samples of `stat`:
     * 5.2 s with the 16 M-sample batches of the host path, 1.7 s with 128 M, profiles/r05_cli_steady.json) */
    pipe_batch_limit(&P, &o.run, 128ull << 20);
    /* rows as text from the GPU: the three large-output grammars, when the whole file is read in order (with read ids
     * on the command line, and for the other subtools, the option changes nothing) */
    P.gpu_text = o.gpu_text && (tool->mode == MODE_PA || tool->mode == MODE_EVENT) && P.n_ids == 0;
    P.normalise = o.normalise;
    run_params(&P, &o, &seg_p, &pre_p);
    run_pipeline(&P, t_init);
    fflush(stdout);
    b5_close(f);
    return 0;
}

/* ------------------------------------------------------------------ qtsmain (src/qts.c:46-165)
 * Same options as the reference (-o FILE, -b INT in [1,8], -m floor|round|fill-ones).  The output keeps the
 * input's header block and compression settings verbatim (the reference re-serialises the header through slow5lib
 * and always writes zlib + svb-zd); records carry the same fields, auxiliary data included, with the quantised
 * signal -- quantised and re-encoded (svb-zd) on the GPU, deflated on the host thread pool, or with --gpu-deflate
 * assembled and deflated on the GPU as well (Z_RLE-like streams of csrc/deflate_kernels.hip: other bytes, same records).
 * With --gpu-inflate (which implies --gpu-deflate) the records of a file the other subtools would send to the GPU as
 * they sit in the file go there for qts too: only their heads are inflated here, k_qts_assemble takes head and tail of
 * every record from where k_inflate / k_zstd left it, and the records stay on the GPU from file to file.
 * A text SLOW5 file is written back as a text SLOW5 file (both through slow5lib by extension in the reference,
 * src/qts.c:101-108): the header as it stands, every line with its four doubles re-printed as slow5lib prints them
 * (b5_s5_qts_head), the quantised column written on the GPU between the line's head and its auxiliary columns
 * (SGK_SIGNAL_TEXT | SGK_QTS_RECORDS).  Text in with BLOW5 out, or the reverse, is refused. */
static struct option qts_long_options[] = {
    {"verbose", required_argument, 0, 'v'}, {"help", no_argument, 0, 'h'},   {"version", no_argument, 0, 'V'},
    {"output", required_argument, 0, 'o'},  {"bits", required_argument, 0, 'b'}, {"method", required_argument, 0, 'm'},
    {"gpus", required_argument, 0, OPT_GPUS}, {"batch-samples", required_argument, 0, OPT_BATCH_SAMPLES}, {"threads", required_argument, 0, 't'},
    {"gpu-text", no_argument, 0, OPT_GPU_TEXT}, /* accepted, changes nothing: qts writes records, not rows */
    {"gpu-deflate", no_argument, 0, OPT_GPU_DEFLATE}, /* records assembled and deflated on the GPU (k_qts_assemble, k_deflate) */
    {"gpu-inflate", no_argument, 0, OPT_GPU_INFLATE}, /* ... and inflated there too: they stay on the GPU from file to file (implies --gpu-deflate) */
    {"aux-slack", required_argument, 0, OPT_AUX_SLACK}, /* test option, as in cmain: room per array column of a zlib record sent to the GPU */
    {0, 0, 0, 0}};

static void qts_die(const char *msg) {
    fprintf(stderr, "%s\n", msg);
    die_now();
}

/* the header goes out as it stands: a text file's is everything in front of the first record, a BLOW5's the fixed 68
 * bytes and the header text */
static void qts_copy_header(b5_file_t *f, FILE *out) {
    const size_t hb = f->text ? (size_t)f->first_rec : 68 + (size_t)f->hdr_size;
    uint8_t *h = (uint8_t *)grow_or_die(NULL, hb, 1);
    const int ok = fseek(f->fp, 0, SEEK_SET) == 0 && fread(h, 1, hb, f->fp) == hb;
    if (ok && !f->text && h[9] == 2) h[9] = 1;   /* zstd records in, zlib records out (row_qts) */
    if (!ok || fwrite(h, 1, hb, out) != hb || fseek(f->fp, (long)f->first_rec, SEEK_SET) != 0) qts_die("Error writing header!");
    free(h);
}

int qtsmain(int argc, char *argv[], const tool_t *tool, cli_times_t *times) {
    int c;
    FILE *fp_help = stderr;
    char *out_fn = NULL;
    int b = 1, gpu_deflate = 0, gpu_inflate = 0;
    const char *method = "round";
    run_opts_t ro = {1, 0, 0, tool->batch_samples, 256};
    while ((c = getopt_long(argc, argv, "hVv:o:b:m:t:", qts_long_options, NULL)) >= 0) {
        if (run_option(c, &ro)) continue;
        switch (c) {
            case 'V': version_exit(); break;
            case 'h': fp_help = stdout; break;
            case 'o': out_fn = optarg; break;
            case 'b':
                b = atoi(optarg);
                if (b < 1 || b > 8) qts_die("Error: number of bits to truncate must be between 1 and 8");
                break;
            case 'm': method = optarg; break;
            case OPT_GPU_INFLATE: gpu_inflate = 1; /* fall through */
            case OPT_GPU_DEFLATE: gpu_deflate = 1; break;
            default: break;
        }
    }
    if (argc - optind != 1 || fp_help == stdout) {
        fprintf(fp_help, "Usage: sigtk qts a.blow5 -o out.blow5   (or a.slow5 -o out.slow5: text in, text out)\n");
        fprintf(fp_help, "\nbasic options:\n");
        fprintf(fp_help, "   -h                            help\n");
        fprintf(fp_help, "   -o FILE                       output file\n");
        fprintf(fp_help, "   --version                     print version\n");
        fprintf(fp_help, "   -b INT                        number of lower significant bits to eliminate [%d]\n", b);
        fprintf(fp_help, "   -m [floor|round|fill-ones]    quantisation method [round]\n");
        exit(fp_help == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
    }
    if (out_fn == NULL) qts_die("Error: output file not specified");
    int q_method = SGK_QTS_FLOOR;
    if (strcmp(method, "round") == 0) q_method = SGK_QTS_ROUND;
    else if (strcmp(method, "fill-ones") == 0) q_method = SGK_QTS_FILL_ONES;
    else if (strcmp(method, "floor") != 0) qts_die("Unknown method for -m. Available options are floor,round,fill-ones.");
    /* Records are rewritten around the new signal in the container they came in: BLOW5 records byte for byte, text lines
     * with their auxiliary columns as they stand.  Going from one container to the other would mean re-serialising the
     * header and every typed auxiliary field: refused, whichever way the names or the content say it is mixed. */
    static const char mixed[] = "Error: qts on text SLOW5 files is not supported: use BLOW5 for the input and the output";
    const size_t ni = strlen(argv[optind]), no = strlen(out_fn);
    const int in_text = ni >= 6 && strcmp(argv[optind] + ni - 6, ".slow5") == 0;
    const int out_text = no >= 6 && strcmp(out_fn + no - 6, ".slow5") == 0;
    if (in_text != out_text) qts_die(mixed);
    b5_file_t *f = b5_open(argv[optind]);
    if (!f) qts_die("Error in opening file");
    if ((f->text != 0) != out_text) qts_die(mixed);   /* (text under a name that does not say so) */
    FILE *out = fopen(out_fn, "wb");
    if (!out) qts_die("Error opening file!");
    qts_copy_header(f, out);
    const double t_init = devices_and_threads(&ro, "qtsmain", 0);
    pipe_t P;
    pipe_init(&P, f, tool, times, &ro, out);
    P.q_bits = b;
    P.q_method = q_method;
    P.gpu_deflate = gpu_deflate && f->record_press != 0;   /* (uncompressed records: nothing to deflate, the flag changes nothing) */
    P.q_text = f->text;   /* lines out: no record sizes and no end-of-file marker */
    /* --gpu-inflate: the records go to the GPU as they sit in the file, under cmain's conditions for that (qts has no
     * read-id mode); on any other file the option is --gpu-deflate alone.  Then in batches of 64 M samples unless
     * --batch-samples says otherwise: the inflate kernel wants several hundred records in flight, and the 128 M of the
     * other subtools cost more in growing the record and stream buffers than they gain (profiles/qts_gpu_inflate.md:
     * 0.34 s at 64 M against 0.39 - 0.75 s at 128 M and 0.39 - 0.46 s at 16 M on 4e8 samples). */
    if (gpu_inflate) P.zrec = pipe_zrec_setup(&P, ro.aux_slack) && f->signal_press == 1;   /* (an uncompressed signal: --gpu-deflate alone) */
    pipe_batch_limit(&P, &ro, 64ull << 20);
    run_pipeline(&P, t_init);
    if ((!f->text && fwrite("5WOLB", 1, 5, out) != 5) || fclose(out) != 0) qts_die("Error writing record!");
    b5_close(f);
    return 0;
}
