/* sigtk_amd.c -- `sigtk-amd`: drop-in host CLI for sigtk's subtools with the compute on MI355X through
 * libsigtk_gpu.so.  This unit is the reference's src/main.c:76-123: subcommand dispatch, version/usage, stderr footer.
 * The rest mirrors the reference's front end unit by unit:
 *   cmain.c      src/cmain.c:40-156, src/qts.c:46-165: options, DNA/RNA and pore detection, sequential or read-id mode
 *   rows.c       src/cfunc.c: the TSV grammar of every subtool (byte-identical output)
 *   pipeline.c   what differs by design: records go through a reader, a loader and a writer in batches, several in
 *                flight, on the threads of pool.c (BLOW5 and text SLOW5 alike; whole batches shard over GPUs)
 *   sref.c ss.c  subtools with pipelines of their own;  selftest.c  what the tests drive without a GPU */
#include <sys/resource.h>

#include "pipeline.h"
#include "sref.h"
#include "ss.h"
#include "version.h"

/* SGK_CLI_TIMING: where the wall time of a run goes that the pipeline's stage sums do not show (process start,
 * HIP initialisation, first launch = code object load, buffer set-up, teardown).  Seconds since the process was
 * started (execve), from /proc: starttime of /proc/self/stat against /proc/uptime. */
static double since_exec(void) {
    FILE *f = fopen("/proc/self/stat", "r");
    if (!f) return -1.0;
    char buf[1024];
    const size_t n = fread(buf, 1, sizeof buf - 1, f);
    fclose(f);
    buf[n] = 0;
    const char *p = strrchr(buf, ')');   /* the command name may hold spaces */
    if (!p) return -1.0;
    unsigned long long start = 0;
    int field = 2;
    for (p++; *p && field < 22; p++)
        if (*p == ' ') field++;
    if (sscanf(p, "%llu", &start) != 1) return -1.0;
    double up = 0.0;
    f = fopen("/proc/uptime", "r");
    if (!f) return -1.0;
    if (fscanf(f, "%lf", &up) != 1) up = -1.0;
    fclose(f);
    return up < 0 ? -1.0 : up - (double)start / (double)sysconf(_SC_CLK_TCK);
}

static void print_usage(FILE *fp) {
    fprintf(fp, "Usage: sigtk <command> [options]\n\n");
    fprintf(fp, "command:\n");
    fprintf(fp, "         pa        print raw signal in pico-amperes\n");
    fprintf(fp, "         event     segment raw signal into events\n");
    fprintf(fp, "         stat      print statistics of the raw signal\n");
    fprintf(fp, "         prefix    prefix segments such as adaptor and polyA\n");
    fprintf(fp, "         jnn       print segments found using JNN segmenter\n");
    fprintf(fp, "         ent       calculate entropies\n");
    fprintf(fp, "         qts       quantise the raw signal in a S/BLOW5 files\n");
    fprintf(fp, "         sref      print synthetic reference signal (needs --kmer-model FILE)\n");
    fprintf(fp, "         ss        ss string conversion\n");
    fprintf(fp, "\n(sigtk-amd: every command of sigtk on MI355X; gzipped PAF input for ss is not part of it)\n");
    exit(fp == stdout ? EXIT_SUCCESS : EXIT_FAILURE);
}

/* the subcommands beside the pipeline's (those are the rows of the table in rows.c); the hidden ones return at once,
 * without the footer */
static const struct {
    const char *name;
    int (*fn)(int argc, char *argv[]);
    int hidden;
} others[] = {{"sref", srefmain, 0},       {"ss", ssmain, 0},           {"_fadump", fadumpmain, 1},
              {"_modelcheck", modelcheckmain, 1}, {"_dump", dumpmain, 1},      {"_zstd", zstdmain, 1},
              {"_fmtcheck", fmtcheckmain, 1},     {"_textcheck", textcheckmain, 1}, {"_qtsframes", qtsframesmain, 1}};

static int other_index(const char *name) {
    for (int i = 0; i < (int)(sizeof others / sizeof others[0]); i++)
        if (strcmp(name, others[i].name) == 0) return i;
    return -1;
}

int main(int argc, char *argv[]) {
    const double realtime0 = realtime();
    cli_times_t T = {realtime0, -1.0, 0.0, 0.0, 0.0};
    if (getenv("SGK_CLI_TIMING")) T.exec_to_main = since_exec();
    int ret = 1;
    const tool_t *tool = argc < 2 ? NULL : tool_by_name(argv[1]);
    const int other = argc < 2 ? -1 : other_index(argv[1]);
    if (argc < 2) {
        print_usage(stderr);
    } else if (tool) {
        ret = (tool->mode == MODE_QTS ? qtsmain : cmain)(argc - 1, argv + 1, tool, &T);
    } else if (other >= 0) {
        ret = others[other].fn(argc - 1, argv + 1);
        if (others[other].hidden) return ret;
    } else if (strcmp(argv[1], "--version") == 0 || strcmp(argv[1], "-V") == 0) {
        version_exit();
    } else if (strcmp(argv[1], "--help") == 0 || strcmp(argv[1], "-h") == 0) {
        print_usage(stdout);
    } else {
        fprintf(stderr, "[sigtk] Unrecognised command %s\n", argv[1]);
        print_usage(stderr);
    }
    fprintf(stderr, "[%s] Version: %s\n", __func__, SIGTK_VERSION);
    fprintf(stderr, "[%s] CMD:", __func__);
    for (int i = 0; i < argc; ++i) fprintf(stderr, " %s", argv[i]);
    struct rusage r;
    getrusage(RUSAGE_SELF, &r);
    fprintf(stderr, "\n[%s] Real time: %.3f sec; CPU time: %.3f sec; Peak RAM: %.3f GB\n\n", __func__, realtime() - realtime0,
            r.ru_utime.tv_sec + r.ru_stime.tv_sec + 1e-6 * (r.ru_utime.tv_usec + r.ru_stime.tv_usec),
            r.ru_maxrss * 1024 / 1024.0 / 1024.0 / 1024.0);
    if (getenv("SGK_CLI_TIMING") && T.t_pipeline_end > 0.0)
        fprintf(stderr,
                "[sigtk-amd] timeline: exec -> main %.3f s (loader, library constructors) | main -> first batch submitted "
                "%.3f s (HIP init, job buffers, first launches = code object load) | -> pipeline drained %.3f s | teardown "
                "%.3f s | total since exec %.3f s\n",
                T.exec_to_main, T.t_first_submit > 0.0 ? T.t_first_submit - T.t_main : -1.0,
                T.t_pipeline_end - (T.t_first_submit > 0.0 ? T.t_first_submit : T.t_main), T.t_destroyed - T.t_pipeline_end,
                T.exec_to_main + (realtime() - T.t_main));
    /* everything is written; leave without running the HIP runtime's exit handlers (they take longer than a
     * small input does) */
    if (fflush(stdout) != 0 || ferror(stdout)) {
        /* a short final write (ENOSPC, EPIPE) must not leave a truncated TSV behind exit code 0 */
        fprintf(stderr, "[%s::ERROR] writing to stdout failed\n", __func__);
        ret = EXIT_FAILURE;
    }
    fflush(stderr);
    _exit(ret);
}
