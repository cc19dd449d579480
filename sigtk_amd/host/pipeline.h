/* pipeline.h -- the three-thread pipeline of the per-record subtools (pipeline.c), the table of those subtools with
 * their row formatters (rows.c), and their front ends (cmain.c).
 *
 *   reader thread                 loader (main thread)                       writer thread
 *   -------------                 --------------------                       -------------
 *   take a free batch             take the next filled batch                 take the oldest submitted batch
 *   read the records' bytes       N threads: inflate + parse                 sgk_job_wait
 *   off the file, in order        sgk_job_begin (layout, pinned staging)     N threads: format rows into chunks
 *   hand it over                  N threads: copy svb-zd blobs / samples     fwrite the chunks in order
 *                                 sgk_job_submit (async H2D, decode,         return the batch to the free list
 *                                 kernels, D2H)
 *
 * n_gpus + 3 batches circulate; batch k runs on GPU k mod n_gpus (whole batches are the sharding unit:
 * every output row depends on one record only, src/cmain.c:118-120, so there is no collective). */
#ifndef SIGTK_AMD_PIPELINE_H
#define SIGTK_AMD_PIPELINE_H

#include "blow5.h"
#include "cli.h"
#include "pool.h"
#include "sigtk_gpu.h"

typedef struct {
    int8_t rna, compact, p_stat, pore; /* opt_t, src/sigtk.h:115-120 */
} opt_t;

enum { MODE_EVENT, MODE_STAT, MODE_PREFIX, MODE_JNN, MODE_PA, MODE_ENT, MODE_QTS };

typedef struct {
    uint64_t raw_off, raw_size; /* the record's on-disk bytes inside batch_t.raw ... */
    const uint8_t *raw_ptr;     /* ... or, when the file is mapped, in the mapping */
    uint8_t *scratch;           /* inflated record (kept per slot; grows only) */
    uint64_t scratch_cap;
    b5_view_t v;
    uint32_t room;              /* zrec: what the inflated record may take (load_parse) */
    uint64_t head_len;          /* qts on a text file: bytes of the line's head as it is written back, in `scratch` (load_parse) */
    int err;
} lrec_t;

typedef struct batch {
    qnode_t link;   /* first: the queues hand batches round by this node */
    sgk_job_t *job;
    sgk_job_input_t in;
    lrec_t *recs;
    uint32_t n, cap;
    uint8_t *raw;
    uint64_t raw_len, raw_cap;
    uint64_t bytes;  /* on-disk bytes gathered so far (the batch limit applies to it) */
    uint32_t *lengths, *blob_bytes;
    uint32_t *sig_off, *sig_len, *room; /* zrec: where the signal sits in the inflated record, its bytes, the record's inflated size */
    int svb;        /* signal staged as svb-zd blobs (GPU decode) */
    int sigtext;    /* signal staged as the raw_signal column of text SLOW5 records (GPU parse) */
    int zrec;       /* whole zlib records staged: inflated and decoded on the GPU */
    int last;       /* sentinel: no more batches */
    uint8_t *id_blob;   /* --gpu-text: the batch's read ids back to back, id r at id_offs[r] .. id_offs[r + 1] */
    uint32_t *id_offs;
    uint64_t id_blob_cap, id_offs_cap;
    uint8_t *fr_blob;   /* qts --gpu-deflate: per record its bytes in front of len_raw_signal, then those behind the signal */
    uint32_t *fr_offs, *fr_heads;   /* frame r at fr_offs[r] .. fr_offs[r + 1], its first fr_heads[r] bytes the head */
    uint64_t fr_blob_cap, fr_offs_cap;
} batch_t;

/* SGK_CLI_TIMING: where the wall time of a run goes that the pipeline's stage sums do not show; main owns it */
typedef struct {
    double t_main, exec_to_main, t_first_submit, t_pipeline_end, t_destroyed;
} cli_times_t;

struct pipe;
typedef void (*row_fn)(sbuf_t *o, const struct pipe *P, const batch_t *b, const sgk_job_output_t *out, uint32_t r);

/* one row per subtool that goes through the pipeline (rows.c) */
typedef struct {
    const char *name;
    int mode, sgk_tool;       /* MODE_*, SGK_TOOL_* (qts: -1, it has a submit call of its own) */
    row_fn row;
    uint64_t batch_samples;   /* default of --batch-samples */
    const char *header;       /* the TSV header line ... */
    const char *header_alt;   /* ... and what it is with -c (event) or --print-stat (prefix) */
} tool_t;
const tool_t *tool_by_name(const char *name);   /* NULL: not one of them */

typedef struct pipe {
    b5_file_t *f;
    const tool_t *tool;
    int nthreads, host_decode;
    int gpu_text;        /* --gpu-text (pa / event, whole-file mode): the rows come from the GPU as text */
    const sgk_event_params_t *ev_params; /* event --detector: every job's detector parameters (NULL: the presets) */
    const sgk_jnn_param_t *jnn_params;       /* jnn --segmenter (NULL: the presets) */
    const sgk_prefix_params_t *prefix_params; /* prefix --adaptor / --polya (NULL: the presets) */
    int normalise;       /* pa --normalise: SGK_NORM_* (0: pA) */
    uint64_t text_bytes; /* ... their bytes over PCIe */
    int zrec;            /* records go to the GPU as they sit in the file (zlib / zstd records, svb-zd or uncompressed signal, auxiliary columns of known types) */
    sgk_aux_field_t *aux_tab; /* ... those columns, in header order */
    uint32_t n_aux, n_aux_arrays; /* ... how many, and how many of them are arrays (u64 count + elements) */
    uint64_t aux_fixed;  /* ... the bytes of the others */
    uint64_t aux_slack;  /* ... zlib records: room per array column behind its count word (--aux-slack) */
    uint64_t n_zrec_reads;    /* records the GPU decompressed */
    uint64_t n_redone;        /* zrec batches redone on the host path (an array longer than its slack) */
    opt_t opt;
    queue_t free_q, filled_q, ready_q;
    /* reader thread input */
    uint64_t limit_bytes;
    char **ids;      /* read-id mode: ids[0..n_ids) */
    int n_ids;
    /* qts */
    int q_bits, q_method;
    int gpu_deflate;  /* qts --gpu-deflate on a file with compressed records: records assembled and deflated on the GPU */
    int q_text;       /* qts on a text file: the lines are written on the GPU around the new signal column */
    FILE *out_fp;    /* rows / records go here (stdout except for qts) */
    pool_t *load_pool; /* the loader's worker pool (the writer creates its own) */
    batch_t *pool; /* all batch slots; [0, n_created) have a job */
    int n_created, n_max, n_gpus;
    uint64_t batches_read;
    double t_read, t_parse, t_stage, t_wait, t_format, t_write; /* --verbose timing */
    uint64_t n_long_declined; /* long reads the 16-workgroup path of stat / jnn / prefix declined (redone on one wavefront) */
    uint64_t n_reads, n_samples;
    cli_times_t *times;
} pipe_t;

/* What a pipeline needs to send the records of P->f to the GPU as they sit in the file; returns whether the file is one
 * of those (pipeline.c) */
int pipe_zrec_setup(pipe_t *P, uint64_t aux_slack);
void run_pipeline(pipe_t *P, double t_init);   /* P->n_gpus GPUs; t_init: what initialising HIP took (for the report) */

int cmain(int argc, char *argv[], const tool_t *tool, cli_times_t *times);
int qtsmain(int argc, char *argv[], const tool_t *tool, cli_times_t *times);

#endif
