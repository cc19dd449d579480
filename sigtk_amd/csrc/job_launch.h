// job_launch.h -- launchers that the job units call and other units define.  Every defining unit includes this header
// too, so that a definition is checked against the declaration its callers see.
#pragma once
#include "sgk_common.h"

namespace sgk {

// ---- zstd_kernels.hip
void zstd_release_scratch(int device, hipStream_t st);

// ---- zrec_kernels.hip
int zrec_tail_check(const uint8_t *inflated, const uint64_t *rec_offsets, const uint32_t *rec_lengths,
                    const uint32_t *tail_offsets, const uint32_t *gate, uint32_t n, const sgk_aux_field_t *fields,
                    uint32_t n_fields, uint32_t *status, hipStream_t st);

// ---- deflate_kernels.hip: qts record mode
int launch_qts_record_sizes(const uint32_t *frame_offsets, const uint32_t *head_lengths, const uint32_t *sig_counts,
                            uint32_t sig_unit, uint32_t n, uint64_t *head_offsets, uint64_t *tail_offsets,
                            uint32_t *tail_lengths, uint32_t *rec_lengths, uint32_t *caps, hipStream_t st);
int launch_qts_zrec_sizes(const uint64_t *rec_offsets, const uint32_t *rec_caps, const uint32_t *inflated_lengths,
                          const uint64_t *sig_offsets, const uint32_t *sig_lengths, const uint32_t *inflate_status,
                          const uint32_t *tail_status, const uint32_t *new_counts, uint32_t n, uint64_t *head_offsets,
                          uint32_t *head_lengths, uint64_t *tail_offsets, uint32_t *tail_lengths, uint32_t *rec_lengths,
                          uint32_t *caps, uint32_t *bad, hipStream_t st);
int launch_qts_zrec_mark(const uint32_t *bad, uint32_t n, uint32_t *out_lengths, uint32_t *status, hipStream_t st);
int launch_qts_assemble(const uint8_t *head_src, const uint64_t *head_offsets, const uint32_t *head_lengths,
                        const uint8_t *tail_src, const uint64_t *tail_offsets, const uint32_t *tail_lengths, const uint32_t *skip,
                        const uint8_t *signal, const uint64_t *sig_offsets, const uint32_t *sig_counts, uint32_t sig_unit,
                        uint8_t *arena, const uint64_t *rec_offsets, uint32_t n, hipStream_t st);
int launch_bytes_gather(const uint8_t *src, const uint64_t *src_offsets, const uint32_t *lengths, uint32_t n, uint8_t *dst,
                        const uint64_t *dst_offsets, hipStream_t st);
int launch_deflate_unchecked(const uint8_t *in, const uint64_t *in_offsets, const uint32_t *in_lengths, uint32_t n, uint8_t *out,
                             const uint64_t *out_offsets, const uint32_t *out_caps, uint32_t *out_lengths, uint32_t *status,
                             hipStream_t st);

// ---- job_kernels.hip (like the internals of job.h: not among the library's dynamic symbols)
struct GatherArgs {
    const uint32_t *src[4];
    uint32_t *dst[4];
};
#pragma GCC visibility push(hidden)
// offs[r] = sum of counts[0..r), each clamped to its slot (if any) and rounded up to `align`; offs[n] = the total
int launch_layout(const uint32_t *counts, const uint64_t *slots_or_null, uint32_t n, uint32_t align, uint64_t *offs, hipStream_t st);
// items of read r: g.src[k][slots[r] .. +counts[r]) -> g.dst[k][doffs[r] ..), k < narr (4-byte items)
int launch_gather(const GatherArgs &g, int narr, const uint64_t *slots, const uint32_t *counts, const uint64_t *doffs,
                  uint32_t n_reads, hipStream_t st);
// events of read r: records src[slots[r] .. +counts[r]) -> the dense arrays g.dst[k][doffs[r] ..), k < narr
int launch_gather_events(const sgk_event_rec_t *src, const GatherArgs &g, int narr, const uint64_t *slots,
                         const uint32_t *counts, const uint64_t *doffs, uint32_t n_reads, hipStream_t st);
#pragma GCC visibility pop

}  // namespace sgk
