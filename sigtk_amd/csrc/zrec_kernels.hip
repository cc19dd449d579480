// zrec_kernels.hip -- k_zrec_tail: the auxiliary fields behind the signal of an inflated BLOW5 record, walked on the GPU.
//
// A record whose auxiliary columns include an array (`char*`, `double*`, ...) has no length its head could announce: an
// array field is a u64 element count followed by that many elements (slow5lib/src/slow5.c:3088-3165, binary branch).  The
// job layer therefore gives such a record room with slack, and "inflated to what the head announced" -- implied by an
// exact room -- becomes this check: walk the columns from the end of the signal, every field wholly inside the record's
// inflated length, the walk ending exactly at that length (what slow5_rec_aux_parse and the size check in front of it,
// slow5.c:2937-2949, establish on the host; where the reference reads a count or an array that ends behind its buffer,
// this refuses).
//
// One lane per record: a tail is tens of bytes and the work is one dependent chain per record (the position of a field
// depends on every count in front of it).  The column loop is uniform over the wavefront -- every lane is at column c in
// iteration c -- so a column's descriptor is one address for all lanes.  A record's tail starts at any byte address: a
// count word is read as the eight bytes it occupies (byte loads in the source; gfx950 under the HSA runtime takes global
// loads at any alignment, and the compiler may merge them into wider ones over the same eight bytes, never more).
// Nothing at or behind rec_offsets[r] + rec_lengths[r] is read; only status[r] is written.
#include <stdlib.h>
#include <string.h>

#include "job_launch.h"
#include "sgk_common.h"

namespace sgk {

// a column: bits 0-1 log2 of the element size (1, 2, 4, 8 bytes), bit 7 set for an array
__host__ inline uint8_t zt_descriptor(const sgk_aux_field_t &f) {
    const uint32_t lg = f.elem_bytes == 8 ? 3u : (f.elem_bytes == 4 ? 2u : (f.elem_bytes == 2 ? 1u : 0u));
    return (uint8_t)(lg | (f.is_array ? 0x80u : 0u));
}
constexpr uint32_t ZT_INLINE = 256;   // columns whose descriptors ride in the kernel arguments
struct ZtInline {
    uint8_t b[ZT_INLINE];
};

struct ZtArgs {
    const uint8_t *inflated;
    const uint64_t *rec_offsets;
    const uint32_t *rec_lengths;
    const uint32_t *tail_offsets;
    const uint32_t *gate;      // nullptr, or n words: a record with a non-zero word is not looked at (status 0)
    const uint8_t *fields;     // device, n_fields descriptors; nullptr: they are in `inl`
    uint32_t *status;
    uint32_t n, n_fields;
    ZtInline inl;
};

__device__ inline uint64_t zt_load_u64(const uint8_t *p) {
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k);
    return v;
}

__global__ __launch_bounds__(256) void k_zrec_tail(const ZtArgs a) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const bool live = r < a.n && !(a.gate && a.gate[r] != 0u);
    const uint8_t *rec = a.inflated;
    uint32_t len = 0u, pos = 0u, st = 0u;
    if (live) {
        rec += a.rec_offsets[r];
        len = a.rec_lengths[r];
        pos = a.tail_offsets[r];
        if (pos > len) st = 1u;   // the record ended inside or in front of its signal
    }
    bool walking = live && st == 0u;
    for (uint32_t c = 0; c < a.n_fields; ++c) {
        const uint32_t f = a.fields ? a.fields[c] : a.inl.b[c];   // wave-uniform
        const uint32_t lg = f & 3u, eb = 1u << lg;
        if (!walking) continue;
        const uint32_t left = len - pos;   // pos <= len while walking
        if (!(f & 0x80u)) {
            if (left < eb) { st = 2u; walking = false; }
            else pos += eb;
            continue;
        }
        if (left < 8u) { st = 2u; walking = false; continue; }   // no room for the count word
        const uint64_t count = zt_load_u64(rec + pos);            // bytes [pos, pos + 8) < len
        pos += 8u;
        if ((count >> (32u - lg)) != 0u) { st = 4u; walking = false; continue; }   // count x eb needs more than 32 bits
        const uint32_t bytes = (uint32_t)count << lg;
        if (len - pos < bytes) { st = 2u; walking = false; }
        else pos += bytes;
    }
    if (walking && pos != len) st = 3u;   // bytes behind the last field
    if (r < a.n) a.status[r] = st;
}

int launch_zrec_tail(const ZtArgs &a, hipStream_t st) {
    if (a.n == 0) return SGK_OK;
    SGK_LAUNCH("k_zrec_tail", k_zrec_tail, (a.n + 255u) / 256u, 256, st, a);
    return SGK_OK;
}

// the public entry and the job layer: fields is a HOST table
int zrec_tail_check(const uint8_t *inflated, const uint64_t *rec_offsets, const uint32_t *rec_lengths,
                    const uint32_t *tail_offsets, const uint32_t *gate, uint32_t n, const sgk_aux_field_t *fields,
                    uint32_t n_fields, uint32_t *status, hipStream_t st) {
    if (n == 0) return SGK_OK;
    if (!inflated || !rec_offsets || !rec_lengths || !tail_offsets || !status || (n_fields && !fields)) return SGK_ERR_ARG;
    for (uint32_t c = 0; c < n_fields; ++c) {
        const uint32_t eb = fields[c].elem_bytes;
        if ((eb != 1 && eb != 2 && eb != 4 && eb != 8) || fields[c].is_array > 1) return SGK_ERR_ARG;
    }
    ZtArgs a;
    a.inflated = inflated; a.rec_offsets = rec_offsets; a.rec_lengths = rec_lengths; a.tail_offsets = tail_offsets;
    a.gate = gate; a.fields = nullptr; a.status = status; a.n = n; a.n_fields = n_fields;
    memset(&a.inl, 0, sizeof a.inl);
    if (n_fields <= ZT_INLINE) {
        for (uint32_t c = 0; c < n_fields; ++c) a.inl.b[c] = zt_descriptor(fields[c]);
        return launch_zrec_tail(a, st);
    }
    // more columns than any writer makes: the descriptors go through a device buffer of their own, uploaded and released
    // with blocking calls (the one case in which this entry synchronises)
    uint8_t *host = static_cast<uint8_t *>(malloc(n_fields));
    if (!host) return SGK_ERR_NOMEM;
    for (uint32_t c = 0; c < n_fields; ++c) host[c] = zt_descriptor(fields[c]);
    uint8_t *dev = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&dev), n_fields);
    if (e == hipSuccess) e = hipMemcpy(dev, host, n_fields, hipMemcpyHostToDevice);
    free(host);
    if (e != hipSuccess) {
        set_hip_error(e, "hipMalloc / hipMemcpy", __FILE__, __LINE__);
        if (dev) (void)hipFree(dev);
        return SGK_ERR_HIP;
    }
    a.fields = dev;
    const int rc = launch_zrec_tail(a, st);
    e = hipStreamSynchronize(st);
    (void)hipFree(dev);
    if (rc != SGK_OK) return rc;
    SGK_HIP_TRY(e);
    return SGK_OK;
}

}  // namespace sgk

extern "C" int sgk_zrec_tail_check(const uint8_t *inflated, const uint64_t *rec_offsets, const uint32_t *rec_lengths,
                                   const uint32_t *tail_offsets, uint32_t n, const sgk_aux_field_t *fields,
                                   uint32_t n_fields, uint32_t *status, void *stream) {
    return sgk::zrec_tail_check(inflated, rec_offsets, rec_lengths, tail_offsets, nullptr, n, fields, n_fields, status,
                                static_cast<hipStream_t>(stream));
}
