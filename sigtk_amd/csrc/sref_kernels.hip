// sref_kernels.hip -- `sref`: the synthetic reference signal of a sequence (sgk_sref_*), as floats and as the TSV rows
// of the reference's `sigtk sref` written on the device (src/sref.c:100-210, src/ref.h).
//
// Position j of a strand's row is level[rank(strand bases j .. j + k))], rank with the first base most significant and
// A/a 0, C/c 1, G/g 2, T/t 3, any other byte 0.  The '-' strand is the reverse complement, where the complement of any
// non-ACGT byte is T: base i of the '-' strand is forward base l - 1 - i with code 3 - code.  No reverse-complement
// string is ever made: strand_code() reads the forward bytes through that index map.
//
// The pore model is an argument (4^k floats by k-mer rank); the library carries none.
//
// A chromosome's row is gigabytes, so the unit of work is a span: positions [first, first + count) of one strand of
// one sequence.  Its text is the row head (name \t l \t strand \t ref_len \t) if first == 0, then every value followed
// by ',' -- the last value of the row, position ref_len - 1, by '\n' instead.  A row with ref_len <= 0 is one head-only
// span: the reference prints its head with the negative length and no line end, and so does this.
//
// Text: the tile list, the scan and the staged 16-byte stores are text_tiles.h, shared with text_kernels.hip; a span is
// a row of the tile list, a signal position an item.  What is new is the per-call text table: every value comes from a
// table of at most 4 096 floats, so k_sref_table formats each level once (text_format.h's %f) into a 16-byte entry,
// characters in bytes 0..14 and their count in byte 15.  The measure pass sums counts, the write pass copies at most 15
// bytes per item.  A level whose text is longer than 15 characters (a user's model may hold any float) is marked
// SREF_LONG and takes the general formatter in both passes.  The table stays in global memory and is read through L2,
// or every workgroup keeps a copy in LDS (sgk_sref_batch_t.table_in_lds; profiles/sref.md compares the two).
#include "sgk_common.h"
#include "text_format.h"
#include "text_tiles.h"

namespace sgk {

constexpr uint32_t SREF_STAGE = 8192;       // bytes of a tile's LDS image: 256 values of up to 15 + 1 bytes and a head
constexpr uint32_t SREF_LEVELS_MAX = 4096;  // 4^6
constexpr uint32_t SREF_LONG = 255;         // byte 15 of a table entry whose text does not fit 15 characters
constexpr uint32_t SREF_TABLE_BYTES = SREF_LEVELS_MAX * 16;

struct SrefArgs : TileList {  // (n_rows = the batch's spans)
    const uint8_t *bases;
    uint64_t n_bases;
    const sgk_sref_span_t *spans;
    const float *levels;
    uint32_t k, n_levels;
    const uint8_t *name_bytes;
    const uint32_t *name_offs;
    uint4 *table;           // n_levels entries
    uint64_t *row_offsets;  // n_spans + 1 (measure)
    uint8_t *text;          // (write)
    uint64_t text_cap;
};

__device__ inline uint32_t base_code(uint8_t c) {
    c &= 0xdfu;  // a..z -> A..Z; no other byte lands on a letter
    return c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 0u;
}
// code of base i of the span's strand; a base in front of the span's window or outside `bases` reads as code 0, never
// out of bounds (behind a window that is too small it is whatever the caller put there)
__device__ inline uint32_t strand_code(const SrefArgs &a, const sgk_sref_span_t &sp, uint64_t i) {
    const uint64_t f = sp.strand ? (uint64_t)sp.seq_len - 1u - i : i;
    const uint64_t off = f - sp.base_pos0;
    const bool inside = f >= sp.base_pos0 && sp.base_offset < a.n_bases && off < a.n_bases - sp.base_offset;
    const uint32_t c = inside ? base_code(a.bases[sp.base_offset + off]) : 0u;
    return sp.strand ? 3u - c : c;
}

// ---- floats: 1024 positions per workgroup and step, four consecutive ones per lane with a rolling rank
__global__ __launch_bounds__(256) void k_sref_levels(SrefArgs a, const uint64_t *out_offsets, float *out) {
    const uint32_t mask = a.n_levels - 1u;
    for (uint32_t s = blockIdx.y; s < a.n_rows; s += gridDim.y) {
        const sgk_sref_span_t sp = a.spans[s];
        const uint32_t chunks = sp.count / 1024u + (sp.count % 1024u ? 1u : 0u);
        float *dst = out + out_offsets[s];
        const bool aligned = (reinterpret_cast<uintptr_t>(dst) & 15u) == 0;
        for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
            const uint32_t q0 = c * 1024u + threadIdx.x * 4u;
            if (q0 >= sp.count) continue;
            const uint32_t nq = sp.count - q0 < 4u ? sp.count - q0 : 4u;
            const uint64_t p = (uint64_t)sp.first + q0;
            uint32_t r = 0;
            for (uint32_t m = 0; m + 1 < a.k; ++m) r = (r << 2) | strand_code(a, sp, p + m);
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                if (q < nq) {
                    r = ((r << 2) | strand_code(a, sp, p + a.k - 1u + q)) & mask;
                    v[q] = a.levels[r];
                }
            }
            if (aligned && nq == 4u) {
                *reinterpret_cast<float4 *>(dst + q0) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q)
                    if (q < nq) dst[q0 + q] = v[q];
            }
        }
    }
}

// ---- the text of every level, once per call
__global__ __launch_bounds__(256) void k_sref_table(SrefArgs a) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.n_levels) return;
    const float v = a.levels[r];
    const int n = sgk_tf_f32_len(v);
    uint4 e = make_uint4(0u, 0u, 0u, 0u);
    a.table[r] = e;
    char *p = reinterpret_cast<char *>(a.table + r);
    if (n <= 15) sgk_tf_f32(p, v);
    p[15] = (char)(n <= 15 ? n : (int)SREF_LONG);
}

__global__ __launch_bounds__(1024) void k_sref_tiles(SrefArgs a) {
    text_tiles_body(a, [&](uint32_t s) { return a.spans[s].count; });
}
__global__ __launch_bounds__(1024) void k_sref_scan(SrefArgs a) { text_scan_body(a, a.row_offsets); }

// ---- one tile
struct SrefTile {
    sgk_sref_span_t sp;
    uint32_t j0;      // the tile's first item of the span
    uint32_t nt;      // its items
    int64_t ref_len;  // l + 1 - k, as printed
    bool head;        // the row head belongs to this tile
    uint32_t namel;
    const uint8_t *name;
};

__device__ inline SrefTile sref_tile(const SrefArgs &a, uint32_t t) {
    const uint32_t s = text_tile_row(a, t);
    SrefTile c;
    c.sp = a.spans[s];
    c.j0 = (t - a.tile_first[s]) * TEXT_TILE;
    c.nt = c.sp.count - c.j0 < (uint32_t)TEXT_TILE ? c.sp.count - c.j0 : (uint32_t)TEXT_TILE;
    c.ref_len = (int64_t)c.sp.seq_len + 1 - (int64_t)a.k;
    c.head = c.j0 == 0 && c.sp.first == 0;
    c.namel = a.name_offs[c.sp.seq + 1] - a.name_offs[c.sp.seq];
    c.name = a.name_bytes + a.name_offs[c.sp.seq];
    return c;
}

// the 2-bit codes of the tile's nt + k - 1 strand bases into LDS (codes: TEXT_TILE + 8 bytes), then each lane's rank
__device__ inline uint32_t sref_rank(const SrefArgs &a, const SrefTile &c, uint8_t *codes) {
    const uint64_t p0 = (uint64_t)c.sp.first + c.j0;
    const uint32_t need = c.nt ? c.nt + a.k - 1u : 0u;
    if (threadIdx.x < need) codes[threadIdx.x] = (uint8_t)strand_code(a, c.sp, p0 + threadIdx.x);
    if (threadIdx.x + TEXT_TILE < need) codes[threadIdx.x + TEXT_TILE] = (uint8_t)strand_code(a, c.sp, p0 + threadIdx.x + TEXT_TILE);
    __syncthreads();
    uint32_t r = 0;
    if (threadIdx.x < c.nt)
        for (uint32_t m = 0; m < a.k; ++m) r = (r << 2) | codes[threadIdx.x + m];
    return r;
}

__device__ inline uint32_t sref_head_len(const SrefTile &c) {
    return c.head ? c.namel + 5u + (uint32_t)(sgk_tf_u32_len(c.sp.seq_len) + sgk_tf_i64_len(c.ref_len)) : 0u;
}
// written by the whole workgroup (the name) and its thread 0 (the rest)
__device__ inline void sref_head_emit(const SrefTile &c, char *p) {
    if (!c.head) return;
    for (uint32_t k = threadIdx.x; k < c.namel; k += TEXT_TILE) p[k] = (char)c.name[k];
    if (threadIdx.x != 0) return;
    p += c.namel;
    *p++ = '\t';
    p += sgk_tf_u64(p, c.sp.seq_len);
    *p++ = '\t';
    *p++ = c.sp.strand ? '-' : '+';
    *p++ = '\t';
    p += sgk_tf_i64(p, c.ref_len);
    *p = '\t';
}

// bytes of the lane's item: the table's count, or the general formatter's for a level marked SREF_LONG; + separator
__device__ inline uint32_t sref_item_len(const SrefArgs &a, uint32_t entry_len, uint32_t rank) {
    return (entry_len == SREF_LONG ? (uint32_t)sgk_tf_f32_len(a.levels[rank]) : entry_len) + 1u;
}
__device__ inline void sref_item_emit(const SrefArgs &a, const SrefTile &c, const uint4 &e, uint32_t rank, uint32_t len, char *p) {
    const uint32_t n = e.w >> 24;
    if (n == SREF_LONG) {
        sgk_tf_f32(p, a.levels[rank]);
    } else {
        const uint32_t w[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
        for (uint32_t k = 0; k < 15; ++k)
            if (k < n) p[k] = (char)(w[k >> 2] >> (8u * (k & 3u)));
    }
    p[len - 1u] = (int64_t)((uint64_t)c.sp.first + c.j0 + threadIdx.x) == c.ref_len - 1 ? '\n' : ',';
}

template <bool LDS_TABLE>
__device__ inline void sref_table_load(const SrefArgs &a, uint4 *tbl) {
    if (!LDS_TABLE) return;
    for (uint32_t r = threadIdx.x; r < a.n_levels; r += TEXT_TILE) tbl[r] = a.table[r];
    __syncthreads();
}

template <bool LDS_TABLE>
__global__ __launch_bounds__(TEXT_TILE) void k_sref_measure(SrefArgs a) {
    __shared__ uint32_t wave_tot[TEXT_TILE / 64];
    __shared__ uint8_t codes[TEXT_TILE + 8];
    __shared__ uint4 tbl[LDS_TABLE ? SREF_LEVELS_MAX : 1];
    sref_table_load<LDS_TABLE>(a, tbl);
    const uint32_t n_tiles = a.hdr->n_tiles;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const SrefTile c = sref_tile(a, t);
        const uint32_t rank = sref_rank(a, c, codes);
        uint32_t my_len = 0, my_off;
        if (threadIdx.x < c.nt) {
            const uint32_t n = LDS_TABLE ? tbl[rank].w >> 24 : (uint32_t) reinterpret_cast<const uint8_t *>(a.table)[16u * rank + 15u];
            my_len = sref_item_len(a, n, rank);
        }
        const uint32_t total = text_lane_offsets(my_len, sref_head_len(c), wave_tot, my_off);
        if (threadIdx.x == 0) a.tile_bytes[t] = total;
        __syncthreads();  // wave_tot and codes are reused by the next tile
    }
}

template <bool LDS_TABLE>
__global__ __launch_bounds__(TEXT_TILE) void k_sref_write(SrefArgs a) {
    __shared__ uint32_t wave_tot[TEXT_TILE / 64];
    __shared__ uint8_t codes[TEXT_TILE + 8];
    __shared__ __attribute__((aligned(16))) char stage[SREF_STAGE + 16];
    __shared__ uint4 tbl[LDS_TABLE ? SREF_LEVELS_MAX : 1];
    sref_table_load<LDS_TABLE>(a, tbl);
    const uint32_t n_tiles = a.hdr->n_tiles;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const SrefTile c = sref_tile(a, t);
        const uint32_t rank = sref_rank(a, c, codes);
        uint32_t my_len = 0, my_off;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        if (threadIdx.x < c.nt) {
            e = LDS_TABLE ? tbl[rank] : a.table[rank];
            my_len = sref_item_len(a, e.w >> 24, rank);
        }
        const uint32_t total = text_lane_offsets(my_len, sref_head_len(c), wave_tot, my_off);
        const uint64_t b0 = a.tile_off[t];
        if (b0 + total > a.text_cap) {  // (workgroup-uniform) nothing of this tile is written
            if (threadIdx.x == 0) atomicOr(&a.hdr->flags, TEXT_FLAG_OVERFLOW);
        } else if (total <= SREF_STAGE) {
            uint8_t *dst = a.text + b0;
            char *img = stage + text_image_align(dst);
            sref_head_emit(c, img);
            if (my_len) sref_item_emit(a, c, e, rank, my_len, img + my_off);
            __syncthreads();
            text_image_flush(dst, img, total);
        } else {  // long names or long numbers: every lane writes its own bytes straight to global memory
            char *dst = reinterpret_cast<char *>(a.text + b0);
            sref_head_emit(c, dst);
            if (my_len) sref_item_emit(a, c, e, rank, my_len, dst + my_off);
        }
        __syncthreads();  // the image, codes and wave_tot are reused by the next tile
    }
}

static int sref_batch_check(const sgk_sref_batch_t *b) {
    if (!b) return SGK_ERR_ARG;
    if (b->k < 1 || b->k > 6) return SGK_ERR_ARG;
    if (!b->levels) return SGK_ERR_ARG;
    if (b->n_spans && !b->spans) return SGK_ERR_ARG;
    if (b->n_bases && !b->bases) return SGK_ERR_ARG;
    return SGK_OK;
}

static void sref_fill(const sgk_sref_batch_t *b, SrefArgs *a) {
    a->bases = b->bases;
    a->n_bases = b->n_bases;
    a->spans = b->spans;
    a->levels = b->levels;
    a->k = b->k;
    a->n_levels = 1u << (2u * b->k);
    a->name_bytes = nullptr;
    a->name_offs = nullptr;
    a->table = nullptr;
    a->row_offsets = nullptr;
    a->text = nullptr;
    a->text_cap = 0;
}

// workspace: TextHdr and tile list first (sgk_text_status reads the header), the text table in its last 64 KiB
static int sref_args(const sgk_sref_batch_t *b, const sgk_text_ids_t *names, void *ws, size_t ws_bytes, SrefArgs *a) {
    int rc = sref_batch_check(b);
    if (rc != SGK_OK) return rc;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    if (b->n_spans && (!names || !names->bytes || !names->offsets)) return SGK_ERR_ARG;
    SGK_TRY(text_ws_check(ws, ws_bytes, sizeof(TextHdr) + SREF_TABLE_BYTES + 16));
    const size_t list_bytes = (ws_bytes - SREF_TABLE_BYTES) & ~(size_t)15;
    sref_fill(b, a);
    if (!tile_list_carve(ws, list_bytes, b->n_spans, a)) return SGK_ERR_WORKSPACE;
    a->table = reinterpret_cast<uint4 *>(static_cast<char *>(ws) + list_bytes);
    a->name_bytes = names ? names->bytes : nullptr;
    a->name_offs = names ? names->offsets : nullptr;
    return SGK_OK;
}

}  // namespace sgk

using namespace sgk;

extern "C" {

int sgk_sref_levels(const sgk_sref_batch_t *b, const uint64_t *out_offsets, float *out, void *stream) {
    const int rc = sref_batch_check(b);
    if (rc != SGK_OK) return rc;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    if (b->n_spans == 0) return SGK_OK;
    if (!out_offsets || !out) return SGK_ERR_ARG;
    SrefArgs a;
    sref_fill(b, &a);
    a.n_rows = b->n_spans;
    // few long spans or many short ones: workgroups stride over the spans in y and over a span's chunks in x
    const uint32_t gy = b->n_spans < 64u ? b->n_spans : 64u;
    SGK_LAUNCH("k_sref_levels", k_sref_levels, dim3(1024u / gy, gy), 256, static_cast<hipStream_t>(stream), a, out_offsets, out);
    return SGK_OK;
}

size_t sgk_sref_text_workspace_bytes(uint32_t n_spans, uint64_t n_positions_capacity) {
    return round_up(tile_list_bytes(n_spans, n_positions_capacity) + 64, 16) + SREF_TABLE_BYTES + 16;
}

int sgk_sref_text_measure(const sgk_sref_batch_t *b, const sgk_text_ids_t *names, uint64_t *row_offsets, void *ws,
                          size_t ws_bytes, void *stream) {
    SrefArgs a;
    const int rc = sref_args(b, names, ws, ws_bytes, &a);
    if (rc != SGK_OK) return rc;
    if (!row_offsets) return SGK_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.row_offsets = row_offsets;
    const uint32_t grid = text_grid(a);
    SGK_LAUNCH("k_sref_table", k_sref_table, (a.n_levels + 255u) / 256u, 256, st, a);
    SGK_LAUNCH("k_sref_tiles", k_sref_tiles, 1, 1024, st, a);
    if (b->table_in_lds) SGK_LAUNCH("k_sref_measure_lds", k_sref_measure<true>, grid < 512u ? grid : 512u, TEXT_TILE, st, a);
    else SGK_LAUNCH("k_sref_measure", k_sref_measure<false>, grid, TEXT_TILE, st, a);
    SGK_LAUNCH("k_sref_scan", k_sref_scan, 1, 1024, st, a);
    return SGK_OK;
}

int sgk_sref_text_write(const sgk_sref_batch_t *b, const sgk_text_ids_t *names, uint8_t *text, uint64_t text_capacity,
                        void *ws, size_t ws_bytes, void *stream) {
    SrefArgs a;
    const int rc = sref_args(b, names, ws, ws_bytes, &a);
    if (rc != SGK_OK) return rc;
    if (!text && text_capacity) return SGK_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.text = text;
    a.text_cap = text_capacity;
    const uint32_t grid = text_grid(a);
    // (a workgroup with the table in LDS pays 64 KiB of loads before its first tile: two per CU, striding)
    if (b->table_in_lds) SGK_LAUNCH("k_sref_write_lds", k_sref_write<true>, grid < 512u ? grid : 512u, TEXT_TILE, st, a);
    else SGK_LAUNCH("k_sref_write", k_sref_write<false>, grid, TEXT_TILE, st, a);
    return SGK_OK;
}

}  // extern "C"
