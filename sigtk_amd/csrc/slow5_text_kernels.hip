// slow5_text_kernels.hip -- the raw_signal column of text SLOW5 records written on the device (sgk_slow5_text_*): the
// inverse of k_sigtext_decode (sigtext_kernels.hip), for `qts` on .slow5 files.
//
// Row r of the batch is
//
//   head_r | v0,v1,...,v(n-1) | tail_r        n = lengths[r]; every v as "%d" of an int16 (slow5lib/src/slow5.c:3826-3860)
//
// head_r and tail_r are arbitrary bytes of any length, none included: the caller's line up to and including the tab in
// front of the column, and what follows the column (auxiliary columns, the newline).  The kernels add no tab and no
// newline of their own, so that the same grammar writes bare columns (no heads, no tails) and whole lines.
//
// The tile list, the scan and the staged 16-byte stores are text_tiles.h: a read is a row, a sample an item of 1 to 6
// characters and -- all but the read's last -- a comma.  The head belongs to the read's first tile and the tail to its
// last one; both are copied by the whole workgroup.  A tile whose bytes do not fit the LDS image (a head or a tail of
// thousands of bytes) writes them straight to global memory, every lane its own bytes.
//
// Tiles are dealt out in runs: workgroup b takes tiles [b * per, (b + 1) * per).  The row of a tile is a binary search of
// dependent loads over tile_first (text_tile_row); a workgroup pays it once, for its first tile, and then walks
// tile_first forward -- with 20 000 reads and 7.8 million tiles the search was most of both kernels' time
// (profiles/sigtext_encode.md).  A run's bytes are also consecutive in the output.
//
// Integer arithmetic only.  text_capacity is checked on the device (TEXT_FLAG_OVERFLOW, sgk_text_status); so is a tile
// of 4 GiB or more (its byte count lives in 32 bits): it is not written and reports the same flag.
#include "sgk_common.h"
#include "text_format.h"
#include "text_tiles.h"

namespace sgk {

// bytes of a tile's LDS image: 256 samples take at most 256 * 7; the rest is room for the head and the tail
constexpr uint32_t S5T_STAGE = SGK_SLOW5_TEXT_STAGE_BYTES;

struct S5TextArgs : TileList {  // (n_rows = the batch's reads)
    const int16_t *samples;
    const uint64_t *offsets;
    const uint32_t *lengths;
    const uint8_t *head_bytes, *tail_bytes;  // null: every head / tail is empty
    const uint32_t *head_offs, *tail_offs;
    uint64_t *row_offsets;  // n_reads + 1 (measure)
    uint8_t *text;          // (write)
    uint64_t text_cap;
};

__global__ __launch_bounds__(1024) void k_slow5_text_tiles(S5TextArgs a) {
    text_tiles_body(a, [&](uint32_t r) { return a.lengths[r]; });
}
__global__ __launch_bounds__(1024) void k_slow5_text_scan(S5TextArgs a) { text_scan_body(a, a.row_offsets); }

struct S5Tile {
    uint32_t j0, n;         // the tile's first sample of the read; the read's samples
    uint32_t headl, taill;  // bytes of the head / tail this tile carries (0 unless it is the read's first / last tile)
    const uint8_t *head, *tail;
    const int16_t *src;
};

// the workgroup's run of tiles [lo, hi) and the row of tile lo (workgroup-uniform)
__device__ inline bool s5_run(const S5TextArgs &a, uint32_t &lo, uint32_t &hi, uint32_t &r) {
    const uint32_t n_tiles = a.hdr->n_tiles;
    const uint32_t per = (n_tiles + gridDim.x - 1u) / gridDim.x;
    const uint64_t first = (uint64_t)blockIdx.x * per;
    if (first >= n_tiles) return false;
    lo = (uint32_t)first;
    hi = n_tiles - lo < per ? n_tiles : lo + per;
    r = text_tile_row(a, lo);
    return true;
}
// the row of tile t, at or behind row r (every row has a tile and tile_first[n_rows] = n_tiles > t: r stays a row)
__device__ inline uint32_t s5_next_row(const S5TextArgs &a, uint32_t t, uint32_t r) {
    while (t >= a.tile_first[r + 1]) ++r;
    return r;
}

__device__ inline S5Tile s5_tile(const S5TextArgs &a, uint32_t t, uint32_t r) {
    S5Tile c;
    c.j0 = (t - a.tile_first[r]) * TEXT_TILE;
    c.n = a.lengths[r];
    c.src = a.samples + a.offsets[r];
    c.headl = c.taill = 0;
    c.head = c.tail = nullptr;
    if (a.head_bytes && c.j0 == 0) {
        c.head = a.head_bytes + a.head_offs[r];
        c.headl = a.head_offs[r + 1] - a.head_offs[r];
    }
    if (a.tail_bytes && t + 1 == a.tile_first[r + 1]) {
        c.tail = a.tail_bytes + a.tail_offs[r];
        c.taill = a.tail_offs[r + 1] - a.tail_offs[r];
    }
    return c;
}

// the lane's sample and its bytes with the comma (0: no sample for this lane)
__device__ inline uint32_t s5_item(const S5Tile &c, int16_t &v) {
    const uint32_t j = c.j0 + threadIdx.x;
    v = 0;
    if (j >= c.n) return 0u;
    v = c.src[j];
    return (uint32_t)sgk_tf_i16_len(v) + (j + 1 < c.n ? 1u : 0u);
}

// per-lane byte counts -> the lane's offset and the tile's bytes, head and tail included; false: they do not fit 32 bits
__device__ inline bool s5_offsets(const S5Tile &c, uint32_t my_len, uint32_t *wave_tot, uint32_t &my_off, uint32_t &total) {
    const uint32_t items = text_lane_offsets(my_len, 0u, wave_tot, my_off);  // (at most 256 * 7)
    const uint64_t sum = (uint64_t)c.headl + items + c.taill;
    my_off += c.headl;  // (a lane with my_len == 0 never uses it)
    total = sum > 0xffffffffull ? 0xffffffffu : (uint32_t)sum;
    return sum <= 0xffffffffull;
}

__global__ __launch_bounds__(TEXT_TILE) void k_slow5_text_measure(S5TextArgs a) {
    __shared__ uint32_t wave_tot[TEXT_TILE / 64];
    uint32_t lo, hi, r;
    if (!s5_run(a, lo, hi, r)) return;
    for (uint32_t t = lo; t < hi; ++t) {
        r = s5_next_row(a, t, r);
        const S5Tile c = s5_tile(a, t, r);
        int16_t v;
        uint32_t my_off, total;
        const bool fits = s5_offsets(c, s5_item(c, v), wave_tot, my_off, total);
        if (threadIdx.x == 0) {
            a.tile_bytes[t] = total;
            if (!fits) atomicOr(&a.hdr->flags, TEXT_FLAG_OVERFLOW);
        }
        __syncthreads();  // wave_tot is reused by the next tile
    }
}

// head, the lane's sample, tail at p = the tile's first byte (LDS image or global memory)
__device__ inline void s5_emit(const S5Tile &c, int16_t v, uint32_t my_len, uint32_t my_off, uint32_t total, char *p) {
    for (uint32_t k = threadIdx.x; k < c.headl; k += TEXT_TILE) p[k] = (char)c.head[k];
    if (my_len) {
        const int n = sgk_tf_i16(p + my_off, v);
        if ((uint32_t)n < my_len) p[my_off + (uint32_t)n] = ',';
    }
    char *q = p + (total - c.taill);
    for (uint32_t k = threadIdx.x; k < c.taill; k += TEXT_TILE) q[k] = (char)c.tail[k];
}

__global__ __launch_bounds__(TEXT_TILE) void k_slow5_text_write(S5TextArgs a) {
    __shared__ uint32_t wave_tot[TEXT_TILE / 64];
    __shared__ __attribute__((aligned(16))) char stage[S5T_STAGE + 16];
    uint32_t lo, hi, r;
    if (!s5_run(a, lo, hi, r)) return;
    for (uint32_t t = lo; t < hi; ++t) {
        r = s5_next_row(a, t, r);
        const S5Tile c = s5_tile(a, t, r);
        int16_t v;
        uint32_t my_off, total;
        const uint32_t my_len = s5_item(c, v);
        const bool fits = s5_offsets(c, my_len, wave_tot, my_off, total);
        const uint64_t b0 = a.tile_off[t];
        if (!fits || b0 > a.text_cap || total > a.text_cap - b0) {  // (workgroup-uniform) nothing of this tile is written
            if (threadIdx.x == 0) atomicOr(&a.hdr->flags, TEXT_FLAG_OVERFLOW);
        } else if (total <= S5T_STAGE) {
            uint8_t *dst = a.text + b0;
            char *img = stage + text_image_align(dst);  // img + k and dst + k are congruent modulo 16
            s5_emit(c, v, my_len, my_off, total, img);
            __syncthreads();
            text_image_flush(dst, img, total);
        } else {  // a long head or tail: every lane writes its own bytes straight to global memory
            s5_emit(c, v, my_len, my_off, total, reinterpret_cast<char *>(a.text + b0));
        }
        __syncthreads();  // the image and wave_tot are reused by the next tile
    }
}

static int s5_args(const int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                   const sgk_text_ids_t *heads, const sgk_text_ids_t *tails, void *ws, size_t ws_bytes, S5TextArgs *a) {
    if (n_reads && (!samples || !offsets || !lengths)) return SGK_ERR_ARG;
    if (heads && n_reads && (!heads->bytes || !heads->offsets)) return SGK_ERR_ARG;
    if (tails && n_reads && (!tails->bytes || !tails->offsets)) return SGK_ERR_ARG;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    SGK_TRY(text_ws_check(ws, ws_bytes, sizeof(TextHdr)));
    if (!tile_list_carve(ws, ws_bytes, n_reads, a)) return SGK_ERR_WORKSPACE;
    a->samples = samples;
    a->offsets = offsets;
    a->lengths = lengths;
    a->head_bytes = heads ? heads->bytes : nullptr;
    a->head_offs = heads ? heads->offsets : nullptr;
    a->tail_bytes = tails ? tails->bytes : nullptr;
    a->tail_offs = tails ? tails->offsets : nullptr;
    a->row_offsets = nullptr;
    a->text = nullptr;
    a->text_cap = 0;
    return SGK_OK;
}

}  // namespace sgk

using namespace sgk;

extern "C" {

size_t sgk_slow5_text_workspace_bytes(uint32_t n_reads, uint64_t n_samples_capacity) {
    return tile_list_bytes(n_reads, n_samples_capacity) + 64;
}

int sgk_slow5_text_measure(const int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                           const sgk_text_ids_t *heads, const sgk_text_ids_t *tails, uint64_t *row_offsets, void *ws,
                           size_t ws_bytes, void *stream) {
    S5TextArgs a;
    const int rc = s5_args(samples, offsets, lengths, n_reads, heads, tails, ws, ws_bytes, &a);
    if (rc != SGK_OK) return rc;
    if (!row_offsets) return SGK_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    a.row_offsets = row_offsets;
    const uint32_t grid = text_grid(a);
    SGK_LAUNCH("k_slow5_text_tiles", k_slow5_text_tiles, 1, 1024, st, a);
    SGK_LAUNCH("k_slow5_text_measure", k_slow5_text_measure, grid, TEXT_TILE, st, a);
    SGK_LAUNCH("k_slow5_text_scan", k_slow5_text_scan, 1, 1024, st, a);
    return SGK_OK;
}

int sgk_slow5_text_write(const int16_t *samples, const uint64_t *offsets, const uint32_t *lengths, uint32_t n_reads,
                         const sgk_text_ids_t *heads, const sgk_text_ids_t *tails, uint8_t *text, uint64_t text_capacity,
                         void *ws, size_t ws_bytes, void *stream) {
    S5TextArgs a;
    const int rc = s5_args(samples, offsets, lengths, n_reads, heads, tails, ws, ws_bytes, &a);
    if (rc != SGK_OK) return rc;
    if (!text && text_capacity) return SGK_ERR_ARG;
    a.text = text;
    a.text_cap = text_capacity;
    const uint32_t grid = text_grid(a);
    SGK_LAUNCH("k_slow5_text_write", k_slow5_text_write, grid, TEXT_TILE, static_cast<hipStream_t>(stream), a);
    return SGK_OK;
}

}  // extern "C"
