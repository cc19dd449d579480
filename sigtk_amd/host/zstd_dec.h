/* zstd_dec.h -- scalar decoder of one zstd frame (RFC 8878), written from the format: no libzstd.
 *
 * BLOW5 files with record compression byte 2 hold one frame per record, as ZSTD_compress writes it
 * (slow5lib/src/slow5_press.c:1156-1175).  The decoder takes every frame of that shape -- any block type, literals
 * type, sequence mode and header layout -- and refuses, with one of the statuses below and never with a wrong byte or
 * an access outside its buffers, whatever is not one: no content size, a dictionary, a skippable frame, bytes behind
 * the frame.  The GPU kernel (csrc/zstd_kernels.hip, sgk_zstd_decompress) decodes the same set and reports the same
 * statuses. */
#ifndef SGK_ZSTD_DEC_H
#define SGK_ZSTD_DEC_H

#include <stddef.h>
#include <stdint.h>

enum {
    ZSD_OK = 0,
    ZSD_ERR_HEADER = 1,    /* magic, reserved bit, dictionary, skippable frame, no content size, bytes behind the frame */
    ZSD_ERR_BLOCK = 2,     /* reserved block type, block larger than 128 KB */
    ZSD_ERR_TABLE = 3,     /* Huffman weights / FSE distribution that describe no table, Repeat / Treeless without one */
    ZSD_ERR_SECTION = 4,   /* literals or sequences section: sizes, bitstreams, literals missing */
    ZSD_ERR_OFFSET = 5,    /* offset 0 or in front of the frame's first byte */
    ZSD_ERR_TRUNCATED = 6, /* the input ends inside the frame */
    ZSD_ERR_CHECKSUM = 7,  /* content checksum mismatch */
    ZSD_ERR_SIZE = 8,      /* other than the declared content size, or more than the room given */
    ZSD_ERR_MEM = 9,       /* no memory for the decoder's own state (no status of a frame: the kernel has no such case) */
};

/* the frame's declared content size; ZSD_ERR_HEADER when the header is refused, ZSD_ERR_TRUNCATED when it is cut */
int zsd_content_size(const uint8_t *in, size_t in_len, uint64_t *size);
/* the whole frame into out[0 .. cap): *out_len receives the bytes written (the content size on ZSD_OK) */
int zsd_decode(const uint8_t *in, size_t in_len, uint8_t *out, size_t cap, size_t *out_len);
/* the frame's first `want` bytes into out[0 .. want): stops as soon as they exist (ZSD_OK; nothing behind them is
 * looked at, the checksum included) or at the frame's end (*out_len < want then, the whole frame checked).  Of a block's
 * Huffman-coded literals only the first `want` are decoded, so the cost is the block's tables plus `want` symbols, not
 * the block.  Both decoders keep their state (about 150 KB) per thread, allocated at a thread's first call. */
int zsd_decode_head(const uint8_t *in, size_t in_len, uint8_t *out, size_t want, size_t *out_len);
const char *zsd_status_name(int status);

#endif
