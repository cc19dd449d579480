"""Writes tests/golden/zstd_frames.npz and tests/golden/sp1_dna.zstd_svb.blow5 (run on a machine with libzstd.so.1; the
tests read the files and need no libzstd).

zstd_frames.npz: frames libzstd wrote -- ZSTD_compress at levels -5, 1, 3 and 19, one frame with the content checksum
(ZSTD_c_checksumFlag = 201) and one without a content size (ZSTD_c_contentSizeFlag = 200 set to 0), which the decoders
must refuse -- and for each the recipe of its payload (tests/zstd_craft.py: payload(gen, seed, n)) with the payload's
length and CRC-32.  The large incompressible payloads are kept at one level: they are Raw blocks at every level.

sp1_dna.zstd_svb.blow5: the records of sp1_dna.blow5 with an svb-zd signal, each one ZSTD_compress level 1 frame, as
slow5lib writes a zstd BLOW5 (slow5lib/src/slow5_press.c:1156-1175): header byte 9 = 2, signal byte 1."""
import ctypes
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import zstd_craft  # noqa: E402

Z = ctypes.CDLL("libzstd.so.1")
Z.ZSTD_compressBound.restype = ctypes.c_size_t
Z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
Z.ZSTD_compress.restype = ctypes.c_size_t
Z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
Z.ZSTD_createCCtx.restype = ctypes.c_void_p
Z.ZSTD_CCtx_setParameter.restype = ctypes.c_size_t
Z.ZSTD_CCtx_setParameter.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
Z.ZSTD_compress2.restype = ctypes.c_size_t
Z.ZSTD_compress2.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
Z.ZSTD_freeCCtx.argtypes = [ctypes.c_void_p]
Z.ZSTD_isError.argtypes = [ctypes.c_size_t]


def compress(data, level):
    cap = Z.ZSTD_compressBound(len(data))
    out = ctypes.create_string_buffer(cap)
    n = Z.ZSTD_compress(out, cap, data, len(data), level)
    assert not Z.ZSTD_isError(n)
    return out.raw[:n]


def compress2(data, level, param, value):
    ctx = Z.ZSTD_createCCtx()
    assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(ctx, 100, level))
    assert not Z.ZSTD_isError(Z.ZSTD_CCtx_setParameter(ctx, param, value))
    cap = Z.ZSTD_compressBound(len(data))
    out = ctypes.create_string_buffer(cap)
    n = Z.ZSTD_compress2(ctx, out, cap, data, len(data))
    assert not Z.ZSTD_isError(n)
    Z.ZSTD_freeCCtx(ctx)
    return out.raw[:n]


ALL = (-5, 1, 3, 19)
RECIPES = [("zeros", 0, 0, ALL), ("text", 0, 1, ALL), ("text", 0, 5, ALL), ("zeros", 0, 70000, ALL), ("text", 0, 200000, ALL),
           ("prose", 1, 290000, (1,)), ("prose", 2, 30000, ALL), ("prose", 9, 120, ALL), ("prose", 9, 200, ALL), ("prose", 9, 255, ALL), ("runs", 3, 150000, ALL), ("random", 4, 140000, (1,)),
           ("svb", 5, 100000, (1,)), ("svb", 6, 20000, (-5, 19))]
for n in (31, 32, 1023, 1024, 4095, 4096, 16383, 16384, 131071, 131072, 131073):
    RECIPES.append(("text", 0, n, ALL))
    if n < 20000:
        RECIPES.append(("prose", 7, n, ALL))
    RECIPES.append(("random", 8, n, ALL if n < 5000 else (1,)))


def main():
    frames, meta = [], []
    for gen, seed, n, levels in RECIPES:
        data = zstd_craft.payload(gen, seed, n)
        for level in levels:
            frames.append(compress(data, level))
            meta.append((gen, seed, n, level, "", len(data), zlib.crc32(data)))
    for gen, seed, n, level, param, flag in (("prose", 2, 70000, 3, 201, "checksum"), ("text", 0, 4096, 1, 201, "checksum"),
                                             ("svb", 6, 5000, 1, 201, "checksum")):
        data = zstd_craft.payload(gen, seed, n)
        frames.append(compress2(data, level, param, 1))
        meta.append((gen, seed, n, level, flag, len(data), zlib.crc32(data)))
    data = zstd_craft.payload("text", 0, 4096)
    frames.append(compress2(data, 1, 200, 0))
    meta.append(("text", 0, 4096, 1, "nosize", len(data), zlib.crc32(data)))
    offs = np.concatenate(([0], np.cumsum([len(f) for f in frames]))).astype(np.int64)
    path = os.path.join(HERE, "zstd_frames.npz")
    np.savez(path, frames=np.frombuffer(b"".join(frames), dtype=np.uint8), frame_offsets=offs,
             gen=np.array([m[0] for m in meta]), seed=np.array([m[1] for m in meta], dtype=np.int64),
             n=np.array([m[2] for m in meta], dtype=np.int64), level=np.array([m[3] for m in meta], dtype=np.int64),
             flags=np.array([m[4] for m in meta]), length=np.array([m[5] for m in meta], dtype=np.int64),
             crc32=np.array([m[6] for m in meta], dtype=np.int64))
    print("%s: %d frames, %d bytes" % (path, len(frames), os.path.getsize(path)))
    assert os.path.getsize(path) < (1 << 20)
    src, dst = os.path.join(HERE, "sp1_dna.blow5"), os.path.join(HERE, "sp1_dna.zstd_svb.blow5")
    zstd_craft.recode_blow5(src, dst, 2, lambda rec: compress(rec, 1))
    print("%s: %d bytes (sp1_dna.blow5: %d)" % (dst, os.path.getsize(dst), os.path.getsize(src)))
    assert os.path.getsize(dst) <= os.path.getsize(src)


if __name__ == "__main__":
    main()
