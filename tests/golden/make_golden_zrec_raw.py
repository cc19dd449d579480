"""Writes tests/golden/sp1_24.zstd_raw.blow5 and tests/golden/zrec_raw.json (run on a machine with libzstd.so.1; the tests
read the files and need no libzstd).

sp1_24.zstd_raw.blow5: the first 24 records of sp1_dna.blow5 with their signal NOT compressed -- header byte 14
(signal_press) 0, len_raw_signal the sample count, the samples plain little-endian int16, the six auxiliary columns kept
as they are -- each record one ZSTD_compress level 1 frame, header byte 9 (record_press) 2: what slow5lib writes with
`-c zstd -s none` (slow5lib/src/slow5.c:2918-2935, slow5_press.c:1156-1175).  156 876 bytes (24 records, 118 402 samples).

zrec_raw.json: the file's sha256, its record and sample counts, and the length and CRC-32 of every decompressed record."""
import ctypes
import hashlib
import json
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from sigtk_amd import blow5  # noqa: E402

N_RECORDS = 24

Z = ctypes.CDLL("libzstd.so.1")
Z.ZSTD_compressBound.restype = ctypes.c_size_t
Z.ZSTD_compressBound.argtypes = [ctypes.c_size_t]
Z.ZSTD_compress.restype = ctypes.c_size_t
Z.ZSTD_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
Z.ZSTD_isError.argtypes = [ctypes.c_size_t]


def compress(data, level):
    cap = Z.ZSTD_compressBound(len(data))
    out = ctypes.create_string_buffer(cap)
    n = Z.ZSTD_compress(out, cap, data, len(data), level)
    assert not Z.ZSTD_isError(n)
    return out.raw[:n]


def plain_signal_record(rec):
    """an inflated record with an svb-zd signal -> the same record with plain samples"""
    (idl,) = struct.unpack_from("<H", rec, 0)
    p = 2 + idl + 36
    (ln,) = struct.unpack_from("<Q", rec, p)
    raw = blow5.svb_zd_decode(rec[p + 8:p + 8 + ln])
    return rec[:p] + struct.pack("<Q", raw.size) + raw.astype("<i2").tobytes() + rec[p + 8 + ln:], raw.size


def main():
    src, dst = os.path.join(HERE, "sp1_dna.blow5"), os.path.join(HERE, "sp1_24.zstd_raw.blow5")
    buf = open(src, "rb").read()
    assert tuple(buf[6:9]) >= (0, 2, 0) and buf[9] == 1 and buf[14] == 1
    (hsize,) = struct.unpack_from("<I", buf, 64)
    head = bytearray(buf[:68 + hsize])
    head[9], head[14] = 2, 0
    out, meta, n_samples = [bytes(head)], [], 0
    for rec in blow5.raw_records(src)[:N_RECORDS]:
        plain, n = plain_signal_record(rec)
        n_samples += n
        frame = compress(plain, 1)
        out.append(struct.pack("<Q", len(frame)) + frame)
        meta.append({"length": len(plain), "crc32": zlib.crc32(plain)})
    out.append(blow5.EOF_MARK)
    data = b"".join(out)
    assert len(data) < (1 << 20)
    open(dst, "wb").write(data)
    with open(os.path.join(HERE, "zrec_raw.json"), "w") as fh:
        json.dump({"file": os.path.basename(dst), "sha256": hashlib.sha256(data).hexdigest(), "n_records": len(meta),
                   "n_samples": n_samples, "records": meta}, fh, indent=1)
        fh.write("\n")
    print("%s: %d records, %d samples, %d bytes" % (dst, len(meta), n_samples, len(data)))


if __name__ == "__main__":
    main()
