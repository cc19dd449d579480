#!/usr/bin/env python3
"""Writes tests/golden/svb_cases.json: what slow5lib itself makes of the svb-zd catalogue (tests/svb_cases.py).  Needs the
compiled reference (oracle/_ref/libsigtk_ref.so, built by oracle.build(ref=True)); the tests read the file and need none.

Through ctypes it calls slow5_ptr_depress_solo on every blob of decode_cases() and malformed_cases() that holds all the
data its keys promise (well-formed, or with bytes left over) and slow5_ptr_compress_solo on the samples of every one of
encode_cases(), both with SLOW5_COMPRESS_SVB_ZD.  Every input is followed by 64 bytes of padding: streamvbyte's SSSE3
decoder reads ahead.  Per case name the file holds [byte length, SHA-256] of slow5lib's output, "refused" where it
returned NULL, or "documented" for a blob that is too short for its keys or data (slow5lib would read past it: its status
follows include/sigtk_gpu.h alone).  slow5lib is not told the count a caller expects: a blob whose only defect is a
count word other than the expected one decodes here, by its own count.  The file holds recorded results only.

    python tests/golden/make_golden_svb.py
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import svb_cases  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "libsigtk_ref.so")
SVB_ZD = 2   # enum slow5_press_method: SLOW5_COMPRESS_SVB_ZD
PAD = 64


def holds_its_data(blob) -> bool:
    """all key bytes and all the data bytes they promise are there (more may follow)"""
    if len(blob) < 4:
        return False
    count = int.from_bytes(blob[0:4], "little")
    nkeys = (count + 3) // 4
    if len(blob) < 4 + nkeys:
        return False
    return 4 + nkeys + int((svb_cases.key_codes(blob) + 1).sum()) <= len(blob)


def main():
    if not os.path.exists(REF):
        sys.exit("%s is missing: build it with oracle.build(ref=True)" % REF)
    lib = ctypes.CDLL(REF)
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [ctypes.c_void_p]
    for fn in (lib.slow5_ptr_depress_solo, lib.slow5_ptr_compress_solo):
        fn.restype = ctypes.c_void_p
        fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]

    def call(fn, data: bytes):
        buf = ctypes.create_string_buffer(data + b"\0" * PAD, len(data) + PAD)
        n = ctypes.c_size_t(0)
        devnull, saved = os.open(os.devnull, os.O_WRONLY), os.dup(2)   # slow5lib reports a refusal on stderr
        os.dup2(devnull, 2)
        try:
            p = fn(SVB_ZD, buf, len(data), ctypes.byref(n))
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            os.close(devnull)
        if not p:
            return "refused"
        out = ctypes.string_at(p, n.value)
        libc.free(p)
        return [len(out), hashlib.sha256(out).hexdigest()]

    decode, encode = {}, {}
    for c in svb_cases.decode_cases() + svb_cases.malformed_cases():
        decode[c.name] = call(lib.slow5_ptr_depress_solo, c.blob) if holds_its_data(c.blob) else "documented"
    for c in svb_cases.encode_cases():
        encode[c.name] = call(lib.slow5_ptr_compress_solo, np.ascontiguousarray(c.samples, dtype="<i2").tobytes())
    path = os.path.join(HERE, "svb_cases.json")
    with open(path, "w") as fh:
        fh.write('{\n')
        for k, (section, table) in enumerate((("decode", decode), ("encode", encode))):
            fh.write(' "%s": {\n' % section)
            fh.write(",\n".join('  %s: %s' % (json.dumps(name), json.dumps(v, separators=(",", ":"))) for name, v in table.items()))
            fh.write('\n }%s\n' % ("," if k == 0 else ""))
        fh.write('}\n')
    print("%s: %d decode and %d encode cases, %d bytes; refused: %d, documented: %d"
          % (path, len(decode), len(encode), os.path.getsize(path), sum(v == "refused" for v in decode.values()),
             sum(v == "documented" for v in decode.values())))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
