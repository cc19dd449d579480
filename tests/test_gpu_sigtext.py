"""GPU: the raw_signal column of text SLOW5 records parsed on the device (k_sigtext_decode) against numpy's
",".join(map(str, raw)) and a regex model of the accepted grammar.  Integer work: samples are bit-equal.

Every launch here writes into a sample arena with 4 KB of canary in front of, between and behind the reads; the canaries
must be intact afterwards, whatever the text held."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A          # int16 pattern of the guard zones
GUARD = 2048             # samples (4 KB)
TOKEN = re.compile(rb"0|-?[1-9][0-9]{0,4}")


def model_status(text: bytes, count: int) -> int:
    """the grammar of sgk_sigtext_decode / b5_sigtext_decode: 2 malformed token, 1 token count, 0 ok"""
    if text == b"":
        return 0 if count == 0 else 1
    toks = text.split(b",")
    for t in toks:
        if not TOKEN.fullmatch(t) or not -32768 <= int(t) <= 32767:
            return 2
    return 0 if len(toks) == count else 1


def join(raw) -> bytes:
    return ",".join(map(str, np.asarray(raw).tolist())).encode()


def run(gpu, texts, counts, residues=None):
    """one launch -> (per-read sample arrays, status array); asserts the canaries"""
    import torch
    dev = torch.device("cuda", 0)
    L = gpu.load_library()
    n = len(texts)
    counts = np.asarray(counts, dtype=np.int64)
    tlens = np.array([len(t) for t in texts], dtype=np.uint32)
    toffs = np.zeros(n, dtype=np.int64)
    pos = 16
    for i in range(n):
        pos = (pos + 15) // 16 * 16 + (int(residues[i]) if residues is not None else 0)
        toffs[i] = pos
        pos += int(tlens[i])
    host = np.full((pos + 15) // 16 * 16 + 16, ord("7"), dtype=np.uint8)   # digits around every column: nothing may leak in
    for i, t in enumerate(texts):
        host[int(toffs[i]):int(toffs[i]) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    offs = np.zeros(n, dtype=np.int64)
    o = GUARD
    for i in range(n):
        offs[i] = o
        o += (int(counts[i]) + 63) // 64 * 64 + GUARD
    arena = np.full(o, CANARY, dtype=np.int16)
    guard = np.ones(o, dtype=bool)
    for i in range(n):
        guard[int(offs[i]):int(offs[i]) + int(counts[i])] = False
    d_text = torch.from_numpy(host).to(dev)
    d_toffs = torch.from_numpy(toffs).to(dev)
    d_tlens = torch.from_numpy(tlens.astype(np.int32)).to(dev)
    d_samples = torch.from_numpy(arena).to(dev)
    d_offs = torch.from_numpy(offs).to(dev)
    d_lens = torch.from_numpy(counts.astype(np.int32)).to(dev)
    status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    assert d_text.data_ptr() % 16 == 0
    gpu.check(L.sgk_sigtext_decode(d_text.data_ptr(), d_toffs.data_ptr(), d_tlens.data_ptr(), n, d_samples.data_ptr(),
                                   d_offs.data_ptr(), d_lens.data_ptr(), status.data_ptr(),
                                   int(torch.cuda.current_stream().cuda_stream)), "sgk_sigtext_decode")
    torch.cuda.synchronize()
    got = d_samples.cpu().numpy()
    assert (got[guard] == CANARY).all(), "a store outside a read's sample range"
    return [got[int(offs[i]):int(offs[i]) + int(counts[i])] for i in range(n)], status.cpu().numpy()


def exact_bytes(nbytes: int) -> np.ndarray:
    """samples whose text is exactly nbytes long ("12," repeated, then a token of two to four digits)"""
    k = (nbytes - 2) // 3
    last = {2: 12, 3: 123, 4: 1234}[nbytes - 3 * k]
    raw = np.array([12] * k + [last], dtype=np.int16)
    assert len(join(raw)) == nbytes
    return raw


def test_lengths(gpu):
    rs = np.random.RandomState(17)
    reads = [rs.randint(-32768, 32768, size=int(n)).astype(np.int16) for n in rs.randint(0, 5001, size=300)]
    reads += [np.zeros(0, np.int16), np.array([-7], np.int16), np.array([31000, -1], np.int16)]
    reads += [exact_bytes(n) for n in (1023, 1024, 1025, 2048)]
    got, status = run(gpu, [join(r) for r in reads], [r.size for r in reads])
    assert (status == 0).all(), np.nonzero(status)[0]
    for g, r in zip(got, reads):
        assert np.array_equal(g, r)


def test_token_widths(gpu):
    rs = np.random.RandomState(18)
    n = 6000
    reads = [np.zeros(n, np.int16),                                   # 2 bytes per sample: the densest text
             np.full(n, -32768, np.int16),                            # 7 bytes per sample: the widest token
             np.where(np.arange(n) % 2 == 0, -32768, 0).astype(np.int16),
             rs.randint(-32768, 32768, size=n).astype(np.int16)]
    got, status = run(gpu, [join(r) for r in reads], [r.size for r in reads])
    assert (status == 0).all()
    for g, r in zip(got, reads):
        assert np.array_equal(g, r)


def test_every_alignment(gpu):
    rs = np.random.RandomState(19)
    reads, residues = [], []
    for res in range(16):
        for n in (1, 3, 700):
            reads.append(rs.randint(-32768, 32768, size=n).astype(np.int16))
            residues.append(res)
    got, status = run(gpu, [join(r) for r in reads], [r.size for r in reads], residues)
    assert (status == 0).all()
    for g, r in zip(got, reads):
        assert np.array_equal(g, r)


BAD_TOKENS = [b"32768", b"-32769", b"01", b"-0", b"-", b"1-2", b"", b"123456", b" 1", b"1 2", b"\x01", b"+5", b"1.0"]


def prefix_of(nbytes: int) -> bytes:
    """good tokens, each followed by its comma, nbytes long in all"""
    if nbytes == 0:
        return b""
    k, rem = divmod(nbytes, 4)
    assert rem == 3
    return b"123," * k + b"12,"


def malformed_cases():
    """(text, count) with one bad token at the first token, at the last one, and lying across the 16-byte and the
    1024-byte boundary of its (16-byte aligned) column"""
    tail = b",".join([b"-45"] * 300)   # ~1 200 bytes behind the token: more than one tile in every case
    cases = []
    for bad in BAD_TOKENS:
        cases.append(bad + b"," + tail)                       # first token
        cases.append(tail + b"," + bad)                       # last token
        for boundary in (16, 1024):
            cases.append(prefix_of(boundary - 1) + bad + b"," + tail)   # starts one byte in front of the boundary
    return [(t, len(t.split(b","))) for t in cases]


def test_malformed_reads_and_shared_batch(gpu):
    rs = np.random.RandomState(20)
    good = [rs.randint(-32768, 32768, size=n).astype(np.int16) for n in (900, 1, 2500)]
    texts, counts, expect_raw = [], [], []
    for i, (t, c) in enumerate(malformed_cases()):
        texts.append(t); counts.append(c); expect_raw.append(None)
        if i % 5 == 0:   # good reads between the bad ones
            g = good[(i // 5) % len(good)]
            texts.append(join(g)); counts.append(g.size); expect_raw.append(g)
    # the announced length lies: one short, one over, zero, and a text with ten times the tokens
    g = good[0]
    for c in (g.size - 1, g.size + 1, 0, g.size // 10):
        texts.append(join(g)); counts.append(c); expect_raw.append(None)
    texts.append(b""); counts.append(0); expect_raw.append(np.zeros(0, np.int16))
    texts.append(b""); counts.append(5); expect_raw.append(None)
    texts.append(b"5,"); counts.append(1); expect_raw.append(None)
    texts.append(b",,"); counts.append(3); expect_raw.append(None)
    texts.append(b"1,-,1-2"); counts.append(3); expect_raw.append(None)   # the reference reads 1,0,1 here: we refuse
    got, status = run(gpu, texts, counts)
    want = np.array([model_status(t, c) for t, c in zip(texts, counts)])
    assert (want == 2).sum() >= len(BAD_TOKENS) * 4 and (want == 1).sum() >= 4 and (want == 0).sum() >= 10
    bad = np.nonzero(status != want)[0]
    assert bad.size == 0, [(int(i), texts[i][:40], int(status[i]), int(want[i])) for i in bad[:8]]
    for g_, e in zip(got, expect_raw):
        if e is not None:
            assert np.array_equal(g_, e)
