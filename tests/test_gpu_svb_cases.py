"""GPU: k_svbzd_decode, k_svbzd_size and k_svbzd_encode on the catalogue of tests/svb_cases.py: blobs and reads off the
aligned paths of the kernels, every code mix, malformed blobs, and sentinels around everything a launch may write.  The
expectation is the plain serial codec of the catalogue (tests/test_svb_cases_cpu.py ties it to slow5lib's recorded
answers); every comparison is of integers and bytes."""
import functools

import numpy as np
import pytest

import svb_cases as S

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A   # the int16 every sample holds before a decode
FILL = 0xA5         # the byte the encoder's output buffer holds before a launch


@functools.lru_cache(maxsize=None)
def _expected_all():
    return {c.name: S.ref_decode(c.blob, c.expected_count)[1] for c in S.decode_cases()}


def _expected(name):
    """ref_decode of every valid case, computed once and left unchanged"""
    return _expected_all()[name]


@functools.lru_cache(maxsize=None)
def _encoded():
    return tuple(S.ref_encode(c.samples) for c in S.encode_cases())


def _decode(cases, blob_leads):
    """one launch -> (samples of every read, status, the arena with every read's own range set back to the sentinel)"""
    import torch
    from sigtk_amd import device
    reads, status = device.svbzd_decode([c.blob for c in cases], [c.expected_count for c in cases], torch.device("cuda", 0),
                                        blob_leads=blob_leads, sample_leads=[c.sample_lead for c in cases], fill=SENTINEL)
    torch.cuda.synchronize()
    arena = reads.samples.cpu().numpy()
    got = []
    for r, c in enumerate(cases):
        o = int(reads.offsets_host[r])
        assert o % 64 == c.sample_lead
        got.append(arena[o:o + c.expected_count].copy())
        arena[o:o + c.expected_count] = SENTINEL
    return got, status[:len(cases)].cpu().numpy(), arena


def _load(cases):
    import torch
    from sigtk_amd import device
    b = device.alloc_reads(np.array([c.samples.size for c in cases], dtype=np.int64), torch.device("cuda", 0),
                           leads=[c.sample_lead for c in cases])
    host = np.full(b.n_samples, 12345, dtype=np.int16)   # the samples around a read are arbitrary data
    for r, c in enumerate(cases):
        o = int(b.offsets_host[r])
        host[o:o + c.samples.size] = c.samples
    b.samples.copy_(torch.from_numpy(host))
    return b


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_valid_blobs_at_every_alignment(gpu, lead):
    """every valid case whose blob lies `lead` bytes behind a dword: status 0, the samples of the plain decoder, and the
    sentinel still in every sample that belongs to no read"""
    cases = [c for c in S.decode_cases() if c.blob_lead % 4 == lead]
    assert len(cases) > 100
    got, status, arena = _decode(cases, [c.blob_lead for c in cases])
    bad = [c.name for c, st in zip(cases, status) if st != 0]
    assert not bad, bad
    bad = [c.name for c, g in zip(cases, got) if not np.array_equal(g, _expected(c.name))]
    assert not bad, bad
    assert (arena.view(np.uint16) == SENTINEL).all(), np.flatnonzero(arena.view(np.uint16) != SENTINEL)[:8]


def test_malformed_blobs_among_valid_ones(gpu):
    """every malformed case between two valid ones in one launch: its documented status, nothing written outside its own
    range, and the valid neighbours exact"""
    valid = [c for c in S.decode_cases() if c.expected_count <= 1040 and not c.name.startswith("enc:")]
    cases = []
    for i, m in enumerate(S.malformed_cases()):
        cases += [valid[(5 * i) % len(valid)], m]
    cases.append(valid[1])
    got, status, arena = _decode(cases, [c.blob_lead for c in cases])
    for c, st, g in zip(cases, status, got):
        assert int(st) in c.status, (c.name, int(st), c.status)
        if c.status == (0,):
            exp = _expected(c.name) if not c.kind else np.zeros(0, dtype=np.int16)
            assert np.array_equal(g, exp), c.name
    assert (arena.view(np.uint16) == SENTINEL).all(), np.flatnonzero(arena.view(np.uint16) != SENTINEL)[:8]


def test_encoder_sizes_bytes_and_gaps(gpu):
    """k_svbzd_size gives the length of the canonical blob, k_svbzd_encode its bytes, and between the blobs the buffer
    still holds what it held"""
    from sigtk_amd import device
    cases = S.encode_cases()
    blobs, gaps, lens = device.svbzd_encode(_load(cases), blob_leads=[c.blob_lead for c in cases], fill=FILL, with_gaps=True)
    exp = _encoded()
    bad = [c.name for c, n, e in zip(cases, lens, exp) if int(n) != len(e)]
    assert not bad, bad
    bad = [c.name for c, b, e in zip(cases, blobs, exp) if b != e]
    assert not bad, bad
    assert len(gaps) == len(cases) + 1 and len(gaps[-1]) >= 16
    names = ["(front)"] + [c.name for c in cases]
    bad = [name for name, g in zip(names, gaps) if g != bytes([FILL]) * len(g)]
    assert not bad, bad


def test_round_trip_off_the_encoders_alignment(gpu):
    """what the device encoded, moved 1, 2 and 3 bytes behind a dword, decodes on the device to the input"""
    from sigtk_amd import device
    cases = S.encode_cases()
    blobs = device.svbzd_encode(_load(cases), blob_leads=[c.blob_lead for c in cases], fill=FILL)
    moved, leads = [], []
    for k in (1, 2, 3):     # every blob 1, 2 and 3 bytes behind a dword, the dword anywhere in its 16 bytes
        moved += [S.DecodeCase("%s@%d" % (c.name, k), b, c.samples.size, 0, c.sample_lead) for c, b in zip(cases, blobs)]
        leads += [4 * ((r + k) % 4) + k for r in range(len(cases))]
    got, status, arena = _decode(moved, leads)
    bad = [m.name for m, c, st, g in zip(moved, 3 * cases, status, got) if st != 0 or not np.array_equal(g, c.samples)]
    assert not bad, bad
    assert (arena.view(np.uint16) == SENTINEL).all()
