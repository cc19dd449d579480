"""The svb-zd catalogue (tests/svb_cases.py) against slow5lib's recorded answers (tests/golden/svb_cases.json, written by
tests/golden/make_golden_svb.py), against the vectorised host codec, against the blobs of the bundled BLOW5 file, and
against itself: the classes of alignment and byte counts the GPU tests rely on are counted here from the cases' own
offsets and bytes."""
import collections
import hashlib
import json
import os

import numpy as np
import pytest

import svb_cases as S
from sigtk_amd import blow5

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# slow5lib sums the deltas in an int32, which overflows on this case (undefined in C): its recorded answer is not binding
SUM_OVERFLOWS = {"sum_leaves_int32"}


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "svb_cases.json")) as fh:
        return json.load(fh)


def _digest(data: bytes):
    return [len(data), hashlib.sha256(data).hexdigest()]


def test_fixture_names_are_the_catalogues(fixture):
    assert list(fixture["decode"]) == [c.name for c in S.decode_cases() + S.malformed_cases()]
    assert list(fixture["encode"]) == [c.name for c in S.encode_cases()]


def test_ref_decode_reproduces_slow5lib(fixture):
    """slow5lib is not told the expected count: it decodes a blob by its own count word, or refuses it"""
    n_hash = n_refused = n_documented = 0
    for c in S.decode_cases() + S.malformed_cases():
        rec = fixture["decode"][c.name]
        rules, _ = S.ref_rules(c.blob, c.expected_count)
        assert (rules or (0,)) == c.status, c.name
        st, out = S.ref_decode(c.blob, c.expected_count)
        assert st in c.status and (out is not None) == (st == 0), c.name
        if rec == "documented":     # too short for its keys or data: the header's rule alone
            assert 0 not in c.status, c.name
            n_documented += 1
            continue
        own = int.from_bytes(c.blob[0:4], "little")
        st_own, out_own = S.ref_decode(c.blob, own)
        if rec == "refused":        # bytes left over
            assert st_own == 2 and c.status == (2,), c.name
            n_refused += 1
            continue
        assert st_own == 0, c.name
        if c.expected_count == own:
            assert c.status == (0,) and np.array_equal(out, out_own), c.name
        else:
            assert c.status == (1,), c.name
        if c.name not in SUM_OVERFLOWS:
            assert _digest(out_own.astype("<i2").tobytes()) == rec, c.name
            n_hash += 1
    assert n_documented > 0 and n_refused > 0 and n_hash >= len(S.decode_cases()) - len(SUM_OVERFLOWS)


def test_ref_encode_reproduces_slow5lib(fixture):
    for c in S.encode_cases():
        assert _digest(S.ref_encode(c.samples)) == fixture["encode"][c.name], c.name


def test_vectorised_host_codec_agrees():
    """blow5.svb_zd_decode / svb_zd_encode, the second opinion: wherever they accept (svb_zd_decode knows no expected
    count and refuses a wrong data length with ValueError; blobs cut inside their keys are outside its contract)"""
    for c in S.decode_cases():
        assert np.array_equal(blow5.svb_zd_decode(c.blob), S.ref_decode(c.blob, c.expected_count)[1]), c.name
    for c in S.malformed_cases():
        if c.kind in ("left_over_single", "left_over_multi", "data_short_1", "data_short_2", "data_short_tile",
                      "data_short_second_tile"):
            with pytest.raises(ValueError):
                blow5.svb_zd_decode(c.blob)
        elif c.kind in ("count_mismatch", "count0_len4"):
            own = int.from_bytes(c.blob[0:4], "little")
            assert np.array_equal(blow5.svb_zd_decode(c.blob), S.ref_decode(c.blob, own)[1]), c.name
    for c in S.encode_cases():
        assert blow5.svb_zd_encode(c.samples) == S.ref_encode(c.samples), c.name


def test_bundled_file(sp1):
    recs = blow5.read_signal_blobs(os.path.join(GOLDEN, "sp1_dna.blow5"))
    assert len(recs) == 100 == len(sp1.reads)
    for (_, blob), r in zip(recs, sp1.reads):
        st, out = S.ref_decode(blob, r.raw.size)
        assert st == 0 and np.array_equal(out, r.raw)
        assert S.ref_encode(r.raw) == blob


def test_malformed_kinds():
    kinds = collections.Counter(c.kind for c in S.malformed_cases())
    assert set(kinds) == set(S.MALFORMED_STATUS)
    for c in S.malformed_cases():
        assert c.status == S.MALFORMED_STATUS[c.kind], c.name
    by = {k: [c for c in S.malformed_cases() if c.kind == k] for k in kinds}
    assert sorted(len(c.blob) for c in by["short_blob"]) == [0, 1, 2, 3]
    assert sorted(len(c.blob) for c in by["cut_in_keys"]) == [4, 5, 6, 7, 8]
    assert sorted(int.from_bytes(c.blob[0:4], "little") - c.expected_count for c in by["count_mismatch"]) == [-17, -1, 1, 1, 17]
    for k in ("left_over_single", "left_over_multi"):
        assert len(by[k]) == 4 and all((c.expected_count > S.TILE) == (k == "left_over_multi") for c in by[k])
    assert {c.blob[0:4] for c in by["count_wrap"]} == {b"\xfd\xff\xff\xff", b"\xfe\xff\xff\xff", b"\xff\xff\xff\xff"}
    assert all(c.expected_count < 64 for c in by["count_wrap"])
    print("malformed kinds:", dict(kinds))


def test_decoder_coverage():
    """counted from the cases' leads and the bytes of their blobs, not from the kernel"""
    cls = collections.Counter()
    worst_stage = 0
    four_byte_tile_then_more = 0
    for c in S.decode_cases():
        assert c.status == (0,) and 0 <= c.blob_lead < 16 and 0 <= c.sample_lead < 8
        n = int.from_bytes(c.blob[0:4], "little")
        nkeys = (n + 3) // 4
        multi = n > S.TILE
        cls[(c.blob_lead % 4, nkeys % 4, c.sample_lead % 8 != 0)] += 1
        cls[("multi", c.blob_lead % 4, nkeys % 4)] += multi
        codes = S.key_codes(c.blob)
        for t in range(0, n - S.TILE + 1, S.TILE):
            if (codes[t:t + S.TILE] == 3).all():
                # the tile's data starts at blob_lead + 4 + nkeys + 4 * t behind a 16-byte boundary
                worst_stage += (c.blob_lead + 4 + nkeys) % 4 == 3
                four_byte_tile_then_more += n > t + S.TILE
    for bl4 in range(4):
        for nk4 in range(4):
            assert cls[(bl4, nk4, False)] > 0 and cls[(bl4, nk4, True)] > 0 and cls[("multi", bl4, nk4)] > 0, (bl4, nk4)
    assert worst_stage > 0 and four_byte_tile_then_more > 0
    print("decoder classes (blob_lead % 4, key bytes % 4, sample_lead % 8 != 0):",
          {k: v for k, v in sorted(cls.items(), key=str) if k[0] != "multi"})
    print("multi-tile:", {k[1:]: v for k, v in sorted(cls.items(), key=str) if k[0] == "multi"})
    print("full tiles of 4-byte codes at data %% 4 == 3: %d; followed by more values: %d" % (worst_stage, four_byte_tile_then_more))


def test_encoder_coverage():
    pairs = collections.Counter()
    carries = collections.Counter()
    leads = collections.Counter()
    for c in S.encode_cases():
        assert c.blob_lead in S.ENCODE_BLOB_LEADS and c.sample_lead in S.ENCODE_SAMPLE_LEADS
        blob = S.ref_encode(c.samples)
        n = c.samples.size
        nkeys = (n + 3) // 4
        ndata = len(blob) - 4 - nkeys
        multi = n > S.TILE
        pairs[(nkeys % 4, ndata % 4, multi)] += 1
        leads[(n, c.sample_lead, c.blob_lead)] += 1
        if multi:   # bytes in front of the data's first dword + data bytes of tile 1, modulo 4: carried into tile 2
            carries[((c.blob_lead + 4 + nkeys) % 4 + S.first_tile_data_bytes(blob)) % 4] += 1
    for k in range(4):
        for d in range(4):
            assert pairs[(k, d, False)] > 0 and pairs[(k, d, True)] > 0, (k, d)
    assert all(carries[v] > 0 for v in range(4))
    for n in S.LENGTHS:
        for sl in S.ENCODE_SAMPLE_LEADS:
            for bl in S.ENCODE_BLOB_LEADS:
                assert leads[(n, sl, bl)] > 0, (n, sl, bl)
    print("encoder classes (key bytes % 4, data bytes % 4, multi-tile):", dict(sorted(pairs.items())))
    print("bytes carried into tile 2:", dict(sorted(carries.items())))
