"""The crafted DEFLATE streams of tests/deflate_craft.py, judged by zlib (the library slow5lib inflates records with) on
the CPU: every stream of the valid catalogue inflates to exactly the bytes the token expander says, every stream of the
invalid one is refused with the message its fault should draw, and the valid catalogue reaches what it is there to reach
-- counted from what the writer wrote, not from any kernel.  This is what lets tests/test_gpu_inflate.py trust them."""
import zlib

import numpy as np
import pytest

import deflate_craft as C


@pytest.fixture(scope="module")
def valid():
    return C.valid_streams()


@pytest.fixture(scope="module")
def invalid():
    return C.invalid_streams()


def test_zlib_inflates_every_valid_stream_to_the_expected_bytes(valid):
    names = [n for n, _, _ in valid]
    assert len(set(names)) == len(names)
    assert sum(n.startswith("random_") for n in names) >= 200
    for name, stream, want in valid:
        assert zlib.decompress(stream) == want, name
    sizes = [len(w) for n, _, w in valid if n.startswith("random_")]
    assert min(sizes) == 0 and sum(s > 40000 for s in sizes) >= 10 and max(sizes) > 90000
    assert sum(len(w) for _, _, w in valid) < 4 << 20


def test_the_catalogues_are_the_same_every_time(valid):
    cov = C.Coverage()
    again = C._named_valid(cov) + C._random_valid(cov)          # (a second copy: the module's cache is left alone)
    assert vars(cov) == vars(C.coverage())
    assert [(n, s) for n, s, _ in again] == [(n, s) for n, s, _ in valid]


def test_zlib_refuses_every_invalid_stream_with_the_expected_message(invalid):
    names = [n for n, _, _, _ in invalid]
    assert len(set(names)) == len(names)
    for name, stream, status, fragment in invalid:
        with pytest.raises(zlib.error) as e:
            zlib.decompress(stream)
        assert fragment in str(e.value), (name, str(e.value))
        assert (status == 6) == ("incomplete or truncated" in str(e.value)), name
    by_status = {s: sum(1 for _, _, st, _ in invalid if st == s) for s in range(9)}
    assert all(by_status[s] >= 4 for s in (2, 3, 4, 5, 6, 7)), by_status
    # every kind of fault is there, by name
    for part in ("incomplete_literal_set", "incomplete_distance_set", "incomplete_code_length_code",
                 "oversubscribed_literal_set", "oversubscribed_distance_set", "oversubscribed_code_length_code",
                 "hlit_30", "hlit_31", "hdist_30", "hdist_31", "repeat_16_first", "one_past_the_end",
                 "no_end_of_block_code", "single_distance_code_other_bit", "fixed_literal_length_symbol_286",
                 "fixed_literal_length_symbol_287", "fixed_distance_symbol_30", "fixed_distance_symbol_31",
                 "pattern_no_code_owns", "distance_1_at_position_0", "distance_6001_at_position_6000",
                 "stored_len_nlen_mismatch", "block_type_3", "stored_length_past_the_input", "dynamic_header_cut",
                 "dynamic_symbols_cut", "adler_word_cut", "adler_bit"):
        assert any(part in n for n in names), part


def test_the_single_1bit_code_is_the_one_incomplete_set_zlib_accepts(valid, invalid):
    """the rule the kernel follows (zlib's inflate_table: left > 0 && (type == CODES || max != 1) is an error)"""
    ok = {n for n, _, _ in valid}
    assert {"dynamic_single_1bit_distance_code", "dynamic_single_1bit_end_of_block_code",
            "dynamic_one_distance_code_of_length_0"} <= ok
    bad = {n: s for n, _, s, _ in invalid}
    assert bad["incomplete_distance_set_one_2bit_code"] == 3 and bad["incomplete_code_length_code_single_1bit_code"] == 3


def test_canonical_codes_and_symbol_tables():
    # RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> codes 010 011 100 101 110 00 1110 1111
    assert C.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]
    assert C.kraft(C.FIXED_LIT) == 1 << 15 and C.kraft(C.FIXED_DIST) == 1 << 15
    for ln in range(3, 259):
        s, e, v = C.length_symbol(ln)
        assert 257 <= s <= 285 and C.LBASE[s - 257] + v == ln and 0 <= v < (1 << e) and e == C.LEXT[s - 257]
    assert C.length_symbol(258, alt=True) == (284, 5, 31)
    for d in list(range(1, 1200)) + list(range(32768 - 9000, 32769)) + [4096, 4097, 6144, 6145, 8192, 8193, 16384, 16385,
                                                                       24576, 24577]:
        s, e, v = C.dist_symbol(d)
        assert 0 <= s <= 29 and C.DBASE[s] + v == d and 0 <= v < (1 << e) and e == C.DEXT[s]
    rng = np.random.RandomState(2)
    for k, maxlen, deep in ((2, 15, 0), (3, 15, 2), (19, 7, 7), (30, 15, 15), (30, 15, 9), (286, 15, 15), (286, 15, 11),
                            (286, 9, 0)):
        lens = C.complete_lengths(rng, k, maxlen, deep)
        assert len(lens) == k and C.kraft(lens) == 1 << 15 and max(lens) <= maxlen and (not deep or deep in lens)
    assert bytes(C.expand(C.lits(b"abc") + [("match", 7, 3), ("match", 4, 1), ("match", 3, 10)])) == b"abcabcabcaaaaabca"


def test_the_valid_catalogue_reaches_what_it_is_there_for(valid):
    cov = C.coverage()
    names = {n for n, _, _ in valid}
    # every length symbol and every distance symbol, with the extra bits all zero and all one
    for k in range(29):
        kinds = {kind for s, kind in cov.len_syms if s == 257 + k}
        assert kinds >= ({"zero", "one"} if C.LEXT[k] else {"none"}), (257 + k, kinds)
    for k in range(30):
        kinds = {kind for s, kind in cov.dist_syms if s == k}
        assert kinds >= ({"zero", "one"} if C.DEXT[k] else {"none"}), (k, kinds)
    # literal, length and distance codes of every length written in dynamic blocks
    assert cov.lit_code_lens == set(range(1, 16))
    assert cov.len_code_lens == set(range(1, 16))
    assert cov.dist_code_lens == set(range(1, 16))
    # the ring's seams, the furthest match, overlapping matches either side of 64, 128 and 192
    assert {(258, C.NEAR), (258, C.NEAR + 1), (258, 32768)} <= cov.matches
    for d in (1, 2, 3, 63, 64, 65, 257):
        for ln in (63, 64, 65, 127, 128, 129, 191, 192, 193, 258):
            assert ln <= d or (ln, d) in cov.matches, (ln, d)
    # stored blocks: at every bit offset, of the lengths at the copy loop's and the flush's edges
    assert cov.stored_at == set(range(8))
    assert {0, 1, 63, 64, 65, 1023, 1024, 1025, 65535} <= cov.stored_lens
    # the dynamic header: the extreme counts, every repeat code with its shortest and longest run
    assert {257, 286} <= cov.nlit and {1, 30} <= cov.ndist
    assert {(16, 3), (16, 6), (17, 3), (17, 10), (18, 11), (18, 138)} <= cov.cl_syms
    assert all(cov.block_types[t] >= 100 for t in (0, 1, 2)), cov.block_types
    for part in ("run_1bit", "run_2bit", "run_enders_deep_11", "run_ends_at_input_seam_lead3_+0_match", "cl_repeat_16_across",
                 "empty_fixed_blocks", "empty_dynamic", "adler_ff_70000_stored", "adler_ff00_70000_stored",
                 "seam_dist_equals_position_32768", "seam_far_d32768_pre0", "seam_ring_d3838_body4096_pre1025"):
        assert any(part in n for n in names), part


def test_recode_writes_given_bytes_as_a_stream_zlib_reads_back():
    rng = np.random.RandomState(4)
    text = b"".join(b"%d squared is %d; " % (k % 97, k * k) for k in range(4000))
    for data in (b"", b"a", b"ab" * 50, text[:599], text[:600], text[:601], text[:1801], text,
                 rng.bytes(3000) + text[:40000] + rng.bytes(70000)):
        assert zlib.decompress(C.recode(rng, data)) == data
