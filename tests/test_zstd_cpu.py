"""CPU: the host zstd decoder (sigtk_amd/host/zstd_dec.c, reached through `sigtk-amd _zstd FILE`) and the BLOW5 reader on
files with zstd records.

Frames: tests/golden/zstd_frames.npz (written by libzstd 1.4.8, tests/golden/make_golden_zstd.py) and the hand-built
catalogues of tests/zstd_craft.py.  On the fixture's payloads libzstd wrote Raw and Compressed blocks, Raw, Compressed and
Treeless literals in one and four streams, Predefined, FSE and Repeat modes for all three codings and RLE mode for
offsets; RLE blocks, RLE literals and literal / match lengths in RLE mode come from the crafted set.  libzstd itself is
only an oracle here (loaded with ctypes where the machine has it); nothing of the product links it."""
import ctypes
import os
import struct
import subprocess
import zlib

import pytest

import zstd_craft
from sigtk_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ZSTD_B5 = os.path.join(GOLDEN, "sp1_dna.zstd_svb.blow5")
N_MUTATIONS, MUTATION_SEED = 300, 17


@pytest.fixture(scope="module")
def cli():
    path = build.CLI
    if not os.path.exists(path):
        build.build_lib()
        path = build.build_cli()
    return path


@pytest.fixture(scope="module")
def fixture():
    return zstd_craft.fixture()


@pytest.fixture(scope="module")
def valid():
    return zstd_craft.valid_frames()


@pytest.fixture(scope="module")
def invalid():
    return zstd_craft.invalid_frames()


@pytest.fixture(scope="module")
def mutated(fixture):
    return zstd_craft.mutations([f for _, f, w, _ in fixture if w is not None and len(f) < 60000], N_MUTATIONS, MUTATION_SEED)


def host_decode(exe, frame, path, env=None):
    """`_zstd` on the frame -> (status, bytes): exit 0 and the content, or exit 1 and the status it names"""
    with open(path, "wb") as fh:
        fh.write(frame)
    p = subprocess.run([exe, "_zstd", path], capture_output=True, timeout=120, env=env)
    assert p.returncode in (0, 1), (p.returncode, p.stderr[-600:])
    if p.returncode == 0:
        return 0, p.stdout
    assert p.stderr.startswith(b"zstd status "), p.stderr[-600:]
    return int(p.stderr.split()[2].rstrip(b":")), b""


def test_every_block_type_literals_type_and_mode_is_covered(fixture, valid):
    seen = set()
    for _, frame, want, _ in fixture:
        if want is not None:
            seen |= zstd_craft.walk(frame)
    from_libzstd = set(seen)
    for _, frame, _ in valid:
        seen |= zstd_craft.walk(frame)
    print("only in the crafted set:", sorted(seen - from_libzstd))
    assert not zstd_craft.COVERAGE - seen, sorted(zstd_craft.COVERAGE - seen)


def test_fixture_holds_what_its_generator_promises(fixture):
    levels = {name.split("_level")[1].split("_")[0] for name, *_ in fixture}
    assert levels == {"-5", "1", "3", "19"}
    flags = [f for *_, f in fixture]
    assert "checksum" in flags and flags.count("nosize") == 1
    assert os.path.getsize(os.path.join(GOLDEN, "zstd_frames.npz")) < (1 << 20)
    assert os.path.getsize(ZSTD_B5) <= os.path.getsize(os.path.join(GOLDEN, "sp1_dna.blow5"))
    head = open(ZSTD_B5, "rb").read(16)
    assert head[9] == 2 and head[14] == 1 and tuple(head[6:9]) >= (0, 2, 0)


def test_host_decoder_on_valid_frames(cli, tmp_path, fixture, valid):
    path = str(tmp_path / "f.zst")
    wrong = []
    for name, frame, want in [(n, f, w) for n, f, w, _ in fixture if w is not None] + valid:
        st, got = host_decode(cli, frame, path)
        if st != 0 or got != want:
            wrong.append((name, st, len(got), len(want)))
    assert not wrong, wrong


def test_host_decoder_names_the_status_of_invalid_frames(cli, tmp_path, fixture, invalid):
    path = str(tmp_path / "f.zst")
    cases = [(n, f, s) for n, f, s, _ in invalid] + [(n, f, zstd_craft.ST_HEADER) for n, f, w, _ in fixture if w is None]
    assert len(cases) == len(invalid) + 1
    wrong = [(n, st, s) for n, f, s in cases for st, _ in [host_decode(cli, f, path)] if st != s]
    assert not wrong, "(name, status, expected status): %s" % wrong


@pytest.fixture(scope="module")
def libzstd():
    try:
        z = ctypes.CDLL("libzstd.so.1")
    except OSError as e:
        pytest.skip("no libzstd to compare with: %s" % e)
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    z.ZSTD_getFrameContentSize.restype = ctypes.c_ulonglong
    z.ZSTD_getFrameContentSize.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    z.ZSTD_isError.argtypes = [ctypes.c_size_t]

    def decode(frame):
        """as slow5lib calls it (slow5_press.c:1177-1200): the declared size, then one ZSTD_decompress; None: refused"""
        size = z.ZSTD_getFrameContentSize(frame, len(frame))
        if size >= (1 << 64) - 2 or size > (1 << 28):
            return None
        out = ctypes.create_string_buffer(max(size, 1))
        n = z.ZSTD_decompress(out, size, frame, len(frame))
        return None if z.ZSTD_isError(n) or n != size else out.raw[:n]

    return decode


def test_libzstd_agrees_on_the_catalogues(libzstd, fixture, valid, invalid):
    for name, frame, want in [(n, f, w) for n, f, w, _ in fixture if w is not None] + valid:
        assert libzstd(frame) == want, name
    # the frames libzstd's one-shot decoder takes although they are refused here are marked in the catalogue
    # ("stricter than libzstd"); every other one it refuses too
    wrong = [(n, takes) for n, f, _, takes in invalid if (libzstd(f) is not None) != takes]
    assert not wrong, wrong
    assert sum(1 for *_, takes in invalid if takes) <= 8


def test_libzstd_agrees_on_mutated_frames(libzstd, cli, tmp_path, mutated):
    path = str(tmp_path / "m.zst")
    both = ours_only = theirs_only = 0
    for name, frame in mutated:
        st, got = host_decode(cli, frame, path)
        ref = libzstd(frame)
        if st == 0 and ref is not None:
            both += 1
            assert got == ref, name
        elif st == 0:
            ours_only += 1
        elif ref is not None:
            theirs_only += 1
    print("%d mutations: both accept %d, accepted here and refused by libzstd %d, refused here and accepted by libzstd %d"
          % (len(mutated), both, ours_only, theirs_only))
    assert len(mutated) == N_MUTATIONS and both > 0


def _dump(exe, *args, env=None):
    return subprocess.run([exe, "_dump", *args], capture_output=True, timeout=120, env=env)


def test_reader_on_a_file_with_zstd_records(cli, tmp_path):
    """sp1_dna.zstd_svb.blow5 against its twin with zlib records: the same records through b5_next, the split API and the
    mapped file, and by read id"""
    twin = str(tmp_path / "twin.blow5")
    zstd_craft.recode_blow5(os.path.join(GOLDEN, "sp1_dna.blow5"), twin, 1, zlib.compress)
    zst = str(tmp_path / "z.blow5")          # (a copy: the reader writes an index beside the file it reads by id)
    open(zst, "wb").write(open(ZSTD_B5, "rb").read())
    for extra in ([], ["--split"], ["--map"]):
        a, b = _dump(cli, *extra, zst), _dump(cli, *extra, twin)
        assert a.returncode == 0 and b.returncode == 0, (extra, a.stderr[-300:])
        la, lb = a.stdout.split(b"\n"), b.stdout.split(b"\n")
        assert la[0] == b"#press\t2\t1\tgroups\t1" and lb[0] == b"#press\t1\t1\tgroups\t1"
        assert la[1:] == lb[1:] and len(la) == 102
    rid = la[40].split(b"\t")[0].decode()
    for extra in ([], ["--split"]):
        a, b = _dump(cli, *extra, "--id", rid, zst), _dump(cli, *extra, "--id", rid, twin)
        assert a.returncode == 0 and a.stdout == b.stdout and a.stdout == la[40] + b"\n"
    data = bytearray(open(ZSTD_B5, "rb").read())
    data[9] = 3
    bad = str(tmp_path / "press3.blow5")
    open(bad, "wb").write(bytes(data))
    assert _dump(cli, bad).returncode == 1


@pytest.fixture(scope="module")
def cli_asan():
    try:
        return build.build_cli_asan()
    except (subprocess.CalledProcessError, OSError) as e:  # no libasan in this toolchain
        pytest.skip("sanitizer build not available: %s" % e)


def test_hostile_frames_and_records_under_asan_ubsan(cli_asan, tmp_path, invalid, mutated):
    """the stand-alone CLI built with -fsanitize=address,undefined: `_zstd` on the invalid frames and the mutations,
    `_dump` on the zstd BLOW5 with flipped and truncated records -- exit 0 or 1, no sanitizer report"""
    import numpy as np
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")

    def clean(p, what):
        assert p.returncode in (0, 1), (what, p.returncode, p.stderr[-600:])
        assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, (what, p.stderr[-600:])

    path = str(tmp_path / "f.zst")
    for name, frame in [(n, f) for n, f, _, _ in invalid] + mutated:
        open(path, "wb").write(frame)
        clean(subprocess.run([cli_asan, "_zstd", path], capture_output=True, timeout=120, env=env), name)
    data = open(ZSTD_B5, "rb").read()
    (hsize,) = struct.unpack_from("<I", data, 64)
    rs = np.random.RandomState(23)
    b5 = str(tmp_path / "fz.blow5")
    assert _dump(cli_asan, ZSTD_B5, env=env).returncode == 0
    for it in range(18):
        d = bytearray(data)
        if it % 3 == 0:
            for _ in range(int(rs.randint(1, 5))):
                d[int(rs.randint(68 + hsize, len(d)))] ^= 1 << int(rs.randint(8))
        elif it % 3 == 1:
            d = d[:int(rs.randint(68 + hsize + 9, len(d)))]
        else:
            i = int(rs.randint(68 + hsize, len(d) - 8))
            d[i:i + 8] = rs.bytes(8)
        open(b5, "wb").write(bytes(d))
        for extra in ([], ["--split"], ["--map"]):
            clean(_dump(cli_asan, *extra, b5, env=env), (it, extra))
