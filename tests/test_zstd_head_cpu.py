"""CPU: the head-only mode of the host zstd decoder (zsd_decode_head, what b5_parse_head runs for every record that goes
to the GPU compressed), through `sigtk-amd _zstd --head N FILE`: the first N bytes of every frame, and no more work than
they need -- of a block's Huffman-coded literals only the first N are decoded."""
import os
import subprocess

import pytest

import zstd_craft
from sigtk_amd import build


@pytest.fixture(scope="module")
def cli():
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


@pytest.fixture(scope="module")
def frames():
    return [(name, frame, data) for name, frame, data, _ in zstd_craft.fixture() if data is not None] + \
           [(v[0], v[1], v[2]) for v in zstd_craft.valid_frames()]


def head(cli, path, n):
    return subprocess.run([cli, "_zstd", "--head", str(n), path], capture_output=True)


def test_the_head_is_the_payloads_prefix(cli, frames, tmp_path):
    """sizes around what b5_parse_head asks (512), below and above the first stream of small literals sections, and
    past the frame's end (then the whole frame is decoded and checked)"""
    path = str(tmp_path / "f.zst")
    n_fixture = sum(1 for _, _, data, _ in zstd_craft.fixture() if data is not None)
    seen = 0
    for k, (name, frame, data) in enumerate(frames):
        if k < n_fixture and k % 5 and not name.startswith(("svb", "prose")):
            continue                            # (a process per frame and size: a fifth of the fixture, all hand-built frames)
        open(path, "wb").write(frame)
        for n in ((1, 97, 512) if k < n_fixture else (97, len(data) + 1)):
            p = head(cli, path, n)
            assert p.returncode == 0 and p.stdout == data[:n], (name, n, p.returncode, p.stderr[-100:])
        seen += 1
    assert seen >= 150


def _first_block_huffman4(frame):
    """(offset of the literals section's compressed part, its size) when the frame's first block is a Compressed one
    with four Huffman streams, else None"""
    d = frame[4]
    single = (d >> 5) & 1
    fcs = (1 << (d >> 6)) if d >> 6 else single
    at = 5 + (0 if single else 1) + fcs
    bh = int.from_bytes(frame[at:at + 3], "little")
    if (bh >> 1) & 3 != 2:
        return None
    p = at + 3
    ltype, sf = frame[p] & 3, (frame[p] >> 2) & 3
    if ltype != 2 or sf == 0:
        return None
    hl, nb = (3, 10) if sf < 2 else ((4, 14) if sf == 2 else (5, 18))
    v = int.from_bytes(frame[p:p + hl], "little") >> 4
    return p + hl, (v >> nb) & ((1 << nb) - 1)


def test_the_head_does_not_decode_the_later_streams(cli, frames, tmp_path):
    """The fourth Huffman stream of the first block loses its end mark (its last byte, the last of the literals section,
    becomes 0): the whole-frame decode refuses the frame (status 4), the head decode never looks there."""
    path = str(tmp_path / "f.zst")
    done = 0
    for name, frame, data in frames:
        where = _first_block_huffman4(frame)
        if where is None or len(data) < 20000:
            continue
        bad = bytearray(frame)
        bad[where[0] + where[1] - 1] = 0
        open(path, "wb").write(bytes(bad))
        p = subprocess.run([cli, "_zstd", path], capture_output=True)
        assert p.returncode == 1 and b"zstd status 4" in p.stderr, (name, p.returncode, p.stderr[-100:])
        for n in (97, 512):
            p = head(cli, path, n)
            assert p.returncode == 0 and p.stdout == data[:n], (name, n, p.returncode, p.stderr[-100:])
        done += 1
        if done == 5:
            break
    assert done == 5
