"""GPU: sgk_zstd_decompress (csrc/zstd_kernels.hip) -- zstd frames decoded one wavefront each -- on the frames libzstd
wrote (tests/golden/zstd_frames.npz) and the hand-built catalogues of tests/zstd_craft.py; the host decoder
(`sigtk-amd _zstd`) is the second opinion on mutated frames.  No libzstd here."""
import os
import subprocess

import pytest

import zstd_craft
from sigtk_amd import build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    """every well-formed frame: (name, frame, payload)"""
    return [(n, f, w) for n, f, w, _ in zstd_craft.fixture() if w is not None] + zstd_craft.valid_frames()


@pytest.fixture(scope="module")
def invalid():
    return zstd_craft.invalid_frames()


# The output buffer starts out as FILL bytes, and behind every frame's room lie the bytes up to the next multiple of 16
# and GUARD more before the next frame's room begins: a stray write there shows, a zero byte too, also one that reaches
# past the alignment gap (which the next frame's own bytes would cover otherwise).
CANARY = dict(with_gaps=True, fill=0xA5, guard=64)


def _touched(gap):
    return gap != b"\xa5" * len(gap) or len(gap) < 64


def _check_exact(cases, res):
    """status 0, the declared length, the payload, and nothing written behind it (the room given is the exact length)"""
    got, olen, st, gaps = res
    wrong = [(n, int(st[r]), int(olen[r]), len(w)) for r, (n, _, w) in enumerate(cases)
             if st[r] != 0 or olen[r] != len(w) or got[r] != w or _touched(gaps[r])]
    assert not wrong, "(name, status, out_length, expected length):\n" + "\n".join(map(str, wrong))


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_valid_frame_at_every_input_alignment(gpu, frames, lead):
    from sigtk_amd import device
    leads = [lead] * len(frames)
    offs, _ = device.inflate_input_offsets([f for _, f, _ in frames], leads)
    assert {int(o) % 4 for o in offs} == {lead}
    _check_exact(frames, device.zstd_decompress([f for _, f, _ in frames], caps=[len(w) for _, _, w in frames],
                                                leads=leads, **CANARY))


def test_room(gpu, frames):
    """exactly the content size is enough; one byte less, and none, give status 8 and write nothing behind the room"""
    from sigtk_amd import device
    pick = [c for c in frames if c[0] in ("svb_100000_level1", "prose_290000_level1", "text_5_level3", "rle_block",
                                          "match_length_code_52", "seam_pre1023_off4033")]
    assert len(pick) == 6
    cases, caps = [], []
    for n, f, w in pick:
        for cap in (len(w), len(w) - 1, 0, len(w) + 100):
            cases.append((n, f, w)); caps.append(cap)
    got, olen, st, gaps = device.zstd_decompress([f for _, f, _ in cases], caps=caps, **CANARY)
    for r, ((n, f, w), cap) in enumerate(zip(cases, caps)):
        assert not _touched(gaps[r]), (n, cap)
        if cap >= len(w):
            assert st[r] == 0 and olen[r] == len(w) and got[r] == w, (n, cap, st[r])
        else:
            assert st[r] == zstd_craft.ST_SIZE and olen[r] <= cap, (n, cap, st[r], olen[r])


def test_invalid_frames_give_their_status(gpu, frames, invalid):
    """one defect per frame, the status include/sigtk_gpu.h documents for it -- with valid frames in between, which
    must not notice"""
    from sigtk_amd import device
    good = frames[::29]
    streams, expect = [], []
    for k, (name, frame, status, _) in enumerate(invalid):
        streams.append(frame); expect.append((name, status, None))
        if k % 4 == 0:
            g = good[(k // 4) % len(good)]
            streams.append(g[1]); expect.append((g[0], 0, g[2]))
    nosize = [(n, f) for n, f, w, _ in zstd_craft.fixture() if w is None]
    assert len(nosize) == 1
    streams.append(nosize[0][1]); expect.append((nosize[0][0], zstd_craft.ST_HEADER, None))
    got, olen, st, gaps = device.zstd_decompress(streams, caps=[1 << 19] * len(streams), **CANARY)
    wrong = [(name, int(st[r]), status) for r, (name, status, w) in enumerate(expect)
             if st[r] != status or _touched(gaps[r]) or (w is not None and (got[r] != w or olen[r] != len(w)))]
    assert not wrong, "(name, status, expected status):\n" + "\n".join(map(str, wrong))


def test_mutated_frames_like_the_host_decoder(gpu, tmp_path):
    """300 seeded bit flips, truncations and overwritten spans of the fixture's frames: accepted or refused as the host
    decoder does, the same bytes where accepted, nothing written outside the room"""
    from sigtk_amd import device
    src = [f for _, f, w, _ in zstd_craft.fixture() if w is not None and len(f) < 60000]
    mut = zstd_craft.mutations(src, 300, 17)
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    path = str(tmp_path / "m.zst")
    host = []
    for name, frame in mut:
        open(path, "wb").write(frame)
        p = subprocess.run([build.CLI, "_zstd", path], capture_output=True, timeout=60)
        assert p.returncode in (0, 1), (name, p.returncode)
        host.append(p.stdout if p.returncode == 0 else None)
    got, olen, st, gaps = device.zstd_decompress([f for _, f in mut], caps=[1 << 18] * len(mut), **CANARY)
    wrong = [(name, int(st[r]), host[r] is not None) for r, (name, _) in enumerate(mut)
             if _touched(gaps[r]) or (st[r] == 0) != (host[r] is not None) or (st[r] == 0 and got[r] != host[r])]
    assert not wrong, "(name, status, accepted by the host decoder):\n" + "\n".join(map(str, wrong))
    assert sum(h is not None for h in host) > 30


def test_short_and_long_frames_share_a_launch(gpu, frames):
    """0- and 1-byte payloads among the frames of several blocks, more frames than one compute unit holds"""
    from sigtk_amd import device
    by = {n: (n, f, w) for n, f, w in frames}
    tiny = [by["zeros_0_level1"], by["text_1_level1"], by["text_1_level19"], by["empty_raw_block"]]
    big = [by[k] for k in ("prose_290000_level1", "random_140000_level1", "svb_100000_level1", "text_200000_level3",
                           "runs_150000_level19", "many_blocks", "nseq_3_bytes")]
    cases = []
    for k in range(48):
        cases += tiny
        if k % 7 == 0:
            cases.append(big[(k // 7) % len(big)])
    cases += big
    _check_exact(cases, device.zstd_decompress([f for _, f, _ in cases], caps=[len(w) for _, _, w in cases], **CANARY))
