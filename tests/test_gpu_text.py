"""GPU: the TSV rows of pa / event / event -c written on the device (csrc/text_kernels.hip, sgk_text_*, SGK_JOB_TEXT,
`sigtk-amd --gpu-text`).  Every comparison is byte equality: with glibc's snprintf for the numbers, with
tests/tsv_grammar.py (the reference's row grammar) over the oracle's / the library's binary results for the rows, with
the committed goldens for the CLI.  No read is ever left to the host: every test compares the whole text of its batch."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import tsv_grammar as G
from sigtk_amd import blow5, build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
SP1 = os.path.join(GOLDEN, "sp1_dna.blow5")

_libc = C.CDLL(None)
_buf = C.create_string_buffer(512)


def c_f(v) -> bytes:
    """printf("%f", (double)v) by glibc"""
    n = _libc.snprintf(_buf, 512, b"%f", C.c_double(float(v)))
    return _buf.raw[:n]


def c_ld(v) -> bytes:
    n = _libc.snprintf(_buf, 512, b"%ld", C.c_long(int(v)))
    return _buf.raw[:n]


def pa_row_c(read_id: bytes, pa) -> bytes:
    """pa_func's row with every number from snprintf (Python's %f drops the sign of a NaN)"""
    return read_id + b"\t" + str(len(pa)).encode() + b"\t" + b",".join(c_f(v) for v in pa) + b"\n"


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


# ------------------------------------------------------------------------------------------------ 1. the primitive

def _f32_cases():
    w = [0x3c000000, 0x58635fa8, 0x58635fa9, 0x58635faa, 0xd8635faa, 0x7f7fffff, 0xff7fffff, 0, 0x80000000, 0x7f800000,
         0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 1, 2, 0x007fffff, 0x00800000, 0x80000001]
    for e in range(256):                                   # every power of two and its neighbours, both signs
        for d in (-2, -1, 0, 1, 2):
            w += [((e << 23) + d) & 0xffffffff, (((e << 23) + d) & 0xffffffff) ^ 0x80000000]
    vals = [np.array(w, dtype=np.uint32).view(np.float32)]
    # ties and carries around the 6th decimal (the cases of `_fmtcheck` / `_textcheck`)
    k = np.arange(1, 4000, 2, dtype=np.float32)
    for m in range(1, 31):
        f = k / np.float32(1 << m)
        vals += [f, -f, f + np.float32(123456.0), np.float32(999999.0) + f]
    vals.append(np.arange(0, 1 << 32, 3989, dtype=np.uint64).astype(np.uint32).view(np.float32))   # 1 076 713 strided patterns
    return np.concatenate(vals).astype(np.float32)


def test_numbers_on_the_device_equal_snprintf(gpu):
    """pins the device's arithmetic (f64 rint, conversions, the multi-limb division) to the host's"""
    from sigtk_amd import device
    v = _f32_cases()
    assert v.size > 1000000
    slots, lens = device.text_numbers(v)
    assert not (lens == 255).any(), "writer and length-only form disagree at %s" % v[lens == 255][:5]
    bad = []
    for i in range(v.size):
        e = c_f(v[i])
        if int(lens[i]) != len(e) or slots[i, :len(e)].tobytes() != e or slots[i, len(e)] != 35:
            bad.append((hex(int(v[i:i + 1].view(np.uint32)[0])), slots[i, :int(lens[i]) % 48].tobytes(), e))
            if len(bad) > 5:
                break
    assert not bad, bad
    assert int(lens[5]) == 46 and slots[0, :8].tobytes() == b"0.007812"    # FLT_MAX; the tie goes to even

    iv = [0, 1, -1, 12345, -98765, 2 ** 31 - 1, -2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1, -2 ** 63]
    for k in range(19):
        for d in (-1, 0, 1):
            iv += [10 ** k + d, -(10 ** k + d)]
    iv = np.array(iv, dtype=np.int64)
    slots, lens = device.text_numbers(iv)
    for i in range(iv.size):
        e = c_ld(iv[i])
        assert int(lens[i]) == len(e) and slots[i, :len(e)].tobytes() == e and slots[i, len(e)] == 35, (int(iv[i]), e)


# ------------------------------------------------------------------------------------------------ 2. device API, pa

def _ids(n, lens=(36,)):
    """ids of the given lengths, cycled; every one different"""
    out = []
    for r in range(n):
        k = lens[r % len(lens)]
        s = ("%08d-" % r) + "abcdefghijklmnopqrstuvwxyz0123456789-" * 9
        out.append(s[:k].encode())
    return out


def _pa_text(reads, dig, off, rng, ids):
    torch = _torch()
    from sigtk_amd import api, device
    b = device.upload_reads(reads, dig, off, rng, torch.device("cuda", 0))
    w = device.TextWriter(b, ids, api.TEXT_PA)
    text = w.run()
    assert int(w.row_offsets_host[0]) == 0 and int(w.row_offsets_host[-1]) == len(text)
    return text, w.row_offsets_host


def _check_rows(text, row_offsets, rows):
    """the text is the concatenation of the rows and row_offsets delimit them"""
    for r, row in enumerate(rows):
        a, e = int(row_offsets[r]), int(row_offsets[r + 1])
        assert text[a:e] == row, "read %d: %r ... vs %r ..." % (r, text[a:a + 80], row[:80])
    assert text == b"".join(rows)


def test_pa_rows_of_the_bundled_fixture(gpu, oracle, sp1):
    reads = [r.raw for r in sp1.reads]
    dig = np.array([r.digitisation for r in sp1.reads]); off = np.array([r.offset for r in sp1.reads])
    rng = np.array([r.range for r in sp1.reads])
    ids = [r.read_id.encode() for r in sp1.reads]
    text, ro = _pa_text(reads, dig, off, rng, ids)
    rows = [G.pa_row(r.read_id, oracle.pa(r.raw, r.digitisation, r.offset, r.range)).encode() for r in sp1.reads]
    _check_rows(text, ro, rows)
    assert hashlib.sha256(G.HDR_PA.encode() + text).hexdigest() == MANIFEST["sp1_dna.pa.tsv.sha256"]


def test_pa_rows_ragged_lengths_and_id_lengths(gpu, oracle):
    lens = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 100000, 255, 256, 257, 0, 511, 512, 513]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=71, kind=0)
    ids = _ids(len(lens), (0, 1, 36, 300))
    text, ro = _pa_text(reads, dig, off, rng, ids)
    rows = [G.pa_row(ids[r].decode(), oracle.pa(reads[r], dig[r], off[r], rng[r])).encode() for r in range(len(lens))]
    assert rows[0] == b"\t0\t\n" and rows[13] == ids[13] + b"\t0\t\n"
    _check_rows(text, ro, rows)


def test_pa_rows_one_very_long_read_among_short_ones(gpu, oracle):
    lens = [3000 + 17 * k for k in range(100)] + [1600000] + [2500 + 13 * k for k in range(100)]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=72, kind=0)
    ids = _ids(len(lens))
    text, ro = _pa_text(reads, dig, off, rng, ids)
    rows = [G.pa_row(ids[r].decode(), oracle.pa(reads[r], dig[r], off[r], rng[r])).encode() for r in range(len(lens))]
    _check_rows(text, ro, rows)


def test_pa_rows_hostile_scalings(gpu, oracle):
    """negative values, -0.000000, values >= 1e15, inf and nan: every number of the expected rows is glibc's"""
    rnd = np.random.RandomState(5)
    base = rnd.randint(-32768, 32768, size=3000).astype(np.int16)
    base[:8] = [0, -1, 1, -32768, 32767, -7, 7, 0]
    scal = [(8192.0, 7.0, -1402.882324),      # negative values
            (8192.0, 0.0, -1402.882324),      # raw 0 -> -0.000000
            (8192.0, -32767.0, 1e-38),        # tiny values, denormal products
            (1.0, 3.0, 1e30),                 # >= 1e15: the multi-limb path
            (8192.0, 10.0, 1e30),
            (8192.0, 0.0, float("inf")),      # inf, -inf, and 0 * inf = nan
            (0.0, 0.0, 1400.0),               # x / 0 = inf; 0 * inf
            (0.0, 5.0, -1400.0),
            (8192.0, float("nan"), 1400.0),
            (1e-30, 1e30, 1e30)]
    reads = [base.copy() for _ in scal]
    dig = np.array([s[0] for s in scal]); off = np.array([s[1] for s in scal]); rng = np.array([s[2] for s in scal])
    ids = _ids(len(scal), (36, 1, 0, 300))
    text, ro = _pa_text(reads, dig, off, rng, ids)
    rows = [pa_row_c(ids[r], oracle.pa(reads[r], dig[r], off[r], rng[r])) for r in range(len(scal))]
    import re
    assert b"-0.000000" in rows[1] and b"inf" in rows[5] and b"nan" in rows[5] and re.search(rb"[0-9]{30,}\.000000", rows[3])
    _check_rows(text, ro, rows)


# ------------------------------------------------------------------------------------------------ 3. device API, events

def _event_text(reads, dig, off, rng, rna, ids, compact, slots_for=None):
    torch = _torch()
    from sigtk_amd import api, device
    dev = torch.device("cuda", 0)
    b = device.upload_reads(reads, dig, off, rng, dev)
    arena = device.EventArena(b)
    if slots_for is not None:
        slots = np.zeros(len(reads) + 1, dtype=np.int64)
        np.cumsum([slots_for(len(r)) for r in reads], out=slots[1:])
        arena.slots_host, arena.n_slots, arena.slots = slots, int(slots[-1]), torch.from_numpy(slots).to(dev)
    device.event(b, arena, rna)
    w = device.TextWriter(b, ids, api.TEXT_EVENT_COMPACT if compact else api.TEXT_EVENT, arena)
    text = w.run()      # no host round trip between the event kernels and the text kernels: same stream, no sync between
    return text, w.row_offsets_host


def _event_rows(gpu, reads, dig, off, rng, rna, ids, compact, keep=None):
    evs, _ = gpu.event(reads, dig, off, rng, rna)
    rows = []
    for r, e in enumerate(evs):
        k = e.start.size if keep is None else min(e.start.size, keep)
        rows.append(G.event_rows(ids[r].decode(), len(reads[r]), e.start[:k], e.length[:k], e.mean[:k], e.stdv[:k], compact).encode())
    return rows


@pytest.mark.parametrize("compact", [True, False])
def test_event_rows_of_the_bundled_fixture(gpu, sp1, compact):
    reads = [r.raw for r in sp1.reads]
    dig = np.array([r.digitisation for r in sp1.reads]); off = np.array([r.offset for r in sp1.reads])
    rng = np.array([r.range for r in sp1.reads])
    ids = [r.read_id.encode() for r in sp1.reads]
    text, ro = _event_text(reads, dig, off, rng, 0, ids, compact)
    _check_rows(text, ro, _event_rows(gpu, reads, dig, off, rng, 0, ids, compact))
    if compact:
        assert G.HDR_EVENT_COMPACT.encode() + text == open(os.path.join(GOLDEN, "sp1_dna.event_c.tsv"), "rb").read()
    else:
        assert hashlib.sha256(G.HDR_EVENT.encode() + text).hexdigest() == MANIFEST["sp1_dna.event.tsv.sha256"]


@pytest.mark.parametrize("rna", [0, 1])
@pytest.mark.parametrize("compact", [True, False])
def test_event_rows_synthetic_short_and_empty_reads(gpu, rna, compact):
    """reads without events print `.\\t.\\t.\\t.` (compact) or the lone empty line (long form); a read shorter than the
    detector's windows is one event"""
    lens = [30000, 0, 1, 5, 63, 64, 300, 70001, 0, 12345, 2, 0]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=81 + rna, kind=rna)
    ids = _ids(len(lens), (36, 0, 1, 300))
    text, ro = _event_text(reads, dig, off, rng, rna, ids, compact)
    rows = _event_rows(gpu, reads, dig, off, rng, rna, ids, compact)
    assert rows[1] == (ids[1] + b"\t0\t.\t.\t.\t.\n" if compact else b"\n")
    _check_rows(text, ro, rows)


@pytest.mark.parametrize("rna", [0, 1])
@pytest.mark.parametrize("compact", [True, False])
def test_event_rows_packed_whole_and_segmented_reads(gpu, rna, compact):
    """one batch that mixes short reads (several to a wavefront), whole reads and one read long enough to be cut into
    segments: the text kernels see one arena whatever path filled it"""
    lens = [2000 + 37 * (k % 50) for k in range(600)] + [40000 + 1000 * k for k in range(8)] + [450000] + [3000] * 40
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=91 + rna, kind=rna)
    ids = _ids(len(lens))
    text, ro = _event_text(reads, dig, off, rng, rna, ids, compact)
    _check_rows(text, ro, _event_rows(gpu, reads, dig, off, rng, rna, ids, compact))


@pytest.mark.parametrize("compact", [True, False])
def test_event_rows_of_a_read_that_overflowed_its_slots(gpu, compact):
    """written with what fitted, as the dense gather of the jobs does"""
    reads, dig, off, rng = gpu.synth_reads_host(3, [20000, 500, 20000], seed=32, kind=0)
    ids = _ids(3)
    text, ro = _event_text(reads, dig, off, rng, 0, ids, compact, slots_for=lambda n: 100)
    _check_rows(text, ro, _event_rows(gpu, reads, dig, off, rng, 0, ids, compact, keep=100))


# ------------------------------------------------------------------------------------------------ 4. guard bands

@pytest.mark.parametrize("kind", ["pa", "event", "event_c"])
def test_nothing_outside_the_text_range_is_touched(gpu, kind):
    """the text arena sits between two 4 KB canary regions and starts on odd byte addresses; one byte short of the
    total, the status word reports the overflow and nothing is written behind the capacity"""
    torch = _torch()
    from sigtk_amd import api, device
    dev = torch.device("cuda", 0)
    lens = [5000, 0, 777, 30001, 64, 1]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=95, kind=0)
    ids = _ids(len(lens), (36, 5, 0, 41))
    b = device.upload_reads(reads, dig, off, rng, dev)
    arena = None
    if kind != "pa":
        arena = device.EventArena(b)
        device.event(b, arena, 0)
    k = {"pa": api.TEXT_PA, "event": api.TEXT_EVENT, "event_c": api.TEXT_EVENT_COMPACT}[kind]
    w = device.TextWriter(b, ids, k, arena)
    ref = w.run()
    total = len(ref)
    for shift in (1, 3, 7, 13, 16):
        for short in (0, 1):
            w.measure()
            buf = torch.full((4096 + shift + total + 4096,), 0xA5, dtype=torch.uint8, device=dev)
            lo = 4096 + shift
            w.write(buf[lo:], total - short)
            rc, st = w.status()
            host = buf.cpu().numpy()
            assert (host[:lo] == 0xA5).all() and (host[lo + total:] == 0xA5).all(), (shift, short)
            assert st.n_bytes == total
            if short:
                assert rc == api.SGK_ERR_CAPACITY and st.overflow == 1
                assert host[lo + total - 1] == 0xA5                   # nothing behind the capacity
                got = host[lo:lo + total - 1].tobytes()               # what was written is right, the rest untouched
                assert all(g == e or g == 0xA5 for g, e in zip(got, ref))
            else:
                assert rc == api.SGK_OK and st.overflow == 0
                assert host[lo:lo + total].tobytes() == ref


# ------------------------------------------------------------------------------------------------ 5. jobs

def _zrec(read_id: bytes, dig, off, rng, raw):
    """a record as slow5lib writes it (zlib around id, scaling and the svb-zd signal) and where its signal lies"""
    sig = blow5.svb_zd_encode(raw)
    rec = struct.pack("<H", len(read_id)) + read_id + struct.pack("<IddddQ", 0, dig, off, rng, 4000.0, len(sig)) + sig
    return zlib.compress(rec), 2 + len(read_id) + 44, len(sig), len(rec)


def _stage(job, staging, reads, dig, off, rng, ids):
    if staging == "int16":
        job.stage(reads, dig, off, rng, ids=ids)
    elif staging == "svbzd":
        job.stage([blow5.svb_zd_encode(r) for r in reads], dig, off, rng, counts=[r.size for r in reads], ids=ids)
    else:
        z = [_zrec(b"zrec-%d" % r, float(dig[r]), float(off[r]), float(rng[r]), reads[r]) for r in range(len(reads))]
        job.stage_zrec([q[0] for q in z], [r.size for r in reads], [q[1] for q in z], [q[2] for q in z], [q[3] for q in z],
                       dig, off, rng, ids=ids)


@pytest.mark.parametrize("staging", ["int16", "svbzd", "zrec"])
def test_text_jobs_equal_the_rows_of_the_same_job_without_the_flag(gpu, staging):
    """a job reused over a large, then a small, then an empty batch; pa, event and event -c each time"""
    job = gpu.Job(0)
    for b, lens in enumerate(([5000, 100000, 333, 70001, 0, 1, 250] + [20000] * 12, [64, 4096], [])):
        reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=60 + b, kind=0) if lens else ([], [], [], [])
        ids = _ids(len(lens), (36, 7, 0, 120))
        _stage(job, staging, reads, dig, off, rng, ids)
        n = len(lens)

        job.launch(gpu.TOOL_PA)
        pa = job.wait()["pa"]
        job.launch(gpu.TOOL_PA, flags=gpu.JOB_TEXT)
        res = job.wait()
        assert "pa" not in res
        _check_rows(res["text"], res["row_offsets"] if n else [0], [G.pa_row(ids[r].decode(), pa[r]).encode() for r in range(n)])

        job.launch(gpu.TOOL_EVENT)
        ev = job.wait()["events"]
        for flags, compact in ((gpu.JOB_TEXT, False), (gpu.JOB_TEXT | gpu.JOB_EVENTS_LENGTHS, True),
                               (gpu.JOB_TEXT | gpu.JOB_EVENTS_COMPACT, True)):
            job.launch(gpu.TOOL_EVENT, flags=flags)
            res = job.wait()
            assert "events" not in res
            rows = [G.event_rows(ids[r].decode(), lens[r], ev[r].start, ev[r].length, ev[r].mean, ev[r].stdv, compact).encode()
                    for r in range(n)]
            _check_rows(res["text"], res["row_offsets"] if n else [0], rows)
    job.close()


def test_text_jobs_refuse_other_tools_and_missing_ids(gpu):
    reads, dig, off, rng = gpu.synth_reads_host(2, [5000, 6000], seed=7, kind=0)
    job = gpu.Job(0)
    job.stage(reads, dig, off, rng)                      # no ids
    for tool in (gpu.TOOL_PA, gpu.TOOL_EVENT):
        with pytest.raises(gpu.SigtkGpuError, match="argument"):
            job.launch(tool, flags=gpu.JOB_TEXT)
    job.set_ids([b"a", b"bb"])
    for tool in (gpu.TOOL_STAT, gpu.TOOL_JNN, gpu.TOOL_PREFIX, gpu.TOOL_ENT):
        with pytest.raises(gpu.SigtkGpuError, match="argument"):
            job.launch(tool, flags=gpu.JOB_TEXT)
    job.launch(gpu.TOOL_PA, flags=gpu.JOB_TEXT)          # the job is still usable
    assert job.wait()["text"].startswith(b"a\t5000\t")
    job.stage(reads, dig, off, rng)                      # a new batch forgets the ids of the last one
    with pytest.raises(gpu.SigtkGpuError, match="argument"):
        job.launch(gpu.TOOL_PA, flags=gpu.JOB_TEXT)
    job.close()


# ------------------------------------------------------------------------------------------------ 6. the CLI

@pytest.fixture(scope="module")
def cli(gpu):
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


def out(cli, *args, env=None):
    p = subprocess.run([cli, *args], capture_output=True, env=env)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout


def gold(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.fixture(scope="module")
def synth_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("synth_text")
    from sigtk_amd import api
    files = {}
    for name, spec in list(MANIFEST["_synth_specs"].items()) + list(MANIFEST["_synth_long_specs"].items()):
        n, ln, seed, kind, exp, kit = spec
        reads, dig, off, rng = api.synth_reads_host(n, ln, seed, kind)
        recs = [blow5.Read("synth-%08d" % i, 0, float(dig[i]), float(off[i]), float(rng[i]), 4000.0, reads[i])
                for i in range(n)]
        path = str(d / (name + ".blow5"))
        blow5.write_blow5(path, recs, {"experiment_type": exp, "sequencing_kit": kit})
        files[name] = path
    return files


def test_cli_gpu_text_bundled_fixture(cli):
    assert out(cli, "event", "-c", "--gpu-text", SP1) == gold("sp1_dna.event_c.tsv")
    assert sha(out(cli, "event", "--gpu-text", SP1)) == MANIFEST["sp1_dna.event.tsv.sha256"]
    assert sha(out(cli, "pa", "--gpu-text", SP1)) == MANIFEST["sp1_dna.pa.tsv.sha256"]


def test_cli_gpu_text_really_fetches_text(cli):
    """the stage report counts the text bytes that came over PCIe: all of stdout but the header line"""
    env = dict(os.environ, SGK_CLI_TIMING="1")
    for tool in (["event", "-c"], ["event"], ["pa"]):
        p = subprocess.run([cli, *tool, "--gpu-text", SP1], capture_output=True, env=env)
        assert p.returncode == 0
        body = p.stdout.split(b"\n", 1)[1]
        assert b"--gpu-text: %d bytes of rows over PCIe" % len(body) in p.stderr, p.stderr[-600:]
        q = subprocess.run([cli, *tool, SP1], capture_output=True, env=env)
        assert q.stdout == p.stdout and b"--gpu-text" not in q.stderr


@pytest.mark.parametrize("name", list(MANIFEST["_synth_specs"]))
def test_cli_gpu_text_synthetic(cli, synth_files, name):
    f = synth_files[name]
    assert out(cli, "event", "-c", "--gpu-text", f) == gold(name + ".event_c.tsv")
    assert sha(out(cli, "event", "--gpu-text", f)) == MANIFEST[name + ".event.tsv.sha256"]


@pytest.mark.parametrize("name", list(MANIFEST["_synth_long_specs"]))
def test_cli_gpu_text_synthetic_long_reads(cli, synth_files, name):
    assert sha(out(cli, "event", "-c", "--gpu-text", synth_files[name])) == MANIFEST[name + ".event_c.tsv.sha256"]


def test_cli_gpu_text_read_id_mode_and_other_subtools_are_unchanged(cli):
    got = out(cli, "event", "--gpu-text", SP1, "05d90f17-f4a6-4349-924c-3ffd3457a99d")
    assert got.split(b"\n", 1)[1] == gold("event_dna.exp").split(b"\n", 1)[1]
    assert out(cli, "pa", "--gpu-text", SP1, "00011a60-dd92-4aad-be1d-59a33545ab1d", "0448591b-036c-4cc7-a702-6c542ccc07de",
               "03880e3d-b79d-4bd8-aab4-15724f1331af") == gold("sp1_dna.pa3.tsv")
    assert out(cli, "stat", "--gpu-text", SP1) == gold("sp1_dna.stat.tsv")
    assert out(cli, "jnn", "--gpu-text", SP1) == gold("sp1_dna.jnn.tsv")
    assert out(cli, "prefix", "--print-stat", "--gpu-text", SP1) == gold("sp1_dna.prefix_stat.tsv")


@pytest.mark.parametrize("extra", [["-n"], ["--batch-samples", "20000"], ["-t", "1"], ["--host-decode"], ["--host-inflate"]])
def test_cli_gpu_text_with_the_pipeline_options(cli, extra):
    cut = (lambda b: b.split(b"\n", 1)[1]) if extra == ["-n"] else (lambda b: b)
    assert out(cli, "event", "-c", "--gpu-text", *extra, SP1) == cut(gold("sp1_dna.event_c.tsv"))
    full = out(cli, "event", "--gpu-text", SP1)
    assert sha(full) == MANIFEST["sp1_dna.event.tsv.sha256"]
    assert out(cli, "event", "--gpu-text", *extra, SP1) == cut(full)
    full = out(cli, "pa", "--gpu-text", SP1)
    assert sha(full) == MANIFEST["sp1_dna.pa.tsv.sha256"]
    assert out(cli, "pa", "--gpu-text", *extra, SP1) == cut(full)


@pytest.mark.parametrize("rp,sp", [(0, 0), (1, 0), (0, 1)])
def test_cli_gpu_text_other_compression_layouts(cli, tmp_path, sp1, rp, sp):
    path = str(tmp_path / "x.blow5")
    blow5.write_blow5(path, sp1.reads, {"experiment_type": "genomic_dna", "sequencing_kit": "sqk-lsk109"}, rp, sp)
    assert out(cli, "event", "-c", "--gpu-text", path) == gold("sp1_dna.event_c.tsv")
    assert sha(out(cli, "event", "--gpu-text", path)) == MANIFEST["sp1_dna.event.tsv.sha256"]
    assert sha(out(cli, "pa", "--gpu-text", path)) == MANIFEST["sp1_dna.pa.tsv.sha256"]
