"""GPU: BLOW5 records with variable-length auxiliary fields on the record path -- k_zrec_tail (sgk_zrec_tail_check) on
hand-built records, jobs staged with the header's column table (sgk_job_begin_zrec_aux), and the CLI on the reference's
bundled fixture, whose channel_number column is a `char*`: its records are decompressed on the GPU, a record whose array
outgrows its slack sends its batch to the host path, a record whose fields do not fill it ends the run."""
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from sigtk_amd import blow5, build

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SP1 = os.path.join(GOLDEN, "sp1_dna.blow5")
SP1_ZSTD = os.path.join(GOLDEN, "sp1_dna.zstd_svb.blow5")
SLACK = 256          # bytes of room per array column of a zlib record (the CLI's default)
CANARY = 64


# ---------------------------------------------------------------------------------------------- hand-built records

def field_bytes(col, value):
    """col = (elem_bytes, is_array); value: bytes of a fixed field, or (count, data bytes) of an array field"""
    if not col[1]:
        assert len(value) == col[0]
        return value
    count, data = value
    return struct.pack("<Q", count) + data


def shapes():
    """name -> (columns, values): the tails the issue lists, and 300 columns for the table that does not fit a launch"""
    rnd = np.random.RandomState(5)
    by = lambda n: rnd.randint(0, 256, n, dtype=np.uint8).tobytes()
    arr = lambda eb, k: (k, by(eb * k))
    out = {
        "none": ([], []),
        "fixed": ([(8, 0), (4, 0), (1, 0), (2, 0), (1, 0)], [by(8), by(4), by(1), by(2), by(1)]),
        "empty_array": ([(1, 1)], [arr(1, 0)]),
        "double3": ([(8, 1)], [arr(8, 3)]),
    }
    for k in (1, 255, 256, 257):
        out["bytes%d" % k] = ([(1, 1)], [arr(1, k)])
    cols, vals = [], []
    for c in range(40):        # every element size, fixed and array, arrays of 0 - 4 elements; the last column an array
        eb = (1, 2, 4, 8)[c % 4]
        is_arr = 1 if c % 3 != 0 or c == 39 else 0
        cols.append((eb, is_arr))
        vals.append(arr(eb, c % 5) if is_arr else by(eb))
    out["forty"] = (cols, vals)
    cols = [((1, 2, 4, 8)[c % 4], 1 if c % 7 == 6 or c == 299 else 0) for c in range(300)]
    out["threehundred"] = (cols, [arr(eb, 2) if a else by(eb) for eb, a in cols])
    return out


def variants(cols, vals):
    """-> list of (tag, tail bytes, bytes cut off the WHOLE record's end, expected status) for one shape.  The exact
    record: 0; its last byte dropped: 2 (a field is cut) -- with no column the byte is the signal's, which is status 1;
    one more byte: 3; and where the shape has an array, in its last array: a count one too large (the data would end
    behind the record): 2, the largest 32-bit count: 2 for 1-byte elements (it fits 32 bits and overruns) and 4 for wider
    ones, a count of 2^61: 4 (with 8-byte elements the product is 0 modulo 2^64)."""
    tail = b"".join(field_bytes(c, v) for c, v in zip(cols, vals))
    out = [("exact", tail, 0, 0), ("short", tail, 1, 2 if cols else 1), ("long", tail + b"\x5a", 0, 3)]
    last = max([k for k, c in enumerate(cols) if c[1]], default=None)
    if last is not None:
        def with_count(n):
            v = list(vals)
            v[last] = (n, vals[last][1])
            return b"".join(field_bytes(c, x) for c, x in zip(cols, v))
        eb = cols[last][0]
        out.append(("count+1", with_count(vals[last][0] + 1), 0, 2))
        out.append(("count32", with_count(0xffffffff), 0, 2 if eb == 1 else 4))
        out.append(("count61", with_count(1 << 61), 0, 4))
        if eb == 8:    # 2^29 elements of 8 bytes are 2^32 bytes: the first count that does not fit; one fewer fits and overruns
            out.append(("count29", with_count(1 << 29), 0, 4))
            out.append(("count29-1", with_count((1 << 29) - 1), 0, 2))
        # the record ends inside the last array's count word
        upto = b"".join(field_bytes(c, x) for c, x in zip(cols[:last], vals[:last]))
        out.append(("cut_count", upto + struct.pack("<Q", vals[last][0])[:5], 0, 2))
    return out


def head_and_signal(n_samples, k):
    rid = ("read-%03d" % k).encode()[: 4 + k % 6]
    raw = np.arange(n_samples, dtype=np.int16) + 300
    sig = blow5.svb_zd_encode(raw)
    return struct.pack("<H", len(rid)) + rid + struct.pack("<IddddQ", 0, 8192.0, 3.0, 1400.0, 4000.0, len(sig)) + sig


@pytest.fixture(scope="module")
def tail_cases():
    """-> list of (name, columns, records): records = list of (tag, record bytes, tail offset, expected status)"""
    cases = []
    k = 0
    for name, (cols, vals) in shapes().items():
        recs = []
        for n_samples in (0, 1):
            for tag, tail, cut, want in variants(cols, vals):
                hs = head_and_signal(n_samples, k)
                k += 1
                rec = hs + tail
                recs.append(("%s/%d" % (tag, n_samples), rec[:len(rec) - cut], len(hs), want))
            hs = head_and_signal(n_samples, k)
            recs.append(("in_signal/%d" % n_samples, (hs + b"".join(field_bytes(c, v) for c, v in zip(cols, vals)))[:len(hs) - 2], len(hs), 1))
            recs.append(("nothing/%d" % n_samples, b"", len(hs), 1))
        cases.append((name, cols, recs))
    return cases


def layout(recs, shift):
    """the records back to back at odd byte offsets, 64 canary bytes (and 1 - 8 more) behind each -> (buffer, offsets)"""
    offs, pos, chunks = [], shift, [b"\xa5" * shift]
    for k, (_, rec, _, _) in enumerate(recs):
        offs.append(pos)
        pad = 1 + (k * 3) % 8
        chunks.append(rec + b"\xa5" * (CANARY + pad))
        pos += len(rec) + CANARY + pad
    return np.frombuffer(b"".join(chunks), dtype=np.uint8).copy(), offs


def run_tail_check(gpu, cols, recs, shift):
    import torch
    from sigtk_amd import device
    buf, offs = layout(recs, shift)
    dev = torch.device("cuda", 0)
    d_buf = torch.from_numpy(buf).to(dev)
    d_off = torch.from_numpy(np.asarray(offs, dtype=np.uint64).view(np.int64)).to(dev)
    d_len = torch.from_numpy(np.asarray([len(r[1]) for r in recs], dtype=np.uint32).view(np.int32)).to(dev)
    d_tail = torch.from_numpy(np.asarray([r[2] for r in recs], dtype=np.uint32).view(np.int32)).to(dev)
    st = device.zrec_tail_check(d_buf, d_off, d_len, d_tail, cols)
    torch.cuda.synchronize()
    assert np.array_equal(d_buf.cpu().numpy(), buf), "the kernel writes only status"
    return st.cpu().numpy()[:len(recs)], {o % 8 for o in offs}


@pytest.mark.parametrize("shift", [0, 5])
def test_tail_check_on_hand_built_records(gpu, tail_cases, shift):
    n_total = 0
    residues = set()
    for name, cols, recs in tail_cases:
        got, res = run_tail_check(gpu, cols, recs, shift)
        residues |= res
        n_total += len(recs)
        bad = [(name, tag, int(g), want) for (tag, _, _, want), g in zip(recs, got) if int(g) != want]
        assert not bad, bad[:10]
    assert residues == set(range(8)) and n_total > 100
    assert {c[0] for c in tail_cases} >= {"none", "fixed", "empty_array", "bytes1", "bytes255", "bytes256", "bytes257", "double3", "forty"}
    assert len(dict((c[0], c[1]) for c in tail_cases)["forty"]) == 40


def test_tail_check_more_records_than_one_workgroup(gpu, tail_cases):
    """600 records in one launch (three workgroups of 256 lanes, the last one partly empty)"""
    name, cols, recs = next(c for c in tail_cases if c[0] == "forty")
    many = [recs[k % len(recs)] for k in range(600)]
    got, _ = run_tail_check(gpu, cols, many, 3)
    assert [int(g) for g in got] == [r[3] for r in many]


def test_tail_check_refuses_a_bad_table(gpu):
    import torch
    from sigtk_amd import api, device
    dev = torch.device("cuda", 0)
    z8 = torch.zeros(16, dtype=torch.uint8, device=dev)
    z64, z32 = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    for cols in ([(3, 0)], [(0, 1)], [(16, 0)], [(8, 1), (5, 1)]):
        with pytest.raises(api.SigtkGpuError):
            device.zrec_tail_check(z8, z64, z32, z32, cols)


# ---------------------------------------------------------------------------------------------- jobs

def file_records(path):
    """the on-disk records of a BLOW5 file"""
    buf = open(path, "rb").read()
    (hsize,) = struct.unpack_from("<I", buf, 64)
    pos, recs = 68 + hsize, []
    while buf[pos:pos + 5] != b"5WOLB" or pos + 5 != len(buf):
        (size,) = struct.unpack_from("<Q", buf, pos)
        recs.append(buf[pos + 8:pos + 8 + size])
        pos += 8 + size
    return recs


def header_table(path):
    """the auxiliary columns of a file as the host reader parses them: [(elem_bytes, is_array)]"""
    p = subprocess.run([build.CLI, "_dump", "--aux", path], capture_output=True)
    assert p.returncode == 0
    f = p.stdout.decode().split()
    assert f[0] == "#aux" and f[1] != "none" and int(f[1]) == len(f) - 2
    return [(int(x.rstrip("*")), 1 if x.endswith("*") else 0) for x in f[2:]]


def zlib_room(sig_end, table, slack=SLACK):
    return sig_end + sum(eb for eb, a in table if not a) + sum(8 + slack for eb, a in table if a)


def zstd_content_size(frame):
    """Frame_Content_Size of a zstd frame header (RFC 8878 3.1.1.1)"""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    d = frame[4]
    single, fcs_flag, dict_flag = (d >> 5) & 1, d >> 6, d & 3
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[dict_flag]
    n = (1 if single else 0, 2, 4, 8)[fcs_flag]
    assert n
    return int.from_bytes(frame[pos:pos + n], "little") + (256 if n == 2 else 0)


def signal_place(plain):
    (idl,) = struct.unpack_from("<H", plain, 0)
    (ln,) = struct.unpack_from("<Q", plain, 2 + idl + 36)
    return 2 + idl + 44, ln


@pytest.fixture(scope="module")
def sp1_job(gpu, sp1):
    """the first 24 records of sp1_dna.blow5 and what an int16 job gives for them, computed once"""
    n = 24
    reads = sp1.reads[:n]
    plain = [zlib.decompress(r) for r in file_records(SP1)[:n]]
    place = [signal_place(p) for p in plain]
    scal = ([r.digitisation for r in reads], [r.offset for r in reads], [r.range for r in reads])
    job = gpu.Job(0)
    job.stage([r.raw for r in reads], *scal)
    want = {}
    job.launch(gpu.TOOL_STAT)
    want["stat"] = job.wait()["stat"].tobytes()
    job.launch(gpu.TOOL_PA)
    want["pa"] = [p.copy() for p in job.wait()["pa"]]
    job.launch(gpu.TOOL_EVENT)
    want["events"] = [(e.start.copy(), e.length.copy(), e.mean.copy(), e.stdv.copy()) for e in job.wait()["events"]]
    job.close()
    return {"n": n, "reads": reads, "plain": plain, "place": place, "scal": scal, "want": want,
            "lengths": [r.raw.size for r in reads], "table": header_table(SP1)}


def check_results(gpu, job, want):
    job.launch(gpu.TOOL_STAT)
    assert job.wait()["stat"].tobytes() == want["stat"]
    job.launch(gpu.TOOL_PA)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(job.wait()["pa"], want["pa"]))
    job.launch(gpu.TOOL_EVENT)
    got = job.wait()["events"]
    assert len(got) == len(want["events"])
    for e, (s, l, m, d) in zip(got, want["events"]):
        assert np.array_equal(e.start, s) and np.array_equal(e.length, l)
        assert np.array_equal(e.mean.view(np.uint32), m.view(np.uint32)) and np.array_equal(e.stdv.view(np.uint32), d.view(np.uint32))


def test_zlib_records_with_the_headers_table(gpu, sp1_job):
    j = sp1_job
    assert j["table"] == [(8, 0), (4, 0), (1, 0), (8, 0), (1, 0), (1, 1)]
    recs = file_records(SP1)[:j["n"]]
    room = [zlib_room(o + ln, j["table"]) for o, ln in j["place"]]
    assert all(len(p) < r for p, r in zip(j["plain"], room))      # (slack: the room is an upper bound)
    job = gpu.Job(0)
    job.stage_zrec(recs, j["lengths"], [o for o, _ in j["place"]], [ln for _, ln in j["place"]], room, *j["scal"], aux=j["table"])
    check_results(gpu, job, j["want"])
    job.close()


def test_zstd_records_with_exact_room(gpu, sp1_job):
    j = sp1_job
    assert header_table(SP1_ZSTD) == j["table"]
    frames = file_records(SP1_ZSTD)[:j["n"]]
    room = [zstd_content_size(f) for f in frames]
    assert room == [len(p) for p in j["plain"]]
    job = gpu.Job(0)
    job.stage_zrec(frames, j["lengths"], [o for o, _ in j["place"]], [ln for _, ln in j["place"]], room, *j["scal"],
                   record_format=gpu.RECORD_ZSTD, aux=j["table"])
    check_results(gpu, job, j["want"])
    job.close()


def relengthen(plain, table, new_string=None, drop=0):
    """the record with its channel_number (the last column, a char*) replaced and `drop` bytes cut off its end"""
    assert table[-1] == (1, 1)
    o, ln = signal_place(plain)
    fixed = sum(eb for eb, a in table[:-1])
    at = o + ln + fixed
    (count,) = struct.unpack_from("<Q", plain, at)
    assert at + 8 + count == len(plain)
    if new_string is not None:
        plain = plain[:at] + struct.pack("<Q", len(new_string)) + new_string
    return plain[:len(plain) - drop]


def test_a_long_array_and_a_cut_record_get_their_own_status(gpu, sp1_job):
    j = sp1_job
    recs = file_records(SP1)[:j["n"]]
    sig_off, sig_len = [o for o, _ in j["place"]], [ln for _, ln in j["place"]]
    room = [zlib_room(o + ln, j["table"]) for o, ln in j["place"]]
    job = gpu.Job(0)
    # record 5 with a 300-byte string: more than its room (8 + 256 bytes for the column) -> 0x108, for that read only
    long_rec = list(recs)
    long_rec[5] = zlib.compress(relengthen(j["plain"][5], j["table"], b"c" * 300))
    job.stage_zrec(long_rec, j["lengths"], sig_off, sig_len, room, *j["scal"], aux=j["table"])
    job.launch(gpu.TOOL_STAT)
    rc, ds = job.wait_rc()
    assert rc == gpu.SGK_ERR_FORMAT and [int(x) for x in ds] == [0x108 if r == 5 else 0 for r in range(j["n"])]
    # the same record, room to spare, its last byte dropped before deflating: it inflates, its fields do not fill it
    cut_rec = list(recs)
    cut_rec[5] = zlib.compress(relengthen(j["plain"][5], j["table"], b"c" * 300, drop=1))
    big = list(room)
    big[5] += 1000
    job.stage_zrec(cut_rec, j["lengths"], sig_off, sig_len, big, *j["scal"], aux=j["table"])
    job.launch(gpu.TOOL_STAT)
    rc, ds = job.wait_rc()
    assert rc == gpu.SGK_ERR_FORMAT and [int(x) for x in ds] == [0x400 | 2 if r == 5 else 0 for r in range(j["n"])]
    # with that room the whole long record is fine, and a byte too many behind it is 0x400 | 3
    long_rec[5] = zlib.compress(relengthen(j["plain"][5], j["table"], b"c" * 300))
    job.stage_zrec(long_rec, j["lengths"], sig_off, sig_len, big, *j["scal"], aux=j["table"])
    check_results(gpu, job, j["want"])
    long_rec[5] = zlib.compress(relengthen(j["plain"][5], j["table"], b"c" * 300) + b"\x00")
    job.stage_zrec(long_rec, j["lengths"], sig_off, sig_len, big, *j["scal"], aux=j["table"])
    job.launch(gpu.TOOL_STAT)
    rc, ds = job.wait_rc()
    assert rc == gpu.SGK_ERR_FORMAT and [int(x) for x in ds] == [0x400 | 3 if r == 5 else 0 for r in range(j["n"])]
    # the begin without a table keeps its behaviour: the same staging is not checked against any column
    job.stage_zrec(long_rec, j["lengths"], sig_off, sig_len, big, *j["scal"])
    job.launch(gpu.TOOL_STAT)
    assert job.wait()["stat"].tobytes() == j["want"]["stat"]
    job.close()


# ---------------------------------------------------------------------------------------------- CLI

@pytest.fixture(scope="module")
def cli(gpu):
    assert os.path.exists(build.CLI), "sigtk-amd not built (run __graft_entry__.build())"
    return build.CLI


def run_timed(cli, *args):
    p = subprocess.run([cli, *args], capture_output=True, env=dict(os.environ, SGK_CLI_TIMING="1"))
    return p.returncode, p.stdout, p.stderr.decode(errors="replace")


def path_counts(stderr):
    m = re.search(r"records decompressed on the GPU: (\d+) of (\d+); batches redone on the host: (\d+)", stderr)
    assert m, stderr[-1500:]
    return tuple(int(x) for x in m.groups())


def gold(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


@pytest.mark.parametrize("path", [SP1, SP1_ZSTD], ids=["zlib", "zstd"])
@pytest.mark.parametrize("tool,golden", [(["stat"], "sp1_dna.stat.tsv"), (["event", "-c"], "sp1_dna.event_c.tsv")], ids=["stat", "event_c"])
def test_cli_takes_the_record_path_for_the_bundled_fixture(cli, path, tool, golden):
    rc, out, err = run_timed(cli, *tool, path)
    assert rc == 0, err[-1500:]
    assert out == gold(golden)
    assert "records decompressed on the GPU: 100 of 100; batches redone on the host: 0" in err


def test_cli_without_the_timing_variable_prints_nothing_new(cli):
    p = subprocess.run([cli, "stat", SP1], capture_output=True, env={k: v for k, v in os.environ.items() if k != "SGK_CLI_TIMING"})
    assert p.returncode == 0 and p.stdout == gold("sp1_dna.stat.tsv") and b"records decompressed" not in p.stderr


def test_cli_without_slack_redoes_its_batches_on_the_host(cli):
    rc, out, err = run_timed(cli, "stat", "--aux-slack", "0", "--batch-samples", "150000", SP1)
    assert rc == 0, err[-1500:]
    assert out == gold("sp1_dna.stat.tsv")
    on_gpu, total, redone = path_counts(err)
    assert total == 100 and redone >= 1 and on_gpu < 100
    rc, out, err = run_timed(cli, "event", "-c", "--gpu-text", "--aux-slack", "0", "--batch-samples", "150000", SP1)
    assert rc == 0 and out == gold("sp1_dna.event_c.tsv") and path_counts(err)[2] >= 1


def test_cli_redoes_the_one_batch_with_a_long_string(cli, sp1, tmp_path):
    reads = sp1.reads[:12]
    with_aux = [blow5.Read(r.read_id, r.read_group, r.digitisation, r.offset, r.range, r.sampling_rate, r.raw,
                           aux=(b"x" * 300 if i == 7 else b"%d" % (100 + i), 7 + i)) for i, r in enumerate(reads)]
    path = str(tmp_path / "long.blow5")
    blow5.write_blow5(path, with_aux, {a: sp1.attr(a) for a in sp1.attrs}, aux_types=[("channel_number", "char*"), ("start_time", "uint64_t")])
    rc, want, err = run_timed(cli, "stat", "--host-inflate", path)
    assert rc == 0 and want.count(b"\n") == 13 and path_counts(err) == (0, 12, 0)
    rc, out, err = run_timed(cli, "stat", path)
    assert rc == 0, err[-1500:]
    assert out == want and path_counts(err) == (0, 12, 1)
    # the same reads with short strings only: no batch is redone
    short = [blow5.Read(r.read_id, r.read_group, r.digitisation, r.offset, r.range, r.sampling_rate, r.raw, aux=(b"12", r.aux[1]))
             for r in with_aux]
    blow5.write_blow5(path, short, {a: sp1.attr(a) for a in sp1.attrs}, aux_types=[("channel_number", "char*"), ("start_time", "uint64_t")])
    rc, out, err = run_timed(cli, "stat", path)
    assert rc == 0 and out == want and path_counts(err) == (12, 12, 0)


def test_cli_a_record_that_does_not_fill_its_fields_ends_the_run(cli, tmp_path):
    """sp1_dna.blow5 with its fourth record re-deflated one tail byte short (the u64 size in front fixed up)"""
    src = open(SP1, "rb").read()
    (hsize,) = struct.unpack_from("<I", src, 64)
    pos = 68 + hsize
    for _ in range(3):
        pos += 8 + struct.unpack_from("<Q", src, pos)[0]
    (size,) = struct.unpack_from("<Q", src, pos)
    rec = zlib.compress(zlib.decompress(src[pos + 8:pos + 8 + size])[:-1])
    path = str(tmp_path / "cut.blow5")
    open(path, "wb").write(src[:pos] + struct.pack("<Q", len(rec)) + rec + src[pos + 8 + size:])
    rc, out, err = run_timed(cli, "stat", path)
    assert rc == 1 and "Error in slow5_get_next" in err, (rc, err[-500:])
