"""GPU: `ss paf2tsv` -- the CLI against the reference's recorded output for every fixture and batch budget, and the
library through the Python wrappers (sgk_ss_decode: pairs, status and ends bit for bit; sgk_ss_text_*: bytes and row
offsets, the capacity and workspace checks) against the Python model of tests/ss_model.py, which test_ss_cpu.py pins to
the reference."""
import os
import subprocess

import numpy as np
import pytest

import ss_model as M
from sigtk_amd import api, build

pytestmark = pytest.mark.gpu

CANARY = 0x5a5a5a5a


@pytest.fixture(scope="module")
def cli(gpu):
    path = build.CLI
    if not os.path.exists(path):
        build.build_lib()
        path = build.build_cli()
    return path


def ss(cli, path, *opts):
    return subprocess.run([cli, "ss", "paf2tsv", *[str(o) for o in opts], str(path)], capture_output=True, timeout=300)


def rec(ss_bytes, start_raw=0, st_k=0, rid=b"r", rna=False, tlen=None, end_raw=None, end_k=None):
    """a record whose columns agree with what the model makes of the string, unless end_raw / end_k say otherwise"""
    r = M.Record(rid, ss_bytes, start_raw, 0, st_k, st_k, 0)
    st, ends, _ = M.decode(r)
    e_raw = end_raw if end_raw is not None else (ends[0] if st in (0, 3, 4) else 0)
    e_k = end_k if end_k is not None else (ends[1] if st in (0, 3, 4) else st_k)
    tlen = e_k + 3 if tlen is None else tlen
    return M.Record(rid, ss_bytes, start_raw, e_raw, e_k if rna else st_k, st_k if rna else e_k, tlen)


def model_pairs(r, first, count):
    _, _, pairs = M.decode(r)
    out = np.full((count, 2), -1, dtype=np.int32)
    for j in range(count):
        p = pairs.get(r.st_k + first + j)
        if p is not None:
            out[j] = p
    return out


def check_decode(records, **kw):
    """pairs of every span with status 0, status and ends of every span, and the table outside the spans' ranges"""
    from sigtk_amd import device
    pairs, status, ends, b = device.ss_decode(records, gap=3, **kw)
    for s, sp in enumerate(b.spans_host):
        r = records[int(sp["record"])]
        st, e, _ = M.decode(r)
        assert int(status[s]) == st, (s, r.ss[:40], int(status[s]), st)
        assert tuple(int(x) for x in ends[s]) == tuple(e), (s, r.ss[:40], ends[s], e)
        if st == 0:
            assert np.array_equal(pairs[s], model_pairs(r, int(sp["first"]), int(sp["count"]))), (s, r.ss[:40])
    guard = b.table_filled == CANARY
    assert np.array_equal(b.table_after[guard], b.table_filled[guard]), "a store outside the spans' table ranges"
    return status


def string_of_length(rs, n):
    """a valid string of exactly n bytes: tokens of 1 - 4 digits (leading zeros included; one digit in front of a D)"""
    if n < 2:
        return b"7" * n       # one byte: a digit behind no op, which is ignored
    out = b""
    while n - len(out) > 6:
        op = bytes([rs.choice(list(b",,,,ID"))])
        d = 1 if op == b"D" else int(rs.randint(1, 5))
        out += b"%0*d" % (d, rs.randint(0, 10 ** d)) + op
    out += b"%0*d," % (n - len(out) - 1, rs.randint(0, 10))
    assert len(out) == n
    return out


# ------------------------------------------------------------------------------------------------ 1. the CLI

@pytest.mark.parametrize("name", sorted(M.FIXTURES))
def test_cli_equals_the_reference_for_every_batch_budget(cli, name):
    want_rc, want_err = M.FIXTURES[name]
    path = os.path.join(M.GOLDEN, name)
    for opts in ((), ("--batch", 1), ("--batch", 255), ("--batch", 256), ("--batch", 257)):
        p = ss(cli, path, *opts)
        assert p.returncode == want_rc, (opts, p.stderr[-400:])
        assert p.stdout == M.expected(name), opts
        if want_err is not None:
            assert p.stderr == want_err + b"\n"


def test_cli_one_row_per_batch(cli, tmp_path):
    rs = np.random.RandomState(3)
    lines = []
    for i, rows in enumerate((0, 1, 2, 40, 0, 17)):
        s, raw = M.random_ss(rs, rows, p_del=0.2)
        a, b = (5 + rows, 5) if i % 2 else (5, 5 + rows)
        lines.append(M.paf_line(b"read%d" % i, s, 9, 9 + raw, a, b, 20))
    f = tmp_path / "small.paf"
    f.write_bytes(b"".join(lines))
    want = M.paf2tsv(f.read_bytes())[0]
    for budget in (1, 2, 3, 1000):
        p = ss(cli, f, "--batch", budget)
        assert p.returncode == 0 and p.stdout == want, (budget, p.stderr[-300:])


def test_cli_million_row_deletion(cli, tmp_path):
    """8 bytes of string, 10^6 rows: the record is cut into spans over 16 batches"""
    f = tmp_path / "del.paf"
    f.write_bytes(M.paf_line(b"a", b"3,", 0, 3, 0, 1, 5) + M.paf_line(b"del", b"5,1000000D5,", 7, 17, 2000, 1002002, 1002002) +
                  M.paf_line(b"z", b"3,", 0, 3, 1, 0, 5))
    want = M.paf2tsv(f.read_bytes())[0]
    p = ss(cli, f, "--batch", 65536)
    assert p.returncode == 0 and p.stdout == want, p.stderr[-300:]


def test_cli_errors_outside_the_reference_domain(cli, tmp_path):
    good = M.paf_line(b"g", b"4,2D1,", 0, 5, 3000, 3004, 10)
    for line, word in ((M.paf_line(b"b", b"12345678901,", 0, 0, 0, 1, 1), M.MESSAGES[5]),
                       (M.paf_line(b"b", b"2147483647,1,", 0, 0, 0, 2, 1), M.MESSAGES[5]),
                       (b"\n", b"line 2: fewer than 12 fields")):
        f = tmp_path / "bad.paf"
        f.write_bytes(good + line + good)
        p = ss(cli, f)
        out, rc, err = M.paf2tsv(f.read_bytes())
        assert p.returncode == rc == 1 and p.stdout == out and word in p.stderr, p.stderr


# ------------------------------------------------------------------------------------------------ 2. sgk_ss_decode

def test_decode_every_length_and_alignment(gpu):
    rs = np.random.RandomState(11)
    records, aligns = [], []
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, 2049):
        for al in (range(16) if n in (0, 1, 16, 17, 1025) else (0, 5, 15)):
            s = string_of_length(rs, n)
            records.append(rec(s, start_raw=int(rs.randint(0, 1000)), st_k=int(rs.randint(0, 5000))))
            aligns.append(al)
    status = check_decode(records, aligns=aligns)
    assert not status.any()
    check_decode(records, aligns=aligns[::-1], max_span=100, cuts=[1, 255, 256, 257])


def test_decode_tokens_across_lanes_and_tiles(gpu):
    """a 10-digit number whose op is byte 0 of a lane / of a tile; a tile made only of I tokens"""
    records, aligns = [], []
    for op_at in (32, 1024, 2048, 33, 1029, 1039):
        for al in (0, 9):
            for num, op in ((b"2147480000", b"I"), (b"0000000123", b","), (b"0000000002", b"D")):
                n = op_at - 10 - al                            # the op sits at byte op_at of the aligned stream
                head = (b"0" if n % 2 else b"") + (b"1," * 2000)[:n - n % 2]
                records.append(rec(head + num + op + b"2,3D4,"))
                aligns.append(al)
    only_i = b"10I" * 400                                      # 1200 bytes: no ',' in the first tile, the carry crosses it
    records += [rec(only_i + b"5,6,"), rec(b"3," + only_i + b"5,", st_k=77), rec(only_i)]
    aligns += [0, 3, 0]
    assert not check_decode(records, aligns=aligns).any()


def test_decode_every_status(gpu):
    tile = b"12," * 400      # 1200 bytes
    records = [
        rec(b"5,3,"),                                          # 0
        rec(b"5,,3,"), rec(b",5,"), rec(b"5,I"),               # 1
        rec(b"5,x3,"), rec(b"5,3,\x01"), rec(b"5;"), rec(b"\x00"), rec(b"5,3, "),   # 2
        rec(b"5,3,", end_raw=9), rec(b"", end_raw=1),          # 3
        rec(b"5,3,", end_k=3), rec(b"", end_k=1),              # 4
        rec(b"5,3,", end_raw=9, end_k=3),                      # 3 comes before 4
        rec(b"12345678901,"), rec(b"00000000000,"), rec(b"5," + b"9" * 40 + b"I"),   # 5 by digit count
        rec(b"2147483648,"), rec(b"4294967296D"), rec(b"9999999999I"),              # 5 by value
        rec(b"2147483647,1,"), rec(b"2147483647D1,"), rec(b"1073741824I" * 2), rec(b"5,", start_raw=2147483647),
        rec(b"2147483647I" * 200),                             # 5 by running total, far above 2^32
        rec(b"2147483647,"),                                   # 0: INT32_MAX itself is fine
        # two byte errors in different tiles: the earlier one wins, both ways round
        rec(tile + b"7,,3," + tile + b"5x,"), rec(tile + b"5x," + tile + b"7,,3,"),
        rec(b",," + tile * 2 + b"x"), rec(b"x" + tile * 2 + b",,"),
        rec(tile + b"12345678901," + tile + b",,"),            # a byte error behind a number out of range: 1, not 5
    ]
    want = [M.decode(r)[0] for r in records]
    assert sorted(set(want)) == [0, 1, 2, 3, 4, 5]
    status = check_decode(records)
    assert status.tolist() == want
    from sigtk_amd import device
    _, st_v, ends_v, _ = device.ss_decode(records, validate=True)      # spans == NULL: one result per record
    assert st_v.tolist() == want
    assert [tuple(int(x) for x in e) for e in ends_v] == [tuple(M.decode(r)[1]) for r in records]
    big = [rec(b"2147483646D5,", tlen=0), rec(b"5,1000000D5,", st_k=2000)]      # rows by the billion: validated without a table
    _, st_v, ends_v, _ = device.ss_decode(big, validate=True, spans=np.zeros(0, dtype=api.SS_SPAN_DTYPE))
    assert st_v.tolist() == [0, 0] and ends_v.tolist() == [[5, 2147483647], [10, 1002002]]


def test_decode_never_stores_outside_a_span(gpu):
    """a string that maps more k-mers than end_k - st_k announces, in front of, inside and behind the spans"""
    rs = np.random.RandomState(5)
    s, raw = M.random_ss(rs, 3000)
    records = [M.Record(b"r", s, 0, raw, 10, 10 + n, 0) for n in (0, 1, 255, 256, 1000)]
    records.append(M.Record(b"r", s, 0, raw, 2000, 2300, 0))
    records.append(M.Record(b"r", b"5D" + s, 0, raw, 10, 500, 0))
    status = check_decode(records, max_span=300, cuts=[1, 255])
    assert set(status.tolist()) == {4}


# ------------------------------------------------------------------------------------------------ 3. sgk_ss_text_*

def text_records(rs, idl):
    rid = (b"0123456789abcdef" * 20)[:idl]
    out = []
    for i, rows in enumerate((0, 1, 255, 256, 257, 513)):
        s, raw = M.random_ss(rs, rows, p_del=0.1, max_del=3)
        out.append(rec(s, start_raw=int(rs.randint(0, 10 ** 6)), st_k=int(rs.randint(0, 10 ** 5)), rid=rid[:-1] + b"%d" % i,
                       rna=bool(i % 2), tlen=int(rs.randint(0, 10 ** 5))))
    out.append(rec(b"4,300D7,1I2,", start_raw=3, st_k=2 ** 31 - 400, rid=rid, tlen=-5))       # a D run across a tile
    out.append(rec(b"4,700D7,", st_k=5, rid=rid, rna=True, tlen=100))                        # ... and negative indices
    return out


@pytest.mark.parametrize("idl", [1, 36, 300])
def test_text_equals_the_model(gpu, idl):
    from sigtk_amd import device
    records = text_records(np.random.RandomState(idl), idl)
    for kw in (dict(), dict(max_span=256), dict(cuts=[1, 100, 255, 257, 400])):      # 400: a span starts inside the D runs
        t = device.SsText(records, **kw)
        text = t.run()
        want = []
        for sp in t.spans_host:
            r = records[int(sp["record"])]
            want.append(M.rows_text(r, M.decode(r)[2], int(sp["first"]), int(sp["count"])))
        offs = np.zeros(len(want) + 1, dtype=np.uint64)
        np.cumsum([len(w) for w in want], out=offs[1:])
        assert np.array_equal(t.row_offsets_host, offs)
        assert text == b"".join(want)
        assert {int(c) for c in t.spans_host["count"]} >= ({0, 1, 255, 256, 257, 513} if not kw else {0, 1})
    text2, offs2 = device.ss_text(records)
    assert text2 == b"".join(M.rows_text(r, M.decode(r)[2]) for r in records) and int(offs2[-1]) == len(text2)


def test_text_capacity_and_workspace_are_checked_on_the_device(gpu):
    import torch
    from sigtk_amd import device
    records = text_records(np.random.RandomState(2), 36)
    t = device.SsText(records)
    want = t.run()
    total = len(want)
    buf = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device=t.device)
    t.write(buf, total - 1)                       # one byte short
    rc, st = t.status_text()
    assert rc == api.SGK_ERR_CAPACITY and st.overflow == 1 and int(st.n_bytes) == total
    got = buf.cpu().numpy()
    assert (got[total - 1:] == 0xA5).all()        # nothing at or behind the capacity
    last_tile = int(t.row_offsets_host[-2])       # every tile that fits is written
    assert got[:last_tile].tobytes() == want[:last_tile]
    t.measure()                                   # (the status word is the workspace's: a new measure clears it)
    t.write(buf, total)
    rc, st = t.status_text()
    assert rc == api.SGK_OK and buf.cpu().numpy()[:total].tobytes() == want and (buf.cpu().numpy()[total:] == 0xA5).all()
    small = device.SsText(records * 4, rows_capacity=0)      # a workspace sized for a batch without rows
    small.measure()
    rc, st = small.status_text()
    assert rc == api.SGK_ERR_WORKSPACE
    small.write(buf, total)
    rc, st = small.status_text()
    assert rc == api.SGK_ERR_WORKSPACE and (buf.cpu().numpy()[total:] == 0xA5).all()
