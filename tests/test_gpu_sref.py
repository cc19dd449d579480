"""GPU: `sref` -- the CLI against the reference's recorded output for every fixture, batch budget and input form; the
library through the Python wrappers (float bits, span seams, row offsets, the capacity check, a hostile model); one large
case against the numpy model of tests/sref_model.py; the live reference on a slice when it has been built."""
import gzip
import hashlib
import os
import subprocess

import numpy as np
import pytest

import sref_model as M
from sigtk_amd import build

pytestmark = pytest.mark.gpu

REF = os.path.join(M.ROOT, "oracle", "_ref", "sigtk_ref")


@pytest.fixture(scope="module")
def cli(gpu):
    path = build.CLI
    if not os.path.exists(path):
        build.build_lib()
        path = build.build_cli()
    return path


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """model files written from the de Bruijn goldens, k-mers in shuffled order"""
    d = tmp_path_factory.mktemp("models")
    return {k: M.write_model(d / ("k%d.model" % k), M.golden_levels(k), k, order=np.random.RandomState(k).permutation(4 ** k))
            for k in (6, 5)}


def sref(cli, models, path, *opts, rna=False):
    args = [cli, "sref", "--kmer-model", models[5 if rna else 6], *(["--rna"] if rna else []), *[str(o) for o in opts], str(path)]
    p = subprocess.run(args, capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr[-600:]
    return p.stdout


def records(name):
    return M.parse_fasta(M.golden(name))


def span_texts(recs, levels, k, rna, spans):
    """the text of every span, from the numpy model: the row head if first == 0, every value followed by ',' or, for the
    row's last one, by the line end"""
    table = [b"%f" % float(v) for v in np.asarray(levels, dtype=np.float32)]
    out, cache = [], {}
    for sp in spans:
        name, seq = recs[int(sp["seq"])]
        strand, first, count = int(sp["strand"]), int(sp["first"]), int(sp["count"])
        n = len(seq) + 1 - k
        key = (int(sp["seq"]), strand)
        if key not in cache:
            cache.clear()
            cache[key] = M.ranks(seq, k, strand)
        r = cache[key][first:first + count].tolist()
        t = b"".join(table[x] + b"," for x in r)
        if count and first + count == n:
            t = t[:-1] + b"\n"
        if first == 0:
            t = b"%s\t%d\t%s\t%d\t" % (name, len(seq), b"-" if strand else b"+", n) + t
        out.append(t)
    return out


# ------------------------------------------------------------------------------------------------ 1. the CLI

@pytest.mark.parametrize("out", sorted(M.FIXTURES))
def test_cli_equals_the_reference_for_every_batch_budget(cli, models, tmp_path, out):
    src, opts = M.FIXTURES[out]
    rna = "--rna" in opts
    extra = [o for o in opts if o != "--rna"]
    want = M.golden(out)
    path = os.path.join(M.GOLDEN, src)
    assert sref(cli, models, path, *extra, rna=rna) == want
    small = src in ("sref_edge.fa", "sref_crlf.fa")
    for budget in ([1, 2, 3] if small else []) + [7 if small else 97, 255, 256, 257, 512, 1000]:   # rows cut many times
        assert sref(cli, models, path, "--batch", budget, *extra, rna=rna) == want, budget
    gz = tmp_path / (src + ".gz")
    gz.write_bytes(gzip.compress(M.golden(src)))
    assert sref(cli, models, gz, *extra, rna=rna) == want
    assert sref(cli, models, gz, "--batch", 300, *extra, rna=rna) == want


def test_cli_long_names_and_many_records(cli, models, tmp_path):
    """names longer than a tile's LDS image (the tile is written straight to global memory) and more records than a
    batch takes spans"""
    rs = np.random.RandomState(12)
    recs = [(b"n" * 9000 + b"%d" % i, bytes(rs.choice(list(b"ACGT"), size=int(n)).astype(np.uint8)))
            for i, n in enumerate([300, 5, 0, 700])]
    recs += [(b"s%d" % i, bytes(rs.choice(list(b"ACGTN"), size=int(rs.randint(0, 40))).astype(np.uint8))) for i in range(3000)]
    fa = tmp_path / "names.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % r for r in recs))
    levels = M.golden_levels(6)
    want = M.sref_text(recs, levels, 6)
    assert sref(cli, models, fa) == want
    assert sref(cli, models, fa, "--batch", 333) == want


# ------------------------------------------------------------------------------------------------ 2. the library

@pytest.mark.parametrize("out", ["sref_edge.dna.tsv", "sref_edge.rna.tsv", "sref_crlf.dna.tsv", "sref_multi.dna.tsv",
                                 "sref_multi.rna.tsv", "sref_db6.dna.tsv", "sref_db5.rna.tsv"])
def test_levels_and_text_through_the_python_api(gpu, out):
    from sigtk_amd import device
    src, opts = M.FIXTURES[out]
    rna = "--rna" in opts
    k = 5 if rna else 6
    levels = M.golden_levels(k)
    recs = records(src)
    seqs, names = [s for _, s in recs], [n for n, _ in recs]
    body = M.golden(out)[len(M.HEADER):]
    rows = M.rows_of(M.golden(out))
    want_rows = [np.array([float(v) for v in r[4]], dtype=np.float32) for r in rows]
    rs = np.random.RandomState(7)
    longest = max(len(s) for s in seqs)
    for kw in (dict(), dict(max_span=1), dict(max_span=255), dict(max_span=256), dict(max_span=257),
               dict(cuts=[1, 255, 256, 257]), dict(cuts=sorted(rs.randint(1, longest, size=12).tolist())),
               dict(max_span=1000, cuts=sorted(rs.randint(1, longest, size=5).tolist()))):
        if kw.get("max_span") == 1 and longest > 600:
            continue
        got_rows = device.sref_levels(seqs, levels, k, rna, **kw)
        assert len(got_rows) == len(want_rows)
        for g, w in zip(got_rows, want_rows):
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), kw
        for lds in (False, True):
            w = device.SrefText(seqs, names, levels, k, rna, table_in_lds=lds, **kw)
            text = w.run()
            assert text == body, (kw, lds)
            texts = span_texts(recs, levels, k, rna, w.spans_host)
            offs = np.zeros(len(texts) + 1, dtype=np.uint64)
            np.cumsum([len(t) for t in texts], out=offs[1:])
            assert np.array_equal(w.row_offsets_host, offs), (kw, lds)     # row_offsets are exact
            for s in range(0, len(texts), max(1, len(texts) // 50)):
                assert text[int(offs[s]):int(offs[s + 1])] == texts[s]
            rc, st = w.status()
            assert rc == 0 and st.n_bytes == len(body) and st.overflow == 0


@pytest.mark.parametrize("lds", [False, True])
def test_capacity_is_checked_on_the_device(gpu, lds):
    import torch
    from sigtk_amd import api, device
    recs = records("sref_multi.fa")
    levels = M.golden_levels(6)
    body = M.golden("sref_multi.dna.tsv")[len(M.HEADER):]
    w = device.SrefText([s for _, s in recs], [n for n, _ in recs], levels, 6, max_span=700, table_in_lds=lds)
    w.measure()
    torch.cuda.synchronize()
    total = int(w.row_offsets.cpu().numpy().astype(np.uint64)[-1])
    assert total == len(body)
    for short in (1, 2000, total):
        text = torch.full((total + 256,), 0xAB, dtype=torch.uint8, device=w.device)
        w.measure()
        w.write(text, total - short)
        rc, st = w.status()
        assert rc == api.SGK_ERR_CAPACITY and st.overflow == 1 and st.n_bytes == total
        host = text.cpu().numpy()
        assert (host[total - short:] == 0xAB).all(), "bytes behind the capacity were written"
        # what was written is right: a tile that fits is whole, a tile that does not is untouched
        done = host[:total - short] != 0xAB
        assert np.array_equal(host[:total - short][done], np.frombuffer(body, dtype=np.uint8)[:total - short][done])
    text = torch.full((total + 256,), 0xAB, dtype=torch.uint8, device=w.device)
    w.measure()
    w.write(text[3:], total)                      # exact capacity at an odd address
    rc, st = w.status()
    assert rc == 0 and text[3:3 + total].cpu().numpy().tobytes() == body
    assert (text[3 + total:].cpu().numpy() == 0xAB).all() and (text[:3].cpu().numpy() == 0xAB).all()


def hostile_levels(k):
    """any float may be in a user's model: texts longer than a table entry take the general formatter (tiles larger than
    their LDS image: test_long_numbers_overflow_the_tile_image).  Only values whose '%f' glibc and Python print alike (Python drops the sign of a NaN)."""
    rs = np.random.RandomState(99)
    v = M.golden_levels(k).copy()
    special = np.array([0.0, -0.0, 1e-7, -1e-7, -123456.789, 3.4e38, -3.4e38, np.finfo(np.float32).max, 1e15, 9.99999e14,
                        99999999.0, 100000000.0, -99999999.5, 1e-45, -1e-45, 1.1754942e-38, np.inf, -np.inf, np.nan,
                        0.0000005, 0.9999995, 1.0000005, 123456792.0, -1.5], dtype=np.float32)
    idx = rs.permutation(4 ** k)
    v[idx[:special.size]] = special
    v[idx[special.size:special.size + 4 ** k // 4]] = (rs.standard_normal(4 ** k // 4) * 1e30).astype(np.float32)   # long texts
    return v


@pytest.mark.parametrize("k,rna", [(6, False), (5, True), (3, False), (1, False)])
def test_a_hostile_model(gpu, k, rna):
    from sigtk_amd import device
    levels = hostile_levels(k) if k >= 5 else np.array([3.4e38, -0.0, np.inf, 1e-7] * (4 ** k // 4), dtype=np.float32)
    recs = records("sref_multi.fa") + records("sref_edge.fa") + records("sref_db%d.fa" % (5 if rna else 6))
    seqs, names = [s for _, s in recs], [n for n, _ in recs]
    want = M.sref_text(recs, levels, k, rna, header=False)
    if k >= 5:
        assert b"inf," in want and b"-inf" in want and b"nan" in want and b"-0.000000" in want and b"0.000000," in want
        assert b"340282346638528859811704183484516925440.000000" in want
    for kw in (dict(), dict(max_span=257), dict(table_in_lds=True), dict(table_in_lds=True, max_span=100)):
        assert device.SrefText(seqs, names, levels, k, rna, **kw).run() == want, kw
    got = device.sref_levels(seqs, levels, k, rna, max_span=1000)
    want_bits = [levels[M.ranks(s, k, strand)].view(np.uint32) for s in seqs for strand in ((0,) if rna else (0, 1))]
    assert len(got) == len(want_bits)
    for g, w in zip(got, want_bits):
        assert np.array_equal(g.view(np.uint32), w)


@pytest.mark.parametrize("k", [1, 3])
def test_long_numbers_overflow_the_tile_image(gpu, k):
    """every level's text is longer than a table entry (39 - 47 characters), so whole tiles of 256 values exceed the
    8 KB LDS image and are formatted straight into global memory -- head tiles and tiles in the middle of a row"""
    from sigtk_amd import device
    rs = np.random.RandomState(k)
    levels = np.array([3.4e38, -3.4e38, 1e30, -1.5e30] * (4 ** k // 4), dtype=np.float32)
    levels[rs.randint(0, 4 ** k)] = np.finfo(np.float32).max
    recs = [(b"run", b"T" * 700), (b"random", bytes(rs.choice(list(b"ACGTN"), size=1500).astype(np.uint8))), (b"short", b"ACGTA")]
    seqs, names = [s for _, s in recs], [n for n, _ in recs]
    want = M.sref_text(recs, levels, k, header=False)
    tile_bytes = [sum(len(v) + 1 for v in row[4][j:j + 256]) for row in M.rows_of(want, header=False)
                  for j in range(0, len(row[4]), 256)]
    assert sum(b > 8192 for b in tile_bytes) >= 10 and max(tile_bytes) > 11000    # (the image holds 8 192 bytes)
    for kw in (dict(), dict(max_span=255), dict(max_span=256), dict(max_span=257), dict(cuts=[300, 301, 1000])):
        for lds in (False, True):
            assert device.SrefText(seqs, names, levels, k, table_in_lds=lds, **kw).run() == want, (kw, lds)


# ------------------------------------------------------------------------------------------------ 3. large cases

def random_fasta(path, rs, long_len, n_short):
    def seq(n):
        s = rs.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)
        for _ in range(max(1, n // 400000)):
            if n > 200:
                lo = int(rs.randint(0, n - 100))
                s[lo:lo + int(rs.randint(1, min(n - lo, 5000)))] = ord("N")
        return s.tobytes()
    recs = [(b"chrL", seq(long_len))] + [(b"s%d" % i, seq(int(rs.randint(0, 600)))) for i in range(n_short)]
    with open(path, "wb") as f:
        for name, s in recs:
            f.write(b">" + name + b" random\n")
            for i in range(0, len(s), 80):
                f.write(s[i:i + 80] + b"\n")
    return recs


def test_large_case_against_the_numpy_model(cli, models, tmp_path):
    recs = random_fasta(tmp_path / "big.fa", np.random.RandomState(2025), 3000000, 2000)
    for rna in (False, True):
        want = hashlib.sha256(M.sref_text(recs, M.golden_levels(5 if rna else 6), 5 if rna else 6, rna)).hexdigest()
        assert hashlib.sha256(sref(cli, models, tmp_path / "big.fa", rna=rna)).hexdigest() == want
        assert hashlib.sha256(sref(cli, models, tmp_path / "big.fa", "--batch", 1000003, rna=rna)).hexdigest() == want


def test_against_the_live_reference(cli, models, tmp_path):
    """the reference itself on the same file (it is quadratic in the sequence length: 2e5 bases); runs wherever
    oracle/_ref/sigtk_ref has been built"""
    if not os.path.exists(REF):
        pytest.skip("the reference has not been built (oracle.build(ref=True))")
    random_fasta(tmp_path / "slice.fa", np.random.RandomState(31), 200000, 300)
    for rna in (False, True):
        p = subprocess.run([REF, "sref", *(["--rna"] if rna else []), str(tmp_path / "slice.fa")], stdout=subprocess.PIPE,
                           stderr=subprocess.DEVNULL, timeout=900)
        assert p.returncode == 0
        assert sref(cli, models, tmp_path / "slice.fa", rna=rna) == p.stdout
        assert sref(cli, models, tmp_path / "slice.fa", "--batch", 65537, rna=rna) == p.stdout
