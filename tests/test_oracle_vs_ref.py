"""CPU: the oracle restatement against the REAL reference, function by function on seeded inputs.

What the reference (oracle/_ref/libsigtk_ref.so, compiled from its sources by oracle/Makefile) returns on these
inputs is stored in tests/golden/ref_vectors.json: every array as the SHA-256 of its bytes, scalars as they are
(float32 as their bit patterns).  The oracle is checked against that file always; when the reference library has
been built, the reference is checked against it too, so the file stays pinned to the reference.

    python tests/test_oracle_vs_ref.py     (with oracle/_ref built: rewrites tests/golden/ref_vectors.json)
"""
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sigtk_amd import api  # noqa: E402
import event_cases  # noqa: E402
import jnn_cases  # noqa: E402
import median_cases  # noqa: E402
import prefix_cases  # noqa: E402  (tests/ is on the path: conftest.py lies there)

GOLDEN = os.path.join(ROOT, "tests", "golden")
VECTORS = os.path.join(GOLDEN, "ref_vectors.json")
SOAK_FIXTURES = ("soak_seed2024_b6003_r1407.npz", "soak_wvl_seed5_b431_r1525.npz", "soak_wvl_seed5_b797_r3354.npz")


def _h(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _stat(s):
    """raw_median as an int, the five float32 statistics as their bits"""
    return [int(s[4])] + [_bits(s[k]) for k in (0, 1, 2, 3, 5)]


def _random_reads(seed):
    rs = np.random.RandomState(seed)
    reads, dig, off, rng = api.synth_reads_host(6, [250, 1000, 5000, 20000, 50000, 100000], seed, seed % 2)
    reads = list(reads)
    reads.append(rs.randint(-3000, 3000, size=3000).astype(np.int16))
    reads.append(np.repeat(rs.randint(300, 700, size=400), 10).astype(np.int16))
    dig = np.concatenate([dig, [8192.0, 2048.0]])
    off = np.concatenate([off, [12.0, -3.0]])
    rng = np.concatenate([rng, [1402.882324, -748.5]])
    return reads, dig, off, rng


def observe_pa_event_stat(lib, seed):
    """pa and stat bit for bit, event (both presets): starts and lengths by value, mean / stdv bit for bit"""
    reads, dig, off, rng = _random_reads(seed)
    out = {}
    for r, raw in enumerate(reads):
        out["%d.pa" % r] = _h(lib.pa(raw, dig[r], off[r], rng[r]), np.float32)
        for rna in (0, 1):
            e = lib.event_raw(raw, dig[r], off[r], rng[r], rna)
            out["%d.event%d" % (r, rna)] = [_h(e.start, np.uint64), _h(e.length, np.float32),
                                            _h(e.mean, np.float32), _h(e.stdv, np.float32)]
        out["%d.stat" % r] = _stat(lib.stat(raw, dig[r], off[r], rng[r]))
    return out


def observe_jnn_adaptor_polya(lib, seed):
    reads, dig, off, rng = api.synth_reads_host(5, [1500, 2500, 30000, 100000, 100000], seed, 1)
    out = {}
    for r, raw in enumerate(reads):
        for rna in (0, 1):
            x, y = lib.jnn_raw(raw, rna)
            out["%d.jnn%d" % (r, rna)] = [_h(x, np.int64), _h(y, np.int64)]
        for pore in (0, 2):
            out["%d.adaptor%d" % (r, pore)] = list(lib.find_adaptor(raw, pore))
        pa = lib.pa(raw, dig[r], off[r], rng[r])
        for top, bot in ((120.0, 80.0), (110.5, 90.25)):
            out["%d.polya_%g_%g" % (r, top, bot)] = list(lib.find_polya(pa, top, bot, 0))
    return out


def observe_soak_fixtures(lib):
    """event (starts and means), jnn and stat on the reads the soaks found GPU bugs on (tests/golden/soak_*.npz)"""
    out = {}
    for name in SOAK_FIXTURES:
        z = np.load(os.path.join(GOLDEN, name))
        raw = z["samples"].astype(np.int16)
        dig, off, rng = float(np.ravel(z["dig"])[0]), float(np.ravel(z["off"])[0]), float(np.ravel(z["rng"])[0])
        for rna in (0, 1):
            e = lib.event_raw(raw, dig, off, rng, rna)
            out["%s.event%d" % (name, rna)] = [_h(e.start, np.uint64), _h(e.mean, np.float32)]
            x, y = lib.jnn_raw(raw, rna)
            out["%s.jnn%d" % (name, rna)] = [_h(x, np.int64), _h(y, np.int64)]
        out[name + ".stat"] = _stat(lib.stat(raw, dig, off, rng))
    return out


def observe_prefix_catalogue(lib):
    """tests/prefix_cases.py: find_adaptor on every read with either pore; find_polya on pA[adapt_y:] with the thresholds
    cfunc.c:191 forms from the mean of pA[adapt_x:adapt_y] (their bits are recorded too); jnnv2 with the small hi / lo /
    seg_dist sets of the shim cases; find_polya on the direct pA arrays"""
    out = {}
    with np.errstate(all="ignore"):
        for k in prefix_cases.catalogue():
            pa = lib.pa(k.raw, k.dig, k.off, k.rng)
            for pore in (0, 2):
                ax, ay = lib.find_adaptor(k.raw, pore)
                out["%s.adaptor%d" % (k.name, pore)] = [ax, ay]
                if ay > 0:
                    mid = np.float32(lib.statf(pa[ax:ay])[0]) + np.float32(30)
                    top, bot = mid + np.float32(20), mid - np.float32(20)
                    out["%s.polya%d" % (k.name, pore)] = [_bits(top), _bits(bot)] + list(lib.find_polya(pa[ay:], top, bot, pore))
        for k in prefix_cases.shim_cases():
            out["jnnv2:" + k.name] = list(lib.jnnv2(k.raw, k.p.std_scale, k.p.seg_dist, k.p.hi, k.p.lo))
        for k in prefix_cases.pa_cases():
            for pore in (0, 2):
                out["pa:%s.polya%d" % (k.name, pore)] = list(lib.find_polya(k.pa, k.top, k.bot, pore))
    return out


def observe_jnn_catalogue(lib):
    """tests/jnn_cases.py: jnn_raw on every read with the parameters it is run with (both presets, or its own: the err--
    correction, fixed thresholds on the clamp's edges, error 0 / 31 / 32 ...) and jnn_pa on the pA arrays; the preset
    entry point must agree with the presets passed as parameters"""
    out = {}
    with np.errstate(all="ignore"):
        for k in jnn_cases.catalogue():
            for label, p in jnn_cases.case_runs(k):
                x, y = lib.jnn_raw_param(k.raw, lib.jnn_param(**p._asdict()))
                out[label] = [int(x.size), _h(x, np.int64), _h(y, np.int64)]
            if k.params is None:
                for rna in (0, 1):
                    x, y = lib.jnn_raw(k.raw, rna)
                    assert out["%s/rna%d" % (k.name, rna)] == [int(x.size), _h(x, np.int64), _h(y, np.int64)], (k.name, rna)
        for k in jnn_cases.pa_cases():
            x, y = lib.jnn_pa(k.pa, lib.jnn_param(**k.params._asdict()))
            out["pa:" + k.name] = [int(x.size), _h(x, np.int64), _h(y, np.int64)]
    return out


def observe_event_catalogue(lib):
    """tests/event_cases.py: event on every read with the presets it is run with, starts and lengths by value, mean / stdv
    bit for bit.  Only the reads the reference lives through: its getevents() runs the trimming pass first, whose
    assertion fails on reads under 200 samples and on reads whose 100-sample chunks all have the same median absolute
    deviation (event_cases.ref_cli_prints), and what it does with a read that has no peak is undefined -- on those, the
    length edges and the bare seeds among them, the oracle is checked against the branch model alone
    (test_event_cases_cpu.py)"""
    from oracle.oracle import get_oracle
    out = {}
    for k in event_cases.catalogue():
        if not event_cases.ref_cli_prints(k.raw):
            continue
        for label, rna in event_cases.case_runs(k):
            if get_oracle().event_raw(k.raw, *event_cases.SCALE, rna).start.size < 2:
                continue
            e = lib.event_raw(k.raw, *event_cases.SCALE, rna)
            out[label] = [int(e.start.size), _h(e.start, np.uint64), _h(e.length, np.float32), _h(e.mean, np.float32),
                          _h(e.stdv, np.float32)]
    return out


def _nbits(x):
    """float32 bits; every NaN as its sign bit + the quiet pattern: two NaNs are equal iff their sign bits are"""
    b = int(np.float32(x).view(np.uint32))
    return (b & 0x80000000) | 0x7fc00000 if (b & 0x7fffffff) > 0x7f800000 else b


def _median_arrays(seed, count):
    """seeded arrays for the selection: floats with +-0, NaNs of both signs, duplicates, all-equal, sorted, reversed,
    and int16 reads under ordinary, negative and tie-class scales"""
    rs = np.random.RandomState(seed)
    nan_p, nan_n = np.uint32(0x7fc00000).view(np.float32), np.uint32(0xffc00000).view(np.float32)
    for i in range(count):
        n = int(rs.randint(1, 120)) if i % 16 else int(rs.randint(120, 3000))
        kind = i % 8
        if kind < 5:
            x = rs.normal(0, 1, size=n).astype(np.float32) if kind != 1 else rs.randint(-3, 4, size=n).astype(np.float32)
            if kind == 2:
                x[:] = x[0]
            if kind == 3:
                x = np.sort(x) if i % 16 < 8 else np.sort(x)[::-1].copy()
            for v, p in ((0.0, 0.5), (-0.0, 0.5), (nan_p, 0.3), (nan_n, 0.3), (np.inf, 0.1), (-np.inf, 0.1)):
                if rs.rand() < p:
                    x[rs.randint(0, n, size=rs.randint(1, 4))] = v
            yield "f", x
        else:
            raw = rs.randint(-20, 20, size=n).astype(np.int16) if kind < 7 else rs.randint(-32768, 32768, size=n).astype(np.int16)
            if i % 24 == 5:
                raw[:] = raw[0]
            if i % 24 == 13:
                raw = np.sort(raw) if i % 48 < 24 else np.sort(raw)[::-1].copy()
            nm, dig, rng = median_cases.TIE_SCALES[i % 6] if kind == 5 else ("", 8192.0, (1402.882324, -1402.882324)[i % 2])
            yield "i", (raw, dig, float(rs.randint(-10, 10)), rng)


def observe_median_arrays(lib, seed):
    """the selection on 2 600 seeded arrays (x 4 seeds: 10 400): medianf with the other two float statistics, stat's raw
    and pA medians; one hash per 650 arrays, NaNs by their sign"""
    out = {}
    acc = []
    with np.errstate(all="ignore"):
        for i, (kind, v) in enumerate(_median_arrays(seed, 2600)):
            if kind == "f":
                acc += [_nbits(t) for t in lib.statf(v)]
            else:
                s = lib.stat(*v)
                acc += [int(s[4]) & 0xffffffff] + [_nbits(s[k]) for k in (0, 1, 2, 3, 5)]
            if i % 650 == 649:
                out["%04d" % (i - 649)] = hashlib.sha256(np.array(acc, dtype=np.uint32).tobytes()).hexdigest()
                acc = []
    return out


def observe_median_catalogue(lib):
    """tests/median_cases.py: stat on every read, statf on every float array, and the region medians of prefix as
    cfunc.c forms them, NaNs by their sign; one hash per family of cases (the values themselves are in
    tests/golden/median_cases.json, which test_median_cases_cpu.py holds the oracle against case by case)"""
    out = {}
    with np.errstate(all="ignore"):
        for k in median_cases.cases():
            s = lib.stat(k.raw, k.dig, k.off, k.rng)
            out[k.name] = [int(s[4])] + [_nbits(s[i]) for i in (0, 1, 2, 3, 5)]
        for k in median_cases.float_cases():
            out["f:" + k.name] = [_nbits(t) for t in lib.statf(k.x)]
        for k in median_cases.region_cases():
            pa = lib.pa(k.raw, k.dig, k.off, k.rng)
            ax, ay = lib.find_adaptor(k.raw, median_cases.REGION_PORE)
            st = lib.statf(pa[ax:ay])
            mid = np.float32(st[0]) + np.float32(30)
            px, py = lib.find_polya(pa[ay:], mid + np.float32(20), mid - np.float32(20), median_cases.REGION_PORE)
            out["r:" + k.name] = [ax, ay, px, py] + [_nbits(t) for t in st] + \
                ([_nbits(t) for t in lib.statf(pa[ay + px:ay + py])] if py > 0 else [])
    fam = {}
    for name in sorted(out):
        fam.setdefault(name.split("_")[0], []).extend([zlib.crc32(name.encode())] + [int(v) & 0xffffffff for v in out[name]])
    return {k: hashlib.sha256(np.array(v, dtype=np.uint32).tobytes()).hexdigest() for k, v in fam.items()}


OBSERVATIONS = {"pa_event_stat_seed%d" % s: (observe_pa_event_stat, (s,)) for s in (1, 2, 3)}
OBSERVATIONS.update({"jnn_adaptor_polya_seed%d" % s: (observe_jnn_adaptor_polya, (s,)) for s in (4, 5)})
OBSERVATIONS["soak_fixtures"] = (observe_soak_fixtures, ())
OBSERVATIONS["prefix_catalogue"] = (observe_prefix_catalogue, ())
OBSERVATIONS["jnn_catalogue"] = (observe_jnn_catalogue, ())
OBSERVATIONS["event_catalogue"] = (observe_event_catalogue, ())
OBSERVATIONS.update({"median_arrays_seed%d" % s: (observe_median_arrays, (s,)) for s in (11, 12, 13, 14)})
OBSERVATIONS["median_catalogue"] = (observe_median_catalogue, ())


def _check(name, oracle, reflib):
    fn, args = OBSERVATIONS[name]
    want = json.load(open(VECTORS))[name]
    libs = [("oracle", oracle)] + ([("reference", reflib)] if reflib is not None else [])
    for who, lib in libs:
        got = fn(lib, *args)
        assert sorted(got) == sorted(want), (who, name)
        for k in want:
            assert got[k] == want[k], "%s differs from the stored reference output at %s / %s" % (who, name, k)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_pa_event_stat_bitwise(oracle, reflib, seed):
    _check("pa_event_stat_seed%d" % seed, oracle, reflib)


@pytest.mark.parametrize("seed", [4, 5])
def test_jnn_adaptor_polya(oracle, reflib, seed):
    _check("jnn_adaptor_polya_seed%d" % seed, oracle, reflib)


def test_soak_regression_fixtures_are_pinned(oracle, reflib):
    """the reads the round-2 soaks found GPU bugs on (tests/golden/soak_*.npz): what the GPU tests compare against --
    the oracle -- equals the real reference on them (event, stat and jnn)."""
    _check("soak_fixtures", oracle, reflib)


def test_prefix_catalogue(oracle, reflib):
    """every branch of the adaptor and polyA finders (tests/prefix_cases.py): the oracle the GPU tests compare against
    equals the real reference on the whole catalogue"""
    _check("prefix_catalogue", oracle, reflib)


def test_jnn_catalogue(oracle, reflib):
    """every branch of the segmenter, the err-- correction among them (tests/jnn_cases.py): the oracle the GPU tests compare
    against equals the real reference on the whole catalogue"""
    _check("jnn_catalogue", oracle, reflib)


def test_event_catalogue(oracle, reflib):
    """every branch of the peak detector, the boundaries of its long detector among them (tests/event_cases.py): the oracle
    the GPU tests compare against equals the real reference on every read of the catalogue the reference can take"""
    _check("event_catalogue", oracle, reflib)


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_selection_on_seeded_arrays(oracle, reflib, seed):
    """10 400 seeded arrays in all: the oracle's selection leaves the element at n / 2 that the reference's leaves there,
    bit for bit (a NaN: the same sign), with +-0, NaNs, duplicates, constant, sorted and reversed arrays, and int16 reads
    under the tie-class scales"""
    _check("median_arrays_seed%d" % seed, oracle, reflib)


def test_median_catalogue(oracle, reflib):
    """every read and float array of tests/median_cases.py, and the region medians of its prefix reads"""
    _check("median_catalogue", oracle, reflib)


if __name__ == "__main__":
    from oracle.oracle import RefLib
    if not RefLib.available():
        raise SystemExit("build the reference first: make -C oracle ref")
    ref = RefLib()
    vectors = {name: fn(ref, *args) for name, (fn, args) in OBSERVATIONS.items()}
    with open(VECTORS, "w") as fh:
        json.dump(vectors, fh, indent=1, sort_keys=True)
    print("wrote %s (%d groups)" % (VECTORS, len(vectors)))
