"""GPU parity: sgk_normalise_f32 / sgk_normalise / the pa job with sgk_job_set_normalise against the numpy model
(tests/normalise_model.py), y and the records as bit patterns, for both methods.  Two NaNs count as equal whatever their
sign and payload (normalise_model.py says why); everything else, the canaries around the reads included, is compared bit
for bit.  Every call of _check also asserts the memory contract: no value of y outside the reads changes (in front of the
first read and behind the last one too, at whichever 16-byte phase y lies) and x stays as it was when y is not x."""
import zlib

import numpy as np
import pytest

import normalise_model as nm

pytestmark = pytest.mark.gpu

F = np.float32
METHODS = (nm.ZSCORE, nm.MEDMAD)
CANARY = 0x7FC12345   # a quiet NaN with a payload nobody computes
# 0, 1 .. 5 around a group of 4, 15 .. 17 around a lane's 16, 1023 .. 1025 around a tile of 64 x 16, 2047 / 2049, 5000
LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 2047, 2049, 5000)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _signal(rs, n, mean=90.0, sd=12.0):
    return rs.normal(mean, sd, size=n).astype(F)


class _Expect:
    """the model's y and records of a batch, computed once per batch and shared by the calls that check it"""

    def __init__(self, arrays, statf):
        self.arrays = [np.ascontiguousarray(a, dtype=F) for a in arrays]
        self.by_method = {m: [nm.normalise(a, m, statf) for a in self.arrays] for m in METHODS}

    def only(self, keep):
        """the same expectations for the reads `keep` alone"""
        sub = _Expect([], None)
        sub.arrays = [self.arrays[r] for r in keep]
        sub.by_method = {m: [v[r] for r in keep] for m, v in self.by_method.items()}
        return sub


def _call(fb, method, y, ws=None):
    import torch
    from sigtk_amd import api
    y, rec = fb.normalise_f32(method, y=y, ws=ws)
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(api.NORM_DTYPE)[:fb.n_reads].copy()


def _check_records(recs, want, what):
    bad = []
    for r, (_, (shift, scale, n, flags)) in enumerate(want):
        ok = nm.same_bits(recs["shift"][r], shift).all() and nm.same_bits(recs["scale"][r], scale).all()
        if not ok or int(recs["n"][r]) != n or int(recs["flags"][r]) != flags:
            bad.append("%s read %d: gpu %r model %r" % (what, r, recs[r], (shift, scale, n, flags)))
    assert not bad, "\n".join(bad[:10])


def _check(exp, method, leads=None, in_place=False, y_lead=4, what=""):
    """one call on the batch; y lies y_lead elements into a canary-filled allocation with 8 more behind it"""
    import torch
    from sigtk_amd import device
    fb = device.upload_float_reads(exp.arrays, _dev(), leads=leads, fill=-7.5)
    x_before = fb.x.cpu().numpy().copy()
    want = exp.by_method[method]
    if in_place:
        y, y_all = fb.x, fb.x
        expect = x_before.copy()
    else:
        y_all = torch.from_numpy(np.full(fb.n_values + y_lead + 8, CANARY, dtype=np.uint32).view(F)).to(_dev())
        y = y_all[y_lead:y_lead + fb.n_values]
        expect = np.full(fb.n_values, CANARY, dtype=np.uint32).view(F)
    recs = _call(fb, method, y)
    inside = np.zeros(fb.n_values, dtype=bool)
    for o, (yr, _) in zip(fb.offsets_host.tolist(), want):
        expect[o:o + yr.size] = yr
        inside[o:o + yr.size] = True
    got_all = y_all.cpu().numpy()
    got = got_all if in_place else got_all[y_lead:y_lead + fb.n_values]
    wrong = np.flatnonzero(~nm.same_bits(got, expect))
    assert wrong.size == 0, "%s method %d: %d values differ, first at %d: gpu %r model %r" % (
        what, method, wrong.size, wrong[0], got[wrong[0]], expect[wrong[0]])
    # outside the reads nothing changes, bit for bit (same_bits would let one NaN pass for another)
    assert np.array_equal(nm.bits(got)[~inside], nm.bits(expect)[~inside]), what
    if not in_place:
        # ... and inside them everything was written: a read whose y is all NaN must not pass on the canary that was there
        assert not (nm.bits(got)[inside] == CANARY).any(), what + ": a value of a read was not written"
        assert (nm.bits(got_all[:y_lead]) == CANARY).all() and (nm.bits(got_all[y_lead + fb.n_values:]) == CANARY).all(), what
        assert np.array_equal(nm.bits(fb.x.cpu().numpy()), nm.bits(x_before)), what + ": x changed"
    _check_records(recs, want, what)
    return recs


@pytest.fixture(scope="module")
def statf(oracle, reflib):
    return nm.statf_of(oracle, reflib)


@pytest.fixture(scope="module")
def shapes(statf):
    """1. every length of LENGTHS, odd and even (2.), on ordinary signal"""
    rs = np.random.RandomState(101)
    return _Expect([_signal(rs, n) for n in LENGTHS], statf)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_lengths_at_every_residue(shapes, method, gaps, residue):
    n = len(shapes.arrays)
    # touching reads: the lengths themselves move the later reads over all residues; gaps of 0 .. 4 do it another way
    leads = [residue] + ([(r * 7 + 3) % 5 for r in range(1, n)] if gaps else [0] * (n - 1))
    _check(shapes, method, leads=leads, what="residue %d gaps %d" % (residue, gaps))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("y_lead", [1, 2, 3])
def test_y_at_another_16_byte_phase_than_x(shapes, method, y_lead):
    """x 16-byte aligned and y not: the stores go value by value, to the same places"""
    _check(shapes, method, leads=[0] + [1] * (len(shapes.arrays) - 1), y_lead=y_lead, what="y_lead %d" % y_lead)


@pytest.mark.parametrize("method", METHODS)
def test_in_place_is_out_of_place(shapes, method):
    """9. y == x"""
    n = len(shapes.arrays)
    for residue in (0, 3):
        _check(shapes, method, leads=[residue] + [(r * 3) % 4 for r in range(1, n)], in_place=True, what="in place")


@pytest.mark.parametrize("method", METHODS)
def test_symmetric_reads_tie_in_the_deviations(statf, method):
    """3. x symmetric about its median: every deviation but the median's comes twice"""
    rs = np.random.RandomState(102)
    arrays = []
    for half in (1, 2, 7, 8, 500, 1111):
        h = np.sort(np.abs(_signal(rs, half, 0.0, 20.0))) + F(0.5)
        for odd in (True, False):
            a = np.concatenate([F(100) - h, [F(100)] if odd else [], F(100) + h]).astype(F)
            arrays.append(rs.permutation(a))
    arrays.append(np.repeat(np.array([1, 2, 3, 4, 5], dtype=F), 300))   # ties in x as well
    _check(_Expect(arrays, statf), method, leads=[1] + [2] * (len(arrays) - 1), what="symmetric")


@pytest.mark.parametrize("method", METHODS)
def test_wide_range_read(statf, method):
    """4. 1e-30 .. 1e30 in both signs: the deviations' keys spread over many top-level bins and all three levels decide"""
    rs = np.random.RandomState(103)
    arrays = []
    for n in (3000, 2049):
        a = (10.0 ** rs.uniform(-30, 30, size=n) * rs.choice([-1.0, 1.0], size=n)).astype(F)
        arrays.append(a)
    a = (10.0 ** rs.uniform(-30, 30, size=4097)).astype(F)   # one sign: x itself keeps to a bin per binade
    arrays.append(a)
    exp = _Expect(arrays, statf)
    d = np.abs(arrays[0] - exp.by_method[nm.MEDMAD][0][1][0])
    assert np.unique(nm.bits(d) >> 21).size > 100            # (the top-level bins of the first level)
    _check(exp, method, leads=[3, 1, 2], what="wide range")


@pytest.mark.parametrize("method", METHODS)
def test_zero_scale_and_zero_medians(statf, method):
    """5. constant reads, mad == 0 on a read that is not constant, reads of zeros of either sign: SGK_NORM_ZERO_SCALE and
    what IEEE makes of the division; the sign of a zero median shows in shift and, where scale != 0, in y"""
    rs = np.random.RandomState(104)
    pz, nz = F(0.0), F(-0.0)
    arrays = [np.full(n, 87.25, dtype=F) for n in (1, 2, 17, 1500)]                  # constant: std == 0 and mad == 0
    n_const = len(arrays)
    not_const = [np.array([1, 1, 1, 1, 5], dtype=F), np.array([3, 9, 3, 3], dtype=F),
                 rs.permutation(np.concatenate([np.full(1200, 50, dtype=F), _signal(rs, 700)]))]
    arrays += not_const                                                              # mad == 0, std != 0
    zeros = [np.full(5, pz), np.full(5, nz), np.full(1030, nz), np.array([nz, pz, nz, pz], dtype=F),
             np.array([pz, nz, pz, nz, pz], dtype=F)]
    arrays += zeros
    # a zero median and a scale that is not zero
    arrays += [np.array([-2, -1, pz, 1, 2], dtype=F), np.array([-2, -1, nz, 1, 2], dtype=F),
               np.array([-2, -1, nz, pz, 1, 2, nz], dtype=F), rs.permutation(np.concatenate([_signal(rs, 600, 0, 5), np.full(40, nz), np.full(40, pz)]))]
    exp = _Expect(arrays, statf)
    recs = _check(exp, method, leads=[2] + [1] * (len(arrays) - 1), what="zero scale")
    flagged = recs["flags"] == nm.ZERO_SCALE
    assert flagged[:n_const].all() and flagged[n_const + len(not_const):n_const + len(not_const) + len(zeros)].all()
    if method == nm.MEDMAD:
        assert flagged[n_const:n_const + len(not_const)].all()
        y = exp.by_method[method][n_const][0]      # [1, 1, 1, 1, 5]: 0 / 0 four times and 4 / 0
        assert np.isnan(y[:4]).all() and np.isposinf(y[4])
    else:
        assert not flagged[n_const:n_const + len(not_const)].any()
    assert not flagged[-4:].any()


@pytest.mark.parametrize("method", METHODS)
def test_reads_with_a_nan_or_an_infinity(statf, method):
    """6. SGK_NORM_NONFINITE, shift and scale NaN, every y of the read NaN -- and the neighbours untouched by it.  A read
    of finite values whose sum overflows has the same mean as one holding an infinity and is not such a read."""
    rs = np.random.RandomState(105)
    arrays, hostile = [], []
    for n, pos, bad in ((2500, 0, np.nan), (2500, 2499, np.nan), (5000, 1021, np.nan), (5000, 1022, np.nan), (5000, 1023, np.nan),
                        (5000, 1024, np.nan), (5000, 2048, np.nan), (1, 0, np.nan), (3000, 1500, np.inf), (3000, 7, -np.inf),
                        (4, 3, np.inf)):
        a = _signal(rs, n)
        a[pos] = bad
        arrays.append(a)
        hostile.append(True)
        arrays.append(_signal(rs, 33))      # a sound read between every two
        hostile.append(False)
    arrays.append(np.array([3e38, 3e38, 3e38, 1.0], dtype=F))     # finite, the sum is +inf
    hostile.append(False)
    exp = _Expect(arrays, statf)
    recs = _check(exp, method, leads=[1] + [0] * (len(arrays) - 1), what="nonfinite")
    assert ((recs["flags"] & nm.NONFINITE) != 0).tolist() == hostile
    assert np.isnan(recs["shift"][hostile]).all() and np.isnan(recs["scale"][hostile]).all()
    assert all(np.isnan(exp.by_method[method][r][0]).all() for r in range(len(arrays)) if hostile[r])


def test_subnormal_and_overflowing_quotients(statf):
    """7. quotients below FLT_MIN are kept, not flushed; quotients beyond FLT_MAX are infinities"""
    rs = np.random.RandomState(106)
    tiny = (rs.normal(0, 1, size=900) * 1e-20).astype(F)
    # z-score: a cluster of 1e-26 and two values of 1e15 (whose squares still fit): deviations of 1e-26 over a scale of 5e13
    z_sub = np.concatenate([tiny[:450] * F(1e-6), np.array([1e15, -1e15], dtype=F), tiny[450:] * F(1e-6)]).astype(F)
    # med-MAD: most values of 1e20 in either sign, a cluster of 1e-20 in the middle that holds the median
    big = (np.abs(rs.normal(0, 1, size=400)) + 0.5).astype(F) * F(1e20)
    m_sub = rs.permutation(np.concatenate([-big, tiny[:101], big])).astype(F)
    # med-MAD: most values of 1e-20, a few of 1e30: deviations of 1e30 over a scale of 1e-20
    m_inf = rs.permutation(np.concatenate([tiny, np.array([1e30, -1e30, 3e38], dtype=F)])).astype(F)
    exp = _Expect([z_sub, m_sub, m_inf], statf)
    assert nm.is_subnormal(exp.by_method[nm.ZSCORE][0][0]).sum() > 100
    assert nm.is_subnormal(exp.by_method[nm.MEDMAD][1][0]).sum() > 50
    assert np.isinf(exp.by_method[nm.MEDMAD][2][0]).sum() == 3
    for method in METHODS:
        _check(exp, method, leads=[1, 2, 3], what="subnormal / overflow")


@pytest.mark.parametrize("method", METHODS)
def test_many_short_reads_and_a_long_one(statf, method):
    """8. 1 100 short reads and one of 100 000 values: from 1 024 reads on the batch is dispatched longest first"""
    rs = np.random.RandomState(107)
    arrays = [_signal(rs, int(n)) for n in rs.randint(0, 40, size=550)]
    arrays.append(_signal(rs, 100000))
    arrays += [_signal(rs, int(n)) for n in rs.randint(0, 40, size=550)]
    _check(_Expect(arrays, statf), method, leads=[1] + [0] * 1100, what="1101 reads")


def test_short_workspace_writes_nothing(shapes):
    """10. one byte short: SGK_ERR_WORKSPACE, y and the records as they were"""
    import torch
    from sigtk_amd import api, device
    fb = device.upload_float_reads(shapes.arrays, _dev())
    L = api._float_lib()
    need = int(L.sgk_normalise_f32_workspace_bytes(fb.n_reads, fb.n_values, fb.max_read_len))
    ws = torch.zeros(need, dtype=torch.uint8, device=_dev())
    stream = int(torch.cuda.current_stream().cuda_stream)
    for method in METHODS:
        ws.zero_()
        y = torch.from_numpy(np.full(fb.n_values, CANARY, dtype=np.uint32).view(F)).to(_dev())
        rec = torch.full((fb.n_reads * 16,), 0xA5, dtype=torch.uint8, device=_dev())
        rc = L.sgk_normalise_f32(*fb.view(), method, y.data_ptr(), rec.data_ptr(), ws.data_ptr(), need - 1, stream)
        torch.cuda.synchronize()
        assert rc == api.SGK_ERR_WORKSPACE
        assert (nm.bits(y.cpu().numpy()) == CANARY).all() and (rec.cpu().numpy() == 0xA5).all()
        assert (ws.cpu().numpy() == 0).all()
        rc = L.sgk_normalise_f32(*fb.view(), method, y.data_ptr(), rec.data_ptr(), ws.data_ptr(), need, stream)
        torch.cuda.synchronize()
        assert rc == api.SGK_OK and (rec.cpu().numpy().view(api.NORM_DTYPE)["n"] == fb.lengths_host).all()


# ------------------------------------------------------------------------------------------------ int16 batches, jobs

@pytest.fixture(scope="module")
def raw_batch(gpu, oracle, statf):
    """int16 reads of the lengths that matter, their pA by the oracle and the model on it"""
    lens = [5000, 0, 1, 333, 1025, 70001, 16]
    reads, dig, off, rng = gpu.synth_reads_host(len(lens), lens, seed=31, kind=0)
    pa = [oracle.pa(raw, dig[r], off[r], rng[r]) for r, raw in enumerate(reads)]
    return {"reads": reads, "scal": (dig, off, rng), "exp": _Expect(pa, statf)}


@pytest.mark.parametrize("method", METHODS)
def test_int16_batch(gpu, raw_batch, method):
    """11. sgk_normalise: the model on Oracle.pa"""
    import torch
    from sigtk_amd import device
    b = device.upload_reads(raw_batch["reads"], *raw_batch["scal"], _dev())
    y = torch.from_numpy(np.full(b.n_samples, CANARY, dtype=np.uint32).view(F)).to(_dev())
    y, rec = b.normalise(method, y=y)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    want = raw_batch["exp"].by_method[method]
    inside = np.zeros(b.n_samples, dtype=bool)
    for r, (yr, _) in enumerate(want):
        o = int(b.offsets_host[r])
        assert nm.same_bits(got[o:o + yr.size], yr).all(), r
        inside[o:o + yr.size] = True
    assert (nm.bits(got)[~inside] == CANARY).all() and not (nm.bits(got)[inside] == CANARY).any()
    _check_records(rec.cpu().numpy().view(gpu.NORM_DTYPE)[:b.n_reads], want, "int16")


def _job_matches(job, gpu, exp, what):
    for method in METHODS:
        job.set_normalise(method)
        job.launch(gpu.TOOL_PA)
        got = job.wait()["pa"]
        for r, (yr, _) in enumerate(exp.by_method[method]):
            assert got[r].size == yr.size and nm.same_bits(got[r], yr).all(), (what, method, r)
    job.set_normalise(0)   # off again: the pA values
    job.launch(gpu.TOOL_PA)
    got = job.wait()["pa"]
    assert all(np.array_equal(nm.bits(g), nm.bits(a)) for g, a in zip(got, exp.arrays)), what


@pytest.mark.parametrize("fmt", ["int16", "svbzd", "text"])
def test_job_staged_formats(gpu, raw_batch, fmt):
    """12. the pa job with sgk_job_set_normalise: int16 samples, svb-zd blobs, text SLOW5 columns"""
    from sigtk_amd import blow5
    # (a text column holds at least one number)
    keep = [r for r, raw in enumerate(raw_batch["reads"]) if raw.size or fmt != "text"]
    reads = [raw_batch["reads"][r] for r in keep]
    scal = [[s[r] for r in keep] for s in raw_batch["scal"]]
    job = gpu.Job(0)
    if fmt == "int16":
        job.stage(reads, *scal)
    elif fmt == "svbzd":
        job.stage([blow5.svb_zd_encode(r) for r in reads], *scal, counts=[r.size for r in reads])
    else:
        job.stage([blow5.slow5_signal_text(r) for r in reads], *scal, counts=[r.size for r in reads], text=True)
    _job_matches(job, gpu, raw_batch["exp"].only(keep), fmt)
    # only SGK_TOOL_PA looks at the method, and with SGK_JOB_TEXT it is refused
    job.set_normalise(nm.MEDMAD)
    job.launch(gpu.TOOL_STAT)
    assert job.wait()["stat"].size == len(reads)
    job.set_ids([b"read%d" % r for r in range(len(reads))])
    with pytest.raises(gpu.SigtkGpuError):
        job.launch(gpu.TOOL_PA, flags=gpu.JOB_TEXT)
    with pytest.raises(gpu.SigtkGpuError):
        job.set_normalise(3)
    job.close()


@pytest.mark.parametrize("signal", ["svbzd", "int16"])
def test_job_records(gpu, oracle, statf, sp1, signal):
    """12. ... and whole zlib records, inflated on the device, with an svb-zd or a plain signal"""
    import struct
    from sigtk_amd import blow5
    from test_gpu_zrec_raw import SP1, TABLE, plain_signal_record, zlib_room
    n = 12
    reads = sp1.reads[:n]
    scal = ([r.digitisation for r in reads], [r.offset for r in reads], [r.range for r in reads])
    exp = _Expect([oracle.pa(r.raw, r.digitisation, r.offset, r.range) for r in reads], statf)
    recs = blow5.raw_records(SP1)[:n]
    lengths = [r.raw.size for r in reads]
    if signal == "int16":
        made = [plain_signal_record(r) for r in recs]
        recs, sig_off = [m[0] for m in made], [m[1] for m in made]
        sig_bytes = [2 * k for k in lengths]
        fmt = gpu.SIGNAL_INT16
    else:
        sig_off, sig_bytes = [], []
        for rec in recs:
            p = 2 + struct.unpack_from("<H", rec, 0)[0] + 36
            sig_off.append(p + 8)
            sig_bytes.append(struct.unpack_from("<Q", rec, p)[0])
        fmt = gpu.SIGNAL_SVBZD
    room = [zlib_room(o + b, TABLE) for o, b in zip(sig_off, sig_bytes)]
    job = gpu.Job(0)
    job.stage_zrec([zlib.compress(r) for r in recs], lengths, sig_off, sig_bytes, room, *scal, aux=TABLE, signal_format=fmt)
    _job_matches(job, gpu, exp, "records " + signal)
    job.close()
