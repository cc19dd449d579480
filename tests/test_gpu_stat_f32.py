"""GPU parity: sgk_stat_f32, meanf / stdvf / medianf (src/stat.h:17-63) of every read of a float batch, bit for bit
against oracle.statf.  NaN is compared by isnan on both sides (the rule of tests/test_gpu_shims.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
SS_HEAD = 256   # csrc/seqsum.h: the leading terms of a read that are added natively


def _dev():
    import torch
    return torch.device("cuda", 0)


def _records(fb):
    import torch
    from sigtk_amd import api, device
    out = device.stat_f32(fb)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(api.STATF_DTYPE)[:fb.n_reads].copy()


def _run(arrays, leads=None, fill=None):
    from sigtk_amd import device
    return _records(device.upload_float_reads(arrays, _dev(), leads=leads, fill=fill))


def _same(a, b):
    a, b = F(a), F(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def _check(recs, arrays, oracle, what=""):
    assert recs.size == len(arrays)
    bad = []
    with np.errstate(all="ignore"):
        for r, x in enumerate(arrays):
            if x.size == 0:   # the reference divides 0 by 0 and selects from nothing
                e = (F("nan"),) * 3
            else:
                e = oracle.statf(x)
            for name, w in zip(("mean", "std", "median"), e):
                if not _same(recs[name][r], w):
                    bad.append("%s read %d (n=%d) %s: gpu %r oracle %r" % (what, r, x.size, name, recs[name][r], w))
            if recs["flags"][r] != 0:
                bad.append("%s read %d (n=%d): flags %d" % (what, r, x.size, recs["flags"][r]))
    assert not bad, "\n".join(bad[:20])


def _residue_leads(n, first=1):
    """gaps that put consecutive reads on changing residues of 4 elements, whatever their lengths; the first read at `first`"""
    return [first] + [(r * 7 + 3) % 5 for r in range(1, n)]


def _hostile():
    """the arrays of test_seqsum_chains_on_hostile_float_arrays (tests/test_gpu_shims.py), its long ones once"""
    rs = np.random.RandomState(21)
    arrays = []
    for n in (1, 2, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4999):
        arrays.append(rs.normal(90, 12, size=n).astype(F))
        arrays.append(rs.normal(0, 50, size=n).astype(F))                 # sum wanders through zero
        arrays.append((-rs.gamma(2.0, 30.0, size=n)).astype(F))            # all negative
    arrays.append(rs.normal(90, 12, size=70000).astype(F))
    arrays.append(rs.normal(0, 50, size=300000).astype(F))
    arrays.append((-rs.gamma(2.0, 30.0, size=70000)).astype(F))
    arrays.append(np.full(200000, 333.0, dtype=F))                        # integer sum beyond 2^24: ties
    arrays.append(np.where(np.arange(100000) % 2 == 0, 0.5, 1.5).astype(F))
    arrays.append(np.concatenate([np.zeros(3000), np.full(500, 7.25), np.zeros(3000), np.full(4000, -7.25)]).astype(F))
    big = rs.normal(100, 10, size=50000).astype(F); big[20000] = 3e7; big[30000] = -3e7; big[40000] = 1e-30
    arrays.append(big)
    arrays.append((rs.rand(5000) * 1e-38).astype(F))                       # denormal sums
    arrays.append((rs.rand(5000) * 3e38).astype(F))                        # overflows to inf
    nn = rs.normal(100, 10, size=5000).astype(F); nn[2500] = np.nan
    arrays.append(nn)
    ii = rs.normal(100, 10, size=5000).astype(F); ii[2500] = np.inf
    arrays.append(ii)
    ij = ii.copy(); ij[3000] = -np.inf
    arrays.append(ij)
    return arrays


def test_hostile_arrays_in_one_batch(gpu, oracle):
    from sigtk_amd import device
    arrays = _hostile()
    fb = device.upload_float_reads(arrays, _dev(), leads=_residue_leads(len(arrays)), fill=np.nan)
    res = fb.offsets_host.astype(np.int64) % 4
    assert set(res.tolist()) == {0, 1, 2, 3} and int(fb.offsets_host[0]) == 1
    assert len(set(res[-9:].tolist())) > 1   # the special arrays at the end do not share one residue
    _check(_records(fb), arrays, oracle, "hostile")


def test_lengths(gpu, oracle):
    rs = np.random.RandomState(5)
    lens = [1, 2, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, SS_HEAD - 1, SS_HEAD, SS_HEAD + 1]
    for res in range(4):   # every length at every residue
        arrays = [rs.normal(95, 14, size=n).astype(F) for n in lens]
        leads = [res] + [(-n) % 4 for n in lens[:-1]]   # every read starts at residue `res`
        _check(_run(arrays, leads=leads, fill=np.nan), arrays, oracle, "residue %d" % res)


def test_medians(gpu, oracle):
    rs = np.random.RandomState(6)
    z, nz = F(0.0), F(-0.0)
    arrays = [np.array([3.5, -2.0, 3.5, 0.0, -7.25, 1e-3, 3.5, -2.0], dtype=F),          # ties
              np.full(777, 41.5, dtype=F), np.full(778, -41.5, dtype=F),                  # all equal
              np.array([2.0, 1.0], dtype=F), np.array([1.0, 2.0], dtype=F),               # two values
              np.tile(np.array([5.0, 9.0], dtype=F), 500), np.tile(np.array([9.0, 5.0], dtype=F), 501)[:-1],
              np.array([nz] * 7 + [z] + [nz] * 7, dtype=F),                               # +0.0 among -0.0s
              np.array([z] * 7 + [nz] + [z] * 7, dtype=F),                                # ... and the reverse
              np.array([nz, z] * 50, dtype=F), np.array([z, nz] * 50 + [z], dtype=F),
              np.concatenate([np.full(40, -3.0), [z, nz, nz, z, nz], np.full(40, 3.0)]).astype(F),
              (-rs.gamma(2.0, 30.0, size=1000)).astype(F), (-rs.gamma(2.0, 30.0, size=1001)).astype(F),   # all negative
              rs.normal(90, 12, size=600).astype(F), rs.normal(90, 12, size=601).astype(F),     # n even and odd
              np.round(rs.normal(90, 3, size=3000)).astype(F)]                            # many ties, a few values
    for pos in (0, 150, 299):                                                          # one NaN in 300 values
        x = rs.normal(90, 12, size=300).astype(F); x[pos] = np.nan
        arrays.append(x)
    recs = _run(arrays, leads=_residue_leads(len(arrays), first=0), fill=-1e30)
    _check(recs, arrays, oracle, "medians")
    # the sign of a zero median is the reference's pick
    for r in (7, 8, 9, 10, 11):
        assert recs["median"][r] == 0.0
        assert np.signbit(recs["median"][r]) == np.signbit(oracle.statf(arrays[r])[2])


@pytest.fixture(scope="module")
def ragged():
    rs = np.random.RandomState(8)
    lens = np.concatenate([[0, 5000, 0, 1, 0], rs.randint(0, 5001, size=295)])
    return [rs.normal(rs.uniform(60, 120), rs.uniform(2, 20), size=int(n)).astype(F) for n in lens]


def test_batch_shapes(gpu, oracle, ragged):
    one = [ragged[1]]
    _check(_run(one), one, oracle, "one read")
    assert len(ragged) == 300 and min(a.size for a in ragged) == 0 and max(a.size for a in ragged) == 5000
    recs = _run(ragged)
    _check(recs, ragged, oracle, "300 reads")
    perm = np.random.RandomState(9).permutation(len(ragged))
    got = _run([ragged[i] for i in perm])
    assert got.tobytes() == recs[perm].tobytes()


def test_more_reads_than_the_dispatch_order_needs(gpu, oracle):
    """1 100 reads: from 1 024 on the waves take the reads longest first, from the device-side sort"""
    rs = np.random.RandomState(10)
    arrays = [rs.normal(90, 12, size=int(n)).astype(F) for n in rs.randint(0, 600, size=1100)]
    _check(_run(arrays, leads=_residue_leads(len(arrays))), arrays, oracle, "1100 reads")


def test_gaps_do_not_matter(gpu, oracle, ragged):
    from sigtk_amd import device
    arrays = ragged[:64]
    leads = _residue_leads(len(arrays), first=1)
    leads[-1] += 3   # (the last read ends the allocation whatever stands in front of it)
    got = []
    for fill in (np.nan, 3e38, 0.0):
        fb = device.upload_float_reads(arrays, _dev(), leads=leads, fill=fill)
        assert int(fb.offsets_host[0]) == 1 and set((fb.offsets_host.astype(np.int64) % 4).tolist()) == {0, 1, 2, 3}
        assert int(fb.offsets_host[-1]) + int(fb.lengths_host[-1]) == fb.n_values == fb.x.numel()
        got.append(_records(fb))
    _check(got[0], arrays, oracle, "gaps of NaN")
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


def test_workspace(gpu, oracle, ragged):
    import torch
    from sigtk_amd import api, device
    L = api._float_lib()
    arrays = ragged[:40] + [np.zeros(500, dtype=F), np.full(300, np.nan, dtype=F)]   # two reads for the scratch rows
    fb = device.upload_float_reads(arrays, _dev())
    need = int(L.sgk_stat_f32_workspace_bytes(fb.n_reads, fb.n_values, fb.max_read_len))
    ws = torch.zeros(need, dtype=torch.uint8, device=_dev())
    out = torch.full((fb.n_reads * 16 + 64,), 0xA5, dtype=torch.uint8, device=_dev())
    stream = int(torch.cuda.current_stream().cuda_stream)
    rc = L.sgk_stat_f32(*fb.view(), out.data_ptr(), ws.data_ptr(), need - 1, stream)
    torch.cuda.synchronize()
    assert rc == api.SGK_ERR_WORKSPACE and bool((out == 0xA5).all())
    rc = L.sgk_stat_f32(*fb.view(), out.data_ptr(), ws.data_ptr(), need, stream)
    torch.cuda.synchronize()
    assert rc == api.SGK_OK
    host = out.cpu().numpy()
    assert (host[fb.n_reads * 16:] == 0xA5).all()
    recs = host[:fb.n_reads * 16].view(api.STATF_DTYPE)
    _check(recs, arrays, oracle, "documented workspace")   # (every flags word is 0)
