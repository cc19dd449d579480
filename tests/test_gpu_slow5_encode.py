"""GPU: the raw_signal column of text SLOW5 records written on the device (sgk_slow5_text_*, csrc/slow5_text_kernels.hip)
against b",".join in numpy -- rows, row offsets, every alignment of the output, the straight-to-global path, the capacity
and workspace checks -- and sgk_job_submit_qts with SGK_SIGNAL_TEXT on either side."""
import ctypes as C
import os

import numpy as np
import pytest

from sigtk_amd import blow5

pytestmark = pytest.mark.gpu

CANARY = 96          # bytes on both sides of every buffer the kernels write
FILL = 0xA5


def join(x) -> bytes:
    return b",".join(b"%d" % int(v) for v in np.asarray(x).tolist())


def rows_of(arrays, heads, tails):
    return [(heads[r] if heads else b"") + join(a) + (tails[r] if tails else b"") for r, a in enumerate(arrays)]


class Harness:
    """one resident batch and its buffers, each between canaries: workspace, row offsets, text"""

    def __init__(self, gpu, arrays, heads=None, tails=None, ws_items=None):
        import torch
        from sigtk_amd import device
        self.torch, self.gpu, self.L = torch, gpu, gpu.load_library()
        self.dev = torch.device("cuda", 0)
        lens = np.array([len(a) for a in arrays], dtype=np.int64)
        self.b = device.alloc_reads(lens, self.dev)
        host = np.full(self.b.n_samples, 12345, dtype=np.int16)   # gaps are arbitrary data
        for r, a in enumerate(arrays):
            o = int(self.b.offsets_host[r]); host[o:o + len(a)] = a
        self.b.samples.copy_(torch.from_numpy(host).to(self.dev))
        self.n = len(arrays)
        self.keep = []
        self.heads, self.tails = self._ids(heads), self._ids(tails)
        self.ws_bytes = int(self.L.sgk_slow5_text_workspace_bytes(self.n, int(lens.sum()) if ws_items is None else ws_items))
        self.ws = torch.full((CANARY + self.ws_bytes + CANARY,), FILL, dtype=torch.uint8, device=self.dev)
        assert (self.ws.data_ptr() + CANARY) % 16 == 0
        self.roffs = torch.full((CANARY // 8 + self.n + 1 + CANARY // 8,), -2, dtype=torch.int64, device=self.dev)

    def _ids(self, parts):
        if parts is None:
            return None
        offs = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum([len(p) for p in parts], out=offs[1:])
        d_bytes = self.torch.from_numpy(np.frombuffer(b"".join(parts) + b"\0" * 16, dtype=np.uint8).copy()).to(self.dev)
        d_offs = self.torch.from_numpy(offs.astype(np.uint32).view(np.int32)).to(self.dev)
        self.keep += [d_bytes, d_offs]
        return self.gpu.TextIds(d_bytes.data_ptr(), d_offs.data_ptr())

    def _rows(self):
        b = self.b
        return (b.samples.data_ptr(), b.offsets.data_ptr(), b.lengths.data_ptr(), self.n,
                C.byref(self.heads) if self.heads is not None else None, C.byref(self.tails) if self.tails is not None else None)

    def measure(self):
        rc = self.L.sgk_slow5_text_measure(*self._rows(), self.roffs.data_ptr() + CANARY, self.ws.data_ptr() + CANARY,
                                           self.ws_bytes, None)
        self.torch.cuda.synchronize()
        return rc

    def row_offsets(self):
        ro = self.roffs.cpu().numpy()
        k = CANARY // 8
        assert (ro[:k] == -2).all() and (ro[k + self.n + 1:] == -2).all()
        return ro[k:k + self.n + 1].astype(np.uint64)

    def write(self, total, align=0, capacity=None):
        """-> (rc of the call, rc of sgk_text_status, status, the whole text buffer as numpy, offset of `text` in it)"""
        buf = self.torch.full((CANARY + 16 + total + CANARY,), FILL, dtype=self.torch.uint8, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        at = CANARY + align
        rc = self.L.sgk_slow5_text_write(*self._rows(), buf.data_ptr() + at, total if capacity is None else capacity,
                                         self.ws.data_ptr() + CANARY, self.ws_bytes, None)
        self.torch.cuda.synchronize()
        st = self.gpu.TextStatus()
        rc2 = self.L.sgk_text_status(self.ws.data_ptr() + CANARY, C.byref(st))
        ws = self.ws.cpu().numpy()
        assert (ws[:CANARY] == FILL).all() and (ws[CANARY + self.ws_bytes:] == FILL).all()
        return rc, rc2, st, buf.cpu().numpy(), at


def check(gpu, arrays, heads=None, tails=None, aligns=(0,)):
    h = Harness(gpu, arrays, heads, tails)
    want_rows = rows_of(arrays, heads, tails)
    want = b"".join(want_rows)
    assert h.measure() == 0
    ro = h.row_offsets()
    assert np.array_equal(ro, np.concatenate([[0], np.cumsum([len(r) for r in want_rows])]).astype(np.uint64))
    for al in aligns:
        rc, rc2, st, buf, at = h.write(len(want), al)
        assert (rc, rc2, st.overflow, st.n_bytes) == (0, 0, 0, len(want))
        assert buf[at:at + len(want)].tobytes() == want, al
        assert (buf[:at] == FILL).all() and (buf[at + len(want):] == FILL).all(), al
    return h, want


def test_one_read_of_every_int16_value_and_the_round_trip(gpu):
    from sigtk_amd import device
    x = np.random.RandomState(5).permutation(np.arange(-32768, 32768)).astype(np.int16)
    _, text = check(gpu, [x], aligns=(0, 7))
    assert text == join(x)
    reads, status = device.sigtext_decode([text], [x.size], Harness(gpu, [x]).dev)
    import torch
    torch.cuda.synchronize()
    o = int(reads.offsets_host[0])
    assert int(status[0]) == 0 and np.array_equal(reads.samples[o:o + x.size].cpu().numpy(), x)


def fixed_parts(n, seed):
    """head and tail lengths 0, 1, 15, 16, 17 and 300 in every combination, holding tabs, commas and bytes >= 0x80"""
    rs = np.random.RandomState(seed)
    alphabet = np.frombuffer(b"\t,\n-0123456789ab\x80\xff\xe9", dtype=np.uint8)
    sizes = (0, 1, 15, 16, 17, 300)
    heads = [alphabet[rs.randint(0, alphabet.size, sizes[r % 6])].tobytes() for r in range(n)]
    tails = [alphabet[rs.randint(0, alphabet.size, sizes[(r // 6) % 6])].tobytes() for r in range(n)]
    return heads, tails


def test_lengths_fixed_parts_empty_rows_and_every_alignment(gpu):
    rs = np.random.RandomState(9)
    lens = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000] * 3        # 39 reads: all 36 head x tail sizes
    arrays = [rs.randint(-32768, 32768, n).astype(np.int16) for n in lens]
    heads, tails = fixed_parts(len(arrays), 10)
    # a run of rows of 0 bytes between short rows: tiles share 16-byte words of the output
    for r, n in ((len(arrays), 1), (len(arrays) + 1, 0), (len(arrays) + 2, 0), (len(arrays) + 3, 0), (len(arrays) + 4, 0),
                 (len(arrays) + 5, 2), (len(arrays) + 6, 0), (len(arrays) + 7, 1)):
        arrays.append(rs.randint(-9, 10, n).astype(np.int16))
        heads.append(b"" if n == 0 else b"\t"); tails.append(b"" if n == 0 else b"\n")
    assert {(len(h), len(t)) for h, t in zip(heads, tails)} >= {(a, b) for a in (0, 1, 15, 16, 17, 300) for b in (0, 1, 15, 16, 17, 300)}
    check(gpu, arrays, heads, tails, aligns=range(16))
    check(gpu, arrays, None, None, aligns=(0, 3))            # bare columns
    check(gpu, arrays, heads, None, aligns=(5,))
    check(gpu, arrays, None, tails, aligns=(11,))
    check(gpu, [], [], [])                                   # no reads: row_offsets[0] = 0, nothing written


def test_fixed_parts_longer_than_the_lds_image(gpu):
    """a head and a tail longer than a tile's LDS image (SGK_SLOW5_TEXT_STAGE_BYTES): those tiles write straight to
    global memory; the read of 600 samples has a first tile (long head), a middle one and a last one (long tail)"""
    stage = gpu.SLOW5_TEXT_STAGE_BYTES
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(gpu.__file__))), "include", "sigtk_gpu.h")).read()
    assert "#define SGK_SLOW5_TEXT_STAGE_BYTES %d\n" % stage in src
    rs = np.random.RandomState(11)
    arrays = [rs.randint(-32768, 32768, n).astype(np.int16) for n in (600, 3, 0, 256, 70)]
    blob = lambda n: rs.randint(0, 256, n).astype(np.uint8).tobytes()
    heads = [blob(stage + 1), blob(stage - 7 * 3), blob(stage), blob(10), blob(70001)]
    tails = [blob(stage + 5), blob(19), blob(1), blob(stage * 3 + 3), blob(100001)]
    check(gpu, arrays, heads, tails, aligns=(0, 1, 15))


def test_capacity_and_workspace_are_checked_on_the_device(gpu):
    rs = np.random.RandomState(12)
    arrays = [rs.randint(-32768, 32768, n).astype(np.int16) for n in (300, 0, 700, 5)]
    heads, tails = [b"h0\t", b"", b"head-two\t", b"\t"], [b"\n", b"x", b"\tz\n", b"\n"]
    h, want = check(gpu, arrays, heads, tails)
    total = len(want)
    rc, rc2, st, buf, at = h.write(total, 3, capacity=total - 1)
    assert rc == 0 and rc2 == gpu.SGK_ERR_CAPACITY and st.overflow == 1
    # tiles: 2 + 1 + 3 + 1; the last one ("\t" + 5 samples + "\n") does not fit and nothing of it is written
    last = len(rows_of(arrays[3:], heads[3:], tails[3:])[0])
    assert buf[at:at + total - last].tobytes() == want[:total - last]
    assert (buf[:at] == FILL).all() and (buf[at + total - last:] == FILL).all()
    rc, rc2, st, buf, at = h.write(total, 0, capacity=0)
    assert rc2 == gpu.SGK_ERR_CAPACITY and (buf == FILL).all()
    # a workspace sized for fewer samples than the batch holds: nothing is measured or written
    small = Harness(gpu, [rs.randint(-99, 100, 256 * 40).astype(np.int16)], [b"h"], [b"\n"], ws_items=256)   # 40 tiles, room for 8
    assert small.ws_bytes < Harness(gpu, [np.zeros(256 * 40, np.int16)]).ws_bytes
    assert small.measure() == 0
    rc, rc2, st, buf, at = small.write(total)
    assert rc == 0 and rc2 == gpu.SGK_ERR_WORKSPACE and (buf == FILL).all()
    assert small.L.sgk_slow5_text_measure(*small._rows(), small.roffs.data_ptr() + CANARY, small.ws.data_ptr() + CANARY, 32,
                                          None) == gpu.SGK_ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------- jobs

def quantise(x, bits, method):
    """src/qts.c:27-43, 126-142 on int16 (int arithmetic, truncated back to int16 on assignment)"""
    x = np.asarray(x, dtype=np.int64)
    mask = (1 << bits) - 1
    if method == 0:
        e = (x >> bits) << bits
    elif method == 2:
        e = x | mask
    else:
        e = np.where((x & mask) < (1 << (bits - 1)), x & ~mask, (x & ~mask) + (1 << bits))
    return e.astype(np.int16)


@pytest.fixture(scope="module")
def job_reads():
    rs = np.random.RandomState(13)
    lens = [0, 1, 2, 255, 256, 257, 3000, 1025, 17, 64, 700, 1, 0, 513, 90, 2999, 33, 8, 1500, 256]
    raws = [rs.randint(-32768, 32768, n).astype(np.int16) for n in lens]
    raws[3][:8] = [-32768, -32767, 32767, 32766, 32640, 32639, -1, 0]        # the int16 edges, where round wraps
    raws[6][-4:] = [32767, -32768, 32760, 32763]
    heads, tails = fixed_parts(len(raws), 14)
    return raws, heads, tails


@pytest.mark.parametrize("fmt", ["int16", "svbzd", "text"])
def test_qts_jobs_write_text_from_every_input_format(gpu, job_reads, fmt):
    raws, heads, tails = job_reads
    n = len(raws)
    dig, off, rng = [8192.0] * n, [3.0] * n, [1402.882324] * n
    job = gpu.Job(0)
    try:
        def stage():
            if fmt == "int16":
                job.stage(raws, dig, off, rng)
            elif fmt == "svbzd":
                job.stage([blow5.svb_zd_encode(r) for r in raws], dig, off, rng, counts=[r.size for r in raws])
            else:
                job.stage([blow5.slow5_signal_text(r) for r in raws], dig, off, rng, counts=[r.size for r in raws], text=True)
        for method in (0, 1, 2):
            for bits in (1, 3, 8):
                q = [quantise(r, bits, method) for r in raws]
                stage()
                job.launch_qts(bits, method, False, out_text=True)
                res = job.wait()
                want = rows_of(q, None, None)
                assert res["text"] == b"".join(want), (method, bits)
                assert np.array_equal(res["row_offsets"], np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64))
                job.set_record_frames([h + t for h, t in zip(heads, tails)], [len(h) for h in heads])
                job.launch_qts(bits, method, False, records=True, out_text=True)
                res = job.wait()
                want = rows_of(q, heads, tails)
                assert res["text"] == b"".join(want), (method, bits, "frames")
                assert np.array_equal(res["row_offsets"], np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64))
        # a new batch forgets the frames: whole lines without them are refused, as for the deflated records
        stage()
        with pytest.raises(gpu.SigtkGpuError):
            job.launch_qts(3, 1, False, records=True, out_text=True)
        job.launch_qts(3, 1, True)
        blobs = job.wait()["blobs"]
        assert blobs == [blow5.svb_zd_encode(quantise(r, 3, 1)) for r in raws]       # text in, svb-zd out = int16 in, svb-zd out
    finally:
        job.close()


def test_a_text_column_that_does_not_decode_ends_the_qts_job(gpu, job_reads):
    raws = job_reads[0]
    n = len(raws)
    texts = [blow5.slow5_signal_text(r) for r in raws]
    texts[6] = texts[6][:50] + b"x" + texts[6][51:]
    job = gpu.Job(0)
    try:
        job.stage(texts, [8192.0] * n, [3.0] * n, [1402.5] * n, counts=[r.size for r in raws], text=True)
        job.launch_qts(3, 1, False, out_text=True)
        rc, ds = job.wait_rc()
        want = np.zeros(n, np.uint32); want[6] = 2
        assert rc == gpu.SGK_ERR_FORMAT and np.array_equal(ds, want)
    finally:
        job.close()
