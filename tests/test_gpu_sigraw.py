"""GPU: k_sigraw_gather (sgk_sigraw_gather) alone -- the plain int16 signal of BLOW5 records moved from any byte residue
of the record buffer to the aligned sample arena.  The expected samples are a numpy slice of the record bytes; the arena
is pre-filled, so a sample written outside a read's range shows; records lie back to back at odd offsets between 0xA5
canaries, so a byte read from outside a signal shows wherever it lands in a read's samples."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0x5B5B            # what the arena holds beforehand (no sample of the test data equals it: signal() stays below 0x2000)
CANARY = b"\xa5"


def unit():
    from sigtk_amd import device
    return device.sigraw_unit_samples()


def signal(n, seed):
    """n samples, none equal to FILL and no byte pair equal to the canary pair: values in [-0x2000, 0x2000)"""
    return np.random.RandomState(seed).randint(-0x2000, 0x2000, n).astype("<i2")


class Layout:
    """records back to back in one byte buffer (16 canary bytes in front), reads in one arena"""

    def __init__(self):
        self.chunks, self.pos = [CANARY * 16], 16
        self.rec_off, self.rec_len, self.sig_off, self.lengths, self.rec_status, self.want, self.status = [], [], [], [], [], [], []

    def add(self, head, n, seed, gap, rec_len=None, sig_off=None, rec_status=0, want_status=0, tail=b""):
        """a record of `head` bytes, n samples and `tail` bytes at the current position, `gap` canary bytes behind it;
        rec_len / sig_off: what the kernel is told, when that is not the truth"""
        sig = signal(n, seed)
        rec = bytes((seed * 7 + k) % 160 for k in range(head)) + sig.tobytes() + tail
        self.rec_off.append(self.pos)
        self.rec_len.append(len(rec) if rec_len is None else rec_len)
        self.sig_off.append(head if sig_off is None else sig_off)
        self.lengths.append(n)
        self.rec_status.append(rec_status)
        self.status.append(want_status)
        self.want.append(sig if want_status == 0 else None)
        self.chunks.append(rec + CANARY * gap)
        self.pos += len(rec) + gap

    def residues(self):
        return {(o + s) % 16 for o, s, st in zip(self.rec_off, self.sig_off, self.status) if st == 0}

    def run(self, with_rec_status=False, max_len=None, n_samples=None):
        import torch
        from sigtk_amd import device
        dev = torch.device("cuda", 0)
        n = len(self.lengths)
        buf = np.frombuffer(b"".join(self.chunks) + CANARY * 16, dtype=np.uint8)
        buf = np.concatenate((buf, np.full(-buf.size % 16 + 16, 0xA5, dtype=np.uint8)))     # whole words, and one behind
        offs, o = [], 8
        for ln in self.lengths:                 # multiples of 8 samples, 8 - 24 samples of padding between reads
            offs.append(o)
            o += (ln + 7) // 8 * 8 + 8 * (1 + len(offs) % 3)
        arena = np.full(o + 8, FILL, dtype=np.int16)
        i32 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.uint32).view(np.int32)).to(dev)
        i64 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.uint64).view(np.int64)).to(dev)
        d_buf, d_arena = torch.from_numpy(buf.copy()).to(dev), torch.from_numpy(arena.copy()).to(dev)
        assert d_buf.data_ptr() % 16 == 0 and d_arena.data_ptr() % 16 == 0
        st = device.sigraw_gather(d_buf, i64(self.rec_off), i32(self.rec_len), i32(self.sig_off), d_arena, i64(offs),
                                  i32(self.lengths), max(self.lengths) if max_len is None else max_len,
                                  rec_status=i32(self.rec_status) if with_rec_status else None, n_samples=n_samples)
        torch.cuda.synchronize()
        assert np.array_equal(d_buf.cpu().numpy(), buf), "the record buffer is only read"
        got = d_arena.cpu().numpy()
        st = st.cpu().numpy()[:n]
        assert [int(x) for x in st] == self.status
        outside = np.ones(got.size, dtype=bool)
        for r in range(n):
            own = got[offs[r]:offs[r] + self.lengths[r]]
            outside[offs[r]:offs[r] + self.lengths[r]] = False
            if self.status[r] == 0:
                assert np.array_equal(own, self.want[r]), (r, self.lengths[r], (self.rec_off[r] + self.sig_off[r]) % 16)
            elif self.status[r] == 2:
                assert np.all(own == FILL), (r, "a record that did not inflate is not moved")
            else:       # undefined, but never bytes the contract forbids reading: canaries, or the next record's bytes
                lo = self.rec_off[r] // 16 * 16
                hi = (self.rec_off[r] + self.rec_len[r] + 15) // 16 * 16
                seen = np.concatenate((buf[lo:hi], np.frombuffer(np.int16(FILL).tobytes() * 8, dtype=np.uint8)))
                assert np.all(np.isin(own.view(np.uint8), seen)), (r, "bytes from outside the record's words")
        assert np.all(got[outside] == FILL), "samples outside the reads' ranges keep their bytes"
        return got


def lengths_of_interest():
    u = unit()
    return [0, 1, 2, 7, 8, 9, 63, 64, 65, u - 1, u, u + 1, 2 * u + 1, 3 * u + 5]


def test_every_length_at_every_residue(gpu):
    """14 lengths x 16 residues in one launch: the head length steps the residue, record starts are odd and even"""
    lay = Layout()
    k = 0
    for n in lengths_of_interest():
        for res in range(16):
            head = 46 + (res - lay.pos - 46) % 16          # >= the 46 bytes of a head with an empty id
            assert (lay.pos + head) % 16 == res
            lay.add(head, n, 100 + k, gap=1 + (k * 5) % 16, tail=bytes([0x77]) * (k % 4))
            k += 1
    assert lay.residues() == set(range(16))
    assert {o % 2 for o in lay.rec_off} == {0, 1}
    lay.run()
    lay.run(with_rec_status=True)                     # a status array of zeros changes nothing
    lay.run(max_len=1, n_samples=0)                   # a wrong launch bound costs time only: one workgroup per read
    lay.run(n_samples=1)


def test_a_signal_that_ends_with_its_buffers_last_word(gpu):
    """the last record ends exactly at a multiple of 16: the word behind it is not the buffer's (it is allocated, as the
    contract asks, and holds canaries that must not show)"""
    for n in (8, 13, 64):
        for res in (0, 2, 15):
            lay = Layout()
            head = 46 + (res - lay.pos - 46) % 16
            end = lay.pos + head + 2 * n
            lay.add(head, n, n + res, gap=0, tail=b"\x11" * (-end % 16))
            lay.run()


def test_status_cases(gpu):
    lay = Layout()
    u = unit()
    # sound records around the bad ones; every bad record's successor lies directly behind it (gap 0)
    lay.add(51, 100, 1, gap=3)
    lay.add(47, 40, 2, gap=0, rec_len=47 + 80 - 1, want_status=1)            # one byte shorter than its signal
    lay.add(49, 33, 3, gap=0)
    lay.add(60, 40, 4, gap=0, rec_len=59, want_status=1)                     # ends in front of its signal
    lay.add(46, u + 3, 5, gap=0)
    lay.add(46, 9, 6, gap=0, rec_len=0, want_status=1)                       # rec_lengths 0, samples announced
    lay.add(53, 0, 7, gap=0, rec_len=0, sig_off=0, want_status=0)            # ... none announced: nothing to move
    lay.add(46, 2 * u, 8, gap=0, rec_len=46 + 4 * u - 2, want_status=1)      # a long read cut by one sample
    lay.add(57, 17, 9, gap=5)
    lay.add(46, 5, 10, gap=0, sig_off=0xfffffffc, want_status=1)             # the sum needs more than 32 bits
    lay.add(46, 12, 11, gap=2)
    lay.run()
    lay.run(with_rec_status=True)


def test_records_that_did_not_inflate_are_not_read(gpu):
    lay = Layout()
    lay.add(50, 70, 21, gap=0)
    lay.add(48, 300, 22, gap=0, rec_len=0xdeadbeef, rec_status=8, want_status=2)      # garbage length word
    lay.add(46, 64, 23, gap=0)
    lay.add(46, 10, 24, gap=0, rec_len=3, rec_status=6, want_status=2)
    lay.add(46, 0, 25, gap=0, rec_status=1, want_status=2)
    lay.add(61, 129, 26, gap=4)
    lay.run(with_rec_status=True)
    # without rec_status the same records are judged by their lengths alone
    lay.status = [0, 0, 0, 1, 0, 0]
    lay.want[1], lay.want[4] = signal(300, 22), signal(0, 25)
    lay.run(with_rec_status=False)


def test_six_hundred_reads_in_one_launch(gpu):
    lay = Layout()
    lens = [0, 1, 7, 8, 9, 63, 64, 65, 200, 1000]
    for k in range(600):
        bad = k % 37 == 5
        n = lens[k % len(lens)] + k % 3
        lay.add(46 + k % 29, n, 1000 + k, gap=k % 7, rec_len=(46 + k % 29 + 2 * n - 1) if bad and n else None,
                want_status=1 if bad and n else 0)
    assert lay.residues() == set(range(16))
    lay.run()


def test_no_reads(gpu):
    import torch
    from sigtk_amd import api, device
    dev = torch.device("cuda", 0)
    buf = torch.full((64,), 0xA5, dtype=torch.uint8, device=dev)
    arena = torch.full((64,), FILL, dtype=torch.int16, device=dev)
    e64, e32 = torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    st = device.sigraw_gather(buf, e64, e32, e32, arena, e64, e32, 0)
    torch.cuda.synchronize()
    assert int(st[0]) == -1 and bool((arena == FILL).all()) and bool((buf == 0xA5).all())
    # null pointers with reads are refused, a misaligned buffer too
    L = api.load_library()
    assert L.sgk_sigraw_gather(None, None, None, None, None, 1, None, None, None, 8, 0, None, None) == api.SGK_ERR_ARG
    z64, z32 = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(api.SigtkGpuError):
        device.sigraw_gather(buf[1:], z64, z32, z32, arena, z64, z32, 0)
