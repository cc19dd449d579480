"""One job, one staged batch, every kind of result launched back to back: what a submit leaves behind must not leak into
the next one.  After each wait() the results are byte-equal to those of a fresh job given the same staging and the
same single launch."""
import numpy as np
import pytest

from sigtk_amd import blow5

pytestmark = pytest.mark.gpu

LENS = [0, 1, 63, 64, 65, 300, 5000]


def steps(gpu):
    """(name, launch) in the order they run on the one job"""
    tool = lambda t, flags=0: (lambda job: job.launch(t, rna=0, pore=0, flags=flags))
    qts = lambda **kw: (lambda job: job.launch_qts(3, 1, **kw))
    return [
        ("event", tool(gpu.TOOL_EVENT)),
        ("event text", tool(gpu.TOOL_EVENT, gpu.JOB_TEXT)),
        ("pa", tool(gpu.TOOL_PA)),
        ("pa text", tool(gpu.TOOL_PA, gpu.JOB_TEXT)),
        ("qts svb-zd blobs", qts(out_svb=True)),
        ("stat", tool(gpu.TOOL_STAT)),
        ("qts int16 samples", qts(out_svb=False)),
        ("jnn", tool(gpu.TOOL_JNN)),
        ("qts records", qts(out_svb=True, records=True)),
        ("ent", tool(gpu.TOOL_ENT)),
        ("prefix", tool(gpu.TOOL_PREFIX)),
        ("qts text", qts(out_svb=False, out_text=True)),
        ("event lengths", tool(gpu.TOOL_EVENT, gpu.JOB_EVENTS_LENGTHS)),
        ("event compact", tool(gpu.TOOL_EVENT, gpu.JOB_EVENTS_COMPACT)),
    ]


def frozen(x):
    """a result of Job.wait() as nested tuples of bytes: copied out of the job's buffers, comparable with =="""
    if isinstance(x, dict):
        return tuple((k, frozen(x[k])) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (bytes, int)):
        return x
    return bytes(x)   # (the event status: a ctypes structure)


def staged(gpu, svb):
    reads, dig, off, rng = gpu.synth_reads_host(len(LENS), LENS, seed=20, kind=0)
    rs = np.random.RandomState(5)
    heads = [rs.bytes(40 + r) for r in range(len(LENS))]
    tails = [rs.bytes((0, 1, 37)[r % 3]) for r in range(len(LENS))]
    job = gpu.Job(0)
    if svb:
        job.stage([blow5.svb_zd_encode(r) for r in reads], dig, off, rng, counts=[r.size for r in reads])
    else:
        job.stage(reads, dig, off, rng)
    job.set_ids(["read_%d_%s" % (r, "x" * r) for r in range(len(LENS))])
    job.set_record_frames([h + t for h, t in zip(heads, tails)], [len(h) for h in heads])
    return job


@pytest.mark.parametrize("svb", [False, True], ids=["int16", "svbzd"])
def test_every_result_kind_back_to_back_on_one_staged_batch(gpu, svb):
    fresh = {}
    for name, launch in steps(gpu):
        job = staged(gpu, svb)
        try:
            launch(job)
            fresh[name] = frozen(job.wait())
        finally:
            job.close()
    job = staged(gpu, svb)
    try:
        for name, launch in steps(gpu):
            launch(job)
            got = frozen(job.wait())
            assert [k for k, _ in got] == [k for k, _ in fresh[name]], name
            for (k, a), (_, b) in zip(got, fresh[name]):
                assert a == b, "%s: %s differs from a fresh job's" % (name, k)
    finally:
        job.close()
