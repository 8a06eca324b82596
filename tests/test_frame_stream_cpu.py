"""The streamed frame loop without a device (moephoto_amd/procedure.py: FrameStream, genFrameStream, runFramesStreamed; include/moephoto_amd.h: moe_stitch_out,
moe_run_plan_out): the ring's ordering logic against a fake backend whose events refuse to be waited on before they are recorded, the loop against runFrames, and
what the new entry points and genFrameStream refuse before anything touches a device."""
import ctypes
import io

import numpy as np
import pytest

from moephoto_amd import _lib, imageProcess as ip, procedure

H, W = 4, 6


class FakeEvent(object):
    """recorded: how often it was enqueued behind a stage; fired: how many of those stages have run.  A wait refers to the record in front of it, as a HIP event's."""
    def __init__(self):
        self.recorded = self.fired = 0

    def target(self):
        assert self.recorded > 0, 'an event was waited on before it was recorded'
        return self.recorded


class FakeBackend(object):
    """Three in-order queues that run NOTHING until the host waits, and then only what that wait needs, picking among the runnable queue heads in the order of
    `priority` -- so a stage runs before another one of a different queue only if an event says so, and a missing wait shows as a broken hazard below.  Per slot it
    keeps what the hazards are about: whether the compute has read the raw buffer, whether the download has read the output buffer.  The stand-in computation halves
    every sample, as the stand-in process of test_video_buffer_edges_and_frame_loop does."""

    def __init__(self, depth, bitDepth=16, priority=('upload', 'compute', 'download')):
        self.dtype = np.uint16 if bitDepth > 8 else np.uint8
        self.priority = priority
        self.queues = dict(upload=[], compute=[], download=[])
        self.pinned = [None] * depth       # host side of the upload: written by the host at push time
        self.raw = [None] * depth          # [frame bytes, consumed by compute?]
        self.out = [None] * depth          # [result bytes, consumed by download?]
        self.host = [None] * depth
        self.log = []                      # (stage, slot, number of waits) in enqueue order
        self.ran = []                      # (stage, slot) in execution order
        self.aborted = self.closed_calls = 0

    def event(self):
        return FakeEvent()

    def _enqueue(self, name, slot, wait, record, work):
        targets = [(e, e.target()) for e in wait]
        record.recorded += 1
        self.log.append((name, slot, len(wait)))
        self.queues[name].append((slot, targets, record, work))

    def _run_one(self):
        for name in self.priority:
            q = self.queues[name]
            if q and all(e.fired >= t for e, t in q[0][1]):
                slot, _, record, work = q.pop(0)
                work()
                self.ran.append((name, slot))
                record.fired += 1
                return
        raise AssertionError('deadlock: no queue head is runnable')

    def upload(self, slot, raw, wait, record):
        self.pinned[slot] = raw            # (the ring guarantees the previous H2D of this slot is over: checked in work())

        def work():
            assert self.raw[slot] is None or self.raw[slot][1], 'slot {}: uploaded into before its previous compute'.format(slot)
            assert self.pinned[slot] is raw, 'slot {}: the pinned input was overwritten before its copy ran'.format(slot)
            self.raw[slot] = [raw, False]
        self._enqueue('upload', slot, wait, record, work)

    def compute(self, slot, wait, record):
        def work():
            assert self.out[slot] is None or self.out[slot][1], 'slot {}: computed into before its previous download'.format(slot)
            assert self.raw[slot] is not None and not self.raw[slot][1], 'slot {}: computed before its upload'.format(slot)
            self.raw[slot][1] = True
            self.out[slot] = [(np.frombuffer(self.raw[slot][0], self.dtype) // 2).tobytes(), False]
        self._enqueue('compute', slot, wait, record, work)

    def download(self, slot, wait, record):
        def work():
            assert self.out[slot] is not None and not self.out[slot][1], 'slot {}: downloaded before its compute'.format(slot)
            self.out[slot][1] = True
            self.host[slot] = self.out[slot][0]
        self._enqueue('download', slot, wait, record, work)

    def wait(self, slot, event):
        t = event.target()
        while event.fired < t:
            self._run_one()
        return self.host[slot]

    def abort(self):
        self.aborted += 1

    def close(self):
        self.closed_calls += 1


PRIORITIES = [('upload', 'compute', 'download'), ('download', 'compute', 'upload'), ('compute', 'upload', 'download'), ('upload', 'download', 'compute')]


def _frames(n, seed=7):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 65536, (H, W, 3), dtype=np.uint16) for _ in range(n)]


@pytest.mark.parametrize('priority', PRIORITIES, ids='-'.join)
@pytest.mark.parametrize('depth', [1, 2, 3, 4])
def test_ring_order_and_hazards(depth, priority):
    frames = _frames(7)
    b = FakeBackend(depth, priority=priority)
    s = procedure.FrameStream(b, W, H, 16, depth)
    got = []
    for k, f in enumerate(frames):
        r = s.push(f.tobytes())
        assert len(r) == (0 if k < depth - 1 else 1), (depth, k)      # nothing until depth - 1 frames are in flight, then exactly one per push
        got += r
    assert s.push(b'') == []                                            # an empty buffer: no frame, as genProcess's pipeline
    rest = s.flush()
    assert len(rest) == depth - 1 and s.flush() == []
    got += rest
    assert got == [(f // 2).tobytes() for f in frames]                  # input order
    # frame k used slot k mod depth, and from the second use of a slot on each stage waited for the hazard of the first
    ups = [e for e in b.log if e[0] == 'upload']
    assert [e[1] for e in ups] == [k % depth for k in range(7)]
    assert [e[2] for e in ups] == [0 if k < depth else 1 for k in range(7)]
    assert [e[2] for e in b.log if e[0] == 'compute'] == [1 if k < depth else 2 for k in range(7)]
    assert all(e[2] == 1 for e in b.log if e[0] == 'download')
    s.close()
    assert b.closed_calls == 1
    with pytest.raises(RuntimeError):
        s.push(frames[0].tobytes())


def test_ring_closes_on_a_failing_stage():
    class Failing(FakeBackend):
        def compute(self, slot, wait, record):
            if len([e for e in self.log if e[0] == 'compute']) == 2:
                raise MemoryError('stage failed')
            FakeBackend.compute(self, slot, wait, record)
    b = Failing(2)
    s = procedure.FrameStream(b, W, H, 16, 2)
    f = _frames(3)
    s.push(f[0].tobytes())
    s.push(f[1].tobytes())
    with pytest.raises(MemoryError):
        s.push(f[2].tobytes())
    assert b.aborted == 1 and s.closed          # one synchronise, nothing retried
    with pytest.raises(RuntimeError):
        s.flush()
    s.close()
    s.close()
    assert b.closed_calls == 1                  # the slots are released once, also behind a failure
    with pytest.raises(ValueError):
        procedure.FrameStream(FakeBackend(2), W, H, 16, 2).push(b'123')
    for depth in (0, 5, True, 2.0):
        with pytest.raises(ValueError):
            procedure.FrameStream(FakeBackend(4), W, H, 16, depth)


def _serial_process(frame):          # the stand-in of test_video_buffer_edges_and_frame_loop
    return [ip.toBuffer(16)(ip.toNumPy(16)(frame) // 2)]


@pytest.mark.parametrize('depth', [1, 2, 3])
def test_run_frames_streamed_against_run_frames(depth):
    frames = _frames(5)
    raw = b''.join(f.tobytes() for f in frames)
    for src, kw in ((raw, dict(start=1)), (raw, dict(stop=0)), (b'', {}), (raw, {}), (raw, dict(start=1, stop=3)), (raw, dict(start=9))):
        want, got = [], []
        n0 = procedure.runFrames(_serial_process, io.BytesIO(src).read, want.append, W, H, bitDepth=16, **kw)
        s = procedure.FrameStream(FakeBackend(depth), W, H, 16, depth)
        n1 = procedure.runFramesStreamed(s, io.BytesIO(src).read, got.append, **kw)
        assert n1 == n0 and got == want, kw
    # a short last frame: every earlier frame is written, then the same ValueError
    got = []
    s = procedure.FrameStream(FakeBackend(depth), W, H, 16, depth)
    with pytest.raises(ValueError, match='short frame'):
        procedure.runFramesStreamed(s, io.BytesIO(raw[:-5]).read, got.append)
    assert got == [(f // 2).tobytes() for f in frames[:4]]
    with pytest.raises(ValueError, match='short frame'):
        procedure.runFrames(_serial_process, io.BytesIO(raw[:-5]).read, [].append, W, H, bitDepth=16)


def test_out_entry_points_validate_their_arguments_without_a_device():
    L = _lib.lib()
    plan = ip.TilePlan((3, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    so = L.moe_stitch_out
    assert so(None, 0, p, None, 3, _lib.F32, 8, p, _lib.U8, None) == _lib.EINVAL
    assert so(plan._h, 0, None, None, 3, _lib.F32, 8, p, _lib.U8, None) == _lib.EINVAL
    assert so(plan._h, 0, p, None, 3, _lib.F32, 8, None, _lib.U8, None) == _lib.EINVAL and b'NULL' in L.moe_last_error()
    assert so(plan._h, 0, p, None, 3, _lib.F32, 12, p, _lib.U16, None) == _lib.EINVAL and b'bits' in L.moe_last_error()
    assert so(plan._h, 0, p, None, 3, _lib.F32, 16, p, _lib.U8, None) == _lib.EINVAL and b'MOE_U8' in L.moe_last_error()
    assert so(plan._h, 0, p, None, 0, _lib.F32, 8, p, _lib.U8, None) == _lib.EINVAL
    assert so(plan._h, 0, p, None, 5, _lib.F32, 8, p, _lib.U8, None) == _lib.EINVAL and b'planes' in L.moe_last_error()
    assert so(plan._h, 0, p, None, 3, _lib.U8, 8, p, _lib.U8, None) == _lib.EINVAL and b'canvas' in L.moe_last_error()
    assert so(plan._h, 0, p, None, 3, _lib.F32, 8, p, _lib.F32, None) == _lib.EINVAL and b'dst dtype' in L.moe_last_error()
    h = ctypes.c_void_p()
    _lib.check(L.moe_net_create(_lib.ARCH_NET2X, 2, ctypes.byref(h)))
    try:
        ro = lambda net, pl, img, cdt, bits, dst, ddt: L.moe_run_plan_out(net, pl, img, _lib.F32, 14000, 140, 1, cdt, bits, dst, ddt, 0, None)
        assert ro(None, plan._h, p, _lib.F32, 8, p, _lib.U8) == _lib.EINVAL
        assert ro(h, None, p, _lib.F32, 8, p, _lib.U8) == _lib.EINVAL
        assert ro(h, plan._h, None, _lib.F32, 8, p, _lib.U8) == _lib.EINVAL
        assert ro(h, plan._h, p, _lib.F32, 8, None, _lib.U8) == _lib.EINVAL and b'NULL' in L.moe_last_error()
        assert ro(h, plan._h, p, _lib.F32, 12, p, _lib.U16) == _lib.EINVAL and b'bits' in L.moe_last_error()
        assert ro(h, plan._h, p, _lib.F32, 16, p, _lib.U8) == _lib.EINVAL and b'MOE_U8' in L.moe_last_error()
        assert ro(h, plan._h, p, _lib.F32, 16, p, _lib.U16) == _lib.ESTATE and b'moe_run_plan_out: net is not finalized' in L.moe_last_error()
    finally:
        L.moe_net_destroy(h)


def test_gen_frame_stream_refusals():
    sr = {'op': 'SR', 'model': 'a', 'scale': 2}
    with pytest.raises(ValueError, match='buffer'):
        procedure.genFrameStream([{'op': 'file'}, sr], 88, 72)
    with pytest.raises(ValueError, match='buffer'):
        procedure.genFrameStream([], 88, 72)
    for depth in (0, 5):
        with pytest.raises(ValueError, match='depth'):
            procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 16}, sr], 88, 72, depth=depth)
    with pytest.raises(ValueError, match='bitDepth'):
        procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 12}, sr], 88, 72)
    with pytest.raises(NotImplementedError):          # an op genProcess refuses, refused before any model is loaded
        procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 16}, {'op': 'dehaze'}, sr], 88, 72)
    with pytest.raises(NotImplementedError):
        procedure.genProcess([{'op': 'buffer', 'bitDepth': 16}, {'op': 'dehaze'}])
