"""Chains on the decoder's own Y'CbCr 4:2:0 planes without a device: the written definition (moephoto_amd/pixfmt.py: planeShapes, toPlanes, fromPlanes), what the
builders refuse before a model is loaded, FrameStream with a frame size of its own, and what the three entry points (include/moephoto_amd.h: moe_planes_to_float,
moe_stitch_planes, moe_run_plan_planes) refuse before anything touches a device."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from moephoto_amd import _lib, imageProcess as ip, pixfmt, procedure, runDN, runSR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = {'yuv420p': 8, 'yuv420p10le': 10, 'yuv420p12le': 12, 'yuv420p16le': 16}


def _every_code(fmt):
    """A frame whose Y plane holds every code of the format's depth, and whose chroma planes hold every second one."""
    D = DEPTH[fmt]
    n = 1 << D
    w, h = (32, 8) if D == 8 else (256, n // 256)              # w * h = 2^D samples of luma
    y = np.arange(n, dtype=np.uint32)
    c = y[1::2]                                                # n / 2 chroma samples
    dt = np.uint8 if D == 8 else np.dtype('<u2')
    return np.concatenate([y, c]).astype(dt).tobytes(), w, h


# ---- the definition -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt,dtype', [('yuv420p', np.float16), ('yuv420p10le', np.float16), ('yuv420p', np.float32), ('yuv420p10le', np.float32),
                                       ('yuv420p12le', np.float32), ('yuv420p16le', np.float32)])
def test_every_code_survives_the_round_trip(fmt, dtype):
    frame, w, h = _every_code(fmt)
    Y, C = pixfmt.toPlanes(frame, fmt, w, h, dtype)
    assert Y.shape == (1, h, w) and C.shape == (2, h // 2, w // 2) and Y.dtype == C.dtype == np.dtype(dtype)
    D = DEPTH[fmt]
    codes = np.frombuffer(frame, np.uint8 if D == 8 else np.dtype('<u2'))
    assert np.array_equal(Y.reshape(-1).astype(np.float64) * (1 << D), codes[:w * h].astype(np.float64))          # code * 2^-D, exactly
    assert pixfmt.fromPlanes(Y, C, fmt) == frame
    assert pixfmt.fromPlanes(Y[0], C, fmt) == frame                      # (a bare (h, w) Y plane is taken too)


def test_fp16_rounds_twelve_bit_codes_to_nearest_even():
    codes = np.array([2049, 2051, 4095, 4094], dtype='<u2')              # 12 significant bits: halfway between two fp16 neighbours
    frame = np.concatenate([codes, np.full(2, 2048, '<u2')]).tobytes()
    Y, _ = pixfmt.toPlanes(frame, 'yuv420p12le', 2, 2, np.float16)
    assert (Y.reshape(-1).astype(np.float64) * 4096).tolist() == [2048.0, 2052.0, 4096.0, 4094.0]


def test_eight_bits_to_ten_is_a_shift_and_neutral_chroma_is_half():
    frame, w, h = _every_code('yuv420p')
    for dtype in (np.float16, np.float32):
        Y, C = pixfmt.toPlanes(frame, 'yuv420p', w, h, dtype)
        out = np.frombuffer(pixfmt.fromPlanes(Y, C, 'yuv420p10le'), '<u2')
        assert np.array_equal(out, np.frombuffer(frame, np.uint8).astype(np.uint16) * 4)
    for fmt, D in DEPTH.items():
        code = 128 << (D - 8)
        f = np.full(6, code, np.uint8 if D == 8 else np.dtype('<u2')).tobytes()
        Y, C = pixfmt.toPlanes(f, fmt, 2, 2, np.float16)
        assert (C == 0.5).all() and (Y == 0.5).all()
    # uint16 codes are taken as they are: a 10-bit frame with a high bit set is a value above 1
    Y, _ = pixfmt.toPlanes(np.array([1024 + 512, 0, 0, 0, 0, 0], '<u2').tobytes(), 'yuv420p10le', 2, 2)
    assert Y[0, 0, 0] == 1.5


@pytest.mark.parametrize('fmt', sorted(DEPTH))
def test_offsets_and_shapes_agree_with_plane_offsets(fmt):
    for w, h in ((2, 2), (16, 2), (18, 10), (140, 100)):
        (yh, yw), (ch, cw) = pixfmt.planeShapes(fmt, w, h)
        assert (yh, yw, ch, cw) == (h, w, h // 2, w // 2)
        es = 1 if DEPTH[fmt] == 8 else 2
        y0, cb, cr, end = pixfmt.planeOffsets(fmt, w, h)
        assert (y0, cb, cr, end) == (0, yh * yw * es, (yh * yw + ch * cw) * es, (yh * yw + 2 * ch * cw) * es) and end == pixfmt.frameBytes(fmt, w, h)
        q = (1 << DEPTH[fmt]) - 1
        Y = np.full((1, h, w), 1 / (1 << DEPTH[fmt]), np.float32)                       # code 1
        C = np.stack([np.full((ch, cw), 2 / (1 << DEPTH[fmt]), np.float32), np.full((ch, cw), 1.0, np.float32)])      # codes 2 and the maximum
        a = np.frombuffer(pixfmt.fromPlanes(Y, C, fmt), np.uint8 if es == 1 else np.dtype('<u2'))
        assert a.size * es == end
        assert (a[:cb // es] == 1).all() and (a[cb // es:cr // es] == 2).all() and (a[cr // es:] == q).all()
        rt = pixfmt.toPlanes(a.tobytes(), fmt, w, h)
        assert rt[0].shape == (1, h, w) and rt[1].shape == (2, ch, cw) and (rt[1][0] * (1 << DEPTH[fmt]) == 2).all()


def test_quantiser_clamps_truncates_and_zeroes_nan():
    for fmt, D in DEPTH.items():
        q = 1 << D
        vals = np.array([-0.25, -0.0, 0.0, 0.5 / q, 0.999 / q, 1.0 / q, 1.999 / q, (q - 1) / q, (q - 0.5) / q, 1.0, 1.25, np.inf, -np.inf, np.nan, 0.5, 0.25],
                        np.float32)
        want = [0, 0, 0, 0, 0, 1, 1, q - 1, q - 1, q - 1, q - 1, q - 1, 0, 0, q // 2, q // 4]
        Y = vals.reshape(1, 4, 4)
        C = np.stack([vals[:4].reshape(2, 2), vals[10:14].reshape(2, 2)])
        a = np.frombuffer(pixfmt.fromPlanes(Y, C, fmt), np.uint8 if D == 8 else np.dtype('<u2'))
        assert a[:16].tolist() == want and a[16:20].tolist() == want[:4] and a[20:].tolist() == want[10:14], fmt
        h16 = np.frombuffer(pixfmt.fromPlanes(Y.astype(np.float16), C.astype(np.float16), fmt), a.dtype)           # an fp16 image is widened, then quantised
        assert h16[[0, 9, 10, 11, 12, 13, 14]].tolist() == [0, q - 1, q - 1, q - 1, 0, 0, q // 2]


def test_definition_refusals():
    for w, h in ((3, 2), (2, 3), (0, 2), (2, 0), (-2, 2), (141, 100)):
        with pytest.raises(ValueError, match='even'):
            pixfmt.planeShapes('yuv420p', w, h)
    with pytest.raises(ValueError, match='pixFmt'):
        pixfmt.planeShapes('nv12', 2, 2)
    with pytest.raises(ValueError, match='bytes'):
        pixfmt.toPlanes(b'\0' * 5, 'yuv420p', 2, 2)
    with pytest.raises(ValueError, match='dtype'):
        pixfmt.toPlanes(b'\0' * 6, 'yuv420p', 2, 2, np.float64)
    with pytest.raises(ValueError, match='chroma'):
        pixfmt.fromPlanes(np.zeros((1, 4, 4), np.float32), np.zeros((2, 2, 3), np.float32), 'yuv420p')
    with pytest.raises(ValueError, match='expected'):
        pixfmt.fromPlanes(np.zeros((3, 4, 4), np.float32), np.zeros((2, 2, 2), np.float32), 'yuv420p')


# ---- the builders ---------------------------------------------------------------------------------------------------------------------------
def test_builders_refuse_before_a_model_is_loaded(monkeypatch):
    def no_model(*_a, **_k):
        raise AssertionError('a model was asked for before the chain was checked')
    monkeypatch.setattr(runSR, 'getOpt', no_model)
    monkeypatch.setattr(runDN, 'getOpt', no_model)
    buf, sr = {'op': 'buffer', 'pixFmt': 'yuv420p10le'}, {'op': 'SR', 'model': 'a', 'scale': 2}
    rs = {'op': 'resize', 'width': 10, 'height': 6}
    for w, h in ((141, 100), (140, 99), (1, 2)):
        with pytest.raises(ValueError, match='even'):
            procedure.genFrameStream([buf, sr], w, h)
    for build in (lambda steps: procedure.genFrameStream(steps, 140, 100), procedure.genProcess):
        with pytest.raises(ValueError, match='resize'):
            build([buf, sr, rs])
        with pytest.raises(ValueError, match='resize'):
            build([buf, rs, sr])
        with pytest.raises(ValueError, match='matrix'):
            build([buf, sr, {'op': 'output', 'pixFmt': 'yuv420p', 'matrix': 'bt709'}])
        with pytest.raises(ValueError, match='order'):
            build([buf, sr, {'op': 'output', 'order': 'bgr'}])
        with pytest.raises(ValueError, match='pixFmt "nv12"'):
            build([{'op': 'buffer', 'pixFmt': 'nv12'}, sr])
        with pytest.raises(ValueError, match='pixFmt "yuv444p"'):
            build([buf, sr, {'op': 'output', 'pixFmt': 'yuv444p'}])
    with pytest.raises(ValueError, match='depth'):
        procedure.genFrameStream([buf, sr], 140, 100, depth=5)
    with pytest.raises(AssertionError, match='a model was asked for'):          # (a chain nothing is wrong with reaches the model)
        procedure.genFrameStream([buf, sr], 140, 100)
    assert procedure._planeFormats([buf, sr]) == ('yuv420p10le', 'yuv420p10le')
    assert procedure._planeFormats([{'op': 'buffer', 'pixFmt': 'yuv420p'}, sr, {'op': 'output', 'pixFmt': 'yuv420p10le'}], 140, 100) == ('yuv420p', 'yuv420p10le')
    assert procedure._planeFormats([{'op': 'buffer', 'bitDepth': 16}, sr, {'op': 'output', 'pixFmt': 'yuv420p10le'}]) is None      # (the RGB source: as before)
    with pytest.raises(ValueError, match='depth'):
        ip.toPlanes(9)
    with pytest.raises(ValueError, match='even'):
        ip.fromPlanes('yuv420p', 3, 2)


# ---- the ring with a frame size of its own ------------------------------------------------------------------------------------------------------
class FakeBackend(object):
    """In-order stand-in for the three queues: every stage runs when it is enqueued, after checking that each event it waits on has been recorded.  The stand-in
    computation reverses the frame's bytes."""

    def __init__(self, depth):
        self.raw, self.out, self.host = [None] * depth, [None] * depth, [None] * depth
        self.recorded, self.closed_calls, self.aborted = set(), 0, 0

    def event(self):
        return object()

    def _stage(self, wait, record, work):
        assert all(id(e) in self.recorded for e in wait), 'an event was waited on before it was recorded'
        work()
        self.recorded.add(id(record))

    def upload(self, slot, raw, wait, record):
        self._stage(wait, record, lambda: self.raw.__setitem__(slot, raw))

    def compute(self, slot, wait, record):
        self._stage(wait, record, lambda: self.out.__setitem__(slot, self.raw[slot][::-1]))

    def download(self, slot, wait, record):
        self._stage(wait, record, lambda: self.host.__setitem__(slot, self.out[slot]))

    def wait(self, slot, event):
        assert id(event) in self.recorded
        return self.host[slot]

    def abort(self):
        self.aborted += 1

    def close(self):
        self.closed_calls += 1


@pytest.mark.parametrize('depth', [1, 2, 3])
def test_frame_stream_with_its_own_frame_size(depth):
    n = pixfmt.frameBytes('yuv420p10le', 6, 4)
    assert n == 72 != 6 * 4 * 3 * 2
    frames = [np.random.default_rng(k).integers(0, 256, n, dtype=np.uint8).tobytes() for k in range(5)]
    b = FakeBackend(depth)
    s = procedure.FrameStream(b, 6, 4, 16, depth, frameBytes=n)
    assert s.frameBytes == n
    got = []
    assert procedure.runFramesStreamed(s, io.BytesIO(b''.join(frames)).read, got.append) == 5
    assert got == [f[::-1] for f in frames]
    with pytest.raises(ValueError, match='short frame: 71 of 72'):
        s.push(frames[0][:-1])
    with pytest.raises(ValueError, match='short frame'):
        s.push(frames[0] + frames[1])                                    # (a bgr48le frame's 144 bytes are no frame of this stream)
    s.close()
    assert b.closed_calls == 1
    # a short last frame: everything before it is written, then the error
    s = procedure.FrameStream(FakeBackend(depth), 6, 4, 16, depth, frameBytes=n)
    got = []
    with pytest.raises(ValueError, match='short frame: 10 of 72'):
        procedure.runFramesStreamed(s, io.BytesIO(frames[0] + frames[1] + frames[2][:10]).read, got.append)
    assert got == [frames[0][::-1], frames[1][::-1]]
    # the default is what it was, and a size that is none is refused
    assert procedure.FrameStream(FakeBackend(1), 6, 4, 16, 1).frameBytes == 144 and procedure.FrameStream(FakeBackend(1), 6, 4, 8, 1).frameBytes == 72
    for bad in (0, -72, 72.0, True):
        with pytest.raises(ValueError, match='frameBytes'):
            procedure.FrameStream(FakeBackend(1), 6, 4, 16, 1, frameBytes=bad)


def test_run_frames_with_a_frame_size_of_its_own():
    n = pixfmt.frameBytes('yuv420p', 6, 4)
    frames = [bytes([k]) * n for k in range(1, 4)]
    got = []
    process = lambda frame: [frame[0][::-1]]
    assert procedure.runFrames(process, io.BytesIO(b''.join(frames)).read, got.append, 6, 4, bitDepth=8, frameBytes=n) == 3 and got == frames
    with pytest.raises(ValueError, match='short frame: 5 of 36'):
        procedure.runFrames(process, io.BytesIO(frames[0] + b'12345').read, got.append, 6, 4, bitDepth=8, frameBytes=n)


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------------
def test_planes_exports_are_declared_and_present():
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    declared = set(re.findall(r'\b(moe_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    for name in ('moe_planes_to_float', 'moe_stitch_planes', 'moe_run_plan_planes'):
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.moe_abi_version() == _lib.ABI_VERSION == 4


def test_planes_entry_points_validate_their_arguments_without_a_device():
    L = _lib.lib()
    err = lambda: L.moe_last_error()
    grey = ip.TilePlan((1, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    five = ip.TilePlan((5, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 1)

    tf = lambda src, depth, H, W, dy, dc, dt: L.moe_planes_to_float(src, depth, H, W, dy, dc, dt, 0, None)
    for args in ((None, 8, 2, 2, p, p, _lib.F32), (p, 8, 2, 2, None, p, _lib.F32), (p, 8, 2, 2, p, None, _lib.F32)):
        assert tf(*args) == _lib.EINVAL and b'moe_planes_to_float: NULL' in err()
    for depth in (0, 9, 14, 24, -8):
        assert tf(p, depth, 2, 2, p, p, _lib.F32) == _lib.EINVAL and 'depth {}'.format(depth).encode() in err()
    for H, W in ((3, 2), (2, 3), (0, 2), (2, 0), (-2, 2), (100, 141)):
        assert tf(p, 8, H, W, p, p, _lib.F32) == _lib.EINVAL and b'even' in err()
    for dt in (_lib.U8, _lib.U16, 7):
        assert tf(p, 8, 2, 2, p, p, dt) == _lib.EINVAL and b'dst dtype' in err()
    assert tf(odd, 10, 2, 2, p, p, _lib.F32) == _lib.EINVAL and b'src is not 2-byte aligned' in err()
    assert tf(p, 8, 2, 2, odd, p, _lib.F16) == _lib.EINVAL and b'not aligned' in err()
    assert tf(p, 8, 2, 2, p, ctypes.c_void_p(p.value + 2), _lib.F32) == _lib.EINVAL and b'not aligned' in err()

    sp = lambda pl, tiles, C, cdt, depth, dst: L.moe_stitch_planes(pl, 0, tiles, None, C, cdt, depth, dst, None)
    assert sp(None, p, 1, _lib.F32, 8, p) == _lib.EINVAL and b'moe_stitch_planes: NULL' in err()
    assert sp(grey._h, None, 1, _lib.F32, 8, p) == _lib.EINVAL and b'NULL' in err()
    assert sp(grey._h, p, 1, _lib.F32, 8, None) == _lib.EINVAL and b'NULL' in err()
    for C in (0, 5, -1):
        assert sp(grey._h, p, C, _lib.F32, 8, p) == _lib.EINVAL and '{} planes (1 to 4'.format(C).encode() in err()
    for cdt in (_lib.U8, _lib.U16):
        assert sp(grey._h, p, 1, cdt, 8, p) == _lib.EINVAL and b'canvas dtype' in err()
    for depth in (0, 7, 9, 11, 14, 17):
        assert sp(grey._h, p, 1, _lib.F16, depth, p) == _lib.EINVAL and 'depth {}'.format(depth).encode() in err()
    assert sp(grey._h, p, 2, _lib.F16, 10, odd) == _lib.EINVAL and b'dst is not 2-byte aligned' in err()

    h = ctypes.c_void_p()
    _lib.check(L.moe_net_create(_lib.ARCH_NET2X, 2, ctypes.byref(h)))
    try:
        rp = lambda net, pl, img, cdt, depth, dst: L.moe_run_plan_planes(net, pl, img, _lib.F32, 14000, 140, 1, cdt, depth, dst, 0, None)
        assert rp(None, grey._h, p, _lib.F32, 8, p) == _lib.EINVAL and b'moe_run_plan_planes: NULL' in err()
        assert rp(h, None, p, _lib.F32, 8, p) == _lib.EINVAL and b'NULL' in err()
        assert rp(h, grey._h, None, _lib.F32, 8, p) == _lib.EINVAL and b'NULL' in err()
        assert rp(h, grey._h, p, _lib.F32, 8, None) == _lib.EINVAL and b'NULL' in err()
        assert rp(h, five._h, p, _lib.F32, 8, p) == _lib.EINVAL and b'5 planes (1 to 4' in err()
        assert rp(h, grey._h, p, _lib.U16, 8, p) == _lib.EINVAL and b'canvas dtype' in err()
        assert rp(h, grey._h, p, _lib.F32, 13, p) == _lib.EINVAL and b'depth 13' in err()
        assert rp(h, grey._h, p, _lib.F32, 12, odd) == _lib.EINVAL and b'2-byte aligned' in err()
        assert rp(h, grey._h, p, _lib.F32, 16, p) == _lib.ESTATE and b'moe_run_plan_planes: net is not finalized' in err()
    finally:
        L.moe_net_destroy(h)
