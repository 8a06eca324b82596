"""Luma-guided chroma on the device (`pytest -m gpu`).  The comparator of the kernel is the written definition (pixfmt.guidedChroma: numpy,
integers) and equality of bytes is the bar; the streams are held to genProcess + runFrames on the whole frame, to the definition fed the frame's OWN Y plane on the
chroma planes and to the 'chroma': 'bicubic' stream on the Y plane.

The tile-edge shape comes from resize_kernel_guided's output tile, GUIDED_TW x GUIDED_TH = 256 x 32 chroma samples of both planes (moephoto_amd/csrc/chroma_guided.hip)."""
import ctypes
import io

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import pixfmt

pytestmark = pytest.mark.gpu
FMT = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le', 16: 'yuv420p16le'}
LOCS = ('center', 'left')
SCALES = (2, 3, 4, 16)
PAIRS = ((8, 8), (10, 10), (8, 10), (16, 10))
PLANES = ((1, 1), (3, 2), (5, 9), (50, 70))          # (h, w) of the chroma planes 1 x 1, 2 x 3, 9 x 5 and 70 x 50: frames 2 x 2 .. 140 x 100
TILE_W, TILE_H = 256, 32          # GUIDED_TW, GUIDED_TH of chroma_guided.hip
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _np_dt(depth):
    return np.uint8 if depth == 8 else np.dtype('<u2')


def _tables(scale, loc):
    (ox, cx), (oy, cy) = pixfmt.guidedTable(scale, loc), pixfmt.guidedTable(scale, 'center')
    flat = lambda rows: [c for r in rows for c in r]
    mk = lambda T, v: (T * len(v))(*v)
    return (mk(ctypes.c_uint8, flat(cx)), mk(ctypes.c_int8, ox), mk(ctypes.c_uint8, flat(cy)), mk(ctypes.c_int8, oy), mk(ctypes.c_uint8, pixfmt.guidedRange()))


def _codes(seed, depth, shape):
    """Uniform noise over the container: all 16 bits at depth 16; 10- and 12-bit planes also hold codes above their depth (uint16 codes are taken as they are)."""
    c = np.random.default_rng(seed).integers(0, 1 << depth, size=shape)
    if depth in (10, 12) and c.size > 2:
        c.reshape(-1)[1::5] |= 0x8000
        c.reshape(-1)[2] = 65535
    return c


def _device_guided(C, Ys, Yo, ds, dd, scale, loc, dev, lead):
    """moe_chroma_guided on a source frame (Y, Cb, Cr) and an output frame (Y given, chroma written), each `lead` SAMPLES behind a 16-byte boundary and between
    sentinel bytes that must survive; the output frame's Y plane must come back as it went in."""
    from moephoto_amd import _lib
    _, h, w = C.shape
    src = np.concatenate([Ys.reshape(-1), C.reshape(-1)]).astype(_np_dt(ds)).view(np.uint8)
    yo = np.ascontiguousarray(Yo.astype(_np_dt(dd))).view(np.uint8).reshape(-1)
    es_s, es_d = (1 if ds == 8 else 2), (1 if dd == 8 else 2)
    a, b = lead * es_s, lead * es_d
    n_c = 2 * h * scale * w * scale * es_d
    s_buf = torch.full((a + src.size + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    d_buf = torch.full((b + yo.size + n_c + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    assert s_buf.data_ptr() % 16 == 0 and d_buf.data_ptr() % 16 == 0
    s_buf[a:a + src.size] = torch.from_numpy(src.copy()).to(dev)
    d_buf[b:b + yo.size] = torch.from_numpy(yo.copy()).to(dev)
    _lib.check(_lib.lib().moe_chroma_guided(s_buf.data_ptr() + a + 4 * h * w * es_s, s_buf.data_ptr() + a, ds, h, w, d_buf.data_ptr() + b + yo.size, d_buf.data_ptr() + b,
                                            dd, scale, LOCS.index(loc), *_tables(scale, loc), 0, torch.cuda.current_stream().cuda_stream))
    out, back = d_buf.cpu().numpy(), s_buf.cpu().numpy()
    assert (out[:b] == SENTINEL).all() and (out[b + yo.size + n_c:] == SENTINEL).all(), 'a sentinel around the destination was overwritten'
    assert (out[b:b + yo.size] == yo).all(), "the destination's Y plane was written"
    assert (back[:a] == SENTINEL).all() and (back[a + src.size:] == SENTINEL).all() and (back[a:a + src.size] == src).all()
    return out[b + yo.size:b + yo.size + n_c].view(_np_dt(dd)).reshape(2, h * scale, w * scale)


def _check(seed, hw, ds, dd, scale, loc, dev, leads=(1,)):
    h, w = hw
    C, Ys, Yo = _codes(seed, ds, (2, h, w)), _codes(seed + 1, ds, (2 * h, 2 * w)), _codes(seed + 2, dd, (2 * h * scale, 2 * w * scale))
    want = pixfmt.guidedChroma(C.astype(np.uint16), Ys.astype(np.uint16), Yo.astype(np.uint16), FMT[ds], FMT[dd], scale, loc)
    for lead in leads:
        got = _device_guided(C, Ys, Yo, ds, dd, scale, loc, dev, lead)
        bad = got != want
        assert not bad.any(), '{} {}x{} x{} {}->{} lead {}: {} of {} samples differ, the first at {} (device {}, definition {})'.format(
            loc, h, w, scale, ds, dd, lead, int(bad.sum()), bad.size, tuple(int(i) for i in np.argwhere(bad)[0]), got[bad][0], want[bad][0])


@pytest.mark.parametrize('loc', LOCS)
@pytest.mark.parametrize('ds,dd', PAIRS)
@pytest.mark.parametrize('scale', SCALES)
def test_kernel_is_the_definition(scale, ds, dd, loc, dev):
    for hw in PLANES:
        _check(7 * scale + ds + sum(hw), hw, ds, dd, scale, loc, dev, leads=(1, 0) if hw != PLANES[-1] else (1,))


@pytest.mark.parametrize('loc', LOCS)
@pytest.mark.parametrize('ds,dd', PAIRS)
def test_two_tiles_each_way_with_a_ragged_last_tile(ds, dd, loc, dev):
    """Scale 2, chroma planes of 131 x 21 samples: 262 x 42 output samples are two tiles of 256 x 32 in each direction, the last 6 columns and 10 rows wide -- a run
    of six samples at every row's end, and rows whose starts are not 16-byte aligned."""
    hw, scale = (TILE_H // 2 + 5, TILE_W // 2 + 3), 2
    assert TILE_W < hw[1] * scale < 2 * TILE_W and TILE_H < hw[0] * scale < 2 * TILE_H and (hw[1] * scale) % 8 and (hw[0] * scale) % 4
    _check(90 + ds, hw, ds, dd, scale, loc, dev, leads=(1, 0))


def test_flat_chroma_and_the_extremes(dev):
    for loc in LOCS:
        for scale in (2, 3):
            h, w = 6, 11
            Ys, Yo = _codes(1, 16, (2 * h, 2 * w)), _codes(2, 16, (2 * h * scale, 2 * w * scale))
            for code in (0, 65535):          # flat stays flat under any guide
                got = _device_guided(np.full((2, h, w), code), Ys, Yo, 16, 16, scale, loc, dev, 1)
                assert (got == code).all(), (loc, scale, code)
            board = np.zeros((2, h, w), np.int64)          # max / 0 at depth 16 under a guide that is far from every tap (all range weights 1) and one that is near
            board[:, ::2, ::2] = board[:, 1::2, 1::2] = 65535
            for ys, yo in ((0, 65535), (65535, 65535)):
                Y1, Y2 = np.full((2 * h, 2 * w), ys), np.full((2 * h * scale, 2 * w * scale), yo)
                want = pixfmt.guidedChroma(board.astype(np.uint16), Y1.astype(np.uint16), Y2.astype(np.uint16), FMT[16], FMT[16], scale, loc)
                assert np.array_equal(_device_guided(board, Y1, Y2, 16, 16, scale, loc, dev, 1), want), (loc, scale, ys, yo)


def test_guidedchroma_wrapper(dev):
    from moephoto_amd import imageProcess as ip
    w, h, scale = 18, 10, 3
    rng = np.random.default_rng(4)
    frame = pixfmt.fromPlanes(rng.random((1, h, w), np.float32), rng.random((2, h // 2, w // 2), np.float32), 'yuv420p10le')
    outFrame = pixfmt.fromPlanes(rng.random((1, h * scale, w * scale), np.float32), np.zeros((2, h * scale // 2, w * scale // 2), np.float32), 'yuv420p')
    raw = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).to(dev)
    out = torch.from_numpy(np.frombuffer(outFrame, np.uint8).copy()).to(dev)
    f = ip.guidedChroma('yuv420p10le', 'yuv420p', w, h, scale, 'left')
    assert f(raw, out) is out
    host, cb = out.cpu().numpy(), pixfmt.planeOffsets('yuv420p', w * scale, h * scale)[1]
    src = np.frombuffer(frame, '<u2')
    Ys, C = src[:w * h].reshape(h, w), src[w * h:].reshape(2, h // 2, w // 2)
    Yo = np.frombuffer(outFrame, np.uint8)[:cb].reshape(h * scale, w * scale)
    assert host[:cb].tobytes() == outFrame[:cb]          # the Y plane is read, not written
    assert host[cb:].tobytes() == pixfmt.guidedChroma(C, Ys, Yo, 'yuv420p10le', 'yuv420p', scale, 'left').tobytes()
    with pytest.raises(ValueError):
        f(raw[:-2], out)
    with pytest.raises(ValueError):
        f(raw, out[:-1])
    for bad in (1, 17):
        with pytest.raises(ValueError):
            ip.guidedChroma('yuv420p10le', 'yuv420p', w, h, bad)
    with pytest.raises(ValueError):
        ip.guidedChroma('yuv420p10le', 'yuv420p', w, h, 2, 'top')


# ---- the streams ------------------------------------------------------------------------------------------------------------------------------
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}
# name -> (width, height, source format, output format)
STREAMS = {'48x32_8': (48, 32, 'yuv420p', 'yuv420p'), '48x32_10': (48, 32, 'yuv420p10le', 'yuv420p10le'), '140x100_8': (140, 100, 'yuv420p', 'yuv420p'),
           '140x100_10': (140, 100, 'yuv420p10le', 'yuv420p10le'), '48x32_8_to_10': (48, 32, 'yuv420p', 'yuv420p10le')}
_serial = {}          # name -> (frames, genProcess + runFrames' frames, nodes): computed once, shared by the modes


def _configure():
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, True
    config.crop_sr = config.crop_dn = config.crop_dns = 48
    config.ensembleSR = 0


def _frame(seed, depth, w, h):
    a = np.random.default_rng(seed).integers(0, 1 << depth, w * h * 3 // 2, dtype=np.uint32)
    a[:2] = (0, (1 << depth) - 1)
    if depth in (10, 12):
        a[2::61] |= 0x8000
    return a.astype(_np_dt(depth)).tobytes()


def _differ(got, want):
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    return 'sizes {} / {}'.format(g.size, w.size) if g.size != w.size else '{} of {} bytes differ, the first at {}'.format(int((g != w).sum()), g.size, int(np.argmax(g != w)))


def _steps(name, chroma, loc='left'):
    _, _, src, dst = STREAMS[name]
    return [{'op': 'buffer', 'pixFmt': src, 'chroma': chroma, 'chromaLoc': loc}, dict(SR)] + ([{'op': 'output', 'pixFmt': dst}] if dst != src else [])


def _stream(name, steps, frames, depth=2, **kw):
    from moephoto_amd import procedure
    w, h = STREAMS[name][:2]
    stream = procedure.genFrameStream(steps, w, h, depth, **kw)
    got = []
    assert procedure.runFramesStreamed(stream, io.BytesIO(b''.join(frames)).read, lambda b: got.append(bytes(b))) == len(frames)
    stream.close()
    return got, stream


def _reference(name):
    from moephoto_amd import procedure
    if name not in _serial:
        w, h, src, _ = STREAMS[name]
        base = [_frame(70 + k, pixfmt.FORMATS[src], w, h) for k in range(3)]
        frames = [base[0], base[1], base[1], base[2], base[0]]          # (a repeated frame: with reuse its Y tiles are not run again, its chroma is written all the same)
        process, nodes = procedure.genProcess(_steps(name, 'guided'))
        serial = []
        assert procedure.runFrames(process, io.BytesIO(b''.join(frames)).read, serial.append, w, h, frameBytes=pixfmt.frameBytes(src, w, h)) == len(frames)
        _serial[name] = (frames, serial, nodes)
    return _serial[name]


@pytest.mark.parametrize('name', sorted(STREAMS))
def test_serial_frames_hold_the_definition_on_their_own_luma(name, dev):
    """genProcess + runFrames: every frame's chroma planes are pixfmt.guidedChroma of the source frame and the frame's OWN Y plane; the Y plane is the 'bicubic'
    stream's."""
    _configure()
    w, h, src, dst = STREAMS[name]
    frames, serial, _ = _reference(name)
    ds, dd = pixfmt.FORMATS[src], pixfmt.FORMATS[dst]
    cb = pixfmt.planeOffsets(dst, 2 * w, 2 * h)[1]
    bicubic, _ = _stream(name, _steps(name, 'bicubic'), frames)
    assert len(set(serial)) == 3
    for k, (f, g, b) in enumerate(zip(frames, serial, bicubic)):
        assert len(g) == pixfmt.frameBytes(dst, 2 * w, 2 * h)
        assert g[:cb] == b[:cb], '{} frame {}: the Y plane is not the bicubic stream\'s: {}'.format(name, k, _differ(g[:cb], b[:cb]))
        s = np.frombuffer(f, _np_dt(ds))
        Yo = np.frombuffer(g[:cb], _np_dt(dd)).reshape(2 * h, 2 * w)
        want = pixfmt.guidedChroma(s[w * h:].reshape(2, h // 2, w // 2), s[:w * h].reshape(h, w), Yo, src, dst, 2, 'left').tobytes()
        assert g[cb:] == want, '{} frame {}: {}'.format(name, k, _differ(g[cb:], want))
        assert g[cb:] != b[cb:]


@pytest.mark.parametrize('mode', ['plain', 'reuse', 'views'])
@pytest.mark.parametrize('name', sorted(STREAMS))
def test_streams_equal_the_serial_frames(name, mode, dev):
    from moephoto_amd import procedure
    _configure()
    frames, serial, nodes = _reference(name)
    steps = _steps(name, 'guided')
    for depth in (1, 2, 3):
        if mode == 'views':
            w, h = STREAMS[name][:2]
            stream, got = procedure.genFrameStream(steps, w, h, depth, views=True), []

            def write(view):
                assert isinstance(view, memoryview) and view.readonly
                got.append(bytes(view))
            assert procedure.runFramesStreamed(stream, io.BytesIO(b''.join(frames)).read, write) == len(frames)
            stream.close()
        else:
            got, stream = _stream(name, steps, frames, depth, reuse=mode == 'reuse')
        assert stream.edge == 'crop' and stream.nodes == nodes
        for k, (g, w_) in enumerate(zip(got, serial)):
            assert g == w_, '{} {} ring depth {} frame {}: {}'.format(name, mode, depth, k, _differ(g, w_))
        if mode == 'reuse':
            tiles = stream.reuse['tiles']
            assert tiles and all(image == 'y' for _, image in tiles), sorted(tiles)          # no chroma image takes part: the chroma call runs every frame
            assert stream.reuse['pixels_run'] < stream.reuse['pixels_planned']


def test_quantise_edge_stream(dev):
    """A chain whose last step cannot fold into the frame (a blended DN behind the SR step): edge 'quantise' writes the Y plane, the guided call runs behind it."""
    from moephoto_amd import procedure
    _configure()
    w, h, fmt = 48, 32, 'yuv420p10le'
    steps = [{'op': 'buffer', 'pixFmt': fmt, 'chroma': 'guided'}, dict(SR), {'op': 'DN', 'model': 'lite5', 'strength': 0.6}]
    frames = [_frame(80 + k, 10, w, h) for k in range(3)]
    process, _ = procedure.genProcess(steps)
    serial = []
    assert procedure.runFrames(process, io.BytesIO(b''.join(frames)).read, serial.append, w, h, frameBytes=pixfmt.frameBytes(fmt, w, h)) == 3
    cb = pixfmt.planeOffsets(fmt, 2 * w, 2 * h)[1]
    for depth in (1, 3):
        stream = procedure.genFrameStream(steps, w, h, depth)
        got = []
        assert procedure.runFramesStreamed(stream, io.BytesIO(b''.join(frames)).read, lambda b: got.append(bytes(b))) == 3
        stream.close()
        assert stream.edge == 'quantise'
        for k, (f, g, w_) in enumerate(zip(frames, got, serial)):
            assert g == w_, 'quantise edge, ring depth {} frame {}: {}'.format(depth, k, _differ(g, w_))
            s = np.frombuffer(f, '<u2')
            Yo = np.frombuffer(g[:cb], '<u2').reshape(2 * h, 2 * w)
            assert g[cb:] == pixfmt.guidedChroma(s[w * h:].reshape(2, h // 2, w // 2), s[:w * h].reshape(h, w), Yo, fmt, fmt, 2, 'center').tobytes()
