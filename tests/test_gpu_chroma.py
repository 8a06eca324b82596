"""Luma-only chains on the device (`pytest -m gpu`).  The comparator of the kernel is the written definition (pixfmt.resampleChroma: numpy,
integers) and equality of bytes is the bar; the streams are held to the 'chroma': 'net' stream on the Y plane, to the definition on the chroma planes and to
genProcess + runFrames on the whole frame.

The tile-edge shapes come from resize_kernel_codes' output tile, CHROMA_TW x CHROMA_TH = 256 x 32 samples of one plane (moephoto_amd/csrc/chroma.hip)."""
import io

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import pixfmt

pytestmark = pytest.mark.gpu
FMT = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le', 16: 'yuv420p16le'}
METHODS = ('nearest', 'bilinear', 'bicubic')
LOCS = ('center', 'left')
CASES = [(m, l) for m in METHODS for l in LOCS]
PAIRS = ((8, 8), (8, 10), (10, 10), (10, 8), (12, 16), (16, 16))
TILE_W, TILE_H = 256, 32          # CHROMA_TW, CHROMA_TH of chroma.hip
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _np_dt(depth):
    return np.uint8 if depth == 8 else np.dtype('<u2')


def _tables(method, scale, loc):
    import ctypes
    (ox, cx), (oy, cy) = pixfmt.chromaTable(method, scale, loc), pixfmt.chromaTable(method, scale, 'center')
    flat = lambda rows: [c for r in rows for c in r]
    mk = lambda T, v: (T * len(v))(*v)
    return pixfmt.CHROMA_METHODS[method], (mk(ctypes.c_int16, flat(cx)), mk(ctypes.c_int8, ox), mk(ctypes.c_int16, flat(cy)), mk(ctypes.c_int8, oy))


def _device_resample(C, ds, dd, scale, method, loc, dev, lead_src, lead_dst):
    """moe_chroma_resample on C's codes, source and destination `lead` SAMPLES behind a 16-byte boundary and between sentinel bytes that must survive."""
    from moephoto_amd import _lib
    _, h, w = C.shape
    src = np.ascontiguousarray(C.astype(_np_dt(ds))).view(np.uint8).reshape(-1)
    es_s, es_d = src.size // C.size, 1 if dd == 8 else 2
    a, b = lead_src * es_s, lead_dst * es_d
    n_out = 2 * h * scale * w * scale * es_d
    s_buf = torch.full((a + src.size + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    d_buf = torch.full((b + n_out + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    assert s_buf.data_ptr() % 16 == 0 and d_buf.data_ptr() % 16 == 0
    s_buf[a:a + src.size] = torch.from_numpy(src.copy()).to(dev)
    taps, tabs = _tables(method, scale, loc)
    _lib.check(_lib.lib().moe_chroma_resample(s_buf.data_ptr() + a, ds, h, w, d_buf.data_ptr() + b, dd, scale, taps, *tabs, 0, torch.cuda.current_stream().cuda_stream))
    out = d_buf.cpu().numpy()
    assert (out[:b] == SENTINEL).all() and (out[b + n_out:] == SENTINEL).all(), 'a sentinel around the destination was overwritten'
    assert (s_buf.cpu().numpy()[a + src.size:] == SENTINEL).all()
    return out[b:b + n_out].view(_np_dt(dd)).reshape(2, h * scale, w * scale)


def _check(C, ds, dd, scale, method, loc, dev, leads=((1, 1),)):
    want = pixfmt.resampleChroma(C, FMT[ds], FMT[dd], scale, method, loc)
    for ls, ld in leads:
        got = _device_resample(C, ds, dd, scale, method, loc, dev, ls, ld)
        bad = got != want
        assert not bad.any(), '{} {} {}x{} x{} {}->{} leads {}/{}: {} of {} samples differ, the first at {}'.format(
            method, loc, C.shape[1], C.shape[2], scale, ds, dd, ls, ld, int(bad.sum()), bad.size, tuple(int(i) for i in np.argwhere(bad)[0]))


def _codes(seed, depth, h, w):
    """Random codes of the container: 10- and 12-bit planes also hold codes above their depth (high bits are not masked on input; the definition's clamp applies)."""
    c = np.random.default_rng(seed).integers(0, 1 << depth, size=(2, h, w))
    if depth in (10, 12) and c.size > 2:
        c.reshape(-1)[1::5] |= 0x8000
        c.reshape(-1)[2] = 65535
    return c


@pytest.mark.parametrize('method,loc', CASES)
def test_small_planes_every_scale_and_depth_pair(method, loc, dev):
    for hw in ((1, 1), (1, 7), (5, 1), (3, 5)):
        for scale in (1, 2, 3, 4, 8) + ((16,) if hw == (3, 5) else ()):
            for ds, dd in PAIRS:
                _check(_codes(sum(hw) + scale + ds, ds, *hw), ds, dd, scale, method, loc, dev, leads=((1, 1), (0, 0)))


@pytest.mark.parametrize('method,loc', CASES)
def test_planes_one_sample_around_the_output_tile(method, loc, dev):
    """Per scale the plane whose scaled size first exceeds the kernel's output tile in both axes (TILE / scale + 1 samples: the second tile holds one source sample's
    worth) and the one that last stays inside it (ceil(TILE / scale) - 1)."""
    for scale in (1, 2, 3, 4, 8):
        larger = (TILE_H // scale + 1, TILE_W // scale + 1)
        smaller = (-(-TILE_H // scale) - 1, -(-TILE_W // scale) - 1)
        assert larger[0] * scale > TILE_H and larger[1] * scale > TILE_W and 0 < smaller[0] * scale < TILE_H and 0 < smaller[1] * scale < TILE_W
        for hw in (larger, smaller):
            for ds, dd in ((10, 10), (8, 8), (16, 8)) if scale in (1, 3) else ((10, 10),):
                _check(_codes(scale + ds, ds, *hw), ds, dd, scale, method, loc, dev, leads=((1, 1), (0, 1)))


@pytest.mark.parametrize('method,loc', CASES)
def test_the_chroma_of_a_140x100_frame(method, loc, dev):
    for scale in (1, 2, 3, 4, 8):          # 50 x 70 samples: up to 13 x 3 tiles per plane
        for ds, dd in PAIRS if scale == 2 else ((10, 10),):
            _check(_codes(scale, ds, 50, 70), ds, dd, scale, method, loc, dev, leads=((1, 1),) if scale > 2 else ((1, 1), (0, 0), (1, 0)))


@pytest.mark.parametrize('method,loc', CASES)
def test_flat_planes_and_the_checkerboard_of_extremes(method, loc, dev):
    for hw in ((3, 5), (TILE_H // 4 + 1, TILE_W // 4 + 1)):
        for scale in (2, 3, 4) + ((16,) if hw == (3, 5) else ()):
            for ds, dd in PAIRS:
                for code in (0, (1 << ds) - 1):
                    _check(np.full((2,) + hw, code), ds, dd, scale, method, loc, dev)
            board = np.zeros((2,) + hw, np.int64)          # max / 0 at depth 16: where an int32 slip or a missing clamp shows
            board[:, ::2, ::2] = 65535
            board[:, 1::2, 1::2] = 65535
            board[1] = 65535 - board[1]
            _check(board, 16, 16, scale, method, loc, dev, leads=((1, 1), (0, 0)))
            _check(board, 16, 8, scale, method, loc, dev)
            high = np.full((2,) + hw, 1023, np.int64)          # a 10-bit plane whose codes lie above 1023
            high[:, ::2, 1::2] = 65535
            high[:, 1::2, ::3] = 0x8000 | 512
            _check(high, 10, 10, scale, method, loc, dev)
            _check(high, 10, 8, scale, method, loc, dev)


def test_resamplechroma_wrapper(dev):
    from moephoto_amd import imageProcess as ip
    w, h, scale = 18, 10, 3
    rng = np.random.default_rng(4)
    frame = rng.integers(0, 1024, w * h * 3 // 2).astype('<u2').tobytes()
    raw = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).to(dev)
    n = pixfmt.frameBytes('yuv420p', w * scale, h * scale)
    out = torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev)
    f = ip.resampleChroma('yuv420p10le', 'yuv420p', w, h, scale, 'bicubic', 'left')
    assert f(raw, out) is out
    host, cb = out.cpu().numpy(), pixfmt.planeOffsets('yuv420p', w * scale, h * scale)[1]
    C = np.frombuffer(frame, '<u2')[w * h:].reshape(2, h // 2, w // 2)
    assert (host[:cb] == SENTINEL).all()          # the Y plane is not the filter's
    assert host[cb:].tobytes() == pixfmt.resampleChroma(C, 'yuv420p10le', 'yuv420p', scale, 'bicubic', 'left').tobytes()
    with pytest.raises(ValueError):
        f(raw[:-2], out)
    with pytest.raises(ValueError):
        f(raw, out[:-1])
    with pytest.raises(ValueError):
        ip.resampleChroma('yuv420p10le', 'yuv420p', w, h, 17, 'bicubic')


# ---- the streams ------------------------------------------------------------------------------------------------------------------------------
W, H = 140, 100
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}


def _configure():
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, True
    config.crop_sr = config.crop_dn = config.crop_dns = 48
    config.ensembleSR = 0


def _frame(seed, depth):
    a = np.random.default_rng(seed).integers(0, 1 << depth, W * H * 3 // 2, dtype=np.uint32)
    a[:2] = (0, (1 << depth) - 1)
    if depth in (10, 12):
        a[2::61] |= 0x8000
    return a.astype(_np_dt(depth)).tobytes()


def _differ(got, want):
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    return 'sizes {} / {}'.format(g.size, w.size) if g.size != w.size else '{} of {} bytes differ, the first at {}'.format(int((g != w).sum()), g.size, int(np.argmax(g != w)))


def _stream(steps, frames, depth=2, **kw):
    from moephoto_amd import procedure
    stream = procedure.genFrameStream(steps, W, H, depth, **kw)
    got = []
    assert procedure.runFramesStreamed(stream, io.BytesIO(b''.join(frames)).read, lambda b: got.append(bytes(b))) == len(frames)
    stream.close()
    return got, stream


def _expect(frames, net, src, dst, scale, method, loc):
    """The luma-only frames: the Y plane of the 'net' stream's frame, the definition's chroma planes of the source frame."""
    ds, cb = pixfmt.FORMATS[src], pixfmt.planeOffsets(dst, W * scale, H * scale)[1]
    want = []
    for f, n in zip(frames, net):
        C = np.frombuffer(f, _np_dt(ds))[W * H:].reshape(2, H // 2, W // 2)
        want.append(n[:cb] + pixfmt.resampleChroma(C, src, dst, scale, method, loc).tobytes())
    return want


# name -> (source format, steps behind the source, output format, scale, edge)
CHAINS = {'sr_a2': ('yuv420p10le', [dict(SR)], 'yuv420p10le', 2, 'crop'),
          'dn_only_1': ('yuv420p10le', [{'op': 'DN', 'model': 'lite5', 'strength': 1.0}], 'yuv420p10le', 1, 'crop'),
          'dn_only_0.6': ('yuv420p10le', [{'op': 'DN', 'model': 'lite5', 'strength': 0.6}], 'yuv420p10le', 1, 'quantise'),
          'dn_0.6_sr_a2': ('yuv420p10le', [{'op': 'DN', 'model': 'lite5', 'strength': 0.6}, dict(SR)], 'yuv420p10le', 2, 'crop'),
          'sr_a2_8_to_10': ('yuv420p', [dict(SR), {'op': 'output', 'pixFmt': 'yuv420p10le'}], 'yuv420p10le', 2, 'crop')}


@pytest.mark.parametrize('chain', sorted(CHAINS))
def test_luma_only_streams(chain, dev):
    from moephoto_amd import procedure
    _configure()
    src, work, dst, scale, edge = CHAINS[chain]
    method, loc = ('bicubic', 'left') if chain != 'dn_0.6_sr_a2' else ('bilinear', 'center')
    frames = [_frame(5 + k, pixfmt.FORMATS[src]) for k in range(5)]
    net, _ = _stream([{'op': 'buffer', 'pixFmt': src, 'chroma': 'net'}] + [dict(s) for s in work], frames)
    plain, _ = _stream([{'op': 'buffer', 'pixFmt': src}] + [dict(s) for s in work], frames)
    assert net == plain                                                     # 'net' is the default, byte for byte
    want = _expect(frames, net, src, dst, scale, method, loc)
    assert len(set(want)) == 5
    steps = [{'op': 'buffer', 'pixFmt': src, 'chroma': method, 'chromaLoc': loc}] + [dict(s) for s in work]
    if scale == 1:          # a DN-only chain: the chroma planes are the source's codes (under the definition's clamp: these frames hold codes above 1023)
        nY = W * H * 2
        assert all(w_[nY:] == np.minimum(np.frombuffer(f[nY:], '<u2'), 1023).astype('<u2').tobytes() for w_, f in zip(want, frames))
    process, nodes = procedure.genProcess(steps)
    serial = []
    assert procedure.runFrames(process, io.BytesIO(b''.join(frames)).read, serial.append, W, H, frameBytes=pixfmt.frameBytes(src, W, H)) == 5
    for k, (g, w_) in enumerate(zip(serial, want)):
        assert g == w_, '{} serial frame {}: {}'.format(chain, k, _differ(g, w_))
    for depth in (1, 2, 3):
        got, stream = _stream(steps, frames, depth)
        assert stream.edge == edge and stream.nodes == nodes
        for k, (g, w_) in enumerate(zip(got, want)):
            assert g == w_, '{} ring depth {} frame {}: {}'.format(chain, depth, k, _differ(g, w_))


def test_luma_only_stream_with_reuse(dev):
    _configure()
    base = [_frame(40 + k, 10) for k in range(3)]
    frames = [base[0], base[1], base[1], base[2], base[2], base[0]]          # repeated frames: their tiles are not run again
    steps = [{'op': 'buffer', 'pixFmt': 'yuv420p10le', 'chroma': 'bicubic'}, {'op': 'DN', 'model': 'lite5', 'strength': 0.6}, dict(SR)]
    want, _ = _stream(steps, frames)
    for depth in (1, 3):
        got, stream = _stream(steps, frames, depth, reuse=True)
        for k, (g, w_) in enumerate(zip(got, want)):
            assert g == w_, 'reuse, ring depth {} frame {}: {}'.format(depth, k, _differ(g, w_))
        tiles = stream.reuse['tiles']
        assert tiles and all(image == 'y' for _, image in tiles), sorted(tiles)          # no chroma image takes part
        assert all(run < planned for planned, run in tiles.values()), tiles
        assert stream.reuse['pixels_run'] < stream.reuse['pixels_planned']


@pytest.mark.parametrize('source', ['planes', 'planes_luma_only', 'rgb'])
def test_frames_handed_out_as_views(source, dev):
    from moephoto_amd import procedure
    _configure()
    if source == 'rgb':
        steps = [{'op': 'buffer', 'bitDepth': 16}, dict(SR)]
        frames = [np.random.default_rng(60 + k).integers(0, 65536, W * H * 3, dtype=np.uint16).tobytes() for k in range(5)]
    else:
        steps = [dict({'op': 'buffer', 'pixFmt': 'yuv420p10le'}, **({'chroma': 'bicubic'} if source == 'planes_luma_only' else {})), dict(SR)]
        frames = [_frame(60 + k, 10) for k in range(5)]
    want, _ = _stream(steps, frames)
    assert all(type(f) is bytes for f in want)
    for depth in (1, 2, 3):
        stream = procedure.genFrameStream(steps, W, H, depth, views=True)
        got = []

        def write(view):
            assert isinstance(view, memoryview) and view.readonly and view.format == 'B' and view.ndim == 1
            with pytest.raises(TypeError):
                view[0] = 0
            got.append(bytes(view))
        assert procedure.runFramesStreamed(stream, io.BytesIO(b''.join(frames)).read, write) == 5
        stream.close()
        for k, (g, w_) in enumerate(zip(got, want)):
            assert g == w_, '{} views, ring depth {} frame {}: {}'.format(source, depth, k, _differ(g, w_))
