"""Fitted sizes on the device (`pytest -m gpu`).  The comparator of the kernel is the written definition (pixfmt.fitPlanes: numpy, integers) and
equality of bytes is the bar; the streams are held to genProcess + runFrames and to the composed definition: fitPlanes of the yuv420p16le frame the same chain gives
without the size.

The tile-edge shapes come from resize_kernel_fit's output tile: FIT_TW = 128 samples wide (moephoto_amd/csrc/common.h) and 32, 16 or 8 high -- the host's choice per
geometry, read back from the handle (moe_fit_info)."""
import ctypes
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
PAIRS = ((8, 8), (8, 10), (10, 10), (16, 10), (16, 8), (12, 16))
TILE_W, TILE_HS = 128, (32, 16, 8)          # FIT_TW of common.h; the heights moe_fit_create chooses from
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _np_dt(depth):
    return np.uint8 if depth == 8 else np.dtype('<u2')


def _device_fit(P, ds, dd, oh, ow, method, loc, dev, lead_src=1, lead_dst=1):
    """moe_fit_create / moe_fit_run on P's codes, source and destination `lead` SAMPLES behind a 16-byte boundary and between sentinel bytes that must survive.
    -> (the planes, the tile the handle chose)."""
    from moephoto_amd import _lib, imageProcess as ip
    C, h, w = P.shape
    src = np.ascontiguousarray(P.astype(_np_dt(ds))).view(np.uint8).reshape(-1)
    es_s, es_d = (1 if ds == 8 else 2), (1 if dd == 8 else 2)
    a, b = lead_src * es_s, lead_dst * es_d
    n_out = C * oh * ow * es_d
    s_buf = torch.full((a + src.size + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    d_buf = torch.full((b + n_out + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    assert s_buf.data_ptr() % 16 == 0 and d_buf.data_ptr() % 16 == 0
    s_buf[a:a + src.size] = torch.from_numpy(src.copy()).to(dev)
    tx, ty = ip.fitTables(method, w, ow, loc), ip.fitTables(method, h, oh, 'center')
    L, handle, info = _lib.lib(), ctypes.c_void_p(), (ctypes.c_int64 * 4)()
    _lib.check(L.moe_fit_create(C, ds, h, w, dd, oh, ow, tx[0], tx[1], tx[2], ty[0], ty[1], ty[2], 0, ctypes.byref(handle)))
    try:
        _lib.check(L.moe_fit_info(handle, info))
        _lib.check(L.moe_fit_run(handle, s_buf.data_ptr() + a, d_buf.data_ptr() + b, torch.cuda.current_stream().cuda_stream))
        out = d_buf.cpu().numpy()
    finally:
        L.moe_fit_destroy(handle)
    assert (out[:b] == SENTINEL).all() and (out[b + n_out:] == SENTINEL).all(), 'a sentinel around the destination was overwritten'
    assert (s_buf.cpu().numpy()[a + src.size:] == SENTINEL).all()
    assert info[0] == TILE_W and info[1] in TILE_HS and info[2] <= 80 * 1024 and info[3] == C
    return out[b:b + n_out].view(_np_dt(dd)).reshape(C, oh, ow), (int(info[0]), int(info[1]))


def _check(P, ds, dd, oh, ow, method, loc, dev, leads=((1, 1),)):
    want = pixfmt.fitPlanes(P, ds, dd, oh, ow, method, loc)
    for ls, ld in leads:
        got, tile = _device_fit(P, ds, dd, oh, ow, method, loc, dev, ls, ld)
        bad = got != want
        assert not bad.any(), '{} {} {}x{} -> {}x{} {}->{} leads {}/{}: {} of {} samples differ, the first at {}'.format(
            method, loc, P.shape[2], P.shape[1], ow, oh, ds, dd, ls, ld, int(bad.sum()), bad.size, tuple(int(i) for i in np.argwhere(bad)[0]))
    return tile


def _codes(seed, depth, C, h, w):
    """Random codes of the container: 10- and 12-bit planes also hold codes above their depth (high bits are not masked on input; the definition's clamp applies)."""
    c = np.random.default_rng(seed).integers(0, 1 << depth, size=(C, h, w))
    if depth in (10, 12) and c.size > 2:
        c.reshape(-1)[1::5] |= 0x8000
        c.reshape(-1)[2] = 65535
    return c


# (h, w) -> (oh, ow): the smallest; a window that overhangs all four plane edges (2 x 2 up, 5 x 5 down: every tap row reaches past both ends); coprime sizes both
# ways, where every output has its own phase; exactly 4 : 1; n = m
SMALL = (((1, 1), (1, 1)), ((2, 2), (7, 5)), ((5, 5), (2, 2)), ((37, 41), (23, 29)), ((23, 29), (37, 41)), ((64, 68), (16, 17)), ((19, 23), (19, 23)))


@pytest.mark.parametrize('method,loc', CASES)
def test_small_planes_every_depth_pair_one_and_two_planes(method, loc, dev):
    for (h, w), (oh, ow) in SMALL:
        for ds, dd in PAIRS:
            for C in (1, 2):
                _check(_codes(h + ow + ds + C, ds, C, h, w), ds, dd, oh, ow, method, loc, dev, leads=((1, 1), (0, 0)) if C == 2 else ((1, 1),))


def _source(m, ratio):
    """The source size of m outputs at ratio 1/4 (exactly) or 3/2 (to the next sample)."""
    return 4 * m if ratio == '1/4' else -(-2 * m // 3)


@pytest.mark.parametrize('ratio', ['1/4', '3/2'])
@pytest.mark.parametrize('method,loc', [('bicubic', 'center'), ('bicubic', 'left'), ('bilinear', 'left'), ('nearest', 'center')])
def test_outputs_one_sample_around_the_tile(ratio, method, loc, dev):
    """Per ratio an output one sample short of the kernel's tile, exactly a tile and one sample over it, in each axis.  The tile's height is the host's choice per
    geometry (8 or 16 at ratio 1/4, 32 at 3/2): 32 rows are a whole number of tiles of every height it chooses from."""
    heights = set()
    for ow in (TILE_W - 1, TILE_W, TILE_W + 1):
        for oh in (31, 32, 33):
            for ds, dd, C in ((10, 10, 2), (8, 8, 1), (16, 8, 1)) if ow == TILE_W + 1 else ((10, 10, 2),):
                tile = _check(_codes(ow + oh + ds, ds, C, _source(oh, ratio), _source(ow, ratio)), ds, dd, oh, ow, method, loc, dev, leads=((1, 1), (0, 1)))
                assert 32 % tile[1] == 0
                heights.add(tile[1])
    assert heights == ({8, 16} if ratio == '1/4' else {32}), heights          # (at 1/4 the 8-bit sources, half the window's bytes, take the higher tile)


@pytest.mark.parametrize('method,loc', CASES)
def test_the_planes_of_a_280x200_frame_to_210x150_and_420x300(method, loc, dev):
    for (oh, ow) in ((150, 210), (300, 420), (50, 70)):          # 3/4 down, 3/2 up, 4 down: several tiles in both axes
        for ds, dd in PAIRS if oh == 150 else ((16, 10),):
            _check(_codes(oh + ds, ds, 1, 200, 280), ds, dd, oh, ow, method, loc, dev, leads=((1, 1), (0, 0)))
        _check(_codes(oh, 16, 2, 100, 140), 16, 10, oh // 2, ow // 2, method, loc, dev, leads=((1, 0),))


@pytest.mark.parametrize('method,loc', CASES)
def test_flat_planes_and_the_checkerboard_of_extremes(method, loc, dev):
    for (h, w), (oh, ow) in (((3, 5), (7, 8)), ((37, 41), (23, 29)), ((64, 136), (16, 34))):
        for ds, dd in PAIRS:
            for code in (0, (1 << ds) - 1):
                _check(np.full((2, h, w), code), ds, dd, oh, ow, method, loc, dev)
        board = np.zeros((2, h, w), np.int64)          # max / 0 at depth 16: where an int32 slip or a missing clamp shows
        board[:, ::2, ::2] = 65535
        board[:, 1::2, 1::2] = 65535
        board[1] = 65535 - board[1]
        _check(board, 16, 16, oh, ow, method, loc, dev, leads=((1, 1), (0, 0)))
        _check(board, 16, 8, oh, ow, method, loc, dev)
        stripes = np.zeros((1, h, w), np.int64)        # the filter's negative lobes against full-scale edges, both axes
        stripes[:, :, w // 2:] = 65535
        stripes[:, h // 2:, :] = 65535 - stripes[:, h // 2:, :]
        _check(stripes, 16, 16, oh, ow, method, loc, dev)
        high = np.full((2, h, w), 1023, np.int64)          # a 10-bit plane whose codes lie above 1023
        high[:, ::2, 1::2] = 65535
        high[:, 1::2, ::3] = 0x8000 | 512
        _check(high, 10, 10, oh, ow, method, loc, dev)
        _check(high, 10, 8, oh, ow, method, loc, dev)


def test_fitplanes_wrapper(dev):
    from moephoto_amd import imageProcess as ip
    w, h, W, H = 18, 10, 26, 14
    frame = np.random.default_rng(4).integers(0, 1024, w * h * 3 // 2).astype('<u2').tobytes()
    raw = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).to(dev)
    n, cb = pixfmt.frameBytes('yuv420p', W, H), pixfmt.planeOffsets('yuv420p', W, H)[1]
    out = torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev)
    f = ip.fitPlanes(10, 8, 2, h // 2, w // 2, H // 2, W // 2, 'bicubic', 'left')
    assert f(raw[w * h * 2:], out[cb:]) is not None
    assert f.info(dev)['tile'][0] == TILE_W and f.info(dev)['planes'] == 2
    host = out.cpu().numpy()
    C = np.frombuffer(frame, '<u2')[w * h:].reshape(2, h // 2, w // 2)
    assert (host[:cb] == SENTINEL).all()          # the Y plane is not this call's
    assert host[cb:].tobytes() == pixfmt.fitPlanes(C, 10, 8, H // 2, W // 2, 'bicubic', 'left').tobytes()
    f(raw[w * h * 2:], out[cb:])                  # (the handle is reused)
    assert out.cpu().numpy().tobytes() == host.tobytes()
    with pytest.raises(ValueError):
        f(raw[w * h * 2:-2], out[cb:])
    with pytest.raises(ValueError):
        f(raw[w * h * 2:], out[cb:-1])
    with pytest.raises(ValueError):
        f(raw[w * h * 2:].to(torch.int8), out[cb:])
    with pytest.raises(Exception):
        f(raw[w * h * 2:].cpu(), out[cb:])
    for bad in (lambda: ip.fitPlanes(10, 8, 2, 50, 70, 12, 70, 'bicubic'), lambda: ip.fitPlanes(10, 8, 2, 5, 7, 5, 114, 'bicubic'), lambda: ip.fitPlanes(10, 9, 2, 5, 7, 5, 7, 'bicubic'),
                lambda: ip.fitPlanes(10, 8, 5, 5, 7, 5, 7, 'bicubic'), lambda: ip.fitPlanes(10, 8, 2, 5, 7, 5, 7, 'lanczos'), lambda: ip.fitPlanes(10, 8, 2, 5, 7, 5, 7, 'bicubic', 'top')):
        with pytest.raises(ValueError):
            bad()


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


def _composed(frames, frames16, src, dst, scale, size, fit, chroma):
    """The definition of a fitted frame: fitPlanes of the planes of the yuv420p16le frame the same chain gives without the size; luma-only: Cb / Cr in one pass from
    the source frame's codes."""
    (Wo, Ho), w, h, Ds, Dd = size, W * scale, H * scale, pixfmt.FORMATS[src], pixfmt.FORMATS[dst]
    want = []
    for f, f16 in zip(frames, frames16):
        p = np.frombuffer(f16, '<u2')
        y = pixfmt.fitPlanes(p[:w * h].reshape(1, h, w), 16, Dd, Ho, Wo, fit)
        if chroma:
            c = pixfmt.fitPlanes(np.frombuffer(f, _np_dt(Ds))[W * H:].reshape(2, H // 2, W // 2), Ds, Dd, Ho // 2, Wo // 2, *chroma)
        else:
            c = pixfmt.fitPlanes(p[w * h:].reshape(2, h // 2, w // 2), 16, Dd, Ho // 2, Wo // 2, fit)
        want.append(y.tobytes() + c.tobytes())
    return want


REFERENCE = {}          # (chroma or None, work) -> the chain's own yuv420p16le frames: computed once, shared by the sizes


@pytest.mark.parametrize('size', [(210, 150), (420, 300)], ids=['210x150', '420x300'])
@pytest.mark.parametrize('chroma', [None, ('bicubic', 'left')], ids=['net', 'bicubic_left'])
def test_fitted_streams(size, chroma, dev):
    """A planar a2 stream at 140 x 100 (the net's own 280 x 200) fitted to 210 x 150 (3/4: antialiased) and to 420 x 300 (3/2)."""
    from moephoto_amd import procedure
    _configure()
    src, dst, fit = 'yuv420p10le', 'yuv420p10le', 'bicubic'
    source = dict({'op': 'buffer', 'pixFmt': src}, **({'chroma': chroma[0], 'chromaLoc': chroma[1]} if chroma else {}))
    frames = [_frame(5 + k, 10) for k in range(4)]
    if chroma not in REFERENCE:
        REFERENCE[chroma] = _stream([dict(source), dict(SR), {'op': 'output', 'pixFmt': 'yuv420p16le'}], frames)[0]
    want = _composed(frames, REFERENCE[chroma], src, dst, 2, size, fit, chroma)
    assert len(set(want)) == 4 and all(len(w_) == pixfmt.frameBytes(dst, *size) for w_ in want)
    steps = [dict(source), dict(SR), {'op': 'output', 'width': size[0], 'height': size[1]}]          # ('fit' defaults to 'bicubic', 'pixFmt' to the source's)
    process, nodes = procedure.genProcess(steps)
    serial = []
    assert procedure.runFrames(process, io.BytesIO(b''.join(frames)).read, serial.append, W, H, frameBytes=pixfmt.frameBytes(src, W, H)) == 4
    for k, (g, w_) in enumerate(zip(serial, want)):
        assert g == w_, 'serial frame {}: {}'.format(k, _differ(g, w_))
    for depth, kw in ((1, {}), (2, {}), (3, {}), (2, dict(reuse=True)), (2, dict(views=True))):
        got, stream = _stream(steps, frames, depth, **kw)
        assert stream.edge == 'crop+fit' and stream.nodes == nodes
        for k, (g, w_) in enumerate(zip(got, want)):
            assert g == w_, 'ring depth {} {} frame {}: {}'.format(depth, kw, k, _differ(g, w_))


def test_fitted_stream_names_its_format_and_method(dev):
    """pixFmt and fit on the same output step: 10-bit planes in, a bilinear 8-bit frame of 212 x 148 out."""
    _configure()
    frames = [_frame(30 + k, 10) for k in range(2)]
    ref, _ = _stream([{'op': 'buffer', 'pixFmt': 'yuv420p10le'}, dict(SR), {'op': 'output', 'pixFmt': 'yuv420p16le'}], frames)
    want = _composed(frames, ref, 'yuv420p10le', 'yuv420p', 2, (212, 148), 'bilinear', None)
    got, stream = _stream([{'op': 'buffer', 'pixFmt': 'yuv420p10le'}, dict(SR), {'op': 'output', 'pixFmt': 'yuv420p', 'width': 212, 'height': 148, 'fit': 'bilinear'}], frames)
    assert stream.edge == 'crop+fit'
    for k, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, 'frame {}: {}'.format(k, _differ(g, w_))


def test_quantise_fit_stream(dev):
    """A chain whose last step cannot fold into samples itself -- a DN of strength 0.6 -- quantises at 16 bits and fits: 140 x 100 -> 106 x 76."""
    from moephoto_amd import procedure
    _configure()
    frames = [_frame(20 + k, 10) for k in range(3)]
    work = [{'op': 'DN', 'model': 'lite5', 'strength': 0.6}]
    source = {'op': 'buffer', 'pixFmt': 'yuv420p10le'}
    ref, plain = _stream([dict(source)] + [dict(s) for s in work] + [{'op': 'output', 'pixFmt': 'yuv420p16le'}], frames)
    assert plain.edge == 'quantise'
    want = _composed(frames, ref, 'yuv420p10le', 'yuv420p10le', 1, (106, 76), 'bicubic', None)
    steps = [dict(source)] + [dict(s) for s in work] + [{'op': 'output', 'width': 106, 'height': 76, 'fit': 'bicubic'}]
    got, stream = _stream(steps, frames)
    assert stream.edge == 'quantise+fit'
    for k, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, 'frame {}: {}'.format(k, _differ(g, w_))
    process, _ = procedure.genProcess(steps)
    serial = []
    assert procedure.runFrames(process, io.BytesIO(b''.join(frames)).read, serial.append, W, H, frameBytes=pixfmt.frameBytes('yuv420p10le', W, H)) == 3
    assert serial == want
