"""RGB frames from chains on 4:2:0 planes on the device (`pytest -m gpu`).  The comparator of the kernel is the written definition (pixfmt.toRGB:
numpy, integers) and equality of bytes is the bar; the streams are held to genProcess + runFrames on the whole frame, and every frame to pixfmt.toRGB of the frame
the same step list yields with 'yuv420p16le' as its output format.

The tile-edge shapes come from to_output_rgb420_kernel's tile, RGB_TW x RGB_TH = 128 x 32 luma pixels (moephoto_amd/csrc/planes_rgb.hip)."""
import ctypes
import io

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import pixfmt, quant

pytestmark = pytest.mark.gpu
FMT = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le', 16: 'yuv420p16le'}
RGB = {(8, 'bgr'): 'bgr24', (8, 'rgb'): 'rgb24', (16, 'bgr'): 'bgr48le', (16, 'rgb'): 'rgb48le'}
LOCS = ('center', 'left')
TILE_W, TILE_H = 128, 32          # RGB_TW, RGB_TH of planes_rgb.hip
# (w, h): one chroma sample (every tap clamped) .. 140 x 100; a width that is a multiple of 8 (whole vector runs in every row); two tiles each way and a ragged third
SIZES = ((2, 2), (4, 2), (6, 4), (18, 10), (34, 6), (136, 34), (140, 100), (2 * TILE_W + 6, 2 * TILE_H + 10))
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _np_dt(depth):
    return np.uint8 if depth == 8 else np.dtype('<u2')


def _tables(method, loc, matrix, depth, bits):
    (ox, cx), (oy, cy) = pixfmt.chromaTable(method, 2, loc), pixfmt.chromaTable(method, 2, 'center')
    taps = pixfmt.CHROMA_METHODS[method]
    return taps, ((ctypes.c_int16 * (2 * taps))(*sum(cx, [])), (ctypes.c_int8 * 2)(*ox), (ctypes.c_int16 * (2 * taps))(*sum(cy, [])), (ctypes.c_int8 * 2)(*oy),
                  (ctypes.c_int32 * 5)(*pixfmt.rgbCoefficients(matrix, depth, bits)))


def _codes(seed, depth, n):
    """Uniform noise over the container: all 16 bits at depth 16; 10- and 12-bit frames also hold codes above their depth (uint16 codes are taken as they are)."""
    c = np.random.default_rng(seed).integers(0, 1 << depth, size=n)
    c[:2] = (0, (1 << depth) - 1)
    if depth in (10, 12):
        c[1::5] |= 0x8000
        c[2] = 65535
    return c.astype(_np_dt(depth))


def _device_rgb(frame, depth, w, h, bits, matrix, order, method, loc, dither, dev, lead):
    """moe_planes_to_rgb on a frame, source and destination `lead` SAMPLES behind a 16-byte boundary and between sentinel bytes that must survive; the source must
    come back as it went in."""
    from moephoto_amd import _lib
    src = frame.view(np.uint8)
    es_s, es_d = (1 if depth == 8 else 2), bits // 8
    a, b, n_out = lead * es_s, lead * es_d, 3 * w * h * es_d
    s_buf = torch.full((a + src.size + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    d_buf = torch.full((b + n_out + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    assert s_buf.data_ptr() % 16 == 0 and d_buf.data_ptr() % 16 == 0
    s_buf[a:a + src.size] = torch.from_numpy(src.copy()).to(dev)
    taps, tabs = _tables(method, loc, matrix, depth, bits)
    flags = quant.Q_ORDERED if dither == 'ordered' else quant.Q_ROUND if dither == 'round' else 0
    _lib.check(_lib.lib().moe_planes_to_rgb(s_buf.data_ptr() + a, depth, h, w, d_buf.data_ptr() + b, bits | flags, pixfmt.MATRICES[matrix], pixfmt.ORDERS[order], taps, *tabs,
                                            0, torch.cuda.current_stream().cuda_stream))
    out, back = d_buf.cpu().numpy(), s_buf.cpu().numpy()
    assert (out[:b] == SENTINEL).all() and (out[b + n_out:] == SENTINEL).all(), 'a sentinel around the destination was overwritten'
    assert (back[:a] == SENTINEL).all() and (back[a + src.size:] == SENTINEL).all() and (back[a:a + src.size] == src).all(), 'the source or a sentinel around it was written'
    return out[b:b + n_out]


def _check(seed, wh, depth, bits, matrix, order, method, loc, dither, dev, leads=(1, 0)):
    w, h = wh
    frame = _codes(seed, depth, w * h * 3 // 2)
    want = np.frombuffer(pixfmt.toRGB(frame.tobytes(), FMT[depth], w, h, RGB[(bits, order)], matrix, method, loc, dither), np.uint8)
    for lead in leads:
        got = _device_rgb(frame, depth, w, h, bits, matrix, order, method, loc, dither, dev, lead)
        bad = got != want
        assert not bad.any(), '{}x{} {} -> {} {} {} {} {} {} lead {}: {} of {} bytes differ, the first at {} (device {}, definition {})'.format(
            w, h, depth, bits, matrix, order, method, loc, dither, lead, int(bad.sum()), bad.size, int(np.argmax(bad)), got[bad][0], want[bad][0])


@pytest.mark.parametrize('method', sorted(pixfmt.CHROMA_METHODS))
@pytest.mark.parametrize('bits', (8, 16))
@pytest.mark.parametrize('depth', (8, 10, 16))
def test_kernel_is_the_definition(depth, bits, method, dev):
    """Every size with both sitings; on each the three matrices, both orders, plain and 'ordered' take turns so that every size sees each value, and the smallest sizes
    and the tile-edge size see the whole cross."""
    combos = [(m, o, d) for m in sorted(pixfmt.MATRICES) for o in ('bgr', 'rgb') for d in (None, 'ordered')]
    for i, wh in enumerate(SIZES):
        whole = wh in (SIZES[0], SIZES[3], SIZES[-1])
        for j, loc in enumerate(LOCS):
            for k, (matrix, order, dither) in enumerate(combos):
                if whole or k % 4 == (i + j) % 4:
                    _check(31 * depth + bits + i, wh, depth, bits, matrix, order, method, loc, dither, dev, leads=(1, 0) if wh != SIZES[-2] else (1,))


def test_the_tile_edge_size_is_what_it_claims():
    w, h = SIZES[-1]
    assert 2 * TILE_W < w < 3 * TILE_W and 2 * TILE_H < h < 3 * TILE_H and w % 8 and h % 4 and w % 2 == 0 and h % 2 == 0


def test_round_is_plain_and_depth_12(dev):
    for wh in ((18, 10), (136, 34)):
        frame = _codes(5, 12, wh[0] * wh[1] * 3 // 2)
        plain = _device_rgb(frame, 12, wh[0], wh[1], 16, 'bt709', 'bgr', 'bicubic', 'center', None, dev, 1)
        assert (_device_rgb(frame, 12, wh[0], wh[1], 16, 'bt709', 'bgr', 'bicubic', 'center', 'round', dev, 1) == plain).all()
        assert plain.tobytes() == pixfmt.toRGB(frame.tobytes(), FMT[12], wh[0], wh[1], 'bgr48le')


def test_planestorgb_wrapper(dev):
    from moephoto_amd import imageProcess as ip
    w, h = 18, 10
    rng = np.random.default_rng(4)
    frame = pixfmt.fromPlanes(rng.random((1, h, w), np.float32), rng.random((2, h // 2, w // 2), np.float32), 'yuv420p10le')
    raw = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).to(dev)
    for fmt, kw in (('bgr48le', {}), ('rgb24', dict(matrix='bt601', method='bilinear', loc='left', dither='ordered')), ('bgr24', dict(dither='round')), ('rgb48le', dict(matrix='bt2020nc', method='nearest'))):
        out = torch.zeros((3 * w * h * pixfmt.RGB_FORMATS[fmt][0] // 8,), dtype=torch.uint8, device=dev)
        f = ip.planesToRGB('yuv420p10le', w, h, fmt, **kw)
        assert f(raw, out) is out
        assert out.cpu().numpy().tobytes() == pixfmt.toRGB(frame, 'yuv420p10le', w, h, fmt, **kw), fmt
        assert raw.cpu().numpy().tobytes() == frame
        with pytest.raises(ValueError):
            f(raw[:-2], out)
        with pytest.raises(ValueError):
            f(raw, out[:-1])


# ---- the chains -------------------------------------------------------------------------------------------------------------------------------
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}
CHROMAS = {'net': {}, 'bicubic': {'chroma': 'bicubic', 'chromaLoc': 'left'}, 'guided': {'chroma': 'guided'}}
EXTRAS = ({}, {'matrix': 'bt601', 'chromaUp': 'bilinear', 'chromaLoc': 'left'}, {'matrix': 'bt2020nc', 'chromaUp': 'nearest', 'dither': 'ordered'})
SINKS = ('bgr24', 'bgr48le', 'rgb48le')
# name -> (width, height, source format, the source step's chroma keys, the output step): on 48 x 32 every 'chroma' with every sink, the sources and the output
# step's own keys taking turns; on 140 x 100 each 'chroma', each sink and both sources once more
CHAINS = {}
for _i, _c in enumerate(sorted(CHROMAS)):
    for _j, _s in enumerate(SINKS):
        CHAINS['48x32_{}_{}_{}'.format((8, 10)[(_i + _j) % 2], _c, _s)] = (48, 32, FMT[(8, 10)[(_i + _j) % 2]], CHROMAS[_c], dict({'op': 'output', 'pixFmt': _s}, **EXTRAS[(_i + _j) % 3]))
    CHAINS['140x100_{}_{}_{}'.format((10, 8)[_i % 2], _c, SINKS[_i])] = (140, 100, FMT[(10, 8)[_i % 2]], CHROMAS[_c], dict({'op': 'output', 'pixFmt': SINKS[_i]}, **EXTRAS[(_i + 1) % 3]))
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


def _frames(depth, w, h, seed=70):
    """Six frames, five of them distinct (a slot mix-up cannot hide): one repeated, then the same with a corner of its Y plane and a few chroma samples changed."""
    f = [_frame(seed + k, depth, w, h) for k in range(4)]
    part = np.frombuffer(f[1], _np_dt(depth)).copy()
    part[:w * h].reshape(h, w)[:16, :16] ^= 1
    part[w * h + 3:w * h + 9] ^= 2
    frames = [f[0], f[1], f[1], part.tobytes(), f[2], f[3]]
    assert len(set(frames)) == 5
    return frames


def _differ(got, want):
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    return 'sizes {} / {}'.format(g.size, w.size) if g.size != w.size else '{} of {} bytes differ, the first at {}'.format(int((g != w).sum()), g.size, int(np.argmax(g != w)))


def _serial_frames(steps, frames, w, h, src):
    from moephoto_amd import procedure
    process, nodes = procedure.genProcess(steps)
    serial = []
    assert procedure.runFrames(process, io.BytesIO(b''.join(frames)).read, serial.append, w, h, frameBytes=pixfmt.frameBytes(src, w, h)) == len(frames)
    return serial, nodes


def _defined(steps, frames, w, h, src, W, H):
    """What the definition says of a step list: the frames the same list gives with its RGB pixFmt replaced by 'yuv420p16le' (and without the keys that go with it),
    each through pixfmt.toRGB."""
    o = steps[-1]
    planar = steps[:-1] + [dict({k: v for k, v in o.items() if k in ('op', 'width', 'height', 'fit')}, pixFmt='yuv420p16le')]
    p16, _ = _serial_frames(planar, frames, w, h, src)
    return [pixfmt.toRGB(f, 'yuv420p16le', W, H, o['pixFmt'], o.get('matrix', 'bt709'), o.get('chromaUp', 'bicubic'), o.get('chromaLoc', 'center'), o.get('dither')) for f in p16]


def _steps(name):
    _, _, src, chroma, out = CHAINS[name]
    return [dict({'op': 'buffer', 'pixFmt': src}, **chroma), dict(SR), dict(out)]


def _reference(name):
    if name not in _serial:
        w, h, src = CHAINS[name][:3]
        frames = _frames(pixfmt.FORMATS[src], w, h)
        _serial[name] = (frames,) + _serial_frames(_steps(name), frames, w, h, src)
    return _serial[name]


def _run_stream(steps, w, h, frames, depth, mode):
    from moephoto_amd import procedure
    stream, got = procedure.genFrameStream(steps, w, h, depth, reuse=mode == 'reuse', views=mode == 'views'), []

    def write(buf):
        if mode == 'views':
            assert isinstance(buf, memoryview) and buf.readonly
        got.append(bytes(buf))
    assert procedure.runFramesStreamed(stream, io.BytesIO(b''.join(frames)).read, write) == len(frames)
    stream.close()
    return got, stream


@pytest.mark.parametrize('name', sorted(CHAINS))
def test_serial_frames_are_the_definition_of_the_planar_frames(name, dev):
    """genProcess + runFrames: every frame is pixfmt.toRGB of the frame the same list yields with 'yuv420p16le'.  (On the parent commit the output step raises
    ValueError: pixFmt "bgr48le" is not supported -- this test and the stream tests below fail there.)"""
    _configure()
    w, h, src, _, out = CHAINS[name]
    frames, serial, _ = _reference(name)
    want = _defined(_steps(name), frames, w, h, src, 2 * w, 2 * h)
    assert len(set(serial)) == 5
    for k, (g, d) in enumerate(zip(serial, want)):
        assert len(g) == 3 * 2 * w * 2 * h * pixfmt.RGB_FORMATS[out['pixFmt']][0] // 8
        assert g == d, '{} frame {}: {}'.format(name, k, _differ(g, d))


@pytest.mark.parametrize('mode', ['plain', 'reuse', 'views'])
@pytest.mark.parametrize('name', sorted(CHAINS))
def test_streams_equal_the_serial_frames(name, mode, dev):
    _configure()
    w, h = CHAINS[name][:2]
    frames, serial, nodes = _reference(name)
    for depth in (1, 2, 3):
        got, stream = _run_stream(_steps(name), w, h, frames, depth, mode)
        assert stream.edge == 'crop+rgb' and stream.nodes == nodes
        for k, (g, w_) in enumerate(zip(got, serial)):
            assert g == w_, '{} {} ring depth {} frame {}: {}'.format(name, mode, depth, k, _differ(g, w_))
        if mode == 'reuse':
            assert stream.reuse['pixels_run'] < stream.reuse['pixels_planned']


@pytest.mark.parametrize('kind', ['quantise', 'fit', 'fit_luma_only'])
def test_quantise_and_fit_edges(kind, dev):
    """A chain whose last step cannot fold into the frame (a blended dn_lite5 behind the SR step: edge 'quantise'), and chains with a size on the output step (P16 is
    then the fitted frame): serial = definition, streams = serial with and without reuse and views."""
    _configure()
    w, h, fmt = 48, 32, 'yuv420p10le'
    if kind == 'quantise':
        steps = [{'op': 'buffer', 'pixFmt': fmt}, dict(SR), {'op': 'DN', 'model': 'lite5', 'strength': 0.6}, {'op': 'output', 'pixFmt': 'bgr48le', 'dither': 'ordered'}]
        W, H, edge = 2 * w, 2 * h, 'quantise+rgb'
    else:
        source = dict({'op': 'buffer', 'pixFmt': fmt}, **(CHROMAS['bicubic'] if kind == 'fit_luma_only' else {}))
        steps = [source, dict(SR), {'op': 'output', 'pixFmt': 'rgb24' if kind == 'fit' else 'bgr48le', 'width': 70, 'height': 50, 'fit': 'bicubic', 'chromaLoc': 'left'}]
        W, H, edge = 70, 50, 'crop+fit+rgb'
    frames = _frames(10, w, h, seed=90)
    serial, nodes = _serial_frames(steps, frames, w, h, fmt)
    want = _defined(steps, frames, w, h, fmt, W, H)
    for k, (g, d) in enumerate(zip(serial, want)):
        assert g == d, '{} frame {}: {}'.format(kind, k, _differ(g, d))
    for depth, mode in ((1, 'plain'), (2, 'reuse'), (3, 'views'), (3, 'plain')):
        got, stream = _run_stream(steps, w, h, frames, depth, mode)
        assert stream.edge == edge and stream.nodes == nodes
        for k, (g, w_) in enumerate(zip(got, serial)):
            assert g == w_, '{} {} ring depth {} frame {}: {}'.format(kind, mode, depth, k, _differ(g, w_))
