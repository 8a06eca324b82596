"""Fitted sizes on interleaved images on the device (`pytest -m gpu`).  The comparator of the kernel is the written definition (pixfmt.fitPixels:
numpy, integers) and equality of bytes is the bar; the chains are held to the composed definition: fitPixels of the 16-bit samples the same step list gives without
its 'fit' resize step.

The tile-edge shapes come from resize_kernel_fit_px's output tile: FIT_TW = 128 ELEMENTS wide whatever the channel count (moephoto_amd/csrc/common.h), so at C = 3 a
tile ends inside a pixel, and 32, 16 or 8 rows high -- the host's choice per geometry, read back from the handle (moe_fit_info)."""
import ctypes
import io
from functools import reduce

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import pixfmt

pytestmark = pytest.mark.gpu
METHODS = ('nearest', 'bilinear', 'bicubic')
PAIRS = ((8, 8), (16, 16), (16, 8), (8, 16))
CHANNELS = (1, 2, 3, 4)
TILE_W, TILE_HS = 128, (32, 16, 8)          # FIT_TW of common.h; the heights the creator chooses from
SENTINEL = 0xA5


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _np_dt(depth):
    return np.uint8 if depth == 8 else np.dtype('<u2')


def _run(create, shape_out, src, ds, dd, tabs, dev, lead_src, lead_dst, planes_or_channels, h, w, oh, ow):
    """One handle, one run: source and destination `lead` SAMPLES behind a 16-byte boundary and between sentinel bytes that must survive.  -> (codes, info)."""
    from moephoto_amd import _lib
    es_s, es_d = (1 if ds == 8 else 2), (1 if dd == 8 else 2)
    a, b = lead_src * es_s, lead_dst * es_d
    n_out = int(np.prod(shape_out)) * es_d
    s_buf = torch.full((a + src.size + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    d_buf = torch.full((b + n_out + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    assert s_buf.data_ptr() % 16 == 0 and d_buf.data_ptr() % 16 == 0
    s_buf[a:a + src.size] = torch.from_numpy(src.copy()).to(dev)
    tx, ty = tabs
    L, handle, info = _lib.lib(), ctypes.c_void_p(), (ctypes.c_int64 * 4)()
    _lib.check(getattr(L, create)(planes_or_channels, ds, h, w, dd, oh, ow, tx[0], tx[1], tx[2], ty[0], ty[1], ty[2], 0, ctypes.byref(handle)))
    try:
        _lib.check(L.moe_fit_info(handle, info))
        _lib.check(L.moe_fit_run(handle, s_buf.data_ptr() + a, d_buf.data_ptr() + b, torch.cuda.current_stream().cuda_stream))
        out = d_buf.cpu().numpy()
    finally:
        L.moe_fit_destroy(handle)
    assert (out[:b] == SENTINEL).all() and (out[b + n_out:] == SENTINEL).all(), 'a sentinel around the destination was overwritten'
    assert (s_buf.cpu().numpy()[a + src.size:] == SENTINEL).all()
    assert info[0] == TILE_W and info[1] in TILE_HS and info[2] <= 80 * 1024 and info[3] == planes_or_channels
    return out[b:b + n_out].view(_np_dt(dd)).reshape(shape_out), tuple(int(v) for v in info)


def _device_fit_px(x, ds, dd, oh, ow, method, dev, lead_src=1, lead_dst=1):
    from moephoto_amd import imageProcess as ip
    h, w, C = x.shape
    src = np.ascontiguousarray(x.astype(_np_dt(ds))).view(np.uint8).reshape(-1)
    return _run('moe_fit_create_px', (oh, ow, C), src, ds, dd, (ip.fitTables(method, w, ow), ip.fitTables(method, h, oh)), dev, lead_src, lead_dst, C, h, w, oh, ow)


def _check(x, ds, dd, oh, ow, method, dev, leads=((1, 1),)):
    """The kernel against the definition, byte for byte -> the handle's info."""
    want = pixfmt.fitPixels(x, ds, dd, oh, ow, method)
    for ls, ld in leads:
        got, info = _device_fit_px(x, ds, dd, oh, ow, method, dev, ls, ld)
        bad = got != want
        assert not bad.any(), '{} {}x{}x{} -> {}x{} {}->{} leads {}/{}: {} of {} samples differ, the first at (row, pixel, channel) {}'.format(
            method, x.shape[1], x.shape[0], x.shape[2], ow, oh, ds, dd, ls, ld, int(bad.sum()), bad.size, tuple(int(i) for i in np.argwhere(bad)[0]))
    return info


def _codes(seed, depth, h, w, C):
    c = np.random.default_rng(seed).integers(0, 1 << depth, size=(h, w, C))
    if c.size > 2:
        c.reshape(-1)[:2] = (0, (1 << depth) - 1)
    return c


# (h, w) -> (oh, ow): the smallest; windows that overhang all four image edges; coprime sizes both ways (at C = 3 a row of 43 pixels is 129 elements: a second tile of
# one element that splits no pixel); exactly 4 : 1; n = m; 16 : 1 up
SMALL = (((1, 1), (1, 1)), ((2, 2), (7, 5)), ((5, 5), (2, 2)), ((37, 41), (23, 43)), ((23, 29), (37, 41)), ((64, 68), (16, 17)), ((19, 23), (19, 23)), ((6, 9), (96, 40)))


@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('method', METHODS)
def test_small_images_every_depth_pair(method, C, dev):
    for (h, w), (oh, ow) in SMALL:
        for ds, dd in PAIRS:
            x = _codes(h + ow + ds + C, ds, h, w, C)
            _check(x, ds, dd, oh, ow, method, dev, leads=((1, 1), (0, 0)) if (ds, dd) == (16, 16) else ((1, 1),))
            if (h, w) == (oh, ow):
                got, _ = _device_fit_px(x, ds, dd, oh, ow, method, dev)
                assert (got == (x << (dd - ds) if dd >= ds else x >> (ds - dd))).all()          # the identity, up to the depth shift


def _source(m, ratio):
    """The source size of m outputs at ratio 1/4 (exactly) or 3/2 (to the next sample)."""
    return 4 * m if ratio == '1/4' else -(-2 * m // 3)


@pytest.mark.parametrize('ratio', ['1/4', '3/2'])
@pytest.mark.parametrize('method', ['bicubic', 'bilinear', 'nearest'])
def test_rows_of_elements_around_the_tile(ratio, method, dev):
    """ow * C in {126 .. 130} wherever C divides it -- one element short of the tile to two over it -- and ow = 85, 86 at C = 3: 255 and 258 elements, where pixel 42 lies
    across elements 127 | 128 and pixel 85 across 255 | 256, each half in another workgroup."""
    rows = sorted({(n // C, C) for n in (126, 127, 128, 129, 130) for C in CHANNELS if n % C == 0} | {(85, 3), (86, 3)})
    assert (42, 3) in rows and (43, 3) in rows and (127, 1) in rows and (32, 4) in rows and (65, 2) in rows
    for ow, C in rows:
        for ds, dd in ((16, 16), (8, 8)) if C == 3 else ((16, 8),):
            _check(_codes(ow + C + ds, ds, _source(9, ratio), _source(ow, ratio), C), ds, dd, 9, ow, method, dev, leads=((1, 1), (0, 1)))


@pytest.mark.parametrize('method', METHODS)
def test_rows_of_several_tiles(method, dev):
    """Rows of four and more tiles: the tiles between the outermost ones hold windows that touch neither the left nor the right edge of the image (no clamp takes part
    in their load), with source and destination at three alignments."""
    for C, (h, w), (oh, ow) in ((3, (20, 300), (10, 150)), (3, (9, 140), (13, 210)), (4, (12, 131), (7, 140)), (1, (8, 1000), (8, 515)), (2, (11, 517), (5, 259))):
        for ds, dd in PAIRS:
            _check(_codes(C + ow + ds, ds, h, w, C), ds, dd, oh, ow, method, dev, leads=((1, 1), (0, 0), (3, 5)))


@pytest.mark.parametrize('ratio', ['1/4', '3/2'])
def test_rows_one_around_the_tiles_height(ratio, dev):
    """oh one row short of the handle's tile, exactly a tile and one over it; the height is the host's choice per geometry and is read from the handle."""
    heights = set()
    for C, ow, ds, dd in ((3, 45, 16, 16), (4, 33, 8, 8), (2, 70, 16, 8)):
        th = _check(_codes(C, ds, _source(32, ratio), _source(ow, ratio), C), ds, dd, 32, ow, 'bicubic', dev)[1]          # (every height it chooses from divides 32)
        heights.add(th)
        for oh in (th - 1, th, th + 1):
            assert _check(_codes(oh + C, ds, _source(oh, ratio), _source(ow, ratio), C), ds, dd, oh, ow, 'bicubic', dev, leads=((1, 1), (0, 0)))[1] in TILE_HS
    assert heights <= set(TILE_HS)


@pytest.mark.parametrize('method', METHODS)
def test_channels_do_not_mix(method, dev):
    """Channel 0 a ramp, the others flat 0 and flat 2^D - 1 (every order of them): the flat channels come back flat exactly -- a tap read at the wrong stride, or a
    window clamped per element at the right edge, takes a neighbour's code."""
    for C in (2, 3, 4):
        for (h, w), (oh, ow) in (((9, 50), (5, 43)), ((7, 11), (20, 47)), ((16, 172), (4, 43)), ((5, 3), (5, 48))):
            for ds, dd in PAIRS:
                top = (1 << ds) - 1
                for ramp in range(C):
                    x = np.zeros((h, w, C), np.int64)
                    flats = {}
                    for c in range(C):
                        if c == ramp:
                            x[:, :, c] = (np.arange(h)[:, None] * 977 + np.arange(w)[None, :] * 3571) % (top + 1)
                        else:
                            flats[c] = top if (c + ramp) % 2 else 0
                            x[:, :, c] = flats[c]
                    _check(x, ds, dd, oh, ow, method, dev)
                    got, _ = _device_fit_px(x, ds, dd, oh, ow, method, dev, 0, 1)
                    for c, code in flats.items():
                        want = code << (dd - ds) if dd >= ds else code >> (ds - dd)
                        assert (got[:, :, c] == want).all(), (C, ramp, c, ds, dd, h, w, oh, ow)


def test_checkerboard_of_extremes_at_bicubic_4_down(dev):
    """0 / 65535 checkerboards, another phase per channel, 4 : 1 down with the 16-tap bicubic rows: the row pass's sums come as close to the int32 bound as codes can
    bring them and the negative lobes ask for the clamp."""
    for C in CHANNELS:
        h, w, oh, ow = 64, 172, 16, 43
        yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
        x = np.stack([(((yy + xx + c) % 2) if c < 2 else ((yy // 2 + xx // (c + 1) + c) % 2)) * 65535 for c in range(C)], axis=2).astype(np.int64)
        assert len({x[:, :, c].tobytes() for c in range(C)}) == C
        for dd in (16, 8):
            _check(x, 16, dd, oh, ow, 'bicubic', dev, leads=((1, 1), (0, 0)))
        _check(x, 16, 16, 23, 61, 'bicubic', dev)
        stripes = np.zeros((h, w, C), np.int64)          # full-scale edges in both axes, channels alternating in sign
        stripes[:, w // 2:, :] = 65535
        stripes[h // 2:, :, :] = 65535 - stripes[h // 2:, :, :]
        stripes[:, :, 1::2] = 65535 - stripes[:, :, 1::2]
        _check(stripes, 16, 16, oh, ow, 'bicubic', dev)


@pytest.mark.parametrize('method', METHODS)
def test_one_channel_is_the_planar_kernel_with_one_plane(method, dev):
    from moephoto_amd import imageProcess as ip
    for (h, w), (oh, ow) in (((37, 41), (23, 43)), ((64, 520), (16, 130)), ((23, 90), (37, 131))):
        for ds, dd in PAIRS:
            x = _codes(h + ow + ds, ds, h, w, 1)
            src = np.ascontiguousarray(x.astype(_np_dt(ds))).view(np.uint8).reshape(-1)
            tabs = (ip.fitTables(method, w, ow), ip.fitTables(method, h, oh))
            px, ipx = _run('moe_fit_create_px', (oh, ow, 1), src, ds, dd, tabs, dev, 1, 1, 1, h, w, oh, ow)
            pl, ipl = _run('moe_fit_create', (1, oh, ow), src, ds, dd, tabs, dev, 1, 1, 1, h, w, oh, ow)
            assert px.tobytes() == pl.tobytes() and ipx == ipl, (h, w, oh, ow, ds, dd)


def test_fitpixels_wrapper(dev):
    from moephoto_amd import imageProcess as ip
    h, w, H, W = 10, 18, 14, 26
    x = np.random.default_rng(4).integers(0, 65536, (h, w, 3)).astype('<u2')
    raw = torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).to(dev)
    lead, n = 6, H * W * 3
    out = torch.full((lead + n + 10,), SENTINEL, dtype=torch.uint8, device=dev)
    f = ip.fitPixels(16, 8, 3, h, w, H, W, 'bicubic')
    assert f(raw, out[lead:lead + n]) is not None
    info = f.info(dev)
    assert info['tile'][0] == TILE_W and info['tile'][1] in TILE_HS and info['planes'] == 3
    host = out.cpu().numpy()
    assert (host[:lead] == SENTINEL).all() and (host[lead + n:] == SENTINEL).all()
    assert host[lead:lead + n].tobytes() == pixfmt.fitPixels(x, 16, 8, H, W, 'bicubic').tobytes()
    f(raw, out[lead:lead + n])                  # (the handle is reused)
    assert out.cpu().numpy().tobytes() == host.tobytes()
    with pytest.raises(ValueError):
        f(raw[:-2], out[lead:lead + n])
    with pytest.raises(ValueError):
        f(raw, out[lead:lead + n - 1])
    with pytest.raises(ValueError):
        f(raw.to(torch.int8), out[lead:lead + n])
    with pytest.raises(Exception):
        f(raw.cpu(), out[lead:lead + n])


# ---- the chains ---------------------------------------------------------------------------------------------------------------------------------
W, H = 140, 100
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}
DN = {'op': 'DN', 'model': 'lite5', 'strength': 0.6}
SIZES = [(210, 150), (420, 300)]


def _configure():
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, True
    config.crop_sr = config.crop_dn = config.crop_dns = 48
    config.ensembleSR = 0


def _frame(seed, depth):
    a = np.random.default_rng(seed).integers(0, 1 << depth, W * H * 3, dtype=np.uint32)
    a[:2] = (0, (1 << depth) - 1)
    return a.astype(_np_dt(depth)).tobytes()


def _differ(got, want):
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    return 'sizes {} / {}'.format(g.size, w.size) if g.size != w.size else '{} of {} bytes differ, the first at {}'.format(int((g != w).sum()), g.size, int(np.argmax(g != w)))


def _stream(steps, frames, depth=2, **kw):
    from moephoto_amd import procedure
    stream = procedure.genFrameStream([dict(s) for s in steps], W, H, depth, **kw)
    got = []
    assert procedure.runFramesStreamed(stream, io.BytesIO(b''.join(frames)).read, lambda b: got.append(bytes(b))) == len(frames)
    stream.close()
    return got, stream


def _unfused16(images, bitDepth, work):
    """The 16-bit samples of a chain from its definition, step by step: toTorch(bitDepth), the steps, toFloat -> toOutput(16).  For the sources whose depth is not 16:
    no chain of the builders writes 16-bit samples from 8-bit frames."""
    from moephoto_amd import imageProcess as ip, runDN, runSR
    from moephoto_amd.config import config
    funcs = [runSR.sr(runSR.getOpt(dict(s))) if s['op'] == 'SR' else ip.RGBFilter(runDN.getOpt(dict(s))) for s in work]
    return [ip.toOutput(16)(ip.toFloat(reduce(lambda x, f: f(x), funcs, ip.toTorch(bitDepth, config.dtype(), config.device())(im)))) for im in images]


SAMPLES = {}          # (bitDepth, work) -> the chain's own 16-bit samples per frame, (h, w, 3): computed once, shared by the sizes and left unchanged


def _samples16(key, bitDepth, work, frames):
    if key not in SAMPLES:
        if bitDepth == 16:          # the chain as the stream builder runs it today, whichever edge that is
            got, stream = _stream([{'op': 'buffer', 'bitDepth': 16}] + work, frames)
            scale = 2 if any(s['op'] == 'SR' for s in work) else 1
            SAMPLES[key] = ([np.frombuffer(g, '<u2').reshape(H * scale, W * scale, 3) for g in got], stream.edge)
        else:
            SAMPLES[key] = (_unfused16([np.frombuffer(f, np.uint8).reshape(H, W, 3).copy() for f in frames], 8, work), None)
    return SAMPLES[key]


def _want(samples, bitDepth, size, fit):
    return [pixfmt.fitPixels(s, 16, bitDepth, size[1], size[0], fit).tobytes() for s in samples]


@pytest.mark.parametrize('size', SIZES, ids=['210x150', '420x300'])
@pytest.mark.parametrize('bitDepth', [8, 16], ids=['bgr24', 'bgr48le'])
def test_fitted_rgb_streams(bitDepth, size, dev):
    """An a2 stream at 140 x 100 (the net's own 280 x 200) fitted to 210 x 150 (3/4: antialiased) and to 420 x 300 (3/2), at every ring depth, with reuse on a frame
    shown twice, and as views."""
    from moephoto_amd import procedure
    _configure()
    frames = [_frame(40 + bitDepth + k, bitDepth) for k in range(3)]
    frames.insert(2, frames[1])          # a repeated frame: with reuse no tile of it runs
    samples, edge = _samples16(('sr', bitDepth), bitDepth, [dict(SR)], frames)
    assert edge in (None, 'crop')
    want = _want(samples, bitDepth, size, 'bicubic')
    es = bitDepth // 8
    assert len(set(want)) == 3 and all(len(w_) == size[0] * size[1] * 3 * es for w_ in want)
    steps = [{'op': 'buffer', 'bitDepth': bitDepth}, dict(SR), {'op': 'resize', 'width': size[0], 'height': size[1], 'fit': 'bicubic'}]
    process, nodes = procedure.genProcess([dict(s) for s in steps])
    assert nodes[-1] == dict(op='resize', mode='bicubic') and len(nodes) == 2
    serial = []
    assert procedure.runFrames(process, io.BytesIO(b''.join(frames)).read, serial.append, W, H, bitDepth) == 4
    for k, (g, w_) in enumerate(zip(serial, want)):
        assert g == w_, 'serial frame {}: {}'.format(k, _differ(g, w_))
    for depth, kw in ((1, {}), (2, {}), (3, {}), (2, dict(reuse=True)), (2, dict(views=True)), (2, dict(reuse=True, views=True))):
        got, stream = _stream(steps, frames, depth, **kw)
        assert stream.edge == 'crop+fit' and stream.nodes == nodes
        for k, (g, w_) in enumerate(zip(got, want)):
            assert g == w_, 'ring depth {} {} frame {}: {}'.format(depth, kw, k, _differ(g, w_))
        if kw.get('reuse'):
            assert stream.reuse['frames'][2] and all(run == 0 for _, run in stream.reuse['frames'][2].values()), stream.reuse['frames'][2]


def test_fitted_stream_takes_scales_and_the_other_methods(dev):
    """The size from 'scaleW' / 'scaleH', rounded as the resize step rounds, with bilinear and nearest."""
    _configure()
    frames = [_frame(56 + k, 16) for k in range(3)]
    frames.insert(2, frames[1])
    samples, _ = _samples16(('sr', 16), 16, [dict(SR)], frames)
    for fit, scaleW, scaleH in (('bilinear', 0.755, 0.5), ('nearest', 1.5, 1.275)):
        size = (round(280 * scaleW), round(200 * scaleH))
        got, stream = _stream([{'op': 'buffer', 'bitDepth': 16}, dict(SR), {'op': 'resize', 'scaleW': scaleW, 'scaleH': scaleH, 'fit': fit}], frames)
        assert stream.nodes[-1] == dict(op='resize', mode=fit)
        for k, (g, w_) in enumerate(zip(got, _want(samples, 16, size, fit))):
            assert g == w_, '{} frame {}: {}'.format(fit, k, _differ(g, w_))


@pytest.mark.parametrize('bitDepth', [8, 16], ids=['bgr24', 'bgr48le'])
def test_fitted_stream_behind_a_blended_dn_step(bitDepth, dev):
    """A DN of strength 0.6 ahead of the SR; and as the chain's last step, where the blend rides in the fold (edge 'filter')."""
    _configure()
    frames = [_frame(70 + bitDepth + k, bitDepth) for k in range(2)]
    for name, work, edge, size in (('dn_sr', [dict(DN), dict(SR)], 'crop', (210, 150)), ('dn', [dict(DN)], 'filter', (106, 76))):
        samples, plain = _samples16((name, bitDepth), bitDepth, work, frames)
        assert plain in (None, edge)
        want = _want(samples, bitDepth, size, 'bicubic')
        steps = [{'op': 'buffer', 'bitDepth': bitDepth}] + work + [{'op': 'resize', 'width': size[0], 'height': size[1], 'fit': 'bicubic'}]
        for kw in ({}, dict(reuse=True)):
            got, stream = _stream(steps, frames, 2, **kw)
            assert stream.edge == edge + '+fit'
            for k, (g, w_) in enumerate(zip(got, want)):
                assert g == w_, '{} {} frame {}: {}'.format(name, kw, k, _differ(g, w_))


@pytest.mark.parametrize('size', SIZES, ids=['210x150', '420x300'])
def test_fitted_stream_behind_a_luma_only_step(size, dev):
    """'chroma': 'bicubic' on the SR step: the fold that merges Y' with the resized chroma planes writes the 16-bit samples, the filter the frame."""
    from moephoto_amd import procedure
    _configure()
    frames = [_frame(90 + k, 16) for k in range(3)]
    frames.insert(1, frames[0])
    sr = dict(SR, chroma='bicubic')
    samples, edge = _samples16(('luma', 16), 16, [sr], frames)
    assert edge == 'crop'
    for bitDepth in (16,):
        want = _want(samples, bitDepth, size, 'bicubic')
        steps = [{'op': 'buffer', 'bitDepth': bitDepth}, dict(sr), {'op': 'resize', 'width': size[0], 'height': size[1], 'fit': 'bicubic'}]
        for kw in ({}, dict(reuse=True), dict(views=True)):
            got, stream = _stream(steps, frames, 2, **kw)
            assert stream.edge == 'crop+fit'
            for k, (g, w_) in enumerate(zip(got, want)):
                assert g == w_, '{} frame {}: {}'.format(kw, k, _differ(g, w_))
        process, _ = procedure.genProcess([dict(s) for s in steps])
        serial = []
        assert procedure.runFrames(process, io.BytesIO(b''.join(frames)).read, serial.append, W, H, bitDepth) == 4
        assert serial == want


def test_fitted_stream_behind_an_ensemble(dev):
    """An SR with ensemble: no fold writes samples, the unfused quantiser does, at 16 bits (edge 'quantise+fit')."""
    _configure()
    frames = [_frame(110 + k, 16) for k in range(2)]
    sr = dict(SR, ensemble=1)
    samples, edge = _samples16(('ens', 16), 16, [sr], frames)
    assert edge == 'quantise'
    got, stream = _stream([{'op': 'buffer', 'bitDepth': 16}, dict(sr), {'op': 'resize', 'width': 210, 'height': 150, 'fit': 'bilinear'}], frames)
    assert stream.edge == 'quantise+fit'
    for k, (g, w_) in enumerate(zip(got, _want(samples, 16, (210, 150), 'bilinear'))):
        assert g == w_, 'frame {}: {}'.format(k, _differ(g, w_))


@pytest.mark.parametrize('size', SIZES, ids=['210x150', '420x300'])
def test_genprocess_on_an_array_source(size, dev):
    """Arrays of 3 and of 4 channels at 16 bits against genProcess without the step; of 3 channels at 8 bits against the unfused definition."""
    from moephoto_amd import procedure
    _configure()
    fit = {'op': 'resize', 'width': size[0], 'height': size[1], 'fit': 'bicubic'}
    for C in (3, 4):
        im = np.random.default_rng(120 + C).integers(0, 65536, (H, W, C)).astype(np.uint16)
        key = ('array', C)
        if key not in SAMPLES:
            SAMPLES[key] = procedure.genProcess([dict(SR)], 16)[0](im)
        process, nodes = procedure.genProcess([dict(SR), dict(fit)], 16)
        got = process(im)
        assert nodes[-1] == dict(op='resize', mode='bicubic')
        assert got.dtype == np.uint16 and got.shape == (size[1], size[0], C)
        assert got.tobytes() == pixfmt.fitPixels(SAMPLES[key], 16, 16, size[1], size[0], 'bicubic').tobytes()
        assert process(im).tobytes() == got.tobytes()          # (the handle is reused)
    im8 = np.random.default_rng(130).integers(0, 256, (H, W, 3)).astype(np.uint8)
    if 'array8' not in SAMPLES:
        SAMPLES['array8'] = _unfused16([im8], 8, [dict(SR)])[0]
    got = procedure.genProcess([dict(SR), dict(fit)], 8)[0](im8)
    assert got.dtype == np.uint8 and got.tobytes() == pixfmt.fitPixels(SAMPLES['array8'], 16, 8, size[1], size[0], 'bicubic').tobytes()


def test_first_frame_refuses_a_ratio_beyond_the_filter(dev):
    """genProcess learns the size with the first image: a ratio beyond 4 down is refused there, by key."""
    from moephoto_amd import procedure
    _configure()
    process, _ = procedure.genProcess([dict(SR), {'op': 'resize', 'width': 69, 'height': 150, 'fit': 'bicubic'}], 16)
    with pytest.raises(ValueError, match="'width' \\(69 samples\\) shrinks the chain's 280 by more than 4"):
        process(np.zeros((H, W, 3), np.uint16))
