"""The 3D LUT colour step on the device (`pytest -m gpu`).  The comparator of the kernel is the written definition (lut3d.apply: numpy, every
operation rounded to float32 on its own) and equality of bytes is the bar; the streams are held to genProcess + runFrames on the whole frame, and every frame to
lut3d.apply of the 16-bit frame the same step list yields without the step.

to_output_lut3d_kernel (moephoto_amd/csrc/lut3d.hip) gives a thread eight consecutive pixels of a row: the shapes are a single pixel, rows shorter than a run, one
whole run, ragged rows, a width that is a multiple of 8 (whole vector runs in every row) and one that is not, over more than one workgroup."""
import io

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import lut3d, pixfmt, quant

pytestmark = pytest.mark.gpu
SIZES = ((1, 1), (3, 2), (8, 1), (17, 5), (136, 34), (262, 74))          # (w, h)
VERTS = ('uniform', 'nonuniform', 'inner')
ORDERS = ('bgr', 'rgb')
DITHERS = (None, 'round', 'ordered')
STRENGTHS = (1.0, 0.6, 0.0)
SENTINEL = 0xA5
_luts, _handles = {}, {}


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _lut(d, kind):
    """A random table with values a little outside [0, 1] (both clamps of the quantiser occur) over: uniform vertices; non-uniform ones with one vertex repeated (a
    zero-width interval; d = 2 has no room for one); vertices that span [0.1, 0.9] only, so that full-range noise extrapolates on both sides."""
    if (d, kind) not in _luts:
        rng = np.random.default_rng(1000 * d + VERTS.index(kind))
        table = (rng.random((3, d, d, d), np.float32) * np.float32(1.4) - np.float32(0.2)).astype(np.float32)
        if kind == 'uniform':
            v = lut3d.uniform(d)
        elif kind == 'inner':
            v = lut3d.uniform(d, 0.1, 0.9)
        else:
            v = np.sort(rng.random((3, d)).astype(np.float32), axis=1)
            v[:, 0], v[:, -1] = 0, 1
            if d > 2:
                v[:, d // 2] = v[:, d // 2 - 1]
        _luts[(d, kind)] = lut3d.check(table, v)
    return _luts[(d, kind)]


def _handle(d, kind):
    from moephoto_amd import imageProcess as ip
    if (d, kind) not in _handles:
        _handles[(d, kind)] = ip._LutHandle(*_lut(d, kind), 0)
    return _handles[(d, kind)]


def _codes(seed, bits, n):
    c = np.random.default_rng(seed).integers(0, 1 << bits, size=n)
    c[:2] = (0, (1 << bits) - 1)
    return c.astype(np.uint8 if bits == 8 else np.uint16)


def _device(samples, srcBits, w, h, d, kind, bits, order, strength, dither, dev, lead):
    """moe_lut3d_run on a frame, source and destination `lead` SAMPLES behind a 16-byte boundary and between sentinel bytes that must survive; the source must come
    back as it went in."""
    from moephoto_amd import _lib
    src = samples.view(np.uint8).reshape(-1)
    a, b, n_out = lead * (srcBits // 8), lead * (bits // 8), 3 * w * h * (bits // 8)
    s_buf = torch.full((a + src.size + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    d_buf = torch.full((b + n_out + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    assert s_buf.data_ptr() % 16 == 0 and d_buf.data_ptr() % 16 == 0
    s_buf[a:a + src.size] = torch.from_numpy(src.copy()).to(dev)
    _lib.check(_lib.lib().moe_lut3d_run(_handle(d, kind)._h, s_buf.data_ptr() + a, srcBits, h, w, d_buf.data_ptr() + b, bits | quant.flags(dither, bits, 'rgb'),
                                        pixfmt.ORDERS[order], strength, torch.cuda.current_stream().cuda_stream))
    out, back = d_buf.cpu().numpy(), s_buf.cpu().numpy()
    assert (out[:b] == SENTINEL).all() and (out[b + n_out:] == SENTINEL).all(), 'a sentinel around the destination was overwritten'
    assert (back[:a] == SENTINEL).all() and (back[a + src.size:] == SENTINEL).all() and (back[a:a + src.size] == src).all(), 'the source or a sentinel around it was written'
    return out[b:b + n_out].view(np.uint8 if bits == 8 else np.uint16).reshape(h, w, 3)


def _check(seed, wh, srcBits, d, kind, bits, order, strength, dither, dev):
    w, h = wh
    samples = _codes(seed, srcBits, 3 * w * h).reshape(h, w, 3)
    want = lut3d.apply(samples, srcBits, *_lut(d, kind), bits, order, strength, dither)
    for lead in (1, 0):
        got = _device(samples, srcBits, w, h, d, kind, bits, order, strength, dither, dev, lead)
        bad = got != want
        assert not bad.any(), '{}x{} {} -> {} d {} {} {} s {} {} lead {}: {} of {} samples differ, the first at {} (device {}, definition {})'.format(
            w, h, srcBits, bits, d, kind, order, strength, dither, lead, int(bad.sum()), bad.size, int(np.argmax(bad)), got[bad][0], want[bad][0])


@pytest.mark.parametrize('bits', (8, 16))
@pytest.mark.parametrize('srcBits', (8, 16))
@pytest.mark.parametrize('d', (2, 17, 33, 65))
def test_kernel_is_the_definition(d, srcBits, bits, dev):
    """17 x 5 sees the whole cross of vertices, orders, quantisers and strengths; every other size nine combinations in which each value of each of the four occurs,
    shifted from size to size.  Every combination runs one sample off a 16-byte boundary and aligned."""
    for i, wh in enumerate(SIZES):
        if wh == (17, 5):
            combos = [(k, o, q, s) for k in VERTS for o in ORDERS for q in DITHERS for s in STRENGTHS]
        else:
            combos = [(VERTS[j % 3], ORDERS[(j + i) % 2], DITHERS[(j // 3 + i) % 3], STRENGTHS[(j + j // 3 + i) % 3]) for j in range(9)]
        for kind, order, dither, strength in combos:
            _check(7 * d + srcBits + bits + i, wh, srcBits, d, kind, bits, order, strength, dither, dev)


def test_identity_returns_every_code_on_the_device(dev):
    codes = np.arange(65536, dtype=np.uint16)
    im = np.ascontiguousarray(np.stack([codes, codes[::-1], np.roll(codes, 77)], -1).reshape(256, 256, 3))
    _luts[(33, 'identity')] = (lut3d.identity(33), lut3d.uniform(33))
    assert (_device(im, 16, 256, 256, 33, 'identity', 16, 'bgr', 1.0, 'round', dev, 0) == im).all()


def test_lut3d_wrapper(dev):
    from moephoto_amd import imageProcess as ip
    w, h = 18, 10
    table, vertices = _lut(17, 'nonuniform')
    for srcBits, bits, kw in ((16, 16, {}), (8, 8, dict(order='rgb', strength=0.6, dither='ordered')), (16, 8, dict(dither='round')), (8, 16, dict(strength=0.0))):
        samples = _codes(3, srcBits, 3 * w * h).reshape(h, w, 3)
        raw = torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev)
        out = torch.zeros((3 * w * h * bits // 8,), dtype=torch.uint8, device=dev)
        f = ip.lut3d(table, vertices, srcBits, bits, **kw)
        assert f(raw, out, h, w) is out
        assert out.cpu().numpy().tobytes() == lut3d.apply(samples, srcBits, table, vertices, bits, **dict(dict(order='bgr'), **kw)).tobytes(), (srcBits, bits)
        assert raw.cpu().numpy().tobytes() == samples.tobytes()
        with pytest.raises(ValueError):
            f(raw[:-2], out, h, w)
        with pytest.raises(ValueError):
            f(raw, out[:-1], h, w)
    assert ip.lut3d(table, vertices).info(dev) == dict(d=17, tableBytes=16 * 17 ** 3, lds=3 * 65 * 4, pixels=8)
    uniform = ip.lut3d(lut3d.identity(5))          # (vertices default to uniform ones)
    samples = _codes(5, 16, 3 * w * h).reshape(h, w, 3)
    out = torch.zeros((3 * w * h * 2,), dtype=torch.uint8, device=dev)
    uniform(torch.from_numpy(samples.view(np.uint8).reshape(-1).copy()).to(dev), out, h, w)
    assert out.cpu().numpy().tobytes() == lut3d.apply(samples, 16, lut3d.identity(5), lut3d.uniform(5), 16).tobytes()


# ---- the chains -------------------------------------------------------------------------------------------------------------------------------
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}
DN = {'op': 'DN', 'model': 'lite5', 'strength': 0.6}
FIT = {'op': 'resize', 'width': 70, 'height': 50, 'fit': 'bicubic'}
BGR24, BGR48, YUV10, YUV8 = {'op': 'buffer', 'bitDepth': 8}, {'op': 'buffer', 'bitDepth': 16}, {'op': 'buffer', 'pixFmt': 'yuv420p10le'}, {'op': 'buffer', 'pixFmt': 'yuv420p'}


def _lutStep(d, kind, **kw):
    table, vertices = _lut(d, kind)
    return dict({'op': 'lut', 'table': table, 'vertices': vertices}, **kw)


# name -> (width, height, source step, compute steps in front of the 'lut' step, the 'lut' step's table and keys, output step or None, stream.edge): the sources and
# the chain's own edges take turns on both sizes
CHAINS = {
    '48x32_bgr48le_sr': (48, 32, BGR48, [SR], (33, 'uniform', {}), None, 'crop+lut'),
    '48x32_bgr24_sr_strength_ordered': (48, 32, BGR24, [SR], (17, 'nonuniform', {'strength': 0.6}), {'op': 'output', 'dither': 'ordered'}, 'crop+lut'),
    '48x32_yuv420p10le_sr_round': (48, 32, YUV10, [SR], (33, 'nonuniform', {}), {'op': 'output', 'pixFmt': 'bgr48le', 'dither': 'round'}, 'crop+rgb+lut'),
    '48x32_bgr48le_sr_fit': (48, 32, BGR48, [SR, FIT], (17, 'inner', {}), None, 'crop+fit+lut'),
    '140x100_bgr48le_sr_dn': (140, 100, BGR48, [SR, DN], (33, 'nonuniform', {'strength': 0.25}), {'op': 'output', 'dither': 'round'}, 'filter+lut'),
    '140x100_bgr48le_sr_luma': (140, 100, BGR48, [dict(SR, chroma='bicubic')], (65, 'uniform', {}), None, 'crop+lut'),
    '140x100_yuv420p_sr_bgr24': (140, 100, YUV8, [SR], (17, 'uniform', {}), {'op': 'output', 'pixFmt': 'bgr24', 'dither': 'ordered'}, 'crop+rgb+lut'),
}
_serial = {}          # name -> (frames, genProcess + runFrames' frames, nodes): computed once, shared by the modes


def _configure():
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, True
    config.crop_sr = config.crop_dn = config.crop_dns = 48
    config.ensembleSR = 0


def _source(name):
    """(frame bytes, numpy dtype of a sample, planar pixFmt or None) of a chain's source step."""
    w, h, src = CHAINS[name][:3]
    if 'pixFmt' in src:
        return pixfmt.frameBytes(src['pixFmt'], w, h), (np.uint8 if src['pixFmt'] == 'yuv420p' else np.uint16), src['pixFmt']
    return 3 * w * h * src['bitDepth'] // 8, (np.uint8 if src['bitDepth'] == 8 else np.uint16), None


def _frames(name, seed=70):
    """Six frames, five of them distinct (a slot mix-up cannot hide): one repeated, then the same with a corner changed."""
    w, h = CHAINS[name][:2]
    nbytes, dt, fmt = _source(name)
    top = (1 << pixfmt.FORMATS[fmt]) if fmt else (1 << (8 * np.dtype(dt).itemsize))
    f = [np.random.default_rng(seed + k).integers(0, top, nbytes // np.dtype(dt).itemsize).astype(dt) for k in range(4)]
    part = f[1].copy()
    if fmt:
        part[:w * h].reshape(h, w)[:16, :16] ^= 1
    else:
        part.reshape(h, w, 3)[:16, :16] ^= 1
    frames = [a.tobytes() for a in (f[0], f[1], f[1], part, f[2], f[3])]
    assert len(set(frames)) == 5
    return frames


def _steps(name, lut=True):
    _, _, src, work, (d, kind, kw), out, _ = CHAINS[name]
    return [dict(src)] + [dict(s) for s in work] + ([_lutStep(d, kind, **kw)] if lut else []) + ([dict(out)] if out else [])


def _differ(got, want):
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    return 'sizes {} / {}'.format(g.size, w.size) if g.size != w.size else '{} of {} bytes differ, the first at {}'.format(int((g != w).sum()), g.size, int(np.argmax(g != w)))


def _serial_frames(steps, frames, w, h, nbytes):
    from moephoto_amd import procedure
    process, nodes = procedure.genProcess(steps)
    serial = []
    assert procedure.runFrames(process, io.BytesIO(b''.join(frames)).read, serial.append, w, h, frameBytes=nbytes) == len(frames)
    return serial, nodes


def _p16(name, frames):
    """The 16-bit frames the chain's list yields without the 'lut' step and without 'dither' -- a planar chain with the 48-bit form of its pixFmt, a bgr48le chain as
    it is.  A bgr24 chain (plain SR) has no step list that writes 16-bit samples of 8-bit frames: its frames are the chain's own pieces put together, toNumPy and
    toTorch at 8 bits, the SR step, the 16-bit quantiser."""
    from moephoto_amd import imageProcess as ip, procedure, runSR
    from moephoto_amd.config import config
    w, h, src, work, _, out, _ = CHAINS[name]
    nbytes, _, fmt = _source(name)
    if fmt is None and src['bitDepth'] == 8:
        assert work == [SR]
        o = runSR.getOpt(dict(SR))
        return [procedure._samplesOnDevice(16)(runSR.sr(o)(ip.toTorch(8, config.dtype(), config.device())(ip.toNumPy(8)((f, h, w))))).cpu().numpy().view(np.uint16) for f in frames]
    steps = _steps(name, lut=False)
    if out:
        steps[-1] = {k: v for k, v in steps[-1].items() if k != 'dither'}
        if fmt:
            steps[-1]['pixFmt'] = {'bgr24': 'bgr48le', 'rgb24': 'rgb48le'}.get(out['pixFmt'], out['pixFmt'])
    return [np.frombuffer(f, np.uint16) for f in _serial_frames(steps, frames, w, h, nbytes)[0]]


def _defined(name, frames):
    w, h, src, work, (d, kind, kw), out, _ = CHAINS[name]
    bits = pixfmt.RGB_FORMATS[out['pixFmt']][0] if 'pixFmt' in src else src['bitDepth']
    W, H = (70, 50) if FIT in work else (2 * w, 2 * h)
    return [lut3d.apply(p.reshape(H, W, 3), 16, *_lut(d, kind), bits, 'bgr', kw.get('strength', 1.0), (out or {}).get('dither')).tobytes() for p in _p16(name, frames)]


def _reference(name):
    if name not in _serial:
        w, h = CHAINS[name][:2]
        frames = _frames(name)
        _serial[name] = (frames,) + _serial_frames(_steps(name), frames, w, h, _source(name)[0])
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
def test_serial_frames_are_the_definition_of_the_16_bit_frames(name, dev):
    """genProcess + runFrames: every frame is lut3d.apply of the 16-bit frame the same list yields without the step.  (On the parent commit the step raises
    NotImplementedError: op "lut" is not part of the SR/DN hot path this engine implements -- this test and the stream tests below fail there.)"""
    _configure()
    frames, serial, nodes = _reference(name)
    assert nodes[-1] == dict(op='lut') and len(set(serial)) == 5
    for k, (g, d) in enumerate(zip(serial, _defined(name, frames))):
        assert g == d, '{} frame {}: {}'.format(name, k, _differ(g, d))


@pytest.mark.parametrize('mode', ['plain', 'reuse', 'views'])
@pytest.mark.parametrize('name', sorted(CHAINS))
def test_streams_equal_the_serial_frames(name, mode, dev):
    _configure()
    w, h = CHAINS[name][:2]
    frames, serial, nodes = _reference(name)
    for depth in (1, 2, 3):
        got, stream = _run_stream(_steps(name), w, h, frames, depth, mode)
        assert stream.edge == CHAINS[name][6] and stream.nodes == nodes
        for k, (g, w_) in enumerate(zip(got, serial)):
            assert g == w_, '{} {} ring depth {} frame {}: {}'.format(name, mode, depth, k, _differ(g, w_))
        if mode == 'reuse':
            assert stream.reuse['pixels_run'] < stream.reuse['pixels_planned']


def test_cube_file_and_still_image(tmp_path, dev):
    """A .cube file written here, behind an SR step on a still 16-bit image (an array source: the samples are in 'rgb' order), with and without alpha."""
    from moephoto_amd import procedure
    _configure()
    table = _lut(17, 'uniform')[0]
    path = tmp_path / 'look.cube'
    path.write_text(lut3d.formatCube(table, 'look'))
    parsed = lut3d.parseCube(path.read_text())
    assert (parsed[0] == table).all() and (parsed[1] == lut3d.uniform(17)).all()
    from moephoto_amd import imageProcess as ip, runSR
    from moephoto_amd.config import config
    images = {16: _codes(9, 16, 40 * 36 * 4).reshape(36, 40, 4), 8: _codes(9, 8, 40 * 36 * 4).reshape(36, 40, 4)}
    plain, _ = procedure.genProcess([dict(SR)], 16)
    sr = runSR.sr(runSR.getOpt(dict(SR)))
    for C in (3, 4):
        for bits, dither in ((16, None), (8, 'ordered')):
            process, nodes = procedure.genProcess([dict(SR), {'op': 'lut', 'file': str(path), 'strength': 0.5}, {'op': 'output', 'dither': dither or 'none'}], bits)
            assert [n['op'] for n in nodes] == ['SR', 'lut']
            im = np.ascontiguousarray(images[bits][:, :, :C])
            # the 16-bit frame the list yields without the step: an 8-bit image has no such list, its frame is the chain's own pieces put together
            p16 = procedure._samplesOnDevice(16)(sr(ip.toTorch(bits, config.dtype(), config.device())(im))).cpu().numpy().view(np.uint16)
            if bits == 16:
                assert (plain(im) == p16).all()
            got = process(im)
            assert got.shape == (72, 80, C) and got.dtype == (np.uint8 if bits == 8 else np.uint16) and p16.dtype == np.uint16
            want = lut3d.apply(np.ascontiguousarray(p16[:, :, :3]), 16, table, lut3d.uniform(17), bits, 'rgb', 0.5, dither)
            assert (got[:, :, :3] == want).all(), (C, bits)
            if C == 4:          # alpha passes around the step: its 16-bit code, at 8 bits that code's high byte
                assert (got[:, :, 3] == (p16[:, :, 3] if bits == 16 else p16[:, :, 3] >> 8)).all(), (C, bits)
    grey, _ = procedure.genProcess([dict(SR), {'op': 'lut', 'file': str(path)}], 16)
    with pytest.raises(ValueError, match='3 or 4 planes'):
        grey(im[:, :, :1])
