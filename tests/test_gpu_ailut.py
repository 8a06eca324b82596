"""The AiLUT generator net on the device (`pytest -m gpu`).  The comparator is the written definition (moephoto_amd/ailut.py, numpy float64).
The tolerance is not a constant: for each case e_ref = the largest absolute difference between a float32 torch-CPU forward of the same functional graph and the
definition, separately for table and vertices, and the device stays within 4 e_ref + 1e-7 (4: another summation order at the same precision; an fp16 path or a
dropped normalisation is three orders of magnitude outside).  Every test prints its figures before it asserts.

The chains: every frame is lut3d.apply(P16, 16, T, V, ..) byte for byte, P16 the frame the same list yields without the step and (T, V) fetched from the handle
behind that frame; (T, V) is within the tolerance of ailut.generate(ailut.thumbnail(P16)).  On the parent commit the step raises NotImplementedError: op "dehaze" is
not part of the SR/DN hot path this engine implements -- every chain, stream and still-image test here fails there (checked once).

Observed (one MI355X), device error / (4 e_ref + 1e-7), the largest over each group of cases: see profiles/ailut/parity.md."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

import ailut_util as au
import golden_defs as gd
from moephoto_amd import ailut, lut3d, pixfmt

pytestmark = pytest.mark.gpu
SIZES = ((1, 1), (3, 2), (17, 5), (256, 256), (140, 100), (300, 260), (523, 259))          # (w, h): tiny, the identity sampling, enlarging, shrinking and ragged
NETS = ((2, 1), (9, 3), (33, 3), (33, 5))                                                    # (d, ranks)
KINDS = ('noise', 'flat', 'ramp')
FORMS = ((16, 'bgr'), (8, 'rgb'), (16, 'rgb'), (8, 'bgr'))
SENTINEL = 0xA5
_params, _gens, _defs = {}, {}, {}


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _net(d, ranks):
    if (d, ranks) not in _params:
        sd = au.stateDict(100 + d + ranks, d, ranks)
        _params[(d, ranks)] = (sd, ailut.loadParams(sd))
    return _params[(d, ranks)]


def _handles(d, ranks, fresh=False):
    from moephoto_amd import imageProcess as ip
    if fresh:
        return ip._AilutHandle(_net(d, ranks)[1], 0), ip._LutHandle(lut3d.identity(d), lut3d.uniform(d), 0)
    if (d, ranks) not in _gens:
        _gens[(d, ranks)] = _handles(d, ranks, True)
    return _gens[(d, ranks)]


def _defined(im, bits, order, d, ranks, key=None):
    """(thumbnail, table, vertices, tolerance of the table, tolerance of the vertices): the definition and 4 e_ref + 1e-7 from a float32 torch-CPU forward."""
    if key is None or key not in _defs:
        sd, params = _net(d, ranks)
        thumb = ailut.thumbnail(im, bits, order)
        table, vertices = ailut.generate(thumb, params)
        _, t32, v32 = au.torchForward(im, bits, order, sd, torch.float32)
        got = (thumb, table, vertices, 4 * np.abs(t32 - table).max() + 1e-7, 4 * np.abs(v32 - vertices).max() + 1e-7)
        if key is None:
            return got
        _defs[key] = got
    return _defs[key]


def _run(im, bits, order, handles, dev, lead=0):
    """moe_ailut_run on a frame `lead` samples behind a 16-byte boundary, between sentinel bytes; the source and the sentinels must come back as they went in, the
    handle's guard bands and parameters intact.  Returns the fetched (table, vertices)."""
    from moephoto_amd import _lib, imageProcess as ip
    gen, lut = handles
    src = im.view(np.uint8).reshape(-1)
    a = lead * (bits // 8)
    s_buf = torch.full((a + src.size + 32,), SENTINEL, dtype=torch.uint8, device=dev)
    assert s_buf.data_ptr() % 16 == 0
    s_buf[a:a + src.size] = torch.from_numpy(src.copy()).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().moe_ailut_run(gen._h, s_buf.data_ptr() + a, bits, im.shape[0], im.shape[1], pixfmt.ORDERS[order], lut._h, stream))
    table, vertices = ip.readLut3d(lut, stream)
    back = s_buf.cpu().numpy()
    assert (back[:a] == SENTINEL).all() and (back[a + src.size:] == SENTINEL).all() and (back[a:a + src.size] == src).all(), 'the source or a sentinel around it was written'
    assert gen.guards(stream) == 0, 'a guard band between the generator\'s buffers, or a parameter, was written'
    return table, vertices


@pytest.mark.parametrize('wh', SIZES)
@pytest.mark.parametrize('net', NETS)
def test_generator_is_the_definition(net, wh, dev):
    """Three cases a size and net: each input kind once, the sample depths and orders shifted from size to size (17 x 5 sees all four forms on noise as well)."""
    (d, ranks), (w, h) = net, wh
    i = SIZES.index(wh) + NETS.index(net)
    cases = [(KINDS[j], FORMS[(i + j) % 4]) for j in range(3)] + ([('noise', f) for f in FORMS] if wh == (17, 5) else [])
    for n, (kind, (bits, order)) in enumerate(cases):
        im = au.frame(kind, w, h, bits, seed=i + n)
        _, table, vertices, tol_t, tol_v = _defined(im, bits, order, d, ranks)
        got_t, got_v = _run(im, bits, order, _handles(d, ranks), dev, lead=n % 2)
        err_t, err_v = np.abs(got_t - table).max(), np.abs(got_v - vertices).max()
        print('ailut parity d {} ranks {} {}x{} {} u{} {}: table {:.3e} of {:.3e} ({:.3f}), vertices {:.3e} of {:.3e} ({:.3f})'.format(
            d, ranks, w, h, kind, bits, order, err_t, tol_t, err_t / tol_t, err_v, tol_v, err_v / tol_v))
        assert np.isfinite(got_t).all() and np.isfinite(got_v).all()
        assert err_t <= tol_t and err_v <= tol_v, (kind, bits, order, err_t, tol_t, err_v, tol_v)
        # the precondition of lut3d.hip's search: the fetched vertices never decrease (and start at 0)
        assert (got_v[:, 0] == 0).all() and (np.diff(got_v, axis=1) >= 0).all()


@pytest.mark.parametrize('wh', SIZES)
def test_thumbnail_alone(wh, dev):
    """moe_ailut_thumbnail against ailut.thumbnail within 2^-22: the interpolation weights are exact in fp32, what remains is three roundings."""
    from moephoto_amd import _lib
    w, h = wh
    for bits, order in FORMS:
        im = au.frame('noise', w, h, bits, seed=w * h + bits)
        want = ailut.thumbnail(im, bits, order)
        src = torch.from_numpy(im.view(np.uint8).reshape(-1).copy()).to(dev)
        n = 3 * 256 * 256
        out = torch.full((n + 16,), float('nan'), dtype=torch.float32, device=dev)
        out.view(torch.uint8)[:] = SENTINEL
        _lib.check(_lib.lib().moe_ailut_thumbnail(src.data_ptr(), bits, h, w, pixfmt.ORDERS[order], out.data_ptr() + 32, 0, torch.cuda.current_stream().cuda_stream))
        raw = out.cpu().numpy()
        assert (raw.view(np.uint8)[:32] == SENTINEL).all() and (raw.view(np.uint8)[32 + 4 * n:] == SENTINEL).all(), 'a sentinel around the thumbnail was overwritten'
        assert (src.cpu().numpy() == im.view(np.uint8).reshape(-1)).all()
        err = np.abs(raw[8:8 + n].reshape(3, 256, 256).astype(np.float64) - want).max()
        print('ailut thumbnail {}x{} u{} {}: {:.3e} of {:.3e}'.format(w, h, bits, order, err, 2.0 ** -22))
        assert err <= 2.0 ** -22, (wh, bits, order, err)
        if wh == (256, 256) and bits == 16:
            assert err == 0          # the identity sampling of exact samples


def test_two_runs_are_bit_equal_and_nothing_of_an_earlier_frame_survives(dev):
    d, ranks = 33, 3
    a, b = au.frame('noise', 300, 260, 16, seed=1), au.frame('ramp', 140, 100, 8, seed=2)
    h = _handles(d, ranks)
    first = _run(a, 16, 'bgr', h, dev)
    second = _run(a, 16, 'bgr', h, dev)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    other = _run(b, 8, 'rgb', h, dev)
    assert other[0].tobytes() != first[0].tobytes()
    again, fresh = _run(a, 16, 'bgr', h, dev), _run(a, 16, 'bgr', _handles(d, ranks, True), dev)
    assert again[0].tobytes() == fresh[0].tobytes() == first[0].tobytes() and again[1].tobytes() == fresh[1].tobytes() == first[1].tobytes()


def test_ailut_wrapper(dev):
    """imageProcess.ailut: the generator and one moe_lut3d_run; the frame is lut3d.apply with the table fetched behind it."""
    from moephoto_amd import imageProcess as ip
    w, h = 40, 36
    params = _net(9, 3)[1]
    for srcBits, bits, kw in ((16, 16, {}), (8, 8, dict(order='rgb', strength=0.6, dither='ordered')), (16, 8, dict(dither='round'))):
        im = au.frame('noise', w, h, srcBits, seed=4)
        raw = torch.from_numpy(im.view(np.uint8).reshape(-1).copy()).to(dev)
        out = torch.zeros((3 * w * h * bits // 8,), dtype=torch.uint8, device=dev)
        seen = []
        f = ip.ailut(params, srcBits, bits, tableOut=lambda t, v: seen.append((t, v)), **kw)
        assert f(raw, out, h, w) is out
        table, vertices = f.read(dev)
        assert len(seen) == 1 and (seen[0][0] == table).all() and (seen[0][1] == vertices).all()
        assert out.cpu().numpy().tobytes() == lut3d.apply(im, srcBits, table, vertices, bits, **dict(dict(order='bgr'), **kw)).tobytes(), (srcBits, bits)
        _, want_t, want_v, tol_t, tol_v = _defined(im, srcBits, kw.get('order', 'bgr'), 9, 3)
        assert np.abs(table - want_t).max() <= tol_t and np.abs(vertices - want_v).max() <= tol_v
        assert f.generator(dev).guards() == 0 and f.table(dev).info()['d'] == 9
        with pytest.raises(ValueError):
            f(raw[:-2], out, h, w)


def test_run_refuses_a_table_handle_of_another_size(dev):
    from moephoto_amd import _lib, imageProcess as ip
    gen, _ = _handles(9, 3)
    other = ip._LutHandle(lut3d.identity(5), lut3d.uniform(5), 0)
    src = torch.zeros((48,), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    assert L.moe_ailut_run(gen._h, src.data_ptr(), 8, 4, 4, 0, other._h, None) == _lib.EINVAL and b'd = 5' in L.moe_last_error()
    assert L.moe_ailut_run(gen._h, src.data_ptr() + 1, 16, 2, 4, 0, _handles(9, 3)[1]._h, None) == _lib.EINVAL and b'2-byte aligned' in L.moe_last_error()
    assert L.moe_ailut_stage(gen._h, 8, src.data_ptr(), 8, 4, 4, 0, _handles(9, 3)[1]._h, None) == _lib.EINVAL and b'stage 8' in L.moe_last_error()


# ---- the chains -------------------------------------------------------------------------------------------------------------------------------
MODEL = 'AiLUT_sRGB_3'
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}
DN = {'op': 'DN', 'model': 'lite5', 'strength': 0.6}
BGR24, BGR48, YUV10 = {'op': 'buffer', 'bitDepth': 8}, {'op': 'buffer', 'bitDepth': 16}, {'op': 'buffer', 'pixFmt': 'yuv420p10le'}
OUT48 = {'op': 'output', 'pixFmt': 'bgr48le'}
# name -> (width, height, source step, compute steps in front of the step, the step's keys, output step or None)
CHAINS = {
    '48x32_bgr24_sr': (48, 32, BGR24, [SR], {}, None),
    '140x100_bgr24_sr': (140, 100, BGR24, [SR], {'strength': 0.6}, None),
    '48x32_bgr48le_sr': (48, 32, BGR48, [SR], {}, None),
    '140x100_bgr48le_sr_dn': (140, 100, BGR48, [SR, DN], {}, None),
    '48x32_bgr48le_sr_luma': (48, 32, BGR48, [dict(SR, chroma='bicubic')], {'strength': 0.25}, None),
    '140x100_bgr48le_sr_luma': (140, 100, BGR48, [dict(SR, chroma='bicubic')], {}, None),
    '48x32_yuv420p10le_sr': (48, 32, YUV10, [SR], {}, OUT48),
    '140x100_yuv420p10le_sr_dn': (140, 100, YUV10, [SR, DN], {}, OUT48),
    '48x32_yuv420p10le_sr_bicubic': (48, 32, dict(YUV10, chroma='bicubic'), [SR], {}, OUT48),          # (a planar chain's luma-only form: the key sits on the source step)
    '140x100_yuv420p10le_sr_bicubic': (140, 100, dict(YUV10, chroma='bicubic'), [SR], {'strength': 0.6}, OUT48),
}
CHAIN_NET = (33, 3)
_serial, _root = {}, {}


def _configure(tmp_path_factory):
    """The zoo's models beside a generator checkpoint made here, under one modelRoot."""
    from moephoto_amd.config import config
    if 'dir' not in _root:
        root = tmp_path_factory.mktemp('ailut_zoo')
        os.makedirs(os.path.join(str(root), 'model'))
        for name in os.listdir(os.path.join(gd.ZOO, 'model')):
            os.symlink(os.path.join(gd.ZOO, 'model', name), os.path.join(str(root), 'model', name))
        au.writeCheckpoint(root, MODEL, _net(*CHAIN_NET)[0])
        _root['dir'] = str(root)
    config.modelRoot, config.deviceId, config.fp16 = _root['dir'], 0, True
    config.crop_sr = config.crop_dn = config.crop_dns = 48
    config.ensembleSR = 0


def _source(name):
    w, h, src = CHAINS[name][:3]
    if 'pixFmt' in src:
        return pixfmt.frameBytes(src['pixFmt'], w, h), np.uint16, src['pixFmt']
    return 3 * w * h * src['bitDepth'] // 8, (np.uint8 if src['bitDepth'] == 8 else np.uint16), None


GAINS = ((0.15, 0.2, 1.0), (1.0, 0.2, 0.1), (0.12, 0.1, 0.1), (1.0, 0.95, 0.9), (0.2, 1.0, 0.3), (0.6, 0.3, 0.7))          # (b, g, r): red-heavy, blue-heavy, dark, bright, ..


def _frames(name, seed=90):
    """Six frames of strongly different colour: noise under per-channel gains (a planar source: the luma's gain and two chroma levels)."""
    w, h = CHAINS[name][:2]
    nbytes, dt, fmt = _source(name)
    frames = []
    for k, gain in enumerate(GAINS):
        rng = np.random.default_rng(seed + k)
        if fmt:
            top = 1 << pixfmt.FORMATS[fmt]
            y = (rng.integers(0, top, w * h) * gain[1]).astype(dt)
            c = [np.clip(top // 2 + (g - 0.5) * top * 0.8 + rng.integers(-8, 9, (w // 2) * (h // 2)), 0, top - 1).astype(dt) for g in (gain[0], gain[2])]
            a = np.concatenate([y] + c)
        else:
            top = 1 << (8 * np.dtype(dt).itemsize)
            a = (rng.integers(0, top, (h, w, 3)) * np.array(gain)).astype(dt).reshape(-1)
        assert a.nbytes == nbytes
        frames.append(a.tobytes())
    return frames


def _steps(name, step=True, **kw):
    _, _, src, work, keys, out = CHAINS[name]
    return [dict(src)] + [dict(s) for s in work] + ([dict({'op': 'dehaze', 'model': MODEL}, **dict(keys, **kw))] if step else []) + ([dict(out)] if out else [])


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
    """The 16-bit frames the chain's list yields without the step.  A bgr24 chain (plain SR) has no step list that writes 16-bit samples of 8-bit frames: its frames
    are the chain's own pieces put together, toNumPy and toTorch at 8 bits, the SR step, the 16-bit quantiser."""
    from moephoto_amd import imageProcess as ip, procedure, runSR
    from moephoto_amd.config import config
    w, h, src, work = CHAINS[name][:4]
    nbytes, _, fmt = _source(name)
    if fmt is None and src['bitDepth'] == 8:
        assert work == [SR]
        o = runSR.getOpt(dict(SR))
        return [procedure._samplesOnDevice(16)(runSR.sr(o)(ip.toTorch(8, config.dtype(), config.device())(ip.toNumPy(8)((f, h, w))))).cpu().numpy().view(np.uint16).reshape(2 * h, 2 * w, 3) for f in frames]
    return [np.frombuffer(f, np.uint16).reshape(2 * h, 2 * w, 3) for f in _serial_frames(_steps(name, False), frames, w, h, nbytes)[0]]


def _reference(name):
    """(frames, genProcess + runFrames' frames, nodes, the tables fetched behind each frame, the 16-bit frames without the step): computed once, shared by the modes."""
    if name not in _serial:
        w, h = CHAINS[name][:2]
        frames, tables = _frames(name), []
        serial, nodes = _serial_frames(_steps(name, tableOut=lambda t, v: tables.append((t, v))), frames, w, h, _source(name)[0])
        _serial[name] = (frames, serial, nodes, tables, _p16(name, frames))
    return _serial[name]


@pytest.mark.parametrize('name', sorted(CHAINS))
def test_serial_frames_are_the_definition_of_the_16_bit_frames(name, dev, tmp_path_factory):
    _configure(tmp_path_factory)
    frames, serial, nodes, tables, p16 = _reference(name)
    src, keys = CHAINS[name][2], CHAINS[name][4]
    bits = 16 if 'pixFmt' in src else src['bitDepth']
    assert nodes[-1] == dict(op='dehaze') and len(set(serial)) == len(frames) == len(tables) == 6
    d = CHAIN_NET[0]
    for k, (g, p, (T, V)) in enumerate(zip(serial, p16, tables)):
        want = lut3d.apply(p, 16, T, V, bits, 'bgr', keys.get('strength', 1.0), None).tobytes()
        assert g == want, '{} frame {}: {}'.format(name, k, _differ(g, want))
        _, table, vertices, tol_t, tol_v = _defined(p, 16, 'bgr', *CHAIN_NET, key=(name, k))
        err_t, err_v = np.abs(T - table).max(), np.abs(V - vertices).max()
        print('ailut chain {} frame {}: table {:.3e} of {:.3e}, vertices {:.3e} of {:.3e}'.format(name, k, err_t, tol_t, err_v, tol_v))
        assert T.shape == (3, d, d, d) and err_t <= tol_t and err_v <= tol_v, (name, k, err_t, tol_t, err_v, tol_v)


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


@pytest.mark.parametrize('mode', ['plain', 'reuse', 'views'])
@pytest.mark.parametrize('name', sorted(CHAINS))
def test_streams_equal_the_serial_frames(name, mode, dev, tmp_path_factory):
    _configure(tmp_path_factory)
    w, h = CHAINS[name][:2]
    frames, serial, nodes, tables, p16 = _reference(name)
    # on the definition: consecutive frames' tables differ by more than 100 times the tolerance, so a frame rendered with its neighbour's table cannot pass
    for k in range(len(frames) - 1):
        a, b = _defined(p16[k], 16, 'bgr', *CHAIN_NET, key=(name, k)), _defined(p16[k + 1], 16, 'bgr', *CHAIN_NET, key=(name, k + 1))
        assert np.abs(a[1] - b[1]).max() > 100 * max(a[3], b[3]), (name, k, np.abs(a[1] - b[1]).max(), a[3], b[3])
    for depth in (1, 2, 3):
        got, stream = _run_stream(_steps(name), w, h, frames, depth, mode)
        assert stream.edge.endswith('+ailut') and '+lut' not in stream.edge and stream.nodes == nodes
        for k, (g, w_) in enumerate(zip(got, serial)):
            assert g == w_, '{} {} ring depth {} frame {}: {}'.format(name, mode, depth, k, _differ(g, w_))


def test_still_image(dev, tmp_path_factory):
    """Behind an SR step on a still image (an array source: the samples are in 'rgb' order), 16 and 8 bits, with and without alpha."""
    from moephoto_amd import imageProcess as ip, procedure, runSR
    from moephoto_amd.config import config
    _configure(tmp_path_factory)
    rng = np.random.default_rng(9)
    images = {16: rng.integers(0, 65536, (36, 40, 4)).astype(np.uint16), 8: rng.integers(0, 256, (36, 40, 4)).astype(np.uint8)}
    sr = runSR.sr(runSR.getOpt(dict(SR)))
    for C in (3, 4):
        for bits, dither in ((16, None), (8, 'ordered')):
            tables = []
            process, nodes = procedure.genProcess([dict(SR), {'op': 'dehaze', 'model': MODEL, 'strength': 0.5, 'tableOut': lambda t, v: tables.append((t, v))},
                                                   {'op': 'output', 'dither': dither or 'none'}], bits)
            assert [n['op'] for n in nodes] == ['SR', 'dehaze']
            im = np.ascontiguousarray(images[bits][:, :, :C])
            p16 = procedure._samplesOnDevice(16)(sr(ip.toTorch(bits, config.dtype(), config.device())(im))).cpu().numpy().view(np.uint16)
            got = process(im)
            assert got.shape == (72, 80, C) and got.dtype == (np.uint8 if bits == 8 else np.uint16) and len(tables) == 1
            rgb = np.ascontiguousarray(p16[:, :, :3])
            assert (got[:, :, :3] == lut3d.apply(rgb, 16, tables[0][0], tables[0][1], bits, 'rgb', 0.5, dither)).all(), (C, bits)
            _, table, vertices, tol_t, tol_v = _defined(rgb, 16, 'rgb', *CHAIN_NET)
            assert np.abs(tables[0][0] - table).max() <= tol_t and np.abs(tables[0][1] - vertices).max() <= tol_v
            if C == 4:          # alpha passes around the step: its 16-bit code, at 8 bits that code's high byte
                assert (got[:, :, 3] == (p16[:, :, 3] if bits == 16 else p16[:, :, 3] >> 8)).all(), (C, bits)
