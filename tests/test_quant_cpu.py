"""Rounding and ordered dither in the quantising edges without a device: the numpy definition (moephoto_amd.quant) -- the Bayer matrix, mode 'none'
against today's three quantisers, the fixed points, the ramp --, what the builders refuse before a model is loaded, and the MOE_Q_* flag checks of the thirteen entry
points."""
import ctypes
import os
import re

import numpy as np
import pytest

from moephoto_amd import _lib, luma, pixfmt, procedure, quant
from moephoto_amd import imageProcess as ip
from oracle import imageio as oio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DITHERS = ('round', 'ordered')


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------
def test_bayer8_is_a_permutation_the_recursion_and_the_closed_form():
    b = quant.bayer8()
    assert b.shape == (8, 8) and sorted(b.ravel().tolist()) == list(range(64))
    b2 = np.array([[0, 2], [3, 1]])
    b4 = np.block([[4 * b2, 4 * b2 + 2], [4 * b2 + 3, 4 * b2 + 1]])
    assert np.array_equal(b, np.block([[4 * b4, 4 * b4 + 2], [4 * b4 + 3, 4 * b4 + 1]]))
    assert b[0].tolist() == [0, 32, 8, 40, 2, 34, 10, 42]
    yy, xx = np.mgrid[0:8, 0:8]
    assert np.array_equal(quant.bayer8Closed(yy, xx), b)
    assert np.array_equal(quant.bayer8Closed(yy + 8, xx + 24), b)          # (x & 7, y & 7)
    t = quant.threshold('ordered', 19, 21)
    assert t.min() == 1 and t.max() == 127 and (t % 2 == 1).all() and np.array_equal(t[8:16, 8:16], 2 * b + 1) and np.array_equal(t[16:19, 16:21], (2 * b + 1)[:3, :5])
    assert (quant.threshold('round', 3, 5) == 64).all()
    with pytest.raises(ValueError, match='dither'):
        quant.threshold('floyd', 4, 4)
    with pytest.raises(ValueError):
        quant.threshold('none', 4, 4)


@pytest.mark.parametrize('dtype', [np.float32, np.float16])
def test_none_is_todays_quantisers(dtype):
    rng = np.random.default_rng(11)
    x = (rng.random((3, 37, 53), dtype=np.float32) * 1.3 - 0.15).astype(dtype)
    x[0, 0, :4] = [np.nan, np.inf, -np.inf, 1.0]
    for bits in (8, 16):
        got = quant.quantiseHWC(x, bits)
        with np.errstate(invalid='ignore'):
            want = oio.to_output(np.nan_to_num(oio.to_hwc(x), nan=0.0, posinf=4.0, neginf=-4.0), bits)
        assert np.array_equal(got.astype(np.int64), want.astype(np.int64) & 0xffff)
        assert np.array_equal(got, luma.quantise(x.astype(np.float32), bits).transpose(1, 2, 0))
    Y, C = luma.lumaSplit(x, 'bt709', 'rgb')
    for bits in (8, 16):
        assert np.array_equal(quant.quantiseHWC(luma.lumaMerge(Y, C), bits), luma.lumaMerge(Y, C, bits=bits))
    y, c = x[:1, :36, :52], x[1:, :18, :26]
    for fmt, D in pixfmt.FORMATS.items():
        dt = np.uint8 if D == 8 else np.dtype('<u2')
        assert quant.quantise(y, D).astype(dt).tobytes() + quant.quantise(c, D).astype(dt).tobytes() == pixfmt.fromPlanes(y, c, fmt)
    with pytest.raises(ValueError, match='unit'):
        quant.quantise(x, 8, 'none', unit=True)
    with pytest.raises(ValueError, match='dither'):
        quant.quantise(x, 8, 'bayer')
    with pytest.raises(ValueError, match='dtype'):
        quant.quantise(x.astype(np.float64), 8)


def test_fixed_points():
    codes = np.arange(256)
    at = lambda v: np.broadcast_to(v[:, None, None], (len(v), 8, 8)).copy()          # every code at every threshold of the matrix
    v32 = codes.astype(np.float32) / np.float32(255)
    for mode in DITHERS:
        assert np.array_equal(quant.quantise(at(v32), 8, mode, unit=True), at(codes))
    v16 = v32.astype(np.float16)          # what an fp16 canvas holds of code / 255
    assert np.array_equal(quant.quantise(at(v16), 8, 'round', unit=True), at(codes))
    assert (quant.quantise(at(v16), 8, 'none')[:, 0, 0] != codes).sum() == 15          # today's writer moves 15 of the 256 exact codes under fp16
    c16 = np.arange(65536)
    v = c16.astype(np.float32) / np.float32(65536)
    for mode in quant.MODES:
        assert np.array_equal(quant.quantise(at(v), 16, mode), at(c16))


def test_ramp_bands_less():
    """0.2 .. 0.3 over the 65536 pixels of a 256 x 256 image in raster order; the worst 8 x 8 block-mean error in codes of / 255 (0.446 / 0.147 / 0.028 as measured when the
    feature was specified)."""
    ramp = np.linspace(0.2, 0.3, 65536).reshape(256, 256).astype(np.float32)
    worst, mean = {}, {}
    for mode in quant.MODES:
        err = quant.quantise(ramp, 8, mode, unit=mode != 'none').astype(np.float64) - ramp.astype(np.float64) * 255
        worst[mode], mean[mode] = np.abs(err.reshape(32, 8, 32, 8).mean((1, 3))).max(), err.mean()
    print(worst, mean)
    assert worst['none'] >= 0.4 and worst['round'] <= 0.2 and worst['ordered'] <= 1 / 16
    assert abs(mean['ordered']) <= 0.01


@pytest.mark.parametrize('fmt', ['yuv420p', 'yuv420p10le'])
def test_yuv_round_is_todays_frame(fmt):
    rng = np.random.default_rng(5)
    for H, W in ((33, 47), (32, 48), (1, 1)):
        a = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
        a[0, 0] = (0, 0, 0)
        a[-1, -1] = (65535, 65535, 65535)
        for matrix in pixfmt.MATRICES:
            for order in pixfmt.ORDERS:
                want = pixfmt.fromSamples16(a, fmt, matrix, order)
                assert quant.yuvFromSamples16(a, fmt, matrix, order, 'round') == want == quant.yuvFromSamples16(a, fmt, matrix, order, 'none')
        got = quant.yuvFromSamples16(a, fmt, mode='ordered')
        assert len(got) == len(want)
        D = pixfmt.FORMATS[fmt]
        d = np.frombuffer(got, np.uint8 if D == 8 else '<u2').astype(np.int64) - np.frombuffer(pixfmt.fromSamples16(a, fmt), np.uint8 if D == 8 else '<u2')
        assert np.abs(d).max() <= 1 and (H * W == 1 or np.abs(d).max() == 1)          # a threshold moves a sample by one code at most
    with pytest.raises(ValueError, match='dither'):
        quant.yuvFromSamples16(a, fmt, mode='x')


def test_flags_helper():
    R, O, U = quant.Q_ROUND, quant.Q_ORDERED, quant.Q_UNIT
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    assert dict((n, int(v, 16)) for n, v in re.findall(r'#define (MOE_Q_[A-Z]+) (0x[0-9a-f]+)', hdr)) == dict(MOE_Q_ROUND=R, MOE_Q_ORDERED=O, MOE_Q_UNIT=U) == \
        dict(MOE_Q_ROUND=0x100, MOE_Q_ORDERED=0x200, MOE_Q_UNIT=0x400)
    assert quant.flags(None, 8, 'rgb') == quant.flags('none', 8, 'rgb') == 0
    assert quant.flags('round', 8, 'rgb') == R | U and quant.flags('ordered', 8, 'rgb') == O | U
    assert quant.flags('round', 16, 'rgb') == R and quant.flags('ordered', 16, 'rgb') == O
    for D in (8, 10, 12, 16):
        assert quant.flags('ordered', D, 'planes') == O and quant.flags('round', D, 'yuv') == R
    with pytest.raises(ValueError, match='dither'):
        quant.flags('bayer', 8, 'rgb')
    with pytest.raises(ValueError, match="'dither'"):
        ip.ditherFlags('doCropOut', 'bayer', 8, 'rgb')
    with pytest.raises(ValueError, match="'dither'"):
        ip.toOutput(8, dither='bayer')
    with pytest.raises(ValueError, match="'dither'"):
        ip.toPlanes(10, dither='bayer')
    with pytest.raises(ValueError, match="'dither'"):
        ip.toYuv('yuv420p', dither='bayer')


# ---- the builders -----------------------------------------------------------------------------------------------------------------------------
SR = {'op': 'SR', 'model': 'a', 'scale': 2}
BAD_OUTPUT = [({'dither': 'bayer'}, "'dither'"), ({'dither': None}, "'dither'"), ({'dither': True}, "'dither'"), ({'dither': 'Ordered'}, "'dither'")]
BAD_FIT = [{'dither': 'ordered', 'width': 64, 'height': 48}, {'dither': 'round', 'width': 64, 'height': 48, 'fit': 'bilinear'}, {'dither': 'round', 'width': 32, 'height': 24, 'fit': 'nearest'}]


def _no_models(monkeypatch):
    def no_model(*a, **k):
        raise AssertionError('a model was loaded before the step list was checked')
    monkeypatch.setattr(ip, 'initModel', no_model)
    monkeypatch.setattr(procedure.runSR, 'initModel', no_model)
    monkeypatch.setattr(procedure.runDN, 'initModel', no_model)


@pytest.mark.parametrize('out,key', BAD_OUTPUT, ids=lambda v: None if isinstance(v, str) else repr(v['dither']))
def test_builders_refuse_an_unknown_value_before_a_model_is_loaded(out, key, monkeypatch):
    _no_models(monkeypatch)
    step = dict(out, op='output')
    for source in ({'op': 'file'}, {'op': 'buffer', 'bitDepth': 8}, {'op': 'buffer', 'pixFmt': 'yuv420p'}, {'op': 'buffer', 'pixFmt': 'yuv420p10le', 'chroma': 'bicubic'}):
        with pytest.raises(ValueError, match=key):
            procedure.genProcess([source, dict(SR), dict(step)])
        if source['op'] == 'buffer':
            with pytest.raises(ValueError, match=key):
                procedure.genFrameStream([source, dict(SR), dict(step)], 64, 48)
    with pytest.raises(ValueError, match=key):
        procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 8}, dict(SR), dict(step, pixFmt='yuv420p')], 64, 48, reuse=True, views=True)


@pytest.mark.parametrize('out', BAD_FIT, ids=lambda v: '-'.join('{}={}'.format(k, v[k]) for k in sorted(v)))
def test_builders_refuse_dither_beside_a_fitted_size(out, monkeypatch):
    _no_models(monkeypatch)
    steps = [{'op': 'buffer', 'pixFmt': 'yuv420p'}, dict(SR), dict(out, op='output')]
    with pytest.raises(ValueError, match="'dither'"):
        procedure.genProcess(steps)
    with pytest.raises(ValueError, match="'dither'"):
        procedure.genFrameStream(steps, 64, 48)
    # the keys on two output steps of one list are refused as well
    split = [{'op': 'buffer', 'pixFmt': 'yuv420p'}, dict(SR), {'op': 'output', 'dither': 'ordered'}, {'op': 'output', 'width': 64, 'height': 48}]
    with pytest.raises(ValueError, match="'dither'"):
        procedure.genFrameStream(split, 64, 48)


def test_output_dither_resolves():
    assert procedure._outputDither([{'op': 'file'}, dict(SR)]) is None
    assert procedure._outputDither([{'op': 'file'}, dict(SR), {'op': 'output', 'dither': 'none'}]) is None
    assert procedure._outputDither([{'op': 'buffer', 'pixFmt': 'yuv420p'}, {'op': 'output', 'dither': 'none', 'width': 64, 'height': 48}]) is None          # (the default, spelled out)
    for mode in DITHERS:
        assert procedure._outputDither([{'op': 'buffer', 'bitDepth': 8}, {'op': 'output', 'dither': mode, 'pixFmt': 'yuv420p'}]) == mode
    assert 'resize_kernel_codes' in procedure._outputDither.__doc__          # (the luma-only planar chain: the key governs Y' alone)


# ---- the entry points -------------------------------------------------------------------------------------------------------------------------
def test_exports_and_version_are_unchanged():
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    declared = set(re.findall(r'\b(moe_[a-z0-9_]+)\s*\(', hdr))
    assert sorted(_lib.EXPORTS) == sorted(declared) and not any('dither' in n or 'quant' in n for n in declared)
    assert _lib.lib().moe_abi_version() == _lib.ABI_VERSION == 4
    from moephoto_amd import build
    assert 'quant.h' in build.HEADERS


def test_flagged_calls_are_refused_without_a_device():
    L = _lib.lib()
    err = lambda: L.moe_last_error()
    R, O, U = quant.Q_ROUND, quant.Q_ORDERED, quant.Q_UNIT
    rgb = ip.TilePlan((3, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    rgb1 = ip.TilePlan((3, 100, 140), 1 << 40, 1e-3, 5, 1, 8, 48)
    grey = ip.TilePlan((1, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    F32, U8, U16 = _lib.F32, _lib.U8, _lib.U16
    h = ctypes.c_void_p()
    _lib.check(L.moe_net_create(_lib.ARCH_NET2X, 2, ctypes.byref(h)))
    try:
        # name -> (call(bits or depth), the value of a valid unflagged argument, whether the entry point has a canvas form at bits = 0)
        float_edges = {
            'moe_to_output': (lambda b: L.moe_to_output(p, F32, 2, 2, 1, b, p, U8, 0, None), 8, False),
            'moe_stitch_out': (lambda b: L.moe_stitch_out(rgb._h, 0, p, None, 3, F32, b, p, U8, None), 8, False),
            'moe_run_plan_out': (lambda b: L.moe_run_plan_out(h, rgb._h, p, F32, 14000, 140, 1, F32, b, p, U8, 0, None), 8, False),
            'moe_stitch_mix': (lambda b: L.moe_stitch_mix(rgb1._h, 0, p, None, 3, p, F32, 14000, 140, 1, None, 0, 0, 0.6, b, p, U8 if b & 0xff else F32, None), 8, True),
            'moe_run_plan_filter': (lambda b: L.moe_run_plan_filter(h, rgb1._h, p, F32, 14000, 140, 1, None, 0, 0, 0.6, b, p, U8 if b & 0xff else F32, 0, None), 8, True),
            'moe_luma_merge': (lambda b: L.moe_luma_merge(p, F32, p, 3, 2, 2, 0, 1, b, p, U8 if b & 0xff else F32, 0, None), 8, True),
            'moe_stitch_luma': (lambda b: L.moe_stitch_luma(grey._h, 0, p, None, 1, F32, p, 0, 1, b, p, U8 if b & 0xff else F32, None), 8, True),
            'moe_run_plan_luma': (lambda b: L.moe_run_plan_luma(h, grey._h, p, F32, 14000, 140, 1, p, 0, 1, b, p, U8 if b & 0xff else F32, 0, None), 8, True),
            'moe_stitch_planes': (lambda d: L.moe_stitch_planes(grey._h, 0, p, None, 1, F32, d, p, None), 10, False),
            'moe_run_plan_planes': (lambda d: L.moe_run_plan_planes(h, grey._h, p, F32, 14000, 140, 1, F32, d, p, 0, None), 10, False),
        }
        yuv_edges = {
            'moe_stitch_yuv': lambda d: L.moe_stitch_yuv(rgb._h, 0, p, None, F32, d, 0, 0, p, None),
            'moe_run_plan_yuv': lambda d: L.moe_run_plan_yuv(h, rgb._h, p, F32, 14000, 140, 1, F32, d, 0, 0, p, 0, None),
            'moe_to_yuv': lambda d: L.moe_to_yuv(p, F32, 2, 2, d, 0, 0, p, 0, None),
        }
        for name, (call, low, canvas) in float_edges.items():
            who = name.encode()
            assert call(low | R | O) == _lib.EINVAL and who in err() and b'both set' in err(), name
            assert call(low | R | O | U) == _lib.EINVAL and b'both set' in err(), name
            assert call(low | U) == _lib.EINVAL and who in err() and b'MOE_Q_UNIT without' in err(), name
            for f in (R, O, R | U, O | U):
                assert call(0 | f) == _lib.EINVAL and who in err() and b'beside bits = 0' in err(), (name, f)
            for f in (0x800, 0x1000, 0x10000, 1 << 30):          # any other high bit: the unknown bits / depth it always was
                assert call(low | f) == _lib.EINVAL and who in err() and b'MOE_Q' not in err(), (name, f)
                assert call(low | f | R) == _lib.EINVAL and b'MOE_Q' not in err(), (name, f)
            assert call(-low) == _lib.EINVAL and call(3 | R) == _lib.EINVAL if name != 'moe_to_output' else call(-low) == _lib.EINVAL          # (the low byte keeps its checks)
            if canvas:          # the unflagged canvas form gets past the flag checks: a scale-1 / finalisation / launch matter from here on, never MOE_Q
                call(0)
                assert b'MOE_Q' not in err(), name
        for name, call in yuv_edges.items():
            who = name.encode()
            assert call(8 | R | O) == _lib.EINVAL and who in err() and b'both set' in err(), name
            assert call(8 | U) == _lib.EINVAL and b'MOE_Q_UNIT without' in err(), name
            for f in (R | U, O | U):
                assert call(10 | f) == _lib.EINVAL and who in err() and b"MOE_Q_UNIT does not apply to the Y'CbCr edge" in err(), (name, f)
            for f in (R, O):
                assert call(0 | f) == _lib.EINVAL and b'beside bits = 0' in err(), (name, f)
                assert call(9 | f) == _lib.EINVAL and b'depth 9' in err(), (name, f)
            assert call(8 | 0x800) == _lib.EINVAL and b'depth' in err() and b'MOE_Q' not in err(), name
        # a flagged call that is otherwise complete gets past every argument check: the two run_plan forms reach the unfinalised net
        assert float_edges['moe_run_plan_out'][0](8 | O | U) == _lib.ESTATE and b'not finalized' in err()
        assert float_edges['moe_run_plan_planes'][0](10 | R) == _lib.ESTATE and yuv_edges['moe_run_plan_yuv'](8 | O) == _lib.ESTATE
        # the integer polyphase kernels are out of scope: such values stay unknown depths
        assert L.moe_chroma_resample(p, 8 | R, 2, 2, p, 8, 2, 1, p, p, p, p, 0, None) == _lib.EINVAL and b'depth' in err()
        out = ctypes.c_void_p()
        assert L.moe_fit_create(1, 8, 2, 2, 8 | O, 2, 2, 1, p, p, 1, p, p, 0, ctypes.byref(out)) == _lib.EINVAL and b'depth' in err()
    finally:
        L.moe_net_destroy(h)


def test_wrappers_refuse_dither_on_a_canvas_form():
    import torch
    x = torch.zeros((1, 4, 4))
    with pytest.raises(ValueError, match="'dither'"):
        ip.lumaMerge()(x, torch.zeros((2, 4, 4)), dither='ordered')
    with pytest.raises(ValueError, match="'dither'"):
        ip.lumaMerge()(x, torch.zeros((2, 4, 4)), 8, dither='bayer')
    with pytest.raises(ValueError, match="'dither'"):
        ip._runPlan('doCrop', None, x, dither='round')
