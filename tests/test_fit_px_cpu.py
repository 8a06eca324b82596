"""Fitted sizes on RGB chains without a device: the definition of the interleaved fit (pixfmt.fitPixels), what the builders refuse of a resize step's 'fit' key before any
model is loaded, that step lists without the key are read as before, and every refusal of moe_fit_create_px."""
import ctypes
import os
import re

import numpy as np
import pytest

from moephoto_amd import _lib, pixfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ('nearest', 'bilinear', 'bicubic')
ONE = 1 << 14


# ---- the definition -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', METHODS)
def test_fitpixels_is_fitplanes_channel_by_channel(method):
    rng = np.random.default_rng(7)
    for C in (1, 2, 3, 4):
        for (h, w), (oh, ow) in (((5, 7), (9, 4)), ((12, 9), (3, 20)), ((1, 1), (3, 2))):
            for ds, dd in ((8, 8), (16, 16), (16, 8), (8, 16)):
                x = rng.integers(0, 1 << ds, size=(h, w, C))
                got = pixfmt.fitPixels(x, ds, dd, oh, ow, method)
                assert got.shape == (oh, ow, C) and got.dtype == (np.uint8 if dd == 8 else np.dtype('<u2')) and got.flags['C_CONTIGUOUS']
                for c in range(C):
                    want = pixfmt.fitPlanes(x[:, :, c][None], ds, dd, oh, ow, method, 'center')[0]
                    assert (got[:, :, c] == want).all(), (C, c, h, w, oh, ow, ds, dd)


@pytest.mark.parametrize('method', METHODS)
def test_fitpixels_at_equal_sizes_is_the_identity(method):
    for C in (1, 3, 4):
        x = np.random.default_rng(C).integers(0, 65536, size=(19, 23, C))
        assert (pixfmt.fitPixels(x, 16, 16, 19, 23, method) == x).all()
        assert (pixfmt.fitPixels(x, 16, 8, 19, 23, method) == x >> 8).all()
        assert (pixfmt.fitPixels(x >> 8, 8, 16, 19, 23, method) == (x >> 8) << 8).all()


def test_fitpixels_refuses_other_shapes():
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 5), np.uint8), np.zeros((4, 4, 0), np.uint8), np.zeros((4, 4, 3), np.float32)):
        with pytest.raises(ValueError, match='fitPixels'):
            pixfmt.fitPixels(bad, 8, 8, 2, 2, 'bicubic')
    with pytest.raises(ValueError, match='depth'):
        pixfmt.fitPixels(np.zeros((4, 4, 3), np.uint8), 9, 8, 2, 2, 'bicubic')
    with pytest.raises(ValueError, match='shrinks'):
        pixfmt.fitPixels(np.zeros((9, 4, 3), np.uint8), 8, 8, 2, 4, 'bicubic')


# ---- the builders -------------------------------------------------------------------------------------------------------------------------------
SR = lambda **kw: dict({'op': 'SR', 'model': 'no such model', 'scale': 2}, **kw)
DN = lambda **kw: dict({'op': 'DN', 'model': 'no such model'}, **kw)
BUF = lambda **kw: dict({'op': 'buffer', 'bitDepth': 16}, **kw)
FIT = lambda **kw: dict({'op': 'resize', 'width': 210, 'height': 150, 'fit': 'bicubic'}, **kw)
OUT = lambda **kw: dict({'op': 'output'}, **kw)


def _without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


REFUSED = [
    ([FIT(), SR()], "must be the last compute step"),
    ([SR(), FIT(), DN()], "must be the last compute step"),
    ([FIT(), SR(), FIT()], "must be the last compute step"),
    ([SR(), FIT(method='bilinear')], "'method' does not apply beside 'fit'"),
    ([SR(), FIT(fit='lanczos')], "'fit' 'lanczos' is not supported"),
    ([SR(), FIT(fit=None)], "'fit' None is not supported"),
    ([SR(), FIT(fit=2)], "'fit' 2 is not supported"),
    ([SR(), _without(FIT(), 'width', 'height')], "'fit' needs a size: 'width' or 'scaleW'"),
    ([SR(), _without(FIT(), 'width')], "'fit' needs a size: 'width' or 'scaleW'"),
    ([SR(), _without(FIT(), 'height')], "'fit' needs a size: 'height' or 'scaleH'"),
    ([SR(), _without(FIT(scaleW=0.5), 'width', 'height')], "'fit' needs a size: 'height' or 'scaleH'"),
    ([SR(), FIT(width=0)], "'width' must be positive"),
    ([SR(), FIT(height=-3)], "'height' must be positive"),
    ([SR(), _without(FIT(scaleW=0.0), 'width')], "'scaleW' must be positive"),
    ([SR(), FIT(), OUT(dither='round')], "'dither' does not apply"),
    ([SR(), FIT(), OUT(dither='ordered')], "'dither' does not apply"),
]


def test_builders_refuse_the_fit_key_before_any_model_is_loaded():
    from moephoto_amd import imageProcess, procedure
    before = dict(imageProcess.modelCache)
    for work, text in REFUSED:
        for depth in (8, 16):
            with pytest.raises(ValueError, match=text):
                procedure.genFrameStream([BUF(bitDepth=depth)] + [dict(s) for s in work], 140, 100)
            with pytest.raises(ValueError, match=text):
                procedure.genProcess([BUF(bitDepth=depth)] + [dict(s) for s in work])
        with pytest.raises(ValueError, match=text):
            procedure.genProcess([dict(s) for s in work], 8)                      # an array source
        with pytest.raises(ValueError, match=text):
            procedure.genProcess([{'op': 'file'}] + [dict(s) for s in work], 16)
    # a Y'CbCr output behind a fit is out of scope: refused by name on the video source (an image source refuses pixFmt as it always did)
    for builder in (lambda s: procedure.genFrameStream(s, 140, 100), procedure.genProcess):
        with pytest.raises(ValueError, match="'pixFmt' does not apply"):
            builder([BUF(), SR(), FIT(), OUT(pixFmt='yuv420p10le')])
    with pytest.raises(ValueError, match="'fit' writes 8- or 16-bit samples"):
        procedure.genProcess([SR(), FIT()], 10)
    # ratios beyond 4 down / 16 up are refused where the chain's size is known, the stream builder (the fit step alone behind 140 x 100 frames: no model, no device)
    for step, text in ((FIT(width=34, height=100), "'width' \\(34 samples\\) shrinks the chain's 140 by more than 4"),
                       (FIT(width=140, height=24), "'height' \\(24 samples\\) shrinks the chain's 100 by more than 4"),
                       (FIT(width=2241, height=100), "'width' \\(2241 samples\\) enlarges the chain's 140 by more than 16"),
                       (_without(FIT(scaleH=0.2), 'height'), "'scaleH' \\(20 samples\\) shrinks the chain's 100")):
        with pytest.raises(ValueError, match=text):
            procedure.genFrameStream([BUF(), step], 140, 100)
    # the same behind steps whose model does not exist: the chain's size comes from the step dicts (SR scale 2: 280 x 200; a plain resize step in between), so the
    # ratio is refused by key and no model is looked for
    for work, text in (([SR(), FIT(width=69, height=150)], "'width' \\(69 samples\\) shrinks the chain's 280 by more than 4"),
                       ([SR(), FIT(width=210, height=49)], "'height' \\(49 samples\\) shrinks the chain's 200 by more than 4"),
                       ([SR(), FIT(width=4481, height=150)], "'width' \\(4481 samples\\) enlarges the chain's 280 by more than 16"),
                       ([SR(), _without(FIT(scaleW=0.2), 'width')], "'scaleW' \\(56 samples\\) shrinks the chain's 280"),
                       ([SR(), {'op': 'resize', 'scaleW': '0.5', 'height': 50, 'method': 'bicubic'}, SR(scale=3), FIT(width=104, height=150)],
                        "'width' \\(104 samples\\) shrinks the chain's 420 by more than 4"),
                       ([DN(), SR(scale=4), FIT(width=139, height=400)], "'width' \\(139 samples\\) shrinks the chain's 560 by more than 4")):
        for depth in (8, 16):
            with pytest.raises(ValueError, match=text):
                procedure.genFrameStream([BUF(bitDepth=depth)] + [dict(s) for s in work], 140, 100)
    assert procedure._chainSize([SR(), {'op': 'resize', 'scaleW': '0.5', 'height': 50}, SR(scale=3)], 100, 140) == (150, 420)
    assert procedure._chainSize([SR(), {'op': 'resize', 'scaleW': 0.5}], 100, 140) is None          # (a step that does not say: the builder's walk raises as before)
    # a ratio within the filter's range goes on to the model, as every accepted list does
    with pytest.raises(ValueError, match='unknown model'):
        procedure.genFrameStream([BUF(), SR(), FIT(width=70, height=50)], 140, 100)
    assert imageProcess.modelCache == before
    # planar chains refuse any resize step, with or without the key, exactly as before
    for step in (FIT(), _without(FIT(), 'fit')):
        with pytest.raises(ValueError, match='cannot hold a resize step'):
            procedure.genProcess([{'op': 'buffer', 'pixFmt': 'yuv420p10le'}, SR(), step])
        with pytest.raises(ValueError, match='cannot hold a resize step'):
            procedure.genFrameStream([{'op': 'buffer', 'pixFmt': 'yuv420p10le'}, SR(), step], 140, 100)
    # the output step's size keys stay refused on an RGB chain, with the message that points here
    with pytest.raises(ValueError, match='an RGB chain takes a resize step'):
        procedure.genProcess([BUF(), SR(), OUT(width=210, height=150, fit='bicubic')])


def test_pixel_fit_size_rounds_as_resize_does():
    from moephoto_amd import procedure
    size = procedure._pixelFitSize
    assert size({'width': 210, 'height': 150}, 200, 280) == (150, 210)
    assert size({'scaleW': 0.75, 'scaleH': 0.75}, 200, 280) == (150, 210)
    assert size({'scaleW': 0.5, 'height': 33}, 101, 101) == (33, round(101 * 0.5))          # (round half to even, as imageProcess.resize: 50)
    assert size({'scaleW': 1.5, 'scaleH': 2.5}, 3, 5) == (round(7.5), round(7.5))
    assert size({'width': 35, 'height': 25}, 100, 140) == (25, 35)                           # exactly 4 down
    assert size({'width': 2240, 'height': 1600}, 100, 140) == (1600, 2240)                   # exactly 16 up


def test_step_lists_without_the_key_are_read_as_before():
    """No 'fit' on the resize step: _pixelFit finds nothing, touches nothing, and the builders go on to where they went before (the model that does not exist)."""
    from moephoto_amd import procedure
    for work in ([SR()], [SR(), _without(FIT(), 'fit')], [_without(FIT(method='bicubic'), 'fit'), SR()], [{'op': 'resize', 'scaleW': '0.5', 'scaleH': 0.5}, SR()]):
        for depth in (8, 10, 16):
            steps = [BUF(bitDepth=depth)] + [dict(s) for s in work] + [OUT(dither='round')]
            copy = [dict(s) for s in steps]
            assert procedure._pixelFit(steps, depth) is None and steps == copy          # (not even the size keys are converted here: the loop does that, as before)
        with pytest.raises(ValueError, match='unknown model'):
            procedure.genFrameStream([BUF()] + [dict(s) for s in work], 140, 100)
        with pytest.raises(ValueError, match='unknown model'):
            procedure.genProcess([BUF()] + [dict(s) for s in work])
    # the step with the key: found, its size keys converted as the loop converts a resize step's
    s = FIT(width='210', scaleH='0.75')
    del s['height']
    got = procedure._pixelFit([BUF(), SR(), s, OUT(dither='none')], 16)
    assert got is s and s['width'] == 210 and s['scaleH'] == 0.75 and isinstance(s['width'], int)


# ---- the entry point ----------------------------------------------------------------------------------------------------------------------------
def test_fit_create_px_is_declared_bound_and_present():
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    declared = set(re.findall(r'\b(moe_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    assert 'moe_fit_create_px' in declared and 'moe_fit_create_px' in _lib.EXPORTS and L.moe_fit_create_px.argtypes is not None
    assert L.moe_fit_create_px.argtypes == L.moe_fit_create.argtypes          # the same tables, the same handle
    assert sorted(_lib.EXPORTS) == sorted(declared)
    assert L.moe_abi_version() == _lib.ABI_VERSION == 4          # an addition: the version stays
    from moephoto_amd import build
    assert 'fit_px.hip' in build.SOURCES and 'fit.hip' in build.SOURCES


def _tabs(method, n, m):
    off, coef = pixfmt.fitTable(method, n, m)
    T = len(coef[0])
    return T, (ctypes.c_int16 * (m * T))(*[c for r in coef for c in r]), (ctypes.c_int32 * m)(*off)


def test_fit_create_px_validates_its_arguments_without_a_device():
    L = _lib.lib()
    h, w, oh, ow = 12, 20, 7, 9
    tx, ty = _tabs('bicubic', w, ow), _tabs('bicubic', h, oh)
    handle = ctypes.c_void_p()

    def create(channels=3, ds=16, dd=8, h=h, w=w, oh=oh, ow=ow, tx=tx, ty=ty, out=ctypes.byref(handle)):
        return L.moe_fit_create_px(channels, ds, h, w, dd, oh, ow, tx[0], tx[1], tx[2], ty[0], ty[1], ty[2], 0, out)

    def refused(rc, text):
        msg = L.moe_last_error()
        assert rc == _lib.EINVAL and text in msg and b'moe_fit_create_px' in msg and not handle.value, (rc, msg, text)
    for c in (0, 5, -1, 1 << 20):
        refused(create(channels=c), b'channels (1 to 4)')
    for k in (1, 2):
        for axis in ('tx', 'ty'):
            bad = list(tx if axis == 'tx' else ty)
            bad[k] = None
            refused(create(**{axis: bad}), b'moe_fit_create_px: NULL')
    refused(create(out=None), b'NULL')
    for d in (0, 7, 9, 14, 17, -8):
        refused(create(ds=d), b'depth')
        refused(create(dd=d), b'depth')
    for key in ('h', 'w', 'oh', 'ow'):
        for v in (0, -2):
            refused(create(**{key: v}), b'must be positive')
        refused(create(**{key: 1 << 31}), b'does not fit an int')
    for key in ('w', 'ow'):          # the pixels fit an int, the row's elements do not
        refused(create(**{key: (1 << 31) // 3 + 1}), b'channels does not fit an int')
        refused(create(channels=4, **{key: 1 << 29}), b'channels does not fit an int')
    for t in (0, 17, -1):
        refused(create(tx=(t,) + tx[1:]), b'taps')
        refused(create(ty=(t,) + ty[1:]), b'taps')
    for axis, name, tab, n, m in (('tx', b'horizontal', tx, w, ow), ('ty', b'vertical', ty, h, oh)):
        T = tab[0]
        for row in (0, m - 1):
            c = list(tab[1])
            c[row * T + T - 1] += 1
            refused(create(**{axis: (T, (ctypes.c_int16 * len(c))(*c), tab[2])}), name + b' coefficients of output ' + str(row).encode())
        c = list(tab[1])
        c[T:2 * T] = [-8193, 16385, 16385, -8193] + [0] * (T - 4)          # sums to 2^14, magnitudes 49156: the int32 bound is part of the contract
        refused(create(**{axis: (T, (ctypes.c_int16 * len(c))(*c), tab[2])}), b'magnitudes 49156')
        for row, value in ((m - 1, n), (0, -T), (m - 1, 1 << 30), (0, -(1 << 31))):
            o = list(tab[2])
            o[row] = value
            refused(create(**{axis: (T, tab[1], (ctypes.c_int32 * m)(*o))}), name + b' offset')
        o = list(tab[2])
        o[3] = o[2] - 1
        refused(create(**{axis: (T, tab[1], (ctypes.c_int32 * m)(*o))}), b'must not decrease')
    # offsets that are valid one by one but step so far that no tile's window fits the LDS: at C = 4 a tile of 128 elements holds 32 pixels, 64 pixels make two tiles
    n_out = 64
    far = (1, (ctypes.c_int16 * n_out)(*[ONE] * n_out), (ctypes.c_int32 * n_out)(*[1024 * k for k in range(n_out)]))
    refused(create(channels=4, h=1 << 16, w=1 << 16, oh=n_out, ow=n_out, tx=far, ty=far), b'bytes of LDS')
    # moe_fit_create itself is as it was: its own name in its messages, and no channels to refuse
    rc = L.moe_fit_create(0, 16, h, w, 8, oh, ow, tx[0], tx[1], tx[2], ty[0], ty[1], ty[2], 0, ctypes.byref(handle))
    assert rc == _lib.EINVAL and b'moe_fit_create: 0 planes' in L.moe_last_error()


def test_python_wrapper_refuses_before_the_library():
    from moephoto_amd import imageProcess as ip
    for bad in (lambda: ip.fitPixels(16, 8, 3, 50, 70, 12, 70, 'bicubic'), lambda: ip.fitPixels(16, 8, 3, 5, 7, 5, 114, 'bicubic'), lambda: ip.fitPixels(16, 9, 3, 5, 7, 5, 7, 'bicubic'),
                lambda: ip.fitPixels(16, 8, 5, 5, 7, 5, 7, 'bicubic'), lambda: ip.fitPixels(16, 8, 0, 5, 7, 5, 7, 'bicubic'), lambda: ip.fitPixels(16, 8, True, 5, 7, 5, 7, 'bicubic'),
                lambda: ip.fitPixels(16, 8, 3, 5, 7, 5, 7, 'lanczos')):
        with pytest.raises(ValueError):
            bad()
    assert callable(ip.fitPixels(16, 8, 3, 5, 7, 9, 4, 'bicubic'))          # (no handle yet: made at the first call, for that call's device)
