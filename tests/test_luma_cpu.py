"""Luma-only steps on RGB sources without a device: the numpy definition (moephoto_amd.luma) -- its constants, the round trip's error, the two
forms of the merge, IEEE's special values --, what the builders refuse before a model is loaded, and the four entry points' argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from moephoto_amd import _lib, luma, pixfmt, procedure
from moephoto_amd import imageProcess as ip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRICES = ('bt709', 'bt601', 'bt2020nc')
ENTRY_POINTS = ('moe_luma_split', 'moe_luma_merge', 'moe_stitch_luma', 'moe_run_plan_luma')


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('matrix', MATRICES)
def test_constants(matrix):
    k = luma.lumaCoefficients(matrix)
    kr, kb = pixfmt.LUMA[matrix]
    assert set(k) == {'kr', 'kg', 'kb', 'ib', 'ir', 'eb', 'er', 'gr', 'gb'}
    assert all(type(v) is np.float32 for v in k.values())
    assert k['kg'] > 0 and 1 - kr - kb > 0
    # each constant is the Python-float expression rounded ONCE to float32: float32 -> Python float -> float32 gives the same bits
    want = dict(kr=kr, kg=1 - kr - kb, kb=kb, ib=1 / (2 * (1 - kb)), ir=1 / (2 * (1 - kr)), eb=2 * (1 - kb), er=2 * (1 - kr),
                gr=kr * (2 * (1 - kr)) / (1 - kr - kb), gb=kb * (2 * (1 - kb)) / (1 - kr - kb))
    for name, v in want.items():
        assert k[name] == np.float32(v) and np.float32(float(k[name])) == k[name], name
    # the merge undoes the split in exact arithmetic: kr er + kg (-gr) .. = the identities behind gr / gb
    assert abs(float(k['ib']) * float(k['eb']) - 1) < 1e-6 and abs(float(k['ir']) * float(k['er']) - 1) < 1e-6
    assert abs(kr * float(k['er']) - float(k['kg']) * float(k['gr'])) < 1e-6 and abs(kb * float(k['eb']) - float(k['kg']) * float(k['gb'])) < 1e-6
    with pytest.raises(ValueError, match='chromaMatrix'):
        luma.lumaCoefficients('bt470')


@pytest.mark.parametrize('order', ['rgb', 'bgr'])
@pytest.mark.parametrize('matrix', MATRICES)
def test_round_trip_stays_within_its_rounding(matrix, order):
    k = luma.lumaCoefficients(matrix)
    bound = 4 * 2.0 ** -23 * (1 + float(k['er']) + float(k['eb']))
    x = np.random.default_rng(7).random((4, 61, 75), dtype=np.float32)
    Y, C = luma.lumaSplit(x, matrix, order)
    assert Y.shape == (2, 61, 75) and Y.dtype == np.float32 and C.shape == (2, 61, 75) and C.dtype == np.float32
    assert np.array_equal(Y[1], x[3])                                          # alpha rides as Y's second plane
    assert C.min() >= -0.5 - 1e-6 and C.max() <= 0.5 + 1e-6                    # full range, no offset
    z = luma.lumaMerge(Y, C, matrix, order)
    assert z.shape == x.shape and z.dtype == np.float32 and np.array_equal(z[3], x[3])
    assert np.abs(z[:3].astype(np.float64) - x[:3]).max() <= bound
    # the planes are named by `order`: the other order on the same planes is the same computation with planes 0 and 2 exchanged
    other = 'bgr' if order == 'rgb' else 'rgb'
    Y2, C2 = luma.lumaSplit(x[[2, 1, 0, 3]], matrix, other)
    assert np.array_equal(Y2, Y) and np.array_equal(C2, C)
    # fp16: one fp16 ulp on top of that, made of two halves -- the merge reads Y' rounded to fp16 (half an ulp of Y'; the chroma planes were formed from the unrounded
    # y), and its result is rounded to fp16 (half an ulp of the result)
    h = x[:3].astype(np.float16)
    Yh, Ch = luma.lumaSplit(h, matrix, order)
    assert Yh.dtype == np.float16 and Yh.shape == (1, 61, 75) and Ch.dtype == np.float32
    zh = luma.lumaMerge(Yh, Ch, matrix, order)
    assert zh.dtype == np.float16
    ulp = 0.5 * np.spacing(np.abs(Yh)).astype(np.float64) + 0.5 * np.spacing(np.abs(zh)).astype(np.float64)
    assert (np.abs(zh.astype(np.float64) - h.astype(np.float64)) <= ulp + bound).all()
    assert ulp.max() <= 2.0 ** -10          # (values in [0, 1]: one ulp of the format's top binade there at the most)


def test_grey_has_no_chroma_and_luma_is_the_weighted_sum():
    g = np.random.default_rng(1).random((1, 5, 7), dtype=np.float32)
    Y, C = luma.lumaSplit(np.repeat(g, 3, 0), 'bt709', 'rgb')
    assert np.abs(Y - g).max() <= 2.0 ** -23 and np.abs(C).max() <= 2.0 ** -23
    Y, C = luma.lumaSplit(np.array([1, 0, 0], np.float32).reshape(3, 1, 1), 'bt601', 'rgb')
    assert Y[0, 0, 0] == np.float32(0.299) and abs(C[1, 0, 0] - 0.5) < 1e-7          # pure red: Cr = 1/2
    Y, C = luma.lumaSplit(np.array([1, 0, 0], np.float32).reshape(3, 1, 1), 'bt601', 'bgr')
    assert Y[0, 0, 0] == np.float32(0.114) and abs(C[0, 0, 0] - 0.5) < 1e-7          # plane 0 is blue: Cb = 1/2


@pytest.mark.parametrize('dtype', [np.float32, np.float16])
def test_sample_form_is_the_canvas_through_the_quantiser(dtype):
    rng = np.random.default_rng(3)
    Y = (rng.random((2, 9, 13), dtype=np.float32) * 1.5 - 0.25).astype(dtype)
    C = (rng.random((2, 9, 13), dtype=np.float32) - 0.5).astype(np.float32)
    for bits in (8, 16):
        canvas = luma.lumaMerge(Y, C, 'bt709', 'bgr')
        got = luma.lumaMerge(Y, C, 'bt709', 'bgr', bits)
        assert got.shape == (9, 13, 4) and got.dtype == (np.uint8 if bits == 8 else np.uint16)
        q = np.float32(1 << bits)
        want = np.clip(canvas.astype(np.float32) * q, 0, q - 1).astype(np.int64).transpose(1, 2, 0)
        assert np.array_equal(got, want)
        assert got.min() == 0 and got.max() == (1 << bits) - 1, 'the values do not reach both clamps'
    with pytest.raises(ValueError):
        luma.lumaMerge(Y, C, 'bt709', 'bgr', 10)


def test_special_values_behave_as_ieee_says():
    x = np.zeros((3, 1, 6), np.float32)
    x[:, 0, 0] = (np.nan, 0.5, 0.5)          # a NaN in red: Y, Cb, Cr are NaN
    x[:, 0, 1] = (np.inf, 0.5, 0.5)          # +inf in red: Y = inf, Cr = inf - inf = NaN, Cb = 0.5 - inf = -inf
    x[:, 0, 2] = (0.5, -np.inf, 0.5)         # -inf in green: Y = -inf, Cb = Cr = +inf
    x[:, 0, 3] = (-0.25, 1.5, 2.0)           # outside [0, 1]: plain arithmetic
    x[:, 0, 4] = (np.inf, -np.inf, 0.0)      # inf - inf inside the luma sum
    Y, C = luma.lumaSplit(x, 'bt709', 'rgb')
    assert np.isnan(Y[0, 0, 0]) and np.isnan(C[:, 0, 0]).all()
    assert Y[0, 0, 1] == np.inf and C[0, 0, 1] == -np.inf and np.isnan(C[1, 0, 1])
    assert Y[0, 0, 2] == -np.inf and (C[:, 0, 2] == np.inf).all()
    assert np.isfinite(Y[0, 0, 3]) and np.isfinite(C[:, 0, 3]).all()
    assert np.isnan(Y[0, 0, 4])
    z = luma.lumaMerge(Y, C, 'bt709', 'rgb')
    assert np.isnan(z[:, 0, 0]).all() and np.isnan(z[:, 0, 1]).any() and np.abs(z[:, 0, 3] - x[:, 0, 3]).max() < 1e-5
    s = luma.lumaMerge(Y, C, 'bt709', 'rgb', 16)
    assert (s[0, 0] == 0).all()                                  # the quantiser turns NaN into 0
    assert tuple(s[0, 3]) == (0, 65535, 65535)                    # and clamps what lies outside [0, 1)
    assert (luma.quantise(np.array([np.nan, np.inf, -np.inf, 0.5, 1.0], np.float32), 8) == (0, 255, 0, 128, 255)).all()
    # fp16: a result beyond the format's range becomes inf when it is rounded
    zh = luma.lumaMerge(np.full((1, 1, 1), 65504, np.float16), np.full((2, 1, 1), 100, np.float32), 'bt709', 'rgb')
    assert zh.dtype == np.float16 and zh[0, 0, 0] == np.inf and zh[2, 0, 0] == np.inf and np.isfinite(zh[1, 0, 0])


def test_definition_refuses_what_it_cannot_take():
    x = np.zeros((3, 2, 2), np.float32)
    for bad in (np.zeros((2, 2, 2), np.float32), np.zeros((5, 2, 2), np.float32), np.zeros((3, 2), np.float32), np.zeros((3, 2, 2), np.float64)):
        with pytest.raises(ValueError):
            luma.lumaSplit(bad)
    with pytest.raises(ValueError, match='order'):
        luma.lumaSplit(x, 'bt709', 'grb')
    Y, C = luma.lumaSplit(x)
    with pytest.raises(ValueError):
        luma.lumaMerge(Y, C.astype(np.float16))
    with pytest.raises(ValueError):
        luma.lumaMerge(Y, C[:, :1])
    with pytest.raises(ValueError):
        luma.lumaMerge(x, C)


# ---- the builders' refusals, before any model is loaded -------------------------------------------------------------------------------------------
SR = {'op': 'SR', 'model': 'a', 'scale': 2}
DN = {'op': 'DN', 'model': 'lite5'}
BAD = [(dict(SR, chroma='lanczos'), "'chroma'"), (dict(DN, chroma='cubic'), "'chroma'"), (dict(SR, chroma=None), "'chroma'"),
       (dict(SR, chroma='bicubic', chromaMatrix='bt470'), "'chromaMatrix'"), (dict(DN, chroma='nearest', order='grb'), "'order'"),
       (dict(SR, chromaMatrix='bt709'), "'chromaMatrix'"), (dict(SR, chroma='net', order='rgb'), "'order'"), (dict(DN, order='bgr'), "'order'"),
       (dict(DN, chroma='net', chromaMatrix='bt601'), "'chromaMatrix'")]


@pytest.mark.parametrize('step,key', BAD, ids=lambda v: None if isinstance(v, str) else '-'.join('{}={}'.format(k, v[k]) for k in ip.LUMA_KEYS if k in v))
def test_builders_refuse_bad_keys_before_a_model_is_loaded(step, key, monkeypatch):
    def no_model(*a, **k):
        raise AssertionError('a model was loaded before the step list was checked')
    monkeypatch.setattr(ip, 'initModel', no_model)
    monkeypatch.setattr(procedure.runSR, 'initModel', no_model)
    monkeypatch.setattr(procedure.runDN, 'initModel', no_model)
    for source in ({'op': 'file'}, {'op': 'buffer', 'bitDepth': 16}):
        with pytest.raises(ValueError, match=key):
            procedure.genProcess([source, dict(step)])
    with pytest.raises(ValueError, match=key):
        procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 16}, dict(step)], 64, 48)
    with pytest.raises(ValueError, match=key):
        (procedure.runSR if step['op'] == 'SR' else procedure.runDN).getOpt(dict(step))


@pytest.mark.parametrize('key,value', [('chroma', 'bicubic'), ('chroma', 'net'), ('chromaMatrix', 'bt709'), ('order', 'bgr')])
def test_builders_refuse_the_keys_on_a_planar_chain(key, value, monkeypatch):
    def no_model(*a, **k):
        raise AssertionError('a model was loaded before the step list was checked')
    monkeypatch.setattr(procedure.runSR, 'initModel', no_model)
    monkeypatch.setattr(procedure.runDN, 'initModel', no_model)
    for step in (SR, DN):
        steps = [{'op': 'buffer', 'pixFmt': 'yuv420p10le'}, dict(step, **{key: value})]
        with pytest.raises(ValueError, match="'{}' does not apply to a step of a chain on planar".format(key)):
            procedure.genProcess(steps)
        with pytest.raises(ValueError, match="'{}' does not apply to a step of a chain on planar".format(key)):
            procedure.genFrameStream(steps, 64, 48)


def test_keys_resolve_to_their_defaults():
    assert ip.lumaKeys({'op': 'SR'}) == ('net', 'bt709', 'rgb')
    assert ip.lumaKeys({'op': 'SR', 'chroma': 'bicubic'}) == ('bicubic', 'bt709', 'rgb')
    assert ip.lumaKeys({'op': 'DN', 'chroma': 'nearest', 'chromaMatrix': 'bt2020nc'}, 'bgr') == ('nearest', 'bt2020nc', 'bgr')
    assert ip.lumaKeys({'op': 'DN', 'chroma': 'bilinear', 'order': 'rgb'}, 'bgr') == ('bilinear', 'bt709', 'rgb')
    # the order's default follows the source step: 'rgb' behind a file, 'bgr' behind a buffer; a list without the key is not touched
    for source, want in (({'op': 'file'}, 'rgb'), ({'op': 'buffer', 'bitDepth': 8}, 'bgr')):
        steps = [source, dict(SR, chroma='bicubic'), dict(DN)]
        procedure._lumaCheck(steps)
        assert steps[1]['order'] == want and steps[1]['chromaMatrix'] == 'bt709' and steps[2] == DN


# ---- the entry points -------------------------------------------------------------------------------------------------------------------------
def test_luma_exports_are_declared_and_present():
    from moephoto_amd import build
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    declared = set(re.findall(r'\b(moe_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert sorted(_lib.EXPORTS) == sorted(declared)
    assert L.moe_abi_version() == _lib.ABI_VERSION == 4
    assert 'luma.hip' in build.SOURCES and 'luma.h' in build.HEADERS


def test_luma_entry_points_validate_their_arguments_without_a_device():
    L = _lib.lib()
    err = lambda: L.moe_last_error()
    grey = ip.TilePlan((1, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    rgb = ip.TilePlan((3, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd, half = ctypes.c_void_p(p.value + 1), ctypes.c_void_p(p.value + 2)
    F32, F16, U8, U16 = _lib.F32, _lib.F16, _lib.U8, _lib.U16

    sp = lambda img, dt, C, H, W, mat, ordr, dy, dc: L.moe_luma_split(img, dt, C, 14000, 140, 1, H, W, mat, ordr, dy, dc, 0, None)
    for args in ((None, F32, 3, 2, 2, 0, 1, p, p), (p, F32, 3, 2, 2, 0, 1, None, p), (p, F32, 3, 2, 2, 0, 1, p, None)):
        assert sp(*args) == _lib.EINVAL and b'moe_luma_split: NULL' in err()
    for C in (0, 1, 2, 5, -3):
        assert sp(p, F32, C, 2, 2, 0, 1, p, p) == _lib.EINVAL and '{} planes (3, or 4'.format(C).encode() in err()
    for dt in (U8, U16, 9):
        assert sp(p, dt, 3, 2, 2, 0, 1, p, p) == _lib.EINVAL and b'dtype' in err()
    for H, W in ((0, 2), (2, 0), (-1, 2)):
        assert sp(p, F32, 3, H, W, 0, 1, p, p) == _lib.EINVAL and b'positive' in err()
    for mat in (-1, 3):
        assert sp(p, F32, 3, 2, 2, mat, 1, p, p) == _lib.EINVAL and 'unknown matrix {}'.format(mat).encode() in err()
    for ordr in (-1, 2):
        assert sp(p, F32, 3, 2, 2, 0, ordr, p, p) == _lib.EINVAL and 'unknown order {}'.format(ordr).encode() in err()
    assert sp(odd, F16, 3, 2, 2, 0, 1, p, p) == _lib.EINVAL and b'not aligned' in err()
    assert sp(half, F32, 3, 2, 2, 0, 1, p, p) == _lib.EINVAL and b'not aligned' in err()
    assert sp(p, F16, 3, 2, 2, 0, 1, odd, p) == _lib.EINVAL and b'not aligned' in err()
    assert sp(p, F16, 3, 2, 2, 0, 1, p, half) == _lib.EINVAL and b'dst_c is not 4-byte aligned' in err()

    mg = lambda y, dt, c, C, mat, ordr, bits, d, ddt, H=2, W=2: L.moe_luma_merge(y, dt, c, C, H, W, mat, ordr, bits, d, ddt, 0, None)
    for args in ((None, F32, p, 3, 0, 1, 0, p, F32), (p, F32, None, 3, 0, 1, 0, p, F32), (p, F32, p, 3, 0, 1, 0, None, F32)):
        assert mg(*args) == _lib.EINVAL and b'moe_luma_merge: NULL' in err()
    for C in (0, 1, 2, 5):
        assert mg(p, F32, p, C, 0, 1, 0, p, F32) == _lib.EINVAL and '{} colour planes (3, or 4'.format(C).encode() in err()
    assert mg(p, U16, p, 3, 0, 1, 0, p, U16) == _lib.EINVAL and b'canvas dtype' in err()
    assert mg(p, F32, p, 3, 0, 1, 0, p, F32, H=0) == _lib.EINVAL and b'positive' in err()
    assert mg(p, F32, p, 3, 3, 1, 0, p, F32) == _lib.EINVAL and b'unknown matrix 3' in err()
    assert mg(p, F32, p, 3, 0, 2, 0, p, F32) == _lib.EINVAL and b'unknown order 2' in err()
    for bits in (1, 10, 12, 32, -8):
        assert mg(p, F32, p, 3, 0, 1, bits, p, U16) == _lib.EINVAL and '{} bits (0 = the canvas, 8 or 16)'.format(bits).encode() in err()
    assert mg(p, F32, p, 3, 0, 1, 0, p, F16) == _lib.EINVAL and b'dst dtype must be the canvas dtype' in err()
    assert mg(p, F32, p, 3, 0, 1, 8, p, F32) == _lib.EINVAL and b'MOE_U8 or MOE_U16' in err()
    assert mg(p, F32, p, 3, 0, 1, 16, p, U8) == _lib.EINVAL and b'do not fit MOE_U8' in err()
    assert mg(p, F32, half, 3, 0, 1, 0, p, F32) == _lib.EINVAL and b'c is not 4-byte aligned' in err()
    assert mg(p, F32, p, 3, 0, 1, 16, odd, U16) == _lib.EINVAL and b'dst is not aligned' in err()
    assert mg(odd, F16, p, 3, 0, 1, 0, p, F16) == _lib.EINVAL and b'y is not aligned' in err()

    st = lambda pl, tiles, P, cdt, c, mat, ordr, bits, d, ddt: L.moe_stitch_luma(pl, 0, tiles, None, P, cdt, c, mat, ordr, bits, d, ddt, None)
    for args in ((None, p, 1, F32, p, 0, 1, 0, p, F32), (grey._h, None, 1, F32, p, 0, 1, 0, p, F32)):
        assert st(*args) == _lib.EINVAL and b'moe_stitch_luma: NULL' in err()
    for args in ((grey._h, p, 1, F32, None, 0, 1, 0, p, F32), (grey._h, p, 1, F32, p, 0, 1, 0, None, F32)):
        assert st(*args) == _lib.EINVAL and b'NULL' in err()
    for P in (0, 3, 4, -1):
        assert st(grey._h, p, P, F32, p, 0, 1, 0, p, F32) == _lib.EINVAL and '{} pool planes'.format(P).encode() in err()
    assert st(grey._h, p, 1, U8, p, 0, 1, 0, p, U8) == _lib.EINVAL and b'canvas dtype' in err()
    assert st(grey._h, p, 1, F16, p, 7, 1, 0, p, F16) == _lib.EINVAL and b'unknown matrix 7' in err()
    assert st(grey._h, p, 2, F16, p, 0, 7, 0, p, F16) == _lib.EINVAL and b'unknown order 7' in err()
    assert st(grey._h, p, 1, F16, p, 0, 0, 12, p, U16) == _lib.EINVAL and b'12 bits' in err()
    assert st(grey._h, p, 1, F16, p, 0, 0, 16, p, U8) == _lib.EINVAL and b'do not fit' in err()
    assert st(grey._h, p, 1, F16, half, 0, 0, 16, p, U16) == _lib.EINVAL and b'c is not 4-byte aligned' in err()
    assert st(grey._h, p, 1, F16, p, 0, 0, 16, odd, U16) == _lib.EINVAL and b'dst is not aligned' in err()
    assert st(grey._h, half, 1, F16, p, 0, 0, 16, p, U16) == _lib.EINVAL and b'tiles_dev is not 4-byte aligned' in err()

    h = ctypes.c_void_p()
    _lib.check(L.moe_net_create(_lib.ARCH_NET2X, 2, ctypes.byref(h)))
    try:
        rp = lambda net, pl, img, dt, c, mat, ordr, bits, d, ddt: L.moe_run_plan_luma(net, pl, img, dt, 14000, 140, 1, c, mat, ordr, bits, d, ddt, 0, None)
        for args in ((None, grey._h, p, F32, p, 0, 1, 0, p, F32), (h, None, p, F32, p, 0, 1, 0, p, F32), (h, grey._h, None, F32, p, 0, 1, 0, p, F32)):
            assert rp(*args) == _lib.EINVAL and b'moe_run_plan_luma: NULL' in err()
        assert rp(h, grey._h, p, F32, None, 0, 1, 0, p, F32) == _lib.EINVAL and b'NULL' in err()
        assert rp(h, grey._h, p, F32, p, 0, 1, 0, None, F32) == _lib.EINVAL and b'NULL' in err()
        assert rp(h, rgb._h, p, F32, p, 0, 1, 0, p, F32) == _lib.EINVAL and b'the plan has 3 planes' in err()
        assert rp(h, grey._h, p, U16, p, 0, 1, 0, p, U16) == _lib.EINVAL and b'canvas dtype' in err()
        assert rp(h, grey._h, p, F32, p, 4, 1, 0, p, F32) == _lib.EINVAL and b'unknown matrix 4' in err()
        assert rp(h, grey._h, p, F32, p, 0, 4, 0, p, F32) == _lib.EINVAL and b'unknown order 4' in err()
        assert rp(h, grey._h, p, F32, p, 0, 1, 10, p, U16) == _lib.EINVAL and b'10 bits' in err()
        assert rp(h, grey._h, p, F32, half, 0, 1, 0, p, F32) == _lib.EINVAL and b'c is not 4-byte aligned' in err()
        assert rp(h, grey._h, p, F32, p, 0, 1, 16, odd, U16) == _lib.EINVAL and b'dst is not aligned' in err()
        assert rp(h, grey._h, half, F32, p, 0, 1, 0, p, F32) == _lib.EINVAL and b'img_y is not aligned' in err()
        assert rp(h, grey._h, p, F32, p, 0, 1, 0, p, F32) == _lib.ESTATE and b'moe_run_plan_luma: net is not finalized' in err()
    finally:
        L.moe_net_destroy(h)


def test_wrappers_refuse_without_a_device():
    import torch
    x = torch.zeros((3, 4, 4))
    with pytest.raises(_lib.EngineError, match='HIP device'):
        ip.lumaSplit()(x)
    with pytest.raises(_lib.EngineError, match='HIP device'):
        ip.lumaMerge()(x[:1], torch.zeros((2, 4, 4)))
    for bad in (dict(matrix='bt470'), dict(order='grb')):
        with pytest.raises(ValueError):
            ip.lumaSplit(**bad)
        with pytest.raises(ValueError):
            ip.lumaMerge(**bad)
    with pytest.raises(ValueError, match='chroma'):
        ip.doCropLuma(None, x, 'lanczos')
    with pytest.raises(ValueError, match='chromaMatrix'):
        ip.doCropLuma(None, x, 'bicubic', 'bt470')
