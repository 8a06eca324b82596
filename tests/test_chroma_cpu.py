"""Luma-only chains without a device: the integer definition of the chroma resampling filter (pixfmt.chromaTable / resampleChroma) -- its tables,
its invariants, its distance from torch's float64 F.interpolate -- and every refusal of moe_chroma_resample, of the builders' 'chroma' / 'chromaLoc' keys and of
genFrameStream(views=..) that needs no device."""
import ctypes

import numpy as np
import pytest

from moephoto_amd import _lib, pixfmt

METHODS = ('nearest', 'bilinear', 'bicubic')
LOCS = ('center', 'left')
DEPTHS = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le', 16: 'yuv420p16le'}


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('loc', LOCS)
def test_tables_sum_to_one_fit_int32_and_keep_their_offsets(method, loc):
    for scale in range(1, 17):
        off, coef = pixfmt.chromaTable(method, scale, loc)
        assert len(off) == scale and len(coef) == scale and all(len(r) == pixfmt.CHROMA_METHODS[method] for r in coef)
        for p in range(scale):
            assert sum(coef[p]) == 1 << 14, (scale, p, coef[p])
            assert sum(abs(c) for c in coef[p]) * 65535 < 1 << 31, (scale, p, coef[p])
            assert -2 <= off[p] <= 1, (scale, p, off[p])


def test_table_refuses_what_it_does_not_know():
    for args in (('lanczos', 2, 'center'), ('bicubic', 2, 'top'), ('bicubic', 0, 'center'), ('bicubic', 17, 'center'), ('bicubic', 2.0, 'center'), ('bicubic', True, 'center')):
        with pytest.raises(ValueError):
            pixfmt.chromaTable(*args)
    with pytest.raises(ValueError):
        pixfmt.resampleChroma(np.zeros((2, 3, 3), np.uint16), 'nv12', 'yuv420p', 2, 'bicubic')
    with pytest.raises(ValueError):
        pixfmt.resampleChroma(np.zeros((3, 3), np.uint16), 'yuv420p', 'yuv420p', 2, 'bicubic')


@pytest.mark.parametrize('method', METHODS)
def test_scale_one_is_the_identity_up_to_the_shift(method):
    rng = np.random.default_rng(1)
    for ds, src in DEPTHS.items():
        C = rng.integers(0, 1 << ds, size=(2, 7, 9))
        for dd, dst in DEPTHS.items():
            for loc in LOCS:
                out = pixfmt.resampleChroma(C, src, dst, 1, method, loc)
                want = C << (dd - ds) if dd >= ds else C >> (ds - dd)
                assert out.dtype == (np.uint8 if dd == 8 else np.dtype('<u2')) and np.array_equal(out, want), (ds, dd, loc)


@pytest.mark.parametrize('method', METHODS)
def test_a_flat_plane_stays_flat(method):
    for ds, src in DEPTHS.items():
        for code in (0, 1, (1 << ds) // 2, (1 << ds) - 1):
            C = np.full((2, 5, 6), code, np.uint16)
            for scale in (2, 3, 4, 7, 16):
                for loc in LOCS:
                    out = pixfmt.resampleChroma(C, src, src, scale, method, loc)
                    assert out.shape == (2, 5 * scale, 6 * scale) and (out == code).all(), (ds, code, scale, loc)


@pytest.mark.parametrize('method', METHODS)
def test_a_checkerboard_of_extremes_stays_in_range(method):
    C = np.zeros((2, 9, 10), np.uint16)
    C[:, ::2, ::2] = C[:, 1::2, 1::2] = 65535
    for scale in (2, 3, 4, 8, 16):
        for loc in LOCS:
            out = pixfmt.resampleChroma(C, 'yuv420p16le', 'yuv420p16le', scale, method, loc).astype(np.int64)
            assert out.min() >= 0 and out.max() <= 65535
            assert out.min() == 0 and out.max() == 65535          # (the overshoot of the cubic is clamped, not wrapped)


@pytest.mark.parametrize('method', METHODS)
def test_left_siting_keeps_the_source_samples_on_their_columns(method):
    C = np.random.default_rng(2).integers(0, 1024, size=(2, 6, 8))
    out = pixfmt.resampleChroma(C, 'yuv420p10le', 'yuv420p10le', 3, method, 'left')
    assert np.array_equal(out[:, 1::3, 0::3], C)          # output [3 i + 1, 3 j] = input [i, j]: the centre phase vertically, phase 0 horizontally


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('scale', (2, 3, 4, 6, 8))
def test_against_torch_float64(method, scale):
    """F.interpolate(align_corners=False) in float64, rounded to nearest, on a 22 x 18 plane of default_rng(0) 10-bit codes: at most one code away on at most 3 % of
    the samples (the 14-bit coefficients and the rounding between the passes)."""
    import torch
    import torch.nn.functional as F
    c = np.random.default_rng(0).integers(0, 1 << 10, size=(22, 18))
    got = pixfmt.resampleChroma(np.stack([c, c]), 'yuv420p10le', 'yuv420p10le', scale, method, 'center').astype(np.int64)
    assert np.array_equal(got[0], got[1])
    kw = {} if method == 'nearest' else {'align_corners': False}
    ref = F.interpolate(torch.tensor(c, dtype=torch.float64)[None, None], scale_factor=scale, mode=method, **kw)[0, 0].numpy()
    d = np.abs(got[0] - np.clip(np.floor(ref + 0.5), 0, 1023))
    print(method, scale, 'max', d.max(), 'share', (d > 0).mean())
    assert d.max() <= 1 and (d > 0).mean() <= 0.03


def _tables(method, scale, loc='center'):
    (ox, cx), (oy, cy) = pixfmt.chromaTable(method, scale, loc), pixfmt.chromaTable(method, scale, 'center')
    taps = pixfmt.CHROMA_METHODS[method]
    mk = lambda T, v: (T * len(v))(*v)
    flat = lambda rows: [c for r in rows for c in r]
    return taps, [mk(ctypes.c_int16, flat(cx)), mk(ctypes.c_int8, ox), mk(ctypes.c_int16, flat(cy)), mk(ctypes.c_int8, oy)]


def test_chroma_resample_refuses_bad_arguments_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    p += -p % 16
    taps, tabs = _tables('bicubic', 2)
    call = lambda src=p, ds=10, h=3, w=5, dst=p + 1024, dd=10, scale=2, taps=taps, tabs=tabs: L.moe_chroma_resample(src, ds, h, w, dst, dd, scale, taps, *tabs, 0, None)
    refused = lambda rc, text: rc == _lib.EINVAL and text in L.moe_last_error()
    assert refused(call(src=None), b'moe_chroma_resample: NULL') and refused(call(dst=None), b'NULL')
    for k in range(4):
        assert refused(call(tabs=tabs[:k] + [None] + tabs[k + 1:]), b'NULL'), k
    for d in (-8, 0, 7, 9, 11, 14, 17, 32):
        assert refused(call(ds=d), b'depth') and refused(call(dd=d), b'depth'), d
    for h, w in ((0, 5), (3, 0), (-1, 5), (3, -7)):
        assert refused(call(h=h, w=w), b'must be positive'), (h, w)
    for s in (0, -1, 17, 64):
        assert refused(call(scale=s), b'scale'), s
    assert refused(call(h=1 << 30, scale=2), b'does not fit') and refused(call(w=1 << 28, scale=16, tabs=_tables('bicubic', 16)[1]), b'does not fit')
    for t in (0, 3, 5, 8, -1):
        assert refused(call(taps=t), b'taps'), t
    assert refused(call(src=p + 1), b'src is not 2-byte aligned') and refused(call(dst=p + 1025), b'dst is not 2-byte aligned')
    assert refused(call(src=p + 1, ds=8, dst=p + 1025), b'dst is not 2-byte aligned') and refused(call(src=p + 1, dd=8, dst=p + 1025), b'src is not 2-byte aligned')
    for k, axis in ((0, b'horizontal'), (2, b'vertical')):          # a row that does not sum to 2^14; one whose magnitudes break the int32 bound
        for row in ([0, 16384, 1, 0], [-1, 16384, 0, 0], [-8192, 16384, 16384, -8193], [-8193, 16385, 16385, -8193]):
            bad = list(tabs)
            bad[k] = (ctypes.c_int16 * 8)(*(list(tabs[k])[:4] + row))
            assert refused(call(tabs=bad), axis + b' coefficients of phase 1'), (k, row)
    for k, axis in ((1, b'horizontal'), (3, b'vertical')):
        for o in (-3, 2, 127, -128):
            bad = list(tabs)
            bad[k] = (ctypes.c_int8 * 2)(tabs[k][0], o)
            assert refused(call(tabs=bad), axis + b' offset'), (k, o)
    assert 'moe_chroma_resample' in _lib.EXPORTS and L.moe_abi_version() == 4


def test_builders_refuse_the_chroma_keys_before_any_model_is_loaded():
    from moephoto_amd import imageProcess, procedure
    before = dict(imageProcess.modelCache)
    sr = lambda scale=2: {'op': 'SR', 'model': 'no such model', 'scale': scale}
    buf = lambda **kw: dict({'op': 'buffer', 'pixFmt': 'yuv420p10le'}, **kw)
    cases = [([buf(chroma='lanczos'), sr()], 'chroma "lanczos"'),
             ([buf(chroma=None), sr()], 'chroma'),
             ([buf(chroma='bicubic', chromaLoc='top'), sr()], 'chromaLoc "top"'),
             ([buf(chromaLoc='top'), sr()], 'chromaLoc "top"'),
             ([buf(chromaLoc='left'), sr()], "'chromaLoc' does not apply"),
             ([buf(chroma='net', chromaLoc='center'), sr()], "'chromaLoc' does not apply"),
             ([buf(chroma='bilinear'), sr(4), sr(4), sr(2)], 'resamples by 16 at most'),
             ([buf(chroma='nearest', chromaLoc='left'), sr(3), sr(3), sr(2)], 'resamples by 16 at most')]
    for steps, text in cases:
        with pytest.raises(ValueError, match=text):
            procedure.genProcess(steps)
        with pytest.raises(ValueError, match=text):
            procedure.genFrameStream(steps, 140, 100, 2)
        with pytest.raises(ValueError, match=text):
            procedure._planeFormats(steps)
    assert procedure._planeFormats([buf(chroma='bicubic', chromaLoc='left'), sr(4), sr(4)]) == ('yuv420p10le', 'yuv420p10le')
    assert procedure._planeChroma([buf(chroma='bicubic', chromaLoc='left'), sr(4), sr(4)]) == ('bicubic', 'left')
    assert procedure._planeChroma([buf(chroma='bilinear'), sr()]) == ('bilinear', 'center')
    assert procedure._planeChroma([buf(), sr()]) is None and procedure._planeChroma([buf(chroma='net'), sr(4), sr(4), sr(4)]) is None
    with pytest.raises(ValueError, match='cannot hold a resize step'):          # (the refusals the planar chains already had are as they were)
        procedure.genProcess([buf(chroma='bicubic'), {'op': 'resize', 'scaleW': 2, 'scaleH': 2, 'method': 'bilinear'}])
    assert imageProcess.modelCache == before


def test_genframestream_refuses_views_that_are_not_a_bool_before_any_model_is_loaded():
    from moephoto_amd import imageProcess, procedure
    before = dict(imageProcess.modelCache)
    sr = {'op': 'SR', 'model': 'no such model', 'scale': 2}
    for bad in (1, 0, 'yes', None, 1.0):
        for steps in ([{'op': 'buffer', 'bitDepth': 16}, sr], [{'op': 'buffer', 'pixFmt': 'yuv420p10le'}, sr],
                      [{'op': 'buffer', 'pixFmt': 'yuv420p10le', 'chroma': 'bicubic'}, sr], [{'op': 'buffer', 'bitDepth': 8}, sr, {'op': 'output', 'pixFmt': 'yuv420p'}]):
            with pytest.raises(ValueError, match='views must be True or False'):
                procedure.genFrameStream(steps, 140, 100, 2, views=bad)
    with pytest.raises(ValueError, match='reuse must be True or False'):          # (reuse is checked first, as before)
        procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 16}, sr], 140, 100, 2, reuse='x', views='x')
    assert imageProcess.modelCache == before
