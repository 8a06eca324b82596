"""The encoder's Y'CbCr 4:2:0 frames without a device: the written definition (moephoto_amd/pixfmt.py) against the real-number formula, the frame layout, what the three
entry points (include/moephoto_amd.h: moe_stitch_yuv, moe_run_plan_yuv, moe_to_yuv) refuse before anything touches a device, and what the builders refuse before a
model is loaded."""
import ctypes
import os
import re

import numpy as np
import pytest

from moephoto_amd import _lib, imageProcess as ip, pixfmt, procedure, runDN, runSR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = ['yuv420p', 'yuv420p10le', 'yuv420p12le', 'yuv420p16le']
MATS = ['bt709', 'bt601', 'bt2020nc']
CORNERS = [(r, g, b) for r in (0, 65535) for g in (0, 65535) for b in (0, 65535)]


def _image():
    """63 x 77 random uint16 samples in 'rgb' order with the eight cube corners planted as whole 2 x 2 blocks (a linear error is largest at a corner)."""
    a = np.random.default_rng(420).integers(0, 65536, (63, 77, 3), dtype=np.uint16)
    for k, c in enumerate(CORNERS):
        a[2 * k:2 * k + 2, 10:12] = c
    return a


IMG = _image()


def _planes(buf, fmt, w, h):
    D = pixfmt.FORMATS[fmt]
    dt = np.uint8 if D == 8 else np.dtype('<u2')
    oy, ou, ov, end = pixfmt.planeOffsets(fmt, w, h)
    assert len(buf) == end == pixfmt.frameBytes(fmt, w, h)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    a = np.frombuffer(buf, np.uint8)
    return (a[oy:ou].view(dt).reshape(h, w).astype(np.int64), a[ou:ov].view(dt).reshape(ch, cw).astype(np.int64), a[ov:end].view(dt).reshape(ch, cw).astype(np.int64))


def _real(rgb, D, matrix):
    """The real-number limited-range formula on E = sample / 2^16, the scale of the definition, with the mean of the 2 x 2 block for chroma."""
    kr, kb = pixfmt.LUMA[matrix]
    H, W = rgb.shape[:2]
    e = np.pad(rgb.astype(np.float64) / 65536.0, ((0, H % 2), (0, W % 2), (0, 0)), mode='edge')
    r, g, b = e[..., 0], e[..., 1], e[..., 2]
    y = kr * r + (1 - kr - kb) * g + kb * b
    k = 2.0 ** (D - 8)
    box = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) / 4
    cb, cr = box((b - y) / (2 * (1 - kb))), box((r - y) / (2 * (1 - kr)))
    return (16 + 219 * y[:H, :W]) * k, (128 + 224 * cb) * k, (128 + 224 * cr) * k


def test_coefficient_tables():
    assert pixfmt.coefficients('bt601') == ((4899, 9617, 1868), (-2765, -5427, 8192), (8192, -6860, -1332))
    assert pixfmt.coefficients('bt709') == ((3483, 11718, 1183), (-1877, -6315, 8192), (8192, -7441, -751))
    assert pixfmt.coefficients('bt2020nc') == ((4304, 11108, 972), (-2288, -5904, 8192), (8192, -7533, -659))
    assert pixfmt.FORMATS == {'yuv420p': 8, 'yuv420p10le': 10, 'yuv420p12le': 12, 'yuv420p16le': 16}
    for m in MATS:
        rows = pixfmt.coefficients(m)
        assert sum(rows[0]) == 16384 and sum(rows[1]) == 0 and sum(rows[2]) == 0


@pytest.mark.parametrize('matrix', MATS)
@pytest.mark.parametrize('fmt', FMTS)
def test_definition_against_the_real_number_formula(fmt, matrix):
    D = pixfmt.FORMATS[fmt]
    k = 1 << (D - 8)
    h, w = IMG.shape[:2]
    got = _planes(pixfmt.fromSamples16(IMG, fmt, matrix, 'rgb'), fmt, w, h)
    want = _real(IMG, D, matrix)
    err = max(float(np.abs(g - r).max()) for g, r in zip(got, want))
    print('{} {}: max distance from the real-number formula {:.3f} LSB'.format(fmt, matrix, err))
    assert err <= (0.6 if D <= 12 else 2.0)
    assert got[0].min() >= 16 * k and got[0].max() <= 235 * k
    for c in got[1:]:
        assert c.min() >= 16 * k and c.max() <= 240 * k
    # the corners: black and white reach the ends of the luma range, blue / red the ends of the chroma ranges
    assert got[0][0, 10] == 16 * k and abs(got[0][14, 10] - 235 * k) <= (1 if D <= 12 else 2)
    assert abs(got[1][1, 5] - 240 * k) <= (1 if D <= 12 else 2)          # block 1 = (0, 0, 65535): blue
    assert abs(got[2][4, 5] - 240 * k) <= (1 if D <= 12 else 2)                   # block 4 = (65535, 0, 0): red
    # a grey image has chroma exactly 128 k
    grey = np.repeat(np.random.default_rng(1).integers(0, 65536, (9, 11, 1), dtype=np.uint16), 3, axis=2)
    blocks = np.repeat(np.repeat(grey[:5, :6], 2, axis=0), 2, axis=1)[:9, :11]      # constant over every 2 x 2 block or not: chroma is linear in the sums
    for im in (grey, blocks):
        _, cb, cr = _planes(pixfmt.fromSamples16(im, fmt, matrix, 'rgb'), fmt, 11, 9)
        assert (cb == 128 * k).all() and (cr == 128 * k).all()


def test_frame_layout():
    want = {(88, 72): (6336, 1584), (135, 111): (14985, 68 * 56), (75, 61): (4575, 38 * 31)}
    for (w, h), (luma, chroma) in want.items():
        assert pixfmt.planeOffsets('yuv420p', w, h) == (0, luma, luma + chroma, luma + 2 * chroma)
        assert pixfmt.frameBytes('yuv420p', w, h) == luma + 2 * chroma
        for fmt in FMTS[1:]:
            assert pixfmt.planeOffsets(fmt, w, h) == (0, 2 * luma, 2 * (luma + chroma), 2 * (luma + 2 * chroma))
            assert pixfmt.frameBytes(fmt, w, h) == 2 * (luma + 2 * chroma)
        a = np.random.default_rng(w).integers(0, 65536, (h, w, 3), dtype=np.uint16)
        assert len(pixfmt.fromSamples16(a, 'yuv420p', 'bt709', 'bgr')) == luma + 2 * chroma


@pytest.mark.parametrize('fmt', ['yuv420p', 'yuv420p10le', 'yuv420p16le'])
def test_odd_image_equals_its_edge_replicated_twin(fmt):
    h, w = IMG.shape[:2]
    twin = np.pad(IMG, ((0, 1), (0, 1), (0, 0)), mode='edge')
    y0, u0, v0 = _planes(pixfmt.fromSamples16(IMG, fmt), fmt, w, h)
    y1, u1, v1 = _planes(pixfmt.fromSamples16(twin, fmt), fmt, w + 1, h + 1)
    assert np.array_equal(y0, y1[:h, :w]) and np.array_equal(u0, u1) and np.array_equal(v0, v1)


def test_order_rgb_on_swapped_planes_equals_bgr():
    for fmt in FMTS:
        for m in MATS:
            assert pixfmt.fromSamples16(IMG[:, :, ::-1], fmt, m, 'rgb') == pixfmt.fromSamples16(IMG, fmt, m, 'bgr')
    assert pixfmt.fromSamples16(IMG, 'yuv420p10le', 'bt709', 'rgb') != pixfmt.fromSamples16(IMG, 'yuv420p10le', 'bt709', 'bgr')
    assert pixfmt.fromSamples16(IMG, 'yuv420p10le') == pixfmt.fromSamples16(IMG, 'yuv420p10le', 'bt709', 'bgr')          # the defaults
    for bad in (dict(fmt='nv12'), dict(fmt='yuv420p', matrix='bt470'), dict(fmt='yuv420p', order='gbr')):
        with pytest.raises(ValueError):
            pixfmt.fromSamples16(IMG, **bad)
    with pytest.raises(ValueError):
        pixfmt.fromSamples16(IMG.astype(np.int32), 'yuv420p')


def test_yuv_exports_are_declared_and_present():
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    declared = set(re.findall(r'\b(moe_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    for name in ('moe_stitch_yuv', 'moe_run_plan_yuv', 'moe_to_yuv'):
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.moe_abi_version() == _lib.ABI_VERSION == 4
    assert 'python/video.py:24,219,230' in hdr
    ids = dict(re.findall(r'#define (MOE_(?:YUV|ORDER)_[A-Z0-9]+) (\d+)', hdr))
    assert {m: int(ids['MOE_YUV_' + m.upper()]) for m in MATS} == pixfmt.MATRICES
    assert {o: int(ids['MOE_ORDER_' + o.upper()]) for o in ('bgr', 'rgb')} == pixfmt.ORDERS


def test_yuv_entry_points_validate_their_arguments_without_a_device():
    L = _lib.lib()
    err = lambda: L.moe_last_error()
    plan = ip.TilePlan((3, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    grey = ip.TilePlan((1, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    rgba = ip.TilePlan((4, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    sy = lambda pl, tiles, cdt, depth, matrix, order, dst: L.moe_stitch_yuv(pl, 0, tiles, None, cdt, depth, matrix, order, dst, None)
    assert sy(None, p, _lib.F32, 8, 0, 0, p) == _lib.EINVAL and b'moe_stitch_yuv: NULL' in err()
    assert sy(plan._h, None, _lib.F32, 8, 0, 0, p) == _lib.EINVAL and b'NULL' in err()
    assert sy(plan._h, p, _lib.F32, 8, 0, 0, None) == _lib.EINVAL and b'NULL' in err()
    for other in (grey, rgba):
        assert sy(other._h, p, _lib.F32, 8, 0, 0, p) == _lib.EINVAL and b'planes (C must be 3)' in err()
    assert sy(plan._h, p, _lib.U8, 8, 0, 0, p) == _lib.EINVAL and b'canvas dtype' in err()
    for depth in (0, 9, 14, 24):
        assert sy(plan._h, p, _lib.F16, depth, 0, 0, p) == _lib.EINVAL and 'depth {}'.format(depth).encode() in err()
    for matrix in (-1, 3):
        assert sy(plan._h, p, _lib.F16, 10, matrix, 0, p) == _lib.EINVAL and 'unknown matrix {}'.format(matrix).encode() in err()
    for order in (-1, 2):
        assert sy(plan._h, p, _lib.F16, 10, 0, order, p) == _lib.EINVAL and 'unknown order {}'.format(order).encode() in err()

    ty = lambda src, sdt, H, W, depth, matrix, order, dst: L.moe_to_yuv(src, sdt, H, W, depth, matrix, order, dst, 0, None)
    assert ty(None, _lib.F32, 4, 4, 8, 0, 0, p) == _lib.EINVAL and b'moe_to_yuv: NULL' in err()
    assert ty(p, _lib.F32, 4, 4, 8, 0, 0, None) == _lib.EINVAL and b'NULL' in err()
    assert ty(p, _lib.F32, 0, 4, 8, 0, 0, p) == _lib.EINVAL and b'size' in err()
    assert ty(p, _lib.U16, 4, 4, 8, 0, 0, p) == _lib.EINVAL and b'dtype' in err()
    assert ty(p, _lib.F32, 4, 4, 11, 0, 0, p) == _lib.EINVAL and b'depth 11' in err()
    assert ty(p, _lib.F32, 4, 4, 12, 7, 0, p) == _lib.EINVAL and b'unknown matrix 7' in err()
    assert ty(p, _lib.F32, 4, 4, 12, 2, 5, p) == _lib.EINVAL and b'unknown order 5' in err()

    h = ctypes.c_void_p()
    _lib.check(L.moe_net_create(_lib.ARCH_NET2X, 2, ctypes.byref(h)))
    try:
        ry = lambda net, pl, img, cdt, depth, matrix, order, dst: L.moe_run_plan_yuv(net, pl, img, _lib.F32, 14000, 140, 1, cdt, depth, matrix, order, dst, 0, None)
        assert ry(None, plan._h, p, _lib.F32, 8, 0, 0, p) == _lib.EINVAL and b'moe_run_plan_yuv: NULL' in err()
        assert ry(h, None, p, _lib.F32, 8, 0, 0, p) == _lib.EINVAL and b'NULL' in err()
        assert ry(h, plan._h, None, _lib.F32, 8, 0, 0, p) == _lib.EINVAL and b'NULL' in err()
        assert ry(h, plan._h, p, _lib.F32, 8, 0, 0, None) == _lib.EINVAL and b'NULL' in err()
        assert ry(h, grey._h, p, _lib.F32, 8, 0, 0, p) == _lib.EINVAL and b'planes (C must be 3)' in err()
        assert ry(h, plan._h, p, _lib.U16, 8, 0, 0, p) == _lib.EINVAL and b'canvas dtype' in err()
        assert ry(h, plan._h, p, _lib.F32, 13, 0, 0, p) == _lib.EINVAL and b'depth 13' in err()
        assert ry(h, plan._h, p, _lib.F32, 16, 3, 0, p) == _lib.EINVAL and b'unknown matrix 3' in err()
        assert ry(h, plan._h, p, _lib.F32, 16, 0, 2, p) == _lib.EINVAL and b'unknown order 2' in err()
        assert ry(h, plan._h, p, _lib.F32, 16, 2, 1, p) == _lib.ESTATE and b'moe_run_plan_yuv: net is not finalized' in err()
    finally:
        L.moe_net_destroy(h)


def test_builders_refuse_before_a_model_is_loaded(monkeypatch):
    def no_model(*_a, **_k):
        raise AssertionError('a model was asked for before the output format was checked')
    monkeypatch.setattr(runSR, 'getOpt', no_model)
    monkeypatch.setattr(runDN, 'getOpt', no_model)
    buf, sr = {'op': 'buffer', 'bitDepth': 16}, {'op': 'SR', 'model': 'a', 'scale': 2}
    with pytest.raises(ValueError, match='pixFmt'):
        procedure.genFrameStream([buf, sr, {'op': 'output', 'pixFmt': 'nv12'}], 88, 72)
    with pytest.raises(ValueError, match='matrix'):
        procedure.genFrameStream([buf, sr, {'op': 'output', 'pixFmt': 'yuv420p10le', 'matrix': 'smpte240m'}], 88, 72)
    with pytest.raises(ValueError, match='order'):
        procedure.genFrameStream([buf, sr, {'op': 'output', 'pixFmt': 'yuv420p10le', 'order': 'gbr'}], 88, 72)
    with pytest.raises(ValueError, match='pixFmt'):
        procedure.genProcess([buf, sr, {'op': 'output', 'pixFmt': 'yuv444p'}])
    with pytest.raises(ValueError, match='buffer'):
        procedure.genProcess([{'op': 'file'}, sr, {'op': 'output', 'pixFmt': 'yuv420p'}])
    with pytest.raises(ValueError, match='buffer'):
        procedure.genProcess([sr, {'op': 'output', 'pixFmt': 'yuv420p'}])
    for fn in (ip.doCropYuv, lambda o, x, fmt, **kw: ip.toYuv(fmt, **kw)):          # the format is checked before the image or the model is looked at
        with pytest.raises(ValueError, match='pixFmt'):
            fn(None, None, 'p010')
        with pytest.raises(ValueError, match='matrix'):
            fn(None, None, 'yuv420p', matrix='bt2020c')


def test_a_step_list_without_pixfmt_builds_what_it_built_before():
    buf = {'op': 'buffer', 'bitDepth': 8}
    rs = {'op': 'resize', 'width': 10, 'height': 6, 'method': 'nearest'}
    plain, nodes0 = procedure.genProcess([buf, dict(rs)])
    with_out, nodes1 = procedure.genProcess([buf, dict(rs), {'op': 'output'}])
    other, nodes2 = procedure.genProcess([buf, dict(rs), {'op': 'output', 'matrix': 'bt601'}])          # (no pixFmt: nothing is asked for)
    assert nodes0 == nodes1 == nodes2 == [dict(op='resize', mode='nearest')]
    assert plain((b'', 4, 6)) == with_out((b'', 4, 6)) == other((b'', 4, 6)) == []
    assert procedure._outputFormat([buf, rs, {'op': 'output'}]) is None
    assert procedure._outputFormat([buf, rs, {'op': 'output', 'pixFmt': 'yuv420p12le'}]) == ('yuv420p12le', 'bt709', 'bgr')
    assert procedure._outputFormat([buf, {'op': 'output', 'pixFmt': 'yuv420p', 'matrix': 'bt601', 'order': 'rgb'}]) == ('yuv420p', 'bt601', 'rgb')
