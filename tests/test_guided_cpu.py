"""Luma-guided chroma without a device: the integer definition of the joint bilateral filter (pixfmt.guidedTable / guidedRange / lumaGuide /
guidedChroma) -- its tables, its invariants, what it gains over the fixed bicubic filter on four synthetic scenes and what it costs -- and every refusal of
moe_chroma_guided and of the builders' 'chroma': 'guided' that needs no device."""
import ctypes
import os
import re
from fractions import Fraction as Fr
from math import exp, floor

import numpy as np
import pytest

from moephoto_amd import _lib, pixfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCS = ('center', 'left')
DEPTHS = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le', 16: 'yuv420p16le'}


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loc', LOCS)
def test_tables_sum_to_256_are_not_negative_and_keep_their_offsets(loc):
    for scale in range(2, 17):
        off, coef = pixfmt.guidedTable(scale, loc)
        assert len(off) == scale and len(coef) == scale and all(len(r) == 4 for r in coef)
        for p in range(scale):
            assert sum(coef[p]) == 256 and min(coef[p]) >= 0, (scale, p, coef[p])
            assert -2 <= off[p] <= 1, (scale, p, off[p])
    # 'left', phase 0 sits on a source sample: the B-spline's (1, 4, 1) / 6
    assert pixfmt.guidedTable(2, 'left')[1][0] == [43, 170, 43, 0] and pixfmt.guidedTable(2, 'left')[0][0] == -1


def test_range_table_is_the_literals_and_never_zero():
    R = pixfmt.guidedRange()
    assert R[:8] == [255, 225, 155, 83, 35, 11, 3, 1] and R[8:] == [1] * 56 and len(R) == 64
    assert R == [max(1, int(round(255 * exp(-(1024 * d) ** 2 / (2 * 2048 ** 2))))) for d in range(64)]
    assert all(a >= b for a, b in zip(R, R[1:])) and min(R) == 1
    R[0] = 0
    assert pixfmt.guidedRange()[0] == 255          # (a copy: the definition cannot be edited through it)


def test_definition_refuses_what_it_does_not_know():
    for args in ((1, 'center'), (17, 'center'), (0, 'center'), (2.0, 'center'), (True, 'center'), (2, 'top')):
        with pytest.raises(ValueError):
            pixfmt.guidedTable(*args)
    C, Ys, Yo = np.zeros((2, 3, 4), np.uint16), np.zeros((6, 8), np.uint16), np.zeros((12, 16), np.uint16)
    assert pixfmt.guidedChroma(C, Ys, Yo, 'yuv420p10le', 'yuv420p10le', 2).shape == (2, 6, 8)
    for bad in (dict(scale=1), dict(scale=17), dict(scale=3), dict(loc='top'), dict(srcFmt='nv12'), dict(dstFmt='nv12'), dict(C=C[0]), dict(C=C[:, :2]), dict(Ys=Ys[:4]),
                dict(Yo=Yo[:, :14]), dict(C=C.astype(np.float32))):
        kw = dict(dict(C=C, Ys=Ys, Yo=Yo, srcFmt='yuv420p10le', dstFmt='yuv420p10le', scale=2, loc='center'), **bad)
        with pytest.raises(ValueError):
            pixfmt.guidedChroma(**kw)
    with pytest.raises(ValueError):
        pixfmt.lumaGuide(Ys, 9)
    with pytest.raises(ValueError):
        pixfmt.lumaGuide(Ys[:5], 10)


def test_the_guide_is_the_block_mean_at_16_bits():
    Y = np.random.default_rng(3).integers(0, 1024, size=(6, 8))
    G = pixfmt.lumaGuide(Y, 10, 'center')
    assert G.shape == (3, 4) and G[1, 2] == ((Y[2, 4] + Y[2, 5] + Y[3, 4] + Y[3, 5]) << 6) >> 2
    G = pixfmt.lumaGuide(Y, 10, 'left')
    assert G[1, 2] == ((Y[2, 3] + Y[3, 3] + 2 * (Y[2, 4] + Y[3, 4]) + Y[2, 5] + Y[3, 5]) << 6) >> 3
    assert G[0, 0] == ((3 * (Y[0, 0] + Y[1, 0]) + Y[0, 1] + Y[1, 1]) << 6) >> 3          # (column -1 is column 0)
    assert pixfmt.lumaGuide(np.full((4, 4), 65535, np.uint16), 16, 'left').max() == 65535


# ---- properties ------------------------------------------------------------------------------------------------------------------------------
def _noise(rng, D, shape):
    return rng.integers(0, 1 << D, size=shape).astype(np.uint16)


def test_flat_chroma_stays_flat_for_any_guide():
    rng = np.random.default_rng(4)
    for ds, src in DEPTHS.items():
        for code in (0, 1, (1 << ds) // 2, (1 << ds) - 1):
            for shape in ((1, 1), (5, 6)):
                C = np.full((2,) + shape, code, np.uint16)
                for scale in (2, 3, 16):
                    for loc in LOCS:
                        Ys, Yo = _noise(rng, ds, (2 * shape[0], 2 * shape[1])), _noise(rng, ds, (2 * shape[0] * scale, 2 * shape[1] * scale))
                        out = pixfmt.guidedChroma(C, Ys, Yo, src, src, scale, loc)
                        assert out.shape == (2, shape[0] * scale, shape[1] * scale) and (out == code).all(), (ds, code, shape, scale, loc)


def test_every_sample_lies_within_the_source_planes_range():
    rng = np.random.default_rng(5)
    for scale in (2, 3, 4, 16):
        for loc in LOCS:
            C = rng.integers(300, 701, size=(2, 7, 9)).astype(np.uint16)
            C[1] += 100
            out = pixfmt.guidedChroma(C, _noise(rng, 10, (14, 18)), _noise(rng, 10, (14 * scale, 18 * scale)), 'yuv420p10le', 'yuv420p10le', scale, loc)
            for c in range(2):
                assert C[c].min() <= out[c].min() and out[c].max() <= C[c].max(), (scale, loc, c)
    C = np.zeros((2, 9, 10), np.uint16)          # a checkerboard of the extremes at 16 bits: no overshoot to clamp, none to wrap
    C[:, ::2, ::2] = C[:, 1::2, 1::2] = 65535
    out = pixfmt.guidedChroma(C, _noise(rng, 16, (18, 20)), _noise(rng, 16, (54, 60)), 'yuv420p16le', 'yuv420p16le', 3)
    assert out.dtype == np.dtype('<u2') and out.min() >= 0 and out.max() <= 65535


def _bspline(f):
    return [(1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6, f ** 3 / 6]


def _axis(scale, loc):
    """Per phase (off, 8-bit weights), written out again from the issue's text in exact fractions."""
    rows = []
    for p in range(scale):
        r = Fr(p, scale) if loc == 'left' else Fr(2 * p + 1 - scale, 2 * scale)
        c = [floor(x * 256 + Fr(1, 2)) for x in _bspline(r - floor(r))]
        c[max(range(4), key=lambda j: (c[j], -j))] += 256 - sum(c)
        rows.append((floor(r) - 1, c))
    return rows


@pytest.mark.parametrize('loc', LOCS)
def test_a_constant_guide_gives_the_pure_b_spline(loc):
    """With one luma value everywhere every range weight is R[0]: the sample is the B-spline's, (sum cy cx code + 2^15) >> 16, computed here tap by tap."""
    rng = np.random.default_rng(6)
    for scale in (2, 3, 5):
        C = _noise(rng, 10, (2, 4, 5))
        Ys, Yo = np.full((8, 10), 600, np.uint16), np.full((8 * scale, 10 * scale), 600, np.uint16)
        got = pixfmt.guidedChroma(C, Ys, Yo, 'yuv420p10le', 'yuv420p10le', scale, loc)
        ax, ay = _axis(scale, loc), _axis(scale, 'center')
        for c in range(2):
            for Y in range(4 * scale):
                oy, cy = ay[Y % scale]
                for X in range(5 * scale):
                    ox, cx = ax[X % scale]
                    acc = sum(cy[i] * cx[j] * int(C[c, min(max(Y // scale + oy + i, 0), 3), min(max(X // scale + ox + j, 0), 4)]) for i in range(4) for j in range(4))
                    assert got[c, Y, X] == (acc + (1 << 15)) >> 16, (scale, c, Y, X)


def test_denominator_and_numerator_stay_in_their_bounds_on_noise():
    rng = np.random.default_rng(7)
    lo, hi, top = 1 << 30, 0, 0
    for scale in (2, 3, 4, 16):
        for loc in LOCS:
            C = _noise(rng, 16, (2, 6, 7)).astype(np.int64)
            GL, GH = pixfmt.lumaGuide(_noise(rng, 16, (12, 14)), 16, loc), pixfmt.lumaGuide(_noise(rng, 16, (12 * scale, 14 * scale)), 16, loc)
            num, den = pixfmt._guidedSums(C, GL, GH, scale, loc)
            lo, hi, top = min(lo, den.min()), max(hi, den.max()), max(top, num.max())
    print('den', lo, hi, 'num', top)
    assert 1 << 16 <= lo and hi < 1 << 24 and top < 1 << 40
    # the extremes themselves: every guide far from every tap (all R = 1), and a flat guide (all R = 255)
    C = np.full((2, 3, 3), 65535, np.int64)
    far = pixfmt._guidedSums(C, np.zeros((3, 3), np.int64), np.full((6, 6), 65535, np.int64), 2, 'center')
    near = pixfmt._guidedSums(C, np.zeros((3, 3), np.int64), np.zeros((6, 6), np.int64), 2, 'center')
    assert (far[1] == 1 << 16).all() and (near[1] == 255 << 16).all() and near[0].max() == (255 << 16) * 65535 < 1 << 40


def test_a_depth_change_is_the_definitions_shift():
    """The same luma at both depths (codes of the lower depth, shifted up: the guide is then the same number): the samples at depth Dd are the samples at depth Ds,
    << (Dd - Ds) or >> (Ds - Dd)."""
    rng = np.random.default_rng(8)
    for ds, src in DEPTHS.items():
        C, Ys = _noise(rng, ds, (2, 5, 4)), _noise(rng, ds, (10, 8))
        for dd, dst in DEPTHS.items():
            low = _noise(rng, min(ds, dd), (30, 24)).astype(np.int64)
            at = lambda D: (low << (D - min(ds, dd))).astype(np.uint16)
            base = pixfmt.guidedChroma(C, Ys, at(ds), src, src, 3, 'left').astype(np.int64)
            got = pixfmt.guidedChroma(C, Ys, at(dd), src, dst, 3, 'left')
            assert got.dtype == (np.uint8 if dd == 8 else np.dtype('<u2'))
            assert np.array_equal(got, base << (dd - ds) if dd >= ds else base >> (ds - dd)), (ds, dd)


# ---- quality: why the filter exists -------------------------------------------------------------------------------------------------------------
# Four scenes as formulas of the position in SOURCE luma pixels, sampled where each siting puts its samples: a luma sample x of a frame s times as dense lies at
# (x + 1/2) / s ('center') or x / s ('left': the horizontal axis is co-sited, as pixfmt.chromaTable's r = p / scale has it), a chroma sample j at the centre of its
# 2 x 2 luma block ('center') or on luma column 2 j ('left'); the vertical axis is always 'center'.  Y' carries noise of sigma = 0.004, everything is quantised to
# 10 bits.  The source frame is the scene at s = 1, the truth the scene at s = scale; bicubic = pixfmt.resampleChroma, guided = the definition fed the true
# high-resolution Y'.
QW, QH = 64, 48


def _scene(name, x, y):
    step = np.clip((x - QW / 2 + 0.35 * (y - QH / 2)) / 1.5, -0.5, 0.5) + 0.5          # a slanted edge, 1.5 source pixels wide
    if name == 'edge':          # a coloured step edge on a luma edge
        return 0.25 + 0.5 * step, 0.35 + 0.3 * step, 0.6 - 0.25 * step
    if name == 'text':          # a coloured checker of 6 x 6 source pixels: "text"
        k = (np.floor(x / 6) + np.floor(y / 6)) % 2
        return 0.2 + 0.6 * k, 0.3 + 0.4 * k, 0.65 - 0.3 * k
    if name == 'smooth':        # smooth chroma under flat luma
        return 0.5 + 0 * x, 0.5 + 0.2 * np.sin(np.pi * x / QW) * np.cos(np.pi * y / QH), 0.5 + 0.2 * np.cos(np.pi * (x / QW + y / QH))
    if name == 'iso':           # the edge scene's chroma with NO luma edge
        return 0.5 + 0 * x, 0.35 + 0.3 * step, 0.6 - 0.25 * step
    raise KeyError(name)


def _sceneFrame(name, s, loc, rng):
    q = lambda a: np.clip(np.floor(a * 1024 + 0.5), 0, 1023).astype(np.uint16)
    ax = 0.0 if loc == 'left' else 0.5
    yy, xx = np.mgrid[0:QH * s, 0:QW * s]
    Y = _scene(name, (xx + ax) / s, (yy + 0.5) / s)[0] + rng.normal(0, 0.004, (QH * s, QW * s))
    cy, cx = np.mgrid[0:QH * s // 2, 0:QW * s // 2]
    _, Cb, Cr = _scene(name, (2 * cx + 2 * ax) / s, (2 * cy + 1) / s)
    return q(Y), np.stack([q(Cb), q(Cr)])


QUALITY = {'edge': 0.5, 'text': 0.5, 'smooth': 2.0, 'iso': 2.0}          # guided MAE <= bound x bicubic MAE


@pytest.mark.parametrize('name', sorted(QUALITY))
def test_quality_against_bicubic(name):
    """Measured (profiles/guided/summary.md), guided MAE / bicubic MAE over scales 2, 3, 4 and both sitings: edge 0.20 - 0.32, text 0.006 - 0.009,
    smooth 0.83 - 1.25, iso 1.23 - 1.62."""
    rng = np.random.default_rng(20)
    fmt = 'yuv420p10le'
    for s in (2, 3, 4):
        for loc in LOCS:
            Ys, C = _sceneFrame(name, 1, loc, rng)
            Yo, truth = _sceneFrame(name, s, loc, rng)
            mae = lambda got: np.abs(got.astype(np.int64) - truth).mean()
            b, g = mae(pixfmt.resampleChroma(C, fmt, fmt, s, 'bicubic', loc)), mae(pixfmt.guidedChroma(C, Ys, Yo, fmt, fmt, s, loc))
            print('{} scale {} {}: bicubic {:.3f} guided {:.3f} ratio {:.3f}'.format(name, s, loc, b, g, g / b))
            assert g <= QUALITY[name] * b, (name, s, loc, b, g)


# ---- refusals and exports -----------------------------------------------------------------------------------------------------------------------
def _tables(scale, loc='center'):
    (ox, cx), (oy, cy) = pixfmt.guidedTable(scale, loc), pixfmt.guidedTable(scale, 'center')
    mk = lambda T, v: (T * len(v))(*v)
    flat = lambda rows: [c for r in rows for c in r]
    return [mk(ctypes.c_uint8, flat(cx)), mk(ctypes.c_int8, ox), mk(ctypes.c_uint8, flat(cy)), mk(ctypes.c_int8, oy), mk(ctypes.c_uint8, pixfmt.guidedRange())]


def test_chroma_guided_refuses_bad_arguments_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 8192)()
    p = ctypes.addressof(buf)
    p += -p % 16
    tabs = _tables(2)
    # a 3 x 5 chroma plane at 10 bits and scale 2: src_c 60 bytes, src_y 120, dst_y 480 at p + 2048, dst_c 240 behind it
    def call(src_c=p, src_y=p + 256, ds=10, h=3, w=5, dst_c=p + 2048 + 480, dst_y=p + 2048, dd=10, scale=2, loc=0, tabs=tabs):
        return L.moe_chroma_guided(src_c, src_y, ds, h, w, dst_c, dst_y, dd, scale, loc, *tabs, 0, None)
    refused = lambda rc, text: rc == _lib.EINVAL and text in L.moe_last_error()
    assert refused(call(src_c=None), b'moe_chroma_guided: NULL') and refused(call(src_y=None), b'NULL') and refused(call(dst_c=None), b'NULL') and refused(call(dst_y=None), b'NULL')
    for k in range(5):
        assert refused(call(tabs=tabs[:k] + [None] + tabs[k + 1:]), b'NULL'), k
    for d in (-8, 0, 7, 9, 11, 14, 17, 32):
        assert refused(call(ds=d), b'depth') and refused(call(dd=d), b'depth'), d
    for h, w in ((0, 5), (3, 0), (-1, 5), (3, -7)):
        assert refused(call(h=h, w=w), b'must be positive'), (h, w)
    for s in (1, 0, -1, 17, 64):
        assert refused(call(scale=s), b'scale'), s
    assert refused(call(h=1 << 29, scale=2), b'does not fit') and refused(call(w=1 << 26, scale=16, tabs=_tables(16)), b'does not fit')
    for loc in (-1, 2, 7):
        assert refused(call(loc=loc), b'loc'), loc
    assert refused(call(src_c=p + 1), b'src is not 2-byte aligned') and refused(call(dst_c=p + 2048 + 481), b'dst is not 2-byte aligned')
    assert refused(call(src_y=p + 257), b'src_y is not 2-byte aligned') and refused(call(dst_y=p + 2049), b'dst_y is not 2-byte aligned')
    assert refused(call(src_c=p + 1, src_y=p + 257, ds=8, dst_y=p + 2049), b'dst_y is not 2-byte aligned')          # (odd sources are fine at 8 bits)
    for k, axis in ((0, b'horizontal'), (2, b'vertical')):
        for row in ([0, 255, 0, 0], [1, 255, 1, 0], [255, 255, 255, 255], [0, 0, 0, 0]):
            bad = list(tabs)
            bad[k] = (ctypes.c_uint8 * 8)(*(list(tabs[k])[:4] + row))
            assert refused(call(tabs=bad), axis + b' coefficients of phase 1'), (k, row)
    for k, axis in ((1, b'horizontal'), (3, b'vertical')):
        for o in (-3, 2, 127, -128):
            bad = list(tabs)
            bad[k] = (ctypes.c_int8 * 2)(tabs[k][0], o)
            assert refused(call(tabs=bad), axis + b' offset'), (k, o)
    for d in (0, 7, 63):
        R = pixfmt.guidedRange()
        R[d] = 0
        assert refused(call(tabs=tabs[:4] + [(ctypes.c_uint8 * 64)(*R)]), b'range weight %d is zero' % d), d
    # dst_c inside, at the start of, and straddling the end of the 480 bytes of dst_y; right behind them it is a frame
    for at in (p + 2048, p + 2048 + 100, p + 2048 + 478, p + 2048 - 238):
        assert refused(call(dst_c=at), b'overlaps'), at - p
    assert 'moe_chroma_guided' in _lib.EXPORTS and L.moe_abi_version() == 4


def test_the_export_is_declared_and_listed():
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    declared = set(re.findall(r'\b(moe_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    assert 'moe_chroma_guided' in declared and 'moe_chroma_guided' in _lib.EXPORTS and L.moe_chroma_guided.argtypes is not None and len(L.moe_chroma_guided.argtypes) == 17
    assert sorted(_lib.EXPORTS) == sorted(declared) and L.moe_abi_version() == _lib.ABI_VERSION == 4
    assert 'pixfmt.py (guidedTable' in hdr          # (the definition is cited as the other blocks cite theirs)
    assert pixfmt.CHROMA_METHODS == {'nearest': 1, 'bilinear': 2, 'bicubic': 4} and pixfmt.CHROMA_LOCS == ('center', 'left')          # (the new method lives beside them)


def test_builders_refuse_guided_where_it_cannot_run_before_any_model_is_loaded(monkeypatch):
    from moephoto_amd import imageProcess, procedure
    before = dict(imageProcess.modelCache)
    sr = lambda scale=2: {'op': 'SR', 'model': 'a2', 'scale': scale}
    dn = {'op': 'DN', 'model': 'dn_lite5'}
    buf = lambda **kw: dict({'op': 'buffer', 'pixFmt': 'yuv420p10le', 'chroma': 'guided'}, **kw)

    class Reached(Exception):
        pass

    def reached(opt):
        raise Reached()
    monkeypatch.setattr(procedure.runSR, 'getOpt', reached)
    monkeypatch.setattr(procedure.runDN, 'getOpt', reached)
    cases = [([buf(), dn], 'needs a chain that enlarges'),
             ([buf(chromaLoc='left'), dn, dn], 'needs a chain that enlarges'),
             ([buf(), sr(), {'op': 'output', 'width': 96, 'height': 64}], "does not go with 'width'"),
             ([buf(), sr(), {'op': 'output', 'height': 64}], "does not go with 'height'"),
             ([buf(), sr(), {'op': 'output', 'fit': 'bilinear'}], "does not go with 'fit'"),
             ([buf(chromaLoc='top'), sr()], 'chromaLoc "top"'),
             ([buf(), sr(4), sr(4), sr(2)], 'resamples by 16 at most'),
             ([buf(chroma='guide'), sr()], 'chroma "guide"'),
             # on an SR / DN step of an RGB chain the value stays refused by the message that path already gives
             ([{'op': 'buffer', 'bitDepth': 16}, dict(sr(), chroma='guided')], '\'chroma\' "guided" is not supported'),
             ([{'op': 'buffer', 'bitDepth': 8}, dict(dn, chroma='guided')], '\'chroma\' "guided" is not supported')]
    for steps, text in cases:
        with pytest.raises(ValueError, match=text):
            procedure.genProcess(steps)
        with pytest.raises(ValueError, match=text):
            procedure.genFrameStream(steps, 48, 32, 2)
    for steps in ([buf(), sr()], [buf(chromaLoc='left'), dn, sr(4), {'op': 'output', 'pixFmt': 'yuv420p'}]):          # nothing wrong with these: they reach the model
        with pytest.raises(Reached):
            procedure.genProcess(steps)
        with pytest.raises(Reached):
            procedure.genFrameStream(steps, 48, 32, 2)
        assert procedure._planeChroma(steps) == ('guided', steps[0].get('chromaLoc', 'center'))
    assert imageProcess.modelCache == before
