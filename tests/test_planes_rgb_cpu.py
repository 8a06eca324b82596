"""RGB frames from chains on 4:2:0 planes without a device: the integer definition of the Y'CbCr -> RGB edge (pixfmt.rgbCoefficients / toRGB) --
grey, its distance from the standard's equations in float64, the round trip of flat colours, the ordered dither, the channel order -- and every refusal of
moe_planes_to_rgb and of the builders' output-step keys that needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from moephoto_amd import _lib, pixfmt, quant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le', 16: 'yuv420p16le'}
RGBS = {8: 'rgb24', 16: 'rgb48le'}
F = pixfmt.RGB_FRAC


def frame(Y, Cb, Cr, D):
    dt = np.uint8 if D == 8 else np.dtype('<u2')
    return b''.join(np.ascontiguousarray(p).astype(dt).tobytes() for p in (Y, Cb, Cr))


def rgb(frame_bytes, D, w, h, bits, **kw):
    out = np.frombuffer(pixfmt.toRGB(frame_bytes, DEPTHS[D], w, h, kw.pop('rgbFmt', RGBS[bits]), **kw), np.uint8 if bits == 8 else np.dtype('<u2'))
    return out.reshape(h, w, 3).astype(np.int64)


def noise(D, w, h, seed, top=None):
    r = np.random.default_rng(seed)
    top = (1 << D) if top is None else top
    return r.integers(0, top, (h, w)), r.integers(0, top, (h // 2, w // 2)), r.integers(0, top, (h // 2, w // 2))


def exact(Y, Cb2, Cr2, D, bits, matrix):
    """The standard's equations in float64 on luma-sized integer planes, times the sample scale: (R, G, B), not rounded, not clamped."""
    kr, kb = pixfmt.LUMA[matrix]
    kg = 1 - kr - kb
    y, u, v = (Y - (16 << (D - 8))).astype(np.float64), (Cb2 - (128 << (D - 8))).astype(np.float64), (Cr2 - (128 << (D - 8))).astype(np.float64)
    S = (255.0 if bits == 8 else 65536.0) / (1 << (D - 8))
    return (S * (y / 219 + 2 * (1 - kr) * v / 224), S * (y / 219 - (kr * 2 * (1 - kr) * v + kb * 2 * (1 - kb) * u) / (kg * 224)), S * (y / 219 + 2 * (1 - kb) * u / 224))


# ---- the constants -------------------------------------------------------------------------------------------------------------------------------
def test_formats_and_constants():
    assert pixfmt.RGB_FORMATS == {'bgr24': (8, 'bgr'), 'rgb24': (8, 'rgb'), 'bgr48le': (16, 'bgr'), 'rgb48le': (16, 'rgb')}
    assert pixfmt.FORMATS == {'yuv420p': 8, 'yuv420p10le': 10, 'yuv420p12le': 12, 'yuv420p16le': 16}          # (untouched)
    for matrix, (kr, kb) in pixfmt.LUMA.items():
        kg = 1 - kr - kb
        for D in DEPTHS:
            for bits in (8, 16):
                c = pixfmt.rgbCoefficients(matrix, D, bits)
                S = (255 if bits == 8 else 65536) / (1 << (D - 8))
                want = (S / 219, S * 2 * (1 - kr) / 224, -S * kb * 2 * (1 - kb) / (kg * 224), -S * kr * 2 * (1 - kr) / (kg * 224), S * 2 * (1 - kb) / 224)
                assert all(isinstance(x, int) for x in c) and len(c) == 5
                assert all(abs(a - b * (1 << F)) <= 0.5 + 1e-6 for a, b in zip(c, want)), (matrix, D, bits, c)
                # what the kernel's arithmetic holds (moe_planes_to_rgb): int32 constants of 2^30 at most; three products and the rounding term inside int64
                assert 1 <= c[0] <= 1 << 30 and all(abs(x) <= 1 << 30 for x in c)
                assert 3 * 65535 * max(abs(x) for x in c) + (127 << (F - 7)) < 1 << 63
    for bad in (('bt2020c', 8, 8), ('bt709', 9, 8), ('bt709', 8, 10)):
        with pytest.raises(ValueError):
            pixfmt.rgbCoefficients(*bad)
    with pytest.raises(ValueError, match='pixFmt "nv12"'):
        pixfmt.check('nv12')
    with pytest.raises(ValueError, match='RGB format'):
        pixfmt.toRGB(b'\0' * 6, 'yuv420p', 2, 2, 'yuv420p')
    with pytest.raises(ValueError, match='even'):
        pixfmt.toRGB(b'\0' * 6, 'yuv420p', 3, 2, 'bgr24')
    with pytest.raises(ValueError, match='bytes'):
        pixfmt.toRGB(b'\0' * 5, 'yuv420p', 2, 2, 'bgr24')
    with pytest.raises(ValueError, match='dither'):
        pixfmt.toRGB(b'\0' * 6, 'yuv420p', 2, 2, 'bgr24', dither='blue')


# ---- grey ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', sorted(DEPTHS))
@pytest.mark.parametrize('bits', (8, 16))
def test_grey_is_grey_black_is_0_white_is_full_scale_and_codes_outside_clamp(D, bits):
    top, sh = (1 << bits) - 1, D - 8
    w, h = 16, 4
    codes = np.array([0, 1 << sh, 16 << sh, 17 << sh, 126 << sh, 235 << sh, (235 << sh) + 1, 240 << sh, (1 << D) - 1] + ([1 << D, 40000, 65535] if 8 < D < 16 else []))
    Y = np.resize(codes, (h, w))
    C = np.full((h // 2, w // 2), 128 << sh)
    for matrix in pixfmt.MATRICES:
        for method in pixfmt.CHROMA_METHODS:
            out = rgb(frame(Y, C, C, D), D, w, h, bits, matrix=matrix, method=method)
            assert (out[:, :, 0] == out[:, :, 1]).all() and (out[:, :, 1] == out[:, :, 2]).all()
            g = dict(zip(Y.reshape(-1).tolist(), out[:, :, 0].reshape(-1).tolist()))
            assert g[0] == 0 and g[1 << sh] == 0 and g[16 << sh] == 0 and g[235 << sh] == top and g[(235 << sh) + 1] == top and g[(1 << D) - 1] == top
            assert 0 < g[17 << sh] < g[126 << sh] < top
            if 8 < D < 16:          # codes above their depth are taken as they are (high bits are not masked): far above white
                assert g[1 << D] == g[40000] == g[65535] == top


# ---- against the standard's equations in float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', sorted(DEPTHS))
@pytest.mark.parametrize('bits', (8, 16))
@pytest.mark.parametrize('matrix', sorted(pixfmt.MATRICES))
def test_within_one_code_of_float64_and_within_the_bound_of_the_fixed_point_width(D, bits, matrix):
    """Two bounds against E S evaluated in float64 on the same integer upsampled chroma.  (a) At most 1 code from the float64 value rounded to nearest and clamped.
    (b) The bound the width F = 20 gives: each constant is round(x 2^F), off by at most 2^-(F+1) of its unit, so the sum in front of the shift differs from the exact
    2^F S E by at most (|y| + |u| + |v|) / 2 (R and B use two of the three terms: the bound is generous there), and the rounding shift adds at most 1/2 code.  Before the clamp
    |sample - S E| <= 1/2 + (|y| + |u| + |v|) 2^-(F+1); the clamp to [0, top] moves neither side away from the other.  For uint16 codes this is below 0.594."""
    w, h = 64, 48
    top = (1 << bits) - 1
    for seed, span in ((1, None), (2, 1 << 16 if D > 8 else None)):          # (codes within their depth, and over all 16 bits where the samples are uint16)
        Y, Cb, Cr = noise(D, w, h, seed + D, span)
        for method, loc in (('bicubic', 'center'), ('bilinear', 'left')):
            out = rgb(frame(Y, Cb, Cr, D), D, w, h, bits, matrix=matrix, method=method, loc=loc)
            C2 = pixfmt.resampleChroma(np.stack([Cb, Cr]), DEPTHS[D], DEPTHS[D], 2, method, loc).astype(np.int64)
            E = np.stack(exact(Y, C2[0], C2[1], D, bits, matrix), axis=2)
            assert np.abs(out - np.clip(np.floor(E + 0.5), 0, top)).max() <= 1
            mag = np.abs(Y - (16 << (D - 8))) + np.abs(C2[0] - (128 << (D - 8))) + np.abs(C2[1] - (128 << (D - 8)))
            bound = 0.5 + mag * 2.0 ** -(F + 1)
            assert bound.max() < 0.594
            err = np.abs(out - np.clip(E, 0, top))
            assert (err <= bound[:, :, None] + 1e-6).all(), (err - bound[:, :, None]).max()


# ---- the round trip of flat colours --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', sorted(DEPTHS))
@pytest.mark.parametrize('matrix', sorted(pixfmt.MATRICES))
def test_flat_colours_come_back_within_the_derived_bound(D, matrix):
    """toRGB(fromSamples16(x)) on flat frames of 16-bit samples x = (R, G, B).  On a flat frame the 2 x 2 sums are 4 x and the chroma filter returns its input (its rows
    sum to 2^14), so only these errors exist, in codes at depth D:
        e_Y  <= 1/2 + 219 2^(D-24) 65535 sum_i |c_i / 2^14 - K_i|      the forward rounding, and the forward 14-bit coefficients against the real luma constants
        e_Cb <= 1/2 + 224 2^(D-24) 65535 sum_i |u_i / 2^14 - U_i|      likewise, U = (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb));  e_Cr with V = (1 - Kr, -Kg, -Kb) / (2 (1 - Kr))
    The inverse is linear; through the absolute values of its real coefficients, in samples of scale S (2^16, or 255 for 8 bits), s = S / 2^(D-8):
        R: s (e_Y / 219 + 2 (1 - Kr) e_Cr / 224)      B: s (e_Y / 219 + 2 (1 - Kb) e_Cb / 224)      G: s (e_Y / 219 + (Kr 2 (1 - Kr) e_Cr + Kb 2 (1 - Kb) e_Cb) / (Kg 224))
    plus the conversion's own 1/2 + 3 * 65535 * 2^-21 (the test above).  The target S x / 65536 lies inside [0, top], so the clamp only brings a sample closer."""
    kr, kb = pixfmt.LUMA[matrix]
    kg = 1 - kr - kb
    crow, urow, vrow = pixfmt.coefficients(matrix)
    dev = lambda row, real: sum(abs(a / 16384 - b) for a, b in zip(row, real))
    eY = 0.5 + 219 * 2.0 ** (D - 24) * 65535 * dev(crow, (kr, kg, kb))
    eCb = 0.5 + 224 * 2.0 ** (D - 24) * 65535 * dev(urow, (-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5))
    eCr = 0.5 + 224 * 2.0 ** (D - 24) * 65535 * dev(vrow, (0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))))
    r = np.random.default_rng(7 + D)
    colours = [(a, b, c) for a in (0, 65535) for b in (0, 65535) for c in (0, 65535)] + [tuple(int(v) for v in r.integers(0, 65536, 3)) for _ in range(24)] + [(32768,) * 3, (4660, 4660, 4661)]
    for bits in (8, 16):
        s = (255.0 if bits == 8 else 65536.0) / (1 << (D - 8))
        own = 0.5 + 3 * 65535 * 2.0 ** -(F + 1)
        bound = np.array([s * (eY / 219 + 2 * (1 - kr) * eCr / 224), s * (eY / 219 + (kr * 2 * (1 - kr) * eCr + kb * 2 * (1 - kb) * eCb) / (kg * 224)),
                          s * (eY / 219 + 2 * (1 - kb) * eCb / 224)]) + own
        for col in colours:
            x = np.empty((4, 4, 3), np.uint16)
            x[:] = col
            out = rgb(pixfmt.fromSamples16(x, DEPTHS[D], matrix, 'rgb'), D, 4, 4, bits, matrix=matrix)
            assert (out == out[0, 0]).all()
            err = np.abs(out[0, 0] - np.array(col) * ((255.0 if bits == 8 else 65536.0) / 65536))
            assert (err <= bound + 1e-9).all(), (col, bits, err, bound)


# ---- dither and order ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', (8, 10, 16))
def test_ordered_dither_is_the_threshold_form_and_round_is_none(D):
    w, h = 24, 20
    Y, Cb, Cr = noise(D, w, h, 11)
    fb = frame(Y, Cb, Cr, D)
    for bits in (8, 16):
        plain = rgb(fb, D, w, h, bits)
        assert (rgb(fb, D, w, h, bits, dither='round') == plain).all() and (rgb(fb, D, w, h, bits, dither='none') == plain).all()
        got = rgb(fb, D, w, h, bits, matrix='bt601', dither='ordered')
        cY, cRV, cGU, cGV, cBU = pixfmt.rgbCoefficients('bt601', D, bits)
        C2 = pixfmt.resampleChroma(np.stack([Cb, Cr]), DEPTHS[D], DEPTHS[D], 2, 'bicubic', 'center').astype(np.int64)
        y, u, v = Y - (16 << (D - 8)), C2[0] - (128 << (D - 8)), C2[1] - (128 << (D - 8))
        T = quant.threshold('ordered', h, w)
        assert T.min() == 1 and T.max() == 127 and (T[:8, :8] == 2 * quant.bayer8() + 1).all()
        want = np.stack([np.clip((cY * y + cRV * v + (T << (F - 7))) >> F, 0, (1 << bits) - 1), np.clip((cY * y + cGU * u + cGV * v + (T << (F - 7))) >> F, 0, (1 << bits) - 1),
                         np.clip((cY * y + cBU * u + (T << (F - 7))) >> F, 0, (1 << bits) - 1)], axis=2)
        assert (got == want).all()
        assert (got != rgb(fb, D, w, h, bits, matrix='bt601')).any() and np.abs(got - rgb(fb, D, w, h, bits, matrix='bt601')).max() <= 1


def test_bgr_and_rgb_differ_by_channel_order_only():
    w, h = 12, 8
    for D in DEPTHS:
        fb = frame(*noise(D, w, h, 3), D)
        for bits, (a, b) in ((8, ('rgb24', 'bgr24')), (16, ('rgb48le', 'bgr48le'))):
            for dither in (None, 'ordered'):
                x, y = rgb(fb, D, w, h, bits, rgbFmt=a, loc='left', dither=dither), rgb(fb, D, w, h, bits, rgbFmt=b, loc='left', dither=dither)
                assert (x == y[:, :, ::-1]).all() and (x != y).any()
            assert len(pixfmt.toRGB(fb, DEPTHS[D], w, h, a)) == 3 * w * h * bits // 8


# ---- the builders --------------------------------------------------------------------------------------------------------------------------------
def test_builders_refuse_before_a_model_is_loaded(monkeypatch):
    from moephoto_amd import procedure, runDN, runSR

    def no_model(*_a, **_k):
        raise AssertionError('a model was asked for before the chain was checked')
    monkeypatch.setattr(runSR, 'getOpt', no_model)
    monkeypatch.setattr(runDN, 'getOpt', no_model)
    buf, sr = {'op': 'buffer', 'pixFmt': 'yuv420p10le'}, {'op': 'SR', 'model': 'a', 'scale': 2}
    out = lambda **kw: dict({'op': 'output'}, **kw)
    for build in (lambda steps: procedure.genFrameStream(steps, 140, 100), procedure.genProcess):
        # the new keys, by name
        for k in ('chromaUp', 'chromaLoc'):
            with pytest.raises(ValueError, match="'{}' applies beside an RGB".format(k)):
                build([buf, sr, out(**{k: 'bicubic' if k == 'chromaUp' else 'left'})])
            with pytest.raises(ValueError, match="'{}' applies beside an RGB".format(k)):
                build([buf, sr, out(pixFmt='yuv420p', **{k: 'bicubic' if k == 'chromaUp' else 'left'})])
        with pytest.raises(ValueError, match="'chromaUp' \"lanczos\""):
            build([buf, sr, out(pixFmt='bgr48le', chromaUp='lanczos')])
        with pytest.raises(ValueError, match="'chromaUp' \"guided\""):
            build([buf, sr, out(pixFmt='bgr48le', chromaUp='guided')])
        with pytest.raises(ValueError, match="'chromaLoc' \"top\""):
            build([buf, sr, out(pixFmt='rgb24', chromaLoc='top')])
        with pytest.raises(ValueError, match="'matrix' \"smpte240m\""):
            build([buf, sr, out(pixFmt='bgr24', matrix='smpte240m')])
        with pytest.raises(ValueError, match="'dither'"):
            build([buf, sr, out(pixFmt='bgr24', dither='blue')])
        # what is pinned stays refused, with the same messages
        with pytest.raises(ValueError, match="'matrix' / 'order' do not apply"):
            build([buf, sr, out(pixFmt='yuv420p', matrix='bt709')])
        with pytest.raises(ValueError, match="'matrix' / 'order' do not apply"):
            build([buf, sr, out(matrix='bt709')])
        with pytest.raises(ValueError, match="'matrix' / 'order' do not apply"):
            build([buf, sr, out(order='bgr')])
        with pytest.raises(ValueError, match="'matrix' / 'order' do not apply"):
            build([buf, sr, out(pixFmt='bgr48le', order='rgb')])          # (the format's name carries the order)
        with pytest.raises(ValueError, match="'chromaLoc' does not apply to 'chroma': 'net'"):
            build([dict(buf, chromaLoc='left'), sr, out(pixFmt='bgr48le')])
        with pytest.raises(ValueError, match="'dither' does not apply beside 'width'"):
            build([buf, sr, out(pixFmt='bgr48le', width=100, height=80, dither='ordered')])
        with pytest.raises(ValueError, match='pixFmt "nv12"'):
            build([{'op': 'buffer', 'pixFmt': 'nv12'}, sr, out(pixFmt='bgr48le')])
        with pytest.raises(ValueError, match='pixFmt "yuv444p"'):
            build([buf, sr, out(pixFmt='yuv444p')])
        with pytest.raises(ValueError, match='pixFmt "gbrp"'):
            build([buf, sr, out(pixFmt='gbrp')])
        with pytest.raises(ValueError, match='resize'):
            build([buf, sr, {'op': 'resize', 'width': 10, 'height': 6}, out(pixFmt='bgr48le')])
        with pytest.raises(AssertionError, match='a model was asked for'):          # (a chain nothing is wrong with reaches the model)
            build([buf, sr, out(pixFmt='bgr48le', matrix='bt601', chromaUp='bilinear', chromaLoc='left', dither='ordered')])
        with pytest.raises(AssertionError, match='a model was asked for'):
            build([dict(buf, chroma='guided', chromaLoc='left'), sr, out(pixFmt='rgb24')])
    with pytest.raises(ValueError, match='even'):
        procedure.genFrameStream([buf, sr, out(pixFmt='bgr48le')], 141, 100)
    assert procedure._planeFormats([buf, sr, out(pixFmt='bgr48le')]) == ('yuv420p10le', 'bgr48le')
    assert procedure._planeFormats([buf, sr, out(pixFmt='rgb24', matrix='bt2020nc')], 140, 100) == ('yuv420p10le', 'rgb24')
    assert procedure._planeFormats([buf, sr, out(pixFmt='yuv420p')]) == ('yuv420p10le', 'yuv420p')
    assert procedure._planeFormats([{'op': 'buffer', 'bitDepth': 16}, sr, out(pixFmt='bgr48le')]) is None          # (the RGB source: as before)
    assert procedure._planeRGBStep([buf, sr, out(pixFmt='bgr48le')], 'bgr48le') == ('bgr48le', 'bt709', 'bicubic', 'center')
    assert procedure._planeRGBStep([buf, sr, out(pixFmt='rgb24', matrix='bt601', chromaUp='nearest', chromaLoc='left')], 'rgb24') == ('rgb24', 'bt601', 'nearest', 'left')
    assert procedure._planeRGBStep([buf, sr], 'yuv420p10le') is None


def test_the_wrapper_refuses_before_it_needs_a_device():
    from moephoto_amd import imageProcess as ip
    with pytest.raises(ValueError, match='RGB format'):
        ip.planesToRGB('yuv420p', 4, 4, 'yuv420p')
    with pytest.raises(ValueError, match='even'):
        ip.planesToRGB('yuv420p', 5, 4, 'bgr24')
    with pytest.raises(ValueError, match='pixFmt "p010"'):
        ip.planesToRGB('p010', 4, 4, 'bgr24')
    with pytest.raises(ValueError, match='matrix'):
        ip.planesToRGB('yuv420p', 4, 4, 'bgr24', matrix='bt2020c')
    with pytest.raises(ValueError, match='chroma "lanczos"'):
        ip.planesToRGB('yuv420p', 4, 4, 'bgr24', method='lanczos')
    with pytest.raises(ValueError, match='chromaLoc'):
        ip.planesToRGB('yuv420p', 4, 4, 'bgr24', loc='top')
    with pytest.raises(ValueError, match='dither'):
        ip.planesToRGB('yuv420p', 4, 4, 'bgr24', dither='blue')
    assert callable(ip.planesToRGB('yuv420p10le', 4, 4, 'bgr48le', 'bt601', 'bilinear', 'left', 'ordered'))


# ---- the export ----------------------------------------------------------------------------------------------------------------------------------
def _tables(method='bicubic', loc='center', coef=None):
    (ox, cx), (oy, cy) = pixfmt.chromaTable(method, 2, loc), pixfmt.chromaTable(method, 2, 'center')
    taps = pixfmt.CHROMA_METHODS[method]
    return [(ctypes.c_int16 * (2 * taps))(*sum(cx, [])), (ctypes.c_int8 * 2)(*ox), (ctypes.c_int16 * (2 * taps))(*sum(cy, [])), (ctypes.c_int8 * 2)(*oy),
            (ctypes.c_int32 * 5)(*(coef or pixfmt.rgbCoefficients('bt709', 10, 16)))]


def test_planes_to_rgb_refuses_bad_arguments_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 8192)()
    p = ctypes.addressof(buf)
    p += -p % 16
    tabs = _tables()
    # a 6 x 4 frame at 10 bits: src 72 bytes at p, dst 144 bytes at p + 1024
    def call(src=p, depth=10, H=4, W=6, dst=p + 1024, bits=16, matrix=0, order=0, taps=4, tabs=tabs):
        return L.moe_planes_to_rgb(src, depth, H, W, dst, bits, matrix, order, taps, *tabs, 0, None)
    refused = lambda rc, text: rc == _lib.EINVAL and text in L.moe_last_error()
    assert refused(call(src=None), b'moe_planes_to_rgb: NULL') and refused(call(dst=None), b'NULL')
    for k in range(5):
        assert refused(call(tabs=tabs[:k] + [None] + tabs[k + 1:]), b'NULL'), k
    for d in (-8, 0, 7, 9, 11, 14, 17, 32, 10 | quant.Q_ROUND):
        assert refused(call(depth=d), b'depth'), d
    for b in (0, 1, 10, 12, 24, 32, -8):
        assert refused(call(bits=b), b'bits'), b
    assert refused(call(bits=16 | quant.Q_UNIT), b'MOE_Q_UNIT') and refused(call(bits=8 | quant.Q_UNIT | quant.Q_ORDERED), b'MOE_Q_UNIT')
    assert refused(call(bits=16 | quant.Q_ROUND | quant.Q_ORDERED), b'both set') and refused(call(bits=16 | 0x800), b'unknown flags') and refused(call(bits=quant.Q_ROUND), b'bits 0')
    for H, W in ((5, 6), (4, 7), (0, 6), (4, 0), (1, 1), (-2, 6), (4, -6), (3, 3)):
        assert refused(call(H=H, W=W), b'an even width and height'), (H, W)
    assert refused(call(H=1 << 15, W=1 << 15), b'do not fit an int') and refused(call(H=2, W=(1 << 30)), b'do not fit an int')
    for m in (-1, 3, 9):
        assert refused(call(matrix=m), b'matrix %d' % m), m
    for o in (-1, 2):
        assert refused(call(order=o), b'order %d' % o), o
    for t in (0, 3, 5, 8, 16, -1):
        assert refused(call(taps=t), b'taps'), t
    assert refused(call(src=p + 1), b'src is not 2-byte aligned') and refused(call(dst=p + 1025), b'dst is not 2-byte aligned')
    assert refused(call(src=p + 1, depth=8, dst=p + 1025), b'dst is not 2-byte aligned')          # (an odd source is fine at 8 bits)
    for k, axis in ((0, b'horizontal'), (2, b'vertical')):
        for row in ([0, 16383, 0, 0], [1, 16384, 0, 0], [-8192, 16384, 16384, -8192], [0, 0, 0, 0]):
            bad = list(tabs)
            bad[k] = (ctypes.c_int16 * 8)(*(list(tabs[k])[:4] + row))
            assert refused(call(tabs=bad), axis + b' coefficients of phase 1'), (k, row)
    for k, axis in ((1, b'horizontal'), (3, b'vertical')):
        for o in (-3, 2, 127, -128):
            bad = list(tabs)
            bad[k] = (ctypes.c_int8 * 2)(tabs[k][0], o)
            assert refused(call(tabs=bad), axis + b' offset'), (k, o)
    good = list(pixfmt.rgbCoefficients('bt709', 10, 16))
    for i, v, name in ((0, 0, b'cY'), (0, -5, b'cY'), (0, (1 << 30) + 1, b'cY'), (1, (1 << 30) + 1, b'cRV'), (2, -(1 << 30) - 1, b'cGU'), (3, -(1 << 31), b'cGV'), (4, (1 << 31) - 1, b'cBU')):
        c = list(good)
        c[i] = v
        assert refused(call(tabs=tabs[:4] + [(ctypes.c_int32 * 5)(*c)]), b'matrix constant ' + name), (i, v)
    # dst at the start of, inside, across the end of and across the start of the 72 bytes of src; right behind them it is fine as far as this check goes
    for at in (p, p + 10, p + 70, p - 142):
        assert refused(call(dst=at), b'overlaps'), at - p
    assert 'moe_planes_to_rgb' in _lib.EXPORTS and L.moe_abi_version() == 4


def test_the_export_is_declared_and_listed():
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    declared = set(re.findall(r'\b(moe_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    assert 'moe_planes_to_rgb' in declared and 'moe_planes_to_rgb' in _lib.EXPORTS and L.moe_planes_to_rgb.argtypes is not None and len(L.moe_planes_to_rgb.argtypes) == 16
    assert sorted(_lib.EXPORTS) == sorted(declared) and L.moe_abi_version() == _lib.ABI_VERSION == 4
    assert 'pixfmt.py (toRGB' in hdr          # (the definition is cited as the other blocks cite theirs)
    assert quant.Q_ROUND == 0x100 and quant.Q_ORDERED == 0x200 and quant.Q_UNIT == 0x400
