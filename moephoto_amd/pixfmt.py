"""The encoder's planar Y'CbCr 4:2:0 frames: the definition the device kernels (stitch_yuv_kernel, to_output_yuv_kernel) are held to, in numpy.  (Below it, the
definition of chains that run on such planes as they come from the decoder, with no conversion at all: planeShapes, toPlanes, fromPlanes; and below that the
integer resampling filter that writes the chroma planes of a luma-only chain: chromaTable, resampleChroma; then its luma-guided form: guidedTable, guidedChroma; at the
end the integer Y'CbCr -> RGB edge of a planar chain that hands back bgr24 / rgb24 / bgr48le / rgb48le frames: RGB_FORMATS, rgbCoefficients, toRGB.)

The reference fixes the pipe's pixel format to bgr24 / bgr48le (python/video.py:24,219,230) and leaves the conversion to the encoder's side; here the last pass over a
frame can write the encoder's own planes.  This module is the written specification and the comparator of the tests; it is on no hot path.

Input: the three colour samples of a pixel at 16 bits, as today's quantiser gives them with bits = 16 (value * 65536, clamped to [0, 65535], truncated, NaN = 0).
`order` names the planes: 'bgr' (plane 0 is blue: the video path's frames) or 'rgb'.

Output: limited-range Y'CbCr at depth D in {8, 10, 12, 16}, 4:2:0 with centre siting (a chroma sample is formed from the sums of its 2 x 2 block), integers only.
With (Kr, Kb) the matrix's luma constants and 14-bit coefficients

    Y row    cR = round(Kr 2^14)   cB = round(Kb 2^14)                  cG = 2^14 - cR - cB
    Cb row   uB = 2^13             uR = -round(Kr / (2 (1 - Kb)) 2^14)  uG = -uB - uR
    Cr row   vR = 2^13             vB = -round(Kb / (2 (1 - Kr)) 2^14)  vG = -vR - vB

and int64 arithmetic, >> an arithmetic (floor) shift:

    L  = cR R + cG G + cB B                                   Y  = (16 << (D - 8)) + ((L 219 + (1 << (37 - D))) >> (38 - D))
    M  = uR sum(R) + uG sum(G) + uB sum(B)  (four samples)    Cb = (128 << (D - 8)) + ((M 224 + (1 << (39 - D))) >> (40 - D));   Cr likewise with the v row

The chroma planes are ceil(H / 2) x ceil(W / 2); a block that hangs over the right or bottom edge of an odd-sized image repeats the edge pixel.  A frame is the Y
plane, then Cb, then Cr, contiguous: uint8 for D = 8, little-endian uint16 otherwise -- ffmpeg's rawvideo yuv420p, yuv420p10le, yuv420p12le, yuv420p16le.
"""
import numpy as np

FORMATS = {'yuv420p': 8, 'yuv420p10le': 10, 'yuv420p12le': 12, 'yuv420p16le': 16}             # pix_fmt -> depth D
LUMA = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722), 'bt2020nc': (0.2627, 0.0593)}      # matrix -> (Kr, Kb)
MATRICES = {'bt709': 0, 'bt601': 1, 'bt2020nc': 2}                                             # matrix -> MOE_YUV_BT709 .. (include/moephoto_amd.h)
ORDERS = {'bgr': 0, 'rgb': 1}                                                                  # order -> MOE_ORDER_BGR, MOE_ORDER_RGB


def coefficients(matrix):
    """((cR, cG, cB), (uR, uG, uB), (vR, vG, vB)) of a matrix, as Python ints."""
    kr, kb = LUMA[matrix]
    cR, cB = int(round(kr * 16384)), int(round(kb * 16384))
    uB, uR = 8192, -int(round(kr / (2 * (1 - kb)) * 16384))
    vR, vB = 8192, -int(round(kb / (2 * (1 - kr)) * 16384))
    return (cR, 16384 - cR - cB, cB), (uR, -uB - uR, uB), (vR, -vR - vB, vB)


def check(fmt, matrix='bt709', order='bgr'):
    """(depth, matrix id, order id) of a request as the library takes it; ValueError names what is unknown."""
    if fmt not in FORMATS:
        raise ValueError('pixFmt "{}" is not supported ({})'.format(fmt, ', '.join(FORMATS)))
    if matrix not in MATRICES:
        raise ValueError('matrix "{}" is not supported ({})'.format(matrix, ', '.join(MATRICES)))
    if order not in ORDERS:
        raise ValueError('order "{}" is not supported ({})'.format(order, ', '.join(ORDERS)))
    return FORMATS[fmt], MATRICES[matrix], ORDERS[order]


def planeOffsets(fmt, w, h):
    """Byte offsets of the Y, Cb and Cr planes in a frame of w x h pixels, and the frame's size behind them: (y, cb, cr, end)."""
    es = 1 if FORMATS[fmt] == 8 else 2
    w, h = int(w), int(h)
    luma, chroma = w * h * es, ((w + 1) // 2) * ((h + 1) // 2) * es
    return 0, luma, luma + chroma, luma + 2 * chroma


def frameBytes(fmt, w, h):
    return planeOffsets(fmt, w, h)[3]


# ---- chains on the decoder's own planes ----------------------------------------------------------------------------------------------------
# None of the SR / DN nets convolves planes jointly (planes are the batch), so a chain can run on a 4:2:0 source as it is: Y' as a one-plane image at full size, Cb and
# Cr as a two-plane image at half size -- half the plane-pixels of the bgr48le pipe, and no colour matrix at either end.  The definition the device kernels
# (to_float_planes_kernel, stitch_planes_kernel, to_output_kernel) are held to:
#
#     toPlanes     value = code * 2^-D for every depth D -- 8 bits is / 256, NOT the RGB path's / 255: a depth change is then an exact shift and neutral chroma
#                  (128 << (D - 8)) is 0.5 at every depth.  uint16 codes are taken as they are (high bits are not masked).  Rounded to dtype: fp32 is exact, fp16
#                  rounds to nearest even.
#     fromPlanes   per sample moe_to_output's quantiser with bits = D': fp32(v) * 2^D', clamped to [0, 2^D' - 1], truncated, NaN = 0.
#
# Limited range is preserved, not expanded: the net sees code / 2^D.
def planeShapes(fmt, w, h):
    """((h, w), (h // 2, w // 2)): the Y plane and each chroma plane of a frame; ValueError for an unknown format or a width / height that is odd or below 2."""
    if fmt not in FORMATS:
        raise ValueError('pixFmt "{}" is not supported ({})'.format(fmt, ', '.join(FORMATS)))
    w, h = int(w), int(h)
    if w < 2 or h < 2 or w % 2 or h % 2:
        raise ValueError('a {} frame needs an even width and height of 2 at least, got {} x {}'.format(fmt, w, h))
    return (h, w), (h // 2, w // 2)


def toPlanes(frame_bytes, fmt, w, h, dtype=np.float32):
    """The frame's bytes -> Y of shape (1, h, w) and C of shape (2, h / 2, w / 2) (Cb, then Cr), code * 2^-D rounded to dtype (float32 or float16)."""
    (yh, yw), (ch, cw) = planeShapes(fmt, w, h)
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise ValueError('toPlanes: dtype must be float32 or float16, got {}'.format(dtype))
    D = FORMATS[fmt]
    _, cb, _, end = planeOffsets(fmt, w, h)
    if len(frame_bytes) != end:
        raise ValueError('toPlanes: a {} frame of {} x {} is {} bytes, got {}'.format(fmt, w, h, end, len(frame_bytes)))
    codes = np.frombuffer(frame_bytes, np.uint8 if D == 8 else np.dtype('<u2'))
    v = (codes.astype(np.float32) * np.float32(2.0 ** -D)).astype(dtype)          # (the product is exact in fp32: 16 bits times a power of two)
    return v[:yh * yw].reshape(1, yh, yw), v[yh * yw:].reshape(2, ch, cw)


def fromPlanes(Y, C, fmt):
    """Y (1, h, w) [or (h, w)] and C (2, h / 2, w / 2) -> the frame's bytes at fmt's depth, laid out as planeOffsets says."""
    Y, C = np.asarray(Y), np.asarray(C)
    if Y.ndim == 2:
        Y = Y[None]
    if Y.ndim != 3 or Y.shape[0] != 1 or C.ndim != 3 or C.shape[0] != 2:
        raise ValueError('fromPlanes: Y of shape (1, h, w) and C of shape (2, h / 2, w / 2) expected, got {} and {}'.format(Y.shape, C.shape))
    (_, _), chroma = planeShapes(fmt, Y.shape[2], Y.shape[1])
    if tuple(C.shape[1:]) != chroma:
        raise ValueError('fromPlanes: chroma planes of {} expected for a Y plane of {}, got {}'.format(chroma, Y.shape[1:], C.shape[1:]))
    D = FORMATS[fmt]
    q = np.float32(1 << D)

    def quantise(p):
        with np.errstate(invalid='ignore', over='ignore'):
            v = p.astype(np.float32) * q
            v = np.fmin(np.fmax(v, np.float32(0)), q - np.float32(1))          # (fmaxf / fminf: a NaN gives way to the bound, so NaN = 0)
        return v.astype(np.int64).astype(np.uint8 if D == 8 else np.dtype('<u2'))
    return quantise(Y).tobytes() + quantise(C).tobytes()


def fromSamples16(hwc, fmt, matrix='bt709', order='bgr'):
    """(H, W, 3) uint16 samples -> the frame's bytes."""
    D = check(fmt, matrix, order)[0]
    a = np.asarray(hwc)
    if a.dtype != np.uint16 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('fromSamples16: an (H, W, 3) uint16 array expected, got {} {}'.format(a.dtype, a.shape))
    a = a.astype(np.int64)
    H, W = a.shape[:2]
    r, g, b = (a[:, :, 2], a[:, :, 1], a[:, :, 0]) if order == 'bgr' else (a[:, :, 0], a[:, :, 1], a[:, :, 2])
    (cR, cG, cB), urow, vrow = coefficients(matrix)
    Y = (16 << (D - 8)) + (((cR * r + cG * g + cB * b) * 219 + (1 << (37 - D))) >> (38 - D))

    def sums(p):          # the 2 x 2 block sums, the edge pixel repeated
        p = np.pad(p, ((0, H % 2), (0, W % 2)), mode='edge')
        return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    sr, sg, sb = sums(r), sums(g), sums(b)
    chroma = lambda k: (128 << (D - 8)) + (((k[0] * sr + k[1] * sg + k[2] * sb) * 224 + (1 << (39 - D))) >> (40 - D))
    dt = np.uint8 if D == 8 else np.dtype('<u2')
    return b''.join(np.ascontiguousarray(p).astype(dt).tobytes() for p in (Y, chroma(urow), chroma(vrow)))


# ---- luma-only chains: the chroma planes by a fixed integer polyphase filter -------------------------------------------------------------------
# The other form of a chain on 4:2:0 planes: the net runs on Y' alone and Cb / Cr are brought to the output's size by a resampling filter -- what the device kernel
# (resize_kernel_codes, moe_chroma_resample) is held to, byte for byte.  The library builds no table of its own: chromaTable is the only definition.
#
# Output index o = q * scale + p reads around the source coordinate q + r(p):
#     'center'   r = (2 p + 1 - scale) / (2 scale)      align_corners = False, moe_resize's and the net path's convention
#     'left'     r = p / scale                          chroma co-sited with the even luma columns (MPEG-2, H.264, HEVC); the horizontal axis only
# nearest: off = floor(r + 1/2), one coefficient 2^14.  Otherwise f = r - floor(r), the weights (1 - f, f) for bilinear (off = floor(r)) or torch's cubic convolution
# with A = -0.75 (off = floor(r) - 1), each rounded as floor(w 2^14 + 1/2), the deficit to exactly 2^14 added to the tap of largest magnitude (the first of equals).
# Tap j reads source index clamp(q + off[p] + j, 0, n - 1): the edge sample repeats.  The weights are evaluated in exact fractions, so no float rounding takes part.
CHROMA_METHODS = {'nearest': 1, 'bilinear': 2, 'bicubic': 4}          # method -> taps
CHROMA_LOCS = ('center', 'left')
CHROMA_ONE = 1 << 14


def _cubic(x):
    """torch's cubic convolution with A = -3/4 at x, an exact fraction (cubic1 / cubic2 of misc_kernels.hip); 0 from |x| = 2 on."""
    from fractions import Fraction as Fr
    A, x = Fr(-3, 4), abs(x)
    if x <= 1:
        return ((A + 2) * x - (A + 3)) * x * x + 1
    return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A if x < 2 else Fr(0)


def _quantRow(weights):
    """Exact weights that sum to 1 -> 14-bit coefficients that sum to 2^14: floor(w 2^14 + 1/2) each, the deficit added to the tap of largest magnitude (the first of equals)."""
    from fractions import Fraction as Fr
    from math import floor
    c = [floor(x * CHROMA_ONE + Fr(1, 2)) for x in weights]
    c[max(range(len(c)), key=lambda j: (abs(c[j]), -j))] += CHROMA_ONE - sum(c)
    return c


def chromaTable(method, scale, loc='center'):
    """(off[scale], coef[scale][taps]) of one axis, as lists of Python ints; ValueError names what is unknown."""
    from fractions import Fraction as Fr
    from math import floor
    if method not in CHROMA_METHODS:
        raise ValueError('chroma "{}" is not supported ({})'.format(method, ', '.join(CHROMA_METHODS)))
    if loc not in CHROMA_LOCS:
        raise ValueError('chromaLoc "{}" is not supported ({})'.format(loc, ', '.join(CHROMA_LOCS)))
    if not isinstance(scale, int) or isinstance(scale, bool) or not 1 <= scale <= 16:
        raise ValueError('chroma: scale must be 1..16, got {!r}'.format(scale))
    off, coef = [], []
    for p in range(scale):
        r = Fr(p, scale) if loc == 'left' else Fr(2 * p + 1 - scale, 2 * scale)
        if method == 'nearest':
            off.append(floor(r + Fr(1, 2)))
            coef.append([CHROMA_ONE])
            continue
        f = r - floor(r)
        off.append(floor(r) - (1 if method == 'bicubic' else 0))
        coef.append(_quantRow([1 - f, f] if method == 'bilinear' else [_cubic(f + 1), _cubic(f), _cubic(1 - f), _cubic(2 - f)]))
    return off, coef


def _polyAxis(x, off, coef, axis):
    """One pass over `axis` of an int64 array, off and coef per output index: out[o] = sum_j coef[o][j] * x[clamp(off[o] + j, 0, n - 1)]."""
    n = x.shape[axis]
    off, coef = np.asarray(off, np.int64), np.asarray(coef, np.int64)
    shape = [1] * x.ndim
    shape[axis] = len(off)
    out = 0
    for j in range(coef.shape[1]):
        out = out + np.take(x, np.clip(off + j, 0, n - 1), axis=axis) * coef[:, j].reshape(shape)
    return out


def _polyPlanes(x, tabX, tabY, Ds, Dd):
    """Both passes and the quantiser on (C, h, w) integer codes; tabX / tabY = (off, coef) per output index.  The arithmetic of csrc/polyphase.h."""
    t = _polyAxis(x.astype(np.int64), tabX[0], tabX[1], 2)
    assert np.abs(t).max() < 1 << 31          # (summed in int64 here; the bound is what lets the device sum in int32)
    v = _polyAxis(t, tabY[0], tabY[1], 1)
    s = np.clip((v + (1 << 27)) >> 28, 0, (1 << Ds) - 1)
    s = s << (Dd - Ds) if Dd >= Ds else s >> (Ds - Dd)
    return s.astype(np.uint8 if Dd == 8 else np.dtype('<u2'))


def resampleChroma(C, srcFmt, dstFmt, scale, method, loc='center'):
    """C = the (2, h, w) codes of a frame's chroma planes at srcFmt's depth Ds (high bits are not masked) -> (2, h scale, w scale) codes at dstFmt's depth Dd, uint8
    for Dd = 8, else little-endian uint16.  Horizontal pass t = sum_j cx[p][j] code (fits int32 for any uint16 code: sum |c| <= 32767), vertical pass
    v = sum_i cy[p'][i] t_i, sample = clamp((v + 2^27) >> 28, 0, 2^Ds - 1), then << (Dd - Ds) or >> (Ds - Dd) -- what code 2^-Ds times 2^Dd, truncated, does to a code."""
    for fmt in (srcFmt, dstFmt):
        if fmt not in FORMATS:
            raise ValueError('pixFmt "{}" is not supported ({})'.format(fmt, ', '.join(FORMATS)))
    Ds, Dd = FORMATS[srcFmt], FORMATS[dstFmt]
    x = np.asarray(C)
    if x.ndim != 3 or x.shape[0] != 2 or x.dtype.kind not in 'ui':
        raise ValueError('resampleChroma: the (2, h, w) integer codes of Cb and Cr expected, got {} {}'.format(x.dtype, x.shape))

    def perOutput(n, off, coef):          # the phase tables as _polyAxis takes them: output o = q * scale + p reads from q + off[p] with coef[p]
        return [o // scale + off[o % scale] for o in range(n * scale)], [coef[o % scale] for o in range(n * scale)]
    return _polyPlanes(x, perOutput(x.shape[2], *chromaTable(method, scale, loc)), perOutput(x.shape[1], *chromaTable(method, scale, 'center')), Ds, Dd)


# ---- fitted sizes: a rational (any n -> m) integer polyphase filter -------------------------------------------------------------------------------
# A planar chain whose output step names a size ({'op': 'output', 'width': W, 'height': H, 'fit': 'bicubic'}) brings each plane from the size the chain gives to the
# size asked for -- what the device kernel (resize_kernel_fit, moe_fit_create / moe_fit_run) is held to, byte for byte.  The library builds no table of its own:
# fitTable is the only definition.
#
# One axis from n to m samples, s = n / m, f = max(1, s): the filter is stretched only when the axis shrinks (then it is the antialiasing filter).  Output o is
# centred on the source coordinate
#     'center'   c = ((2 o + 1) s - 1) / 2
#     'left'     c = o s                                 chroma co-sited with the even luma columns; the horizontal axis only
# nearest: one tap, off = floor(c + 1/2), coefficient 2^14, no stretch.  Otherwise R = 1 (bilinear: the triangle) or R = 2 (bicubic: chromaTable's cubic convolution,
# A = -3/4), taps i = floor(c - R f) + 1 .. ceil(c + R f) - 1 with w_i = k((i - c) / f) / sum_j w_j, coefficients floor(w_i 2^14 + 1/2), the deficit to exactly 2^14
# added to the tap of largest magnitude (the first of equals).  off[o] is the first tap, T the longest row of the axis (shorter rows end in zeros); tap j reads source
# index clamp(off[o] + j, 0, n - 1).  At n / m <= 4, T <= 8 (bilinear) and T <= 16 (bicubic) and sum |c| <= 22 522.  Everything in exact fractions.
FIT_MAX_DOWN, FIT_MAX_UP = 4, 16

_fitCache = {}


def _fitKernel(method):
    """(R, k): the kernel's support [-R, R] and the kernel -- bilinear: the triangle; bicubic: chromaTable's cubic convolution."""
    from fractions import Fraction as Fr
    return (1, lambda x: max(1 - abs(x), Fr(0))) if method == 'bilinear' else (2, _cubic)


def fitTable(method, n, m, loc='center'):
    """(off[m], coef[m][T]) of one axis resampled from n to m samples, as lists of Python ints; ValueError names what is refused."""
    from fractions import Fraction as Fr
    from math import ceil, floor, gcd
    if method not in CHROMA_METHODS:
        raise ValueError('fit "{}" is not supported ({})'.format(method, ', '.join(CHROMA_METHODS)))
    if loc not in CHROMA_LOCS:
        raise ValueError('fit: loc "{}" is not supported ({})'.format(loc, ', '.join(CHROMA_LOCS)))
    for v in (n, m):
        if not isinstance(v, int) or isinstance(v, bool) or v < 1:
            raise ValueError('fit: sizes must be positive ints, got {!r} -> {!r}'.format(n, m))
    if n > FIT_MAX_DOWN * m:
        raise ValueError('fit: {} -> {} shrinks by more than {}'.format(n, m, FIT_MAX_DOWN))
    if m > FIT_MAX_UP * n:
        raise ValueError('fit: {} -> {} enlarges by more than {}'.format(n, m, FIT_MAX_UP))
    key = (method, n, m, loc)
    if key not in _fitCache:
        s = Fr(n, m)
        f = max(Fr(1), s)
        g = gcd(n, m)
        period, step = m // g, n // g          # c(o + period) = c(o) + step: only `period` rows differ
        rows = []
        for o in range(min(m, period)):
            c = Fr(2 * o + 1) * s / 2 - Fr(1, 2) if loc == 'center' else o * s
            if method == 'nearest':
                rows.append((floor(c + Fr(1, 2)), [CHROMA_ONE]))
                continue
            R, k = _fitKernel(method)
            first, last = floor(c - R * f) + 1, ceil(c + R * f) - 1
            w = [k((i - c) / f) for i in range(first, last + 1)]
            tot = sum(w)
            rows.append((first, _quantRow([x / tot for x in w])))
        T = max(len(q) for _, q in rows)
        off = tuple(rows[o % period][0] + (o // period) * step for o in range(m))
        coef = tuple(tuple(rows[o % period][1]) + (0,) * (T - len(rows[o % period][1])) for o in range(m))
        if len(_fitCache) >= 64:
            _fitCache.clear()
        _fitCache[key] = (off, coef)
    off, coef = _fitCache[key]
    return list(off), [list(r) for r in coef]


def fitPlanes(P, srcDepth, dstDepth, oh, ow, method, loc='center'):
    """P = the (C, h, w) integer codes of C planes at depth srcDepth (high bits are not masked) -> (C, oh, ow) codes at dstDepth, uint8 for 8, else little-endian
    uint16.  resampleChroma's arithmetic to the letter: horizontal pass in int32 (`loc` sites this axis only), vertical pass in int64,
    sample = clamp((v + 2^27) >> 28, 0, 2^Ds - 1), then << (Dd - Ds) or >> (Ds - Dd)."""
    for d in (srcDepth, dstDepth):
        if d not in FORMATS.values():
            raise ValueError('fitPlanes: depth must be one of {}, got {!r}'.format(sorted(FORMATS.values()), d))
    x = np.asarray(P)
    if x.ndim != 3 or x.shape[0] < 1 or x.dtype.kind not in 'ui':
        raise ValueError('fitPlanes: the (C, h, w) integer codes of C planes expected, got {} {}'.format(x.dtype, x.shape))
    ox, cx = fitTable(method, int(x.shape[2]), ow, loc)
    oy, cy = fitTable(method, int(x.shape[1]), oh, 'center')
    return _polyPlanes(x, (ox, cx), (oy, cy), srcDepth, dstDepth)


def fitPixels(hwc, srcDepth, dstDepth, oh, ow, method):
    """hwc = the (h, w, C) integer codes of an interleaved image, C = 1 .. 4, at depth srcDepth -> (oh, ow, C) codes at dstDepth: fitPlanes on each channel, 'center'
    on both axes -- what the device kernel of interleaved images (resize_kernel_fit_px, moe_fit_create_px / moe_fit_run) is held to, byte for byte."""
    x = np.asarray(hwc)
    if x.ndim != 3 or not 1 <= x.shape[2] <= 4 or x.dtype.kind not in 'ui':
        raise ValueError('fitPixels: the (h, w, C) integer codes of an interleaved image of 1 to 4 channels expected, got {} {}'.format(x.dtype, x.shape))
    return np.ascontiguousarray(fitPlanes(x.transpose(2, 0, 1), srcDepth, dstDepth, oh, ow, method, 'center').transpose(1, 2, 0))


# ---- luma-guided chroma: a joint bilateral filter steered by the finished Y' --------------------------------------------------------------------
# The third form of a luma-only chain's chroma ('chroma': 'guided' on the source step; Kopf et al., Joint Bilateral Upsampling, 2007): a cubic B-spline over the same
# 4 x 4 source taps resampleChroma reads, each tap weighted once more by how close the source frame's luma AT THE TAP is to the output frame's luma AT THE SAMPLE --
# what the device kernel (resize_kernel_guided, moe_chroma_guided) is held to, byte for byte.  Integers only; the library builds no table of its own.
#
#     guide      a 16-bit luma value at chroma resolution.  'center': G = ((the sample's 2 x 2 luma block, summed) << (16 - D)) >> 2.  'left' (the horizontal axis is
#                co-sited): rows 2i, 2i + 1, columns 2j - 1, 2j, 2j + 1 clamped to the plane with weights (1, 2, 1), G = (sum << (16 - D)) >> 3.
#                GL from the source frame's Y' at depth Ds, GH from the OUTPUT frame's Y' at depth Dd, as the chain wrote it.
#     spatial    output index o = q * scale + p, r(p) as chromaTable has it (`loc` sites the horizontal axis only), f = r - floor(r), off = floor(r) - 1, the weights
#                ((1 - f)^3, 3 f^3 - 6 f^2 + 4, -3 f^3 + 3 f^2 + 3 f + 1, f^3) / 6 in exact fractions, each floor(w 2^8 + 1/2), the deficit to exactly 256 added to the
#                tap of largest magnitude (the first of equals).  All are >= 0.  Tap (i, j) reads the clamped source index, as _polyAxis does.
#     range      d = min(|GH[o] - GL[tap]| >> 10, 63),  R[d] = max(1, round(255 exp(-(1024 d)^2 / (2 2048^2)))) -- GUIDED_RANGE, literals: no libm in the definition.
#     sample     w = cy cx R < 2^24;  den = sum w over the 16 taps, 2^16 <= den < 2^24;  num = sum w code < 2^40;  s = (num + den // 2) // den, then << (Dd - Ds) or
#                >> (Ds - Dd) as resampleChroma does.  s is a convex combination of its taps: no clamp.  uint16 codes are taken as they are.
# Where luma is flat every R is equal and the filter is the B-spline alone: about bicubic's error on smooth colour, 1.4 - 1.6 times it on a colour edge that has no
# luma edge.
GUIDED_ONE = 1 << 8
GUIDED_RANGE = (255, 225, 155, 83, 35, 11, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)


def guidedRange():
    """The 64 range weights R[d], as a list of Python ints."""
    return list(GUIDED_RANGE)


def guidedTable(scale, loc='center'):
    """(off[scale], coef[scale][4]) of one axis of the guided filter's cubic B-spline, 8-bit coefficients that sum to 256; ValueError names what is refused."""
    from fractions import Fraction as Fr
    from math import floor
    if loc not in CHROMA_LOCS:
        raise ValueError('chromaLoc "{}" is not supported ({})'.format(loc, ', '.join(CHROMA_LOCS)))
    if not isinstance(scale, int) or isinstance(scale, bool) or not 2 <= scale <= 16:
        raise ValueError('guided chroma: scale must be 2..16, got {!r} (at scale 1 the filter would blur planes that need no resampling)'.format(scale))
    off, coef = [], []
    for p in range(scale):
        r = Fr(p, scale) if loc == 'left' else Fr(2 * p + 1 - scale, 2 * scale)
        f = r - floor(r)
        w = [(1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6, f ** 3 / 6]
        c = [floor(x * GUIDED_ONE + Fr(1, 2)) for x in w]
        c[max(range(4), key=lambda j: (abs(c[j]), -j))] += GUIDED_ONE - sum(c)
        off.append(floor(r) - 1)
        coef.append(c)
    return off, coef


def lumaGuide(Y, depth, loc='center'):
    """Y = the (2 h, 2 w) Y' codes of a frame at `depth` bits -> the (h, w) int64 guide at chroma resolution."""
    if depth not in FORMATS.values():
        raise ValueError('lumaGuide: depth must be one of {}, got {!r}'.format(sorted(FORMATS.values()), depth))
    if loc not in CHROMA_LOCS:
        raise ValueError('chromaLoc "{}" is not supported ({})'.format(loc, ', '.join(CHROMA_LOCS)))
    y = np.asarray(Y)
    if y.ndim != 2 or y.dtype.kind not in 'ui' or y.shape[0] < 2 or y.shape[1] < 2 or y.shape[0] % 2 or y.shape[1] % 2:
        raise ValueError('lumaGuide: the (2 h, 2 w) integer codes of a Y plane expected, got {} {}'.format(y.dtype, y.shape))
    y = y.astype(np.int64)
    rows = y[0::2] + y[1::2]
    if loc == 'center':
        return ((rows[:, 0::2] + rows[:, 1::2]) << (16 - depth)) >> 2
    n = y.shape[1]
    at = np.arange(0, n, 2)
    return ((rows[:, np.clip(at - 1, 0, n - 1)] + 2 * rows[:, at] + rows[:, np.clip(at + 1, 0, n - 1)]) << (16 - depth)) >> 3


def _guidedSums(C, GL, GH, scale, loc):
    """(num, den) of guidedChroma: int64 arrays of shape (2, h scale, w scale) and (h scale, w scale)."""
    _, h, w = C.shape
    (ox, cx), (oy, cy) = guidedTable(scale, loc), guidedTable(scale, 'center')
    R = np.asarray(GUIDED_RANGE, np.int64)
    Y, X = np.arange(h * scale), np.arange(w * scale)
    fy, fx = Y // scale + np.asarray(oy, np.int64)[Y % scale], X // scale + np.asarray(ox, np.int64)[X % scale]
    wy, wx = np.asarray(cy, np.int64)[Y % scale], np.asarray(cx, np.int64)[X % scale]
    num, den = np.zeros((2, h * scale, w * scale), np.int64), np.zeros((h * scale, w * scale), np.int64)
    for i in range(4):
        sy = np.clip(fy + i, 0, h - 1)[:, None]
        for j in range(4):
            sx = np.clip(fx + j, 0, w - 1)[None, :]
            wgt = wy[:, i][:, None] * wx[:, j][None, :] * R[np.minimum(np.abs(GH - GL[sy, sx]) >> 10, 63)]
            den += wgt
            num += wgt[None] * C[:, sy, sx]
    return num, den


def guidedChroma(C, Ys, Yo, srcFmt, dstFmt, scale, loc='center'):
    """C = the (2, h, w) chroma codes of the source frame at srcFmt's depth Ds, Ys = its (2 h, 2 w) Y' codes, Yo = the OUTPUT frame's (2 h scale, 2 w scale) Y' codes
    at dstFmt's depth Dd exactly as the chain wrote them -> the (2, h scale, w scale) chroma codes of the output frame at Dd, uint8 for Dd = 8, else little-endian
    uint16 (the definition above)."""
    for fmt in (srcFmt, dstFmt):
        if fmt not in FORMATS:
            raise ValueError('pixFmt "{}" is not supported ({})'.format(fmt, ', '.join(FORMATS)))
    Ds, Dd = FORMATS[srcFmt], FORMATS[dstFmt]
    guidedTable(scale, loc)          # (the refusals of scale and loc)
    x, ys, yo = np.asarray(C), np.asarray(Ys), np.asarray(Yo)
    if x.ndim != 3 or x.shape[0] != 2 or x.shape[1] < 1 or x.shape[2] < 1 or x.dtype.kind not in 'ui':
        raise ValueError('guidedChroma: the (2, h, w) integer codes of Cb and Cr expected, got {} {}'.format(x.dtype, x.shape))
    _, h, w = x.shape
    if ys.shape != (2 * h, 2 * w) or yo.shape != (2 * h * scale, 2 * w * scale):
        raise ValueError('guidedChroma: chroma planes of {} x {} at scale {} go with Y planes of {} and {}, got {} and {}'.format(
            w, h, scale, (2 * h, 2 * w), (2 * h * scale, 2 * w * scale), ys.shape, yo.shape))
    num, den = _guidedSums(x.astype(np.int64), lumaGuide(ys, Ds, loc), lumaGuide(yo, Dd, loc), scale, loc)
    assert den.min() >= 1 << 16 and den.max() < 1 << 24 and num.max() < 1 << 40
    s = (num + den // 2) // den
    s = s << (Dd - Ds) if Dd >= Ds else s >> (Ds - Dd)
    return s.astype(np.uint8 if Dd == 8 else np.dtype('<u2'))


# ---- RGB frames from a chain on 4:2:0 planes: the integer Y'CbCr -> RGB edge ---------------------------------------------------------------------
# A chain on the decoder's planes whose output step names an RGB pixFmt ({'op': 'output', 'pixFmt': 'bgr48le'}) hands back interleaved RGB samples -- what the device
# kernel (to_output_rgb420_kernel, moe_planes_to_rgb) is held to, byte for byte.  Integers only; the library builds no table and no constant of its own.
#
#     chroma     C' = resampleChroma(C, fmt, fmt, 2, method, loc): the filter, the table and the clamp to [0, 2^D - 1] defined above, at scale 2 (`loc` sites the
#                horizontal axis only).
#     offsets    y = Y - (16 << (D - 8)),  u = Cb' - (128 << (D - 8)),  v = Cr' - (128 << (D - 8)).  Y codes as they are: high bits are not masked.
#     matrix     the standard's inverse, (Kr, Kb) = LUMA[matrix], Kg = 1 - Kr - Kb, in units of 2^(D - 8):
#                    E_R = y / 219 + 2 (1 - Kr) v / 224      E_B = y / 219 + 2 (1 - Kb) u / 224      E_G = y / 219 - (Kr 2 (1 - Kr) v + Kb 2 (1 - Kb) u) / (Kg 224)
#                times the sample scale S: 2^16 for 16-bit samples (the inverse of how fromSamples16 reads them), 255 for 8-bit ones (the inverse of the reader's / 255,
#                quant.py's `unit`).  As constants with F = RGB_FRAC = 20 fractional bits, each round(x 2^F) of an exact fraction (rgbCoefficients):
#                    cY = S / (219 2^(D-8))    cRV = S 2 (1 - Kr) / (224 2^(D-8))    cBU = S 2 (1 - Kb) / (224 2^(D-8))
#                    cGU = -S Kb 2 (1 - Kb) / (Kg 224 2^(D-8))                       cGV = -S Kr 2 (1 - Kr) / (Kg 224 2^(D-8))
#     sample     int64:  R = (cY y + cRV v + r) >> F,  G = (cY y + cGU u + cGV v + r) >> F,  B = (cY y + cBU u + r) >> F  (>> an arithmetic shift), clamped to
#                [0, 2^bits - 1].  r = 1 << (F - 1): round to nearest; dither 'ordered': r = T << (F - 7) with quant.threshold's T at the pixel's coordinates, one
#                threshold for the three channels of a pixel.  None / 'none' / 'round' give the same bytes (the stance of quant.yuvFromSamples16).
# F = 20: the largest constant (cBU of bt2020nc at D = 8, S = 2^16: 550.4) stays below 2^30, so every constant is an int32 and, with |y|, |u|, |v| < 2^16, the three
# products and r stay below 2^49.  A constant is off by 2^-(F+1) at most, so before the clamp a sample differs from the exact S E by at most
# 1/2 + (|y| + |u| + |v|) 2^-(F+1) <= 1/2 + 3 * 65535 * 2^-21 < 0.594.
RGB_FORMATS = {'bgr24': (8, 'bgr'), 'rgb24': (8, 'rgb'), 'bgr48le': (16, 'bgr'), 'rgb48le': (16, 'rgb')}      # pix_fmt -> (bits, order)
RGB_FRAC = 20


def rgbCoefficients(matrix, D, bits):
    """(cY, cRV, cGU, cGV, cBU) of a matrix for sources at depth D and samples of `bits` bits, as Python ints with RGB_FRAC fractional bits."""
    from fractions import Fraction as Fr
    from math import floor
    if matrix not in MATRICES:
        raise ValueError('matrix "{}" is not supported ({})'.format(matrix, ', '.join(MATRICES)))
    if D not in FORMATS.values():
        raise ValueError('rgbCoefficients: depth must be one of {}, got {!r}'.format(sorted(FORMATS.values()), D))
    if bits not in (8, 16):
        raise ValueError('rgbCoefficients: bits must be 8 or 16, got {!r}'.format(bits))
    kr, kb = (Fr(str(k)) for k in LUMA[matrix])          # (the decimal constants of the standards, exactly)
    kg = 1 - kr - kb
    S = Fr(255 if bits == 8 else 1 << 16, 1 << (D - 8))
    q = lambda x: floor(x * (1 << RGB_FRAC) + Fr(1, 2))
    er, eb = 2 * (1 - kr), 2 * (1 - kb)
    return q(S / 219), q(S * er / 224), -q(S * kb * eb / (kg * 224)), -q(S * kr * er / (kg * 224)), q(S * eb / 224)


def toRGB(frame_bytes, fmt, w, h, rgbFmt, matrix='bt709', method='bicubic', loc='center', dither=None):
    """The bytes of a planar frame of w x h at fmt -> the bytes of the interleaved h x w x 3 frame at rgbFmt (the definition above)."""
    from . import quant
    if rgbFmt not in RGB_FORMATS:
        raise ValueError('pixFmt "{}" is not an RGB format ({})'.format(rgbFmt, ', '.join(RGB_FORMATS)))
    (yh, yw), (ch, cw) = planeShapes(fmt, w, h)
    D = FORMATS[fmt]
    bits, order = RGB_FORMATS[rgbFmt]
    cY, cRV, cGU, cGV, cBU = rgbCoefficients(matrix, D, bits)
    mode = quant._mode(dither)
    end = frameBytes(fmt, w, h)
    if len(frame_bytes) != end:
        raise ValueError('toRGB: a {} frame of {} x {} is {} bytes, got {}'.format(fmt, w, h, end, len(frame_bytes)))
    codes = np.frombuffer(frame_bytes, np.uint8 if D == 8 else np.dtype('<u2'))
    C = resampleChroma(codes[yh * yw:].reshape(2, ch, cw), fmt, fmt, 2, method, loc).astype(np.int64)
    y = codes[:yh * yw].reshape(yh, yw).astype(np.int64) - (16 << (D - 8))
    u, v = C[0] - (128 << (D - 8)), C[1] - (128 << (D - 8))
    r = quant.threshold('round' if mode == 'none' else mode, yh, yw) << (RGB_FRAC - 7)
    base = cY * y + r
    top = (1 << bits) - 1
    R, G, B = (np.clip(a >> RGB_FRAC, 0, top) for a in (base + cRV * v, base + cGU * u + cGV * v, base + cBU * u))
    out = np.stack((R, G, B) if order == 'rgb' else (B, G, R), axis=2)
    return out.astype(np.uint8 if bits == 8 else np.dtype('<u2')).tobytes()
