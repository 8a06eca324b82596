"""Rounding and ordered dither in the quantising edges: the definition the device kernels (quant.h's quant_sample and every kernel that calls it, the two Y'CbCr
kernels) are held to, in numpy.  It is on no hot path; it is the comparator of the tests, as pixfmt.py and luma.py are.

Every edge that turns a float into an 8-, 10-, 12- or 16-bit sample truncates by default, as the reference does (python/imageProcess.py:245-257: v * 2^bits, clamp,
truncate).  At 8 bits that shows: exact codes read as code / 255 do not survive an fp16 canvas, a value halfway between two codes goes down at low levels and up at high
ones, and a smooth ramp bands.  The opt-in modes here replace the truncation's implicit threshold:

    T(mode, y, x)    'round' -> 64        'ordered' -> 2 B8[y & 7][x & 7] + 1  (odd, 1 .. 127)        d = T / 128, exact in float32

with B8 the 8 x 8 Bayer matrix (bayer8: the recursion B2 = [[0, 2], [3, 1]], B2n = [[4B, 4B + 2], [4B + 3, 4B + 1]]; a permutation of 0 .. 63).  x and y are the sample's
coordinates in the plane or image being written: the interleaved channels of a pixel share one threshold, a chroma sample uses its chroma-plane coordinates.

The float edges (quantise): v as the canvas dtype holds it, widened to float32;  t = fl32(v S);  u = fl32(t + d);  clamp to [0, 2^bits - 1], NaN = 0, truncate.  S is 2^bits, or
2^bits - 1 with `unit` -- the inverse of the 8-bit RGB reader's code / 255.  The product and the sum are rounded separately (with S = 255 an FMA gives other bits).  Mode
'none' is today's expression untouched: it adds nothing and has no unit scale.

The integer Y'CbCr edge (yuvFromSamples16): pixfmt.fromSamples16 with its two rounding constants replaced -- luma 1 << (37 - D) -> T << (31 - D), chroma 1 << (39 - D) ->
T << (33 - D) -- so 'round' (T = 64) is today's frame, byte for byte, and 'none' means the same."""
import numpy as np

from . import pixfmt

MODES = ('none', 'round', 'ordered')
Q_ROUND, Q_ORDERED, Q_UNIT = 0x100, 0x200, 0x400          # MOE_Q_ROUND, MOE_Q_ORDERED, MOE_Q_UNIT (include/moephoto_amd.h)


def bayer8():
    """The 8 x 8 Bayer matrix as int64, by the recursion."""
    b = np.array([[0, 2], [3, 1]], np.int64)
    while b.shape[0] < 8:
        b = np.block([[4 * b, 4 * b + 2], [4 * b + 3, 4 * b + 1]])
    return b


def bayer8Closed(y, x):
    """The same matrix in closed form (what the kernels compute): sum over i < 3 of ((x_i ^ y_i) << (2 (2 - i) + 1)) | (y_i << (2 (2 - i))), x_i = bit i of x & 7."""
    y, x = np.asarray(y, np.int64) & 7, np.asarray(x, np.int64) & 7
    b = np.zeros(np.broadcast(y, x).shape, np.int64)
    for i in range(3):
        xi, yi = (x >> i) & 1, (y >> i) & 1
        b = b + (((xi ^ yi) << (2 * (2 - i) + 1)) | (yi << (2 * (2 - i))))
    return b


def _mode(mode):
    mode = 'none' if mode is None else mode
    if mode not in MODES:
        raise ValueError('dither "{}" is not supported ({})'.format(mode, ', '.join(MODES)))
    return mode


def threshold(mode, h, w):
    """The numerators T over a plane of h x w, int64: 64 everywhere for 'round', 2 B8[y & 7][x & 7] + 1 for 'ordered'."""
    mode = _mode(mode)
    if mode == 'none':
        raise ValueError("dither 'none' has no threshold (it truncates)")
    if mode == 'round':
        return np.full((h, w), 64, np.int64)
    return 2 * bayer8()[np.arange(h)[:, None] & 7, np.arange(w)[None, :] & 7] + 1


def flags(mode, bits, kind):
    """The MOE_Q_* flags an edge ORs into its bits / depth argument.  kind: 'rgb' -- interleaved RGB samples: 8 bits take the unit scale (their reader is code / 255),
    16 bits do not (code / 65536); 'planes' -- planar samples at any depth: no unit scale (their reader is code 2^-D); 'yuv' -- the integer Y'CbCr edge: none either."""
    mode = _mode(mode)
    if kind not in ('rgb', 'planes', 'yuv'):
        raise ValueError('unknown edge kind {!r}'.format(kind))
    if mode == 'none':
        return 0
    return (Q_ROUND if mode == 'round' else Q_ORDERED) | (Q_UNIT if kind == 'rgb' and bits == 8 else 0)


def quantise(v, bits, mode='none', unit=False):
    """v: float16 / float32 values whose LAST TWO axes are the plane's (rows, columns) -- (H, W) or (C, H, W); every leading index shares the thresholds.  -> uint8 (bits
    <= 8) / uint16 codes of the same shape."""
    mode = _mode(mode)
    v = np.asarray(v)
    if v.dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise ValueError('quantise: dtype must be float32 or float16, got {}'.format(v.dtype))
    if not isinstance(bits, int) or not 1 <= bits <= 16:
        raise ValueError('quantise: bits must be 1 .. 16, got {!r}'.format(bits))
    if v.ndim < 2:
        raise ValueError('quantise: at least (H, W) expected, got shape {}'.format(v.shape))
    if mode == 'none' and unit:
        raise ValueError("quantise: 'unit' needs a mode (the truncating quantiser has no unit scale)")
    top = np.float32((1 << bits) - 1)
    S = top if unit else np.float32(1 << bits)
    with np.errstate(all='ignore'):
        t = v.astype(np.float32) * S                                                     # fl32(v S)
        if mode != 'none':
            d = threshold(mode, v.shape[-2], v.shape[-1]).astype(np.float32) / np.float32(128)
            t = t + d                                                                    # fl32(t + d): numpy rounds each operation separately
        t = np.fmin(np.fmax(t, np.float32(0)), top)                                      # (fmaxf / fminf: a NaN gives way to the bound)
    t = np.where(np.isnan(t), np.float32(0), t)
    return t.astype(np.int64).astype(np.uint8 if bits <= 8 else np.uint16)


def quantiseHWC(chw, bits, mode='none', unit=False):
    """(C, H, W) -> the interleaved (H, W, C) samples of moe_to_output / moe_stitch_out."""
    return np.ascontiguousarray(quantise(chw, bits, mode, unit).transpose(1, 2, 0))


def yuvFromSamples16(hwc, fmt, matrix='bt709', order='bgr', mode='none'):
    """(H, W, 3) uint16 samples -> the frame's bytes: pixfmt.fromSamples16 with thresholds for its rounding constants ('none' and 'round': the same frame)."""
    mode = _mode(mode)
    D = pixfmt.check(fmt, matrix, order)[0]
    a = np.asarray(hwc)
    if a.dtype != np.uint16 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError('yuvFromSamples16: an (H, W, 3) uint16 array expected, got {} {}'.format(a.dtype, a.shape))
    a = a.astype(np.int64)
    H, W = a.shape[:2]
    mode = 'round' if mode == 'none' else mode
    r, g, b = (a[:, :, 2], a[:, :, 1], a[:, :, 0]) if order == 'bgr' else (a[:, :, 0], a[:, :, 1], a[:, :, 2])
    (cR, cG, cB), urow, vrow = pixfmt.coefficients(matrix)
    Y = (16 << (D - 8)) + (((cR * r + cG * g + cB * b) * 219 + (threshold(mode, H, W) << (31 - D))) >> (38 - D))

    def sums(p):          # the 2 x 2 block sums, the edge pixel repeated
        p = np.pad(p, ((0, H % 2), (0, W % 2)), mode='edge')
        return p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    sr, sg, sb = sums(r), sums(g), sums(b)
    Tc = threshold(mode, (H + 1) // 2, (W + 1) // 2) << (33 - D)
    chroma = lambda k: (128 << (D - 8)) + (((k[0] * sr + k[1] * sg + k[2] * sb) * 224 + Tc) >> (40 - D))
    dt = np.uint8 if D == 8 else np.dtype('<u2')
    return b''.join(np.ascontiguousarray(p).astype(dt).tobytes() for p in (Y, chroma(urow), chroma(vrow)))
