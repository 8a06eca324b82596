"""Luma-only SR / DN steps on RGB images: the definition the device kernels (to_float_luma_kernel, to_output_luma_kernel, stitch_luma_kernel) are held to, in numpy.

None of the zoo's SR / DN nets convolves planes jointly -- they were trained on single planes and planes are the batch (python/runSR.py:37-40) -- so a colour image does
not need three passes through the net: the step runs on Y' alone while Cb / Cr go to the output's size through the existing resize.  The reference has no counterpart
(it sends every plane through the net); this module is the written specification and the comparator of the tests, and is on no hot path.

Full range, no offset: Y' in [0, 1] and Cb, Cr in [-1/2, 1/2] for colours in [0, 1].  With (kr, kb) = pixfmt.LUMA[matrix] the constants are

    kr   kg = 1 - kr - kb   kb        ib = 1 / (2 (1 - kb))   ir = 1 / (2 (1 - kr))        eb = 2 (1 - kb)   er = 2 (1 - kr)        gr = kr er / kg   gb = kb eb / kg

each computed in Python floats and rounded once to float32.  All arithmetic below is float32; every product and every sum is rounded separately, in the order written
(no FMA).  T is the image's dtype, float16 or float32.

    split    y = (kr r + kg g) + kb b        cb = (b - y) ib        cr = (r - y) ir         Y = T(y); cb / cr from the unrounded y; C = (cb, cr) is always float32
    merge    y' = fp32(T(Y'))                r' = y' + er cr'       b' = y' + eb cb'        g' = y' - (gr cr' + gb cb')        each rounded to T

NaN and the infinities follow IEEE 754, which leaves a NaN's sign and payload open: the device's merge emits the one quiet NaN of T for every NaN (so that its fused
and unfused forms agree byte for byte), numpy hands on whichever its host produces, and the tests compare NaN against NaN.

A fourth plane (alpha) rides as Y's second plane, as the reference's SR path sends it through the net, and comes back behind the colour planes unchanged.

A luma-only STEP on an image x:  Y, C = lumaSplit(x);  Y' = the step on Y (doCrop, the ensemble, or the DN step's blend s Y' + (1 - s) Y);  C' = C resized to Y' 's size
by the existing resize on float32 with the method the step's 'chroma' key names (no resize at scale 1);  lumaMerge(Y', C')."""
import numpy as np

from .pixfmt import LUMA, MATRICES, ORDERS

METHODS = ('nearest', 'bilinear', 'bicubic')          # what a step's 'chroma' key may name besides 'net'
_NAMES = ('kr', 'kg', 'kb', 'ib', 'ir', 'eb', 'er', 'gr', 'gb')


def lumaCoefficients(matrix):
    """dict of the nine float32 constants of a matrix ('bt709', 'bt601', 'bt2020nc')."""
    if matrix not in LUMA:
        raise ValueError('chromaMatrix "{}" is not supported ({})'.format(matrix, ', '.join(MATRICES)))
    kr, kb = LUMA[matrix]
    kg = 1 - kr - kb
    eb, er = 2 * (1 - kb), 2 * (1 - kr)
    vals = (kr, kg, kb, 1 / eb, 1 / er, eb, er, kr * er / kg, kb * eb / kg)
    return {n: np.float32(v) for n, v in zip(_NAMES, vals)}


def _order(order):
    if order not in ORDERS:
        raise ValueError('order "{}" is not supported ({})'.format(order, ', '.join(ORDERS)))
    return (0, 1, 2) if order == 'rgb' else (2, 1, 0)          # the planes of red, green, blue


def _image(x, what, planes):
    x = np.asarray(x)
    if x.dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise ValueError('{}: dtype must be float32 or float16, got {}'.format(what, x.dtype))
    if x.ndim != 3 or x.shape[0] not in planes:
        raise ValueError('{}: an image of {} planes expected, got shape {}'.format(what, ' or '.join(str(p) for p in planes), x.shape))
    return x


def lumaSplit(x, matrix='bt709', order='rgb'):
    """x (3 | 4, H, W) of float16 / float32 -> Y (1 | 2, H, W) of x's dtype and C (2, H, W) float32."""
    x = _image(x, 'lumaSplit', (3, 4))
    k, (pr, pg, pb) = lumaCoefficients(matrix), _order(order)
    with np.errstate(all='ignore'):
        r, g, b = (x[p].astype(np.float32) for p in (pr, pg, pb))
        y = (k['kr'] * r + k['kg'] * g) + k['kb'] * b
        cb = (b - y) * k['ib']
        cr = (r - y) * k['ir']
        Y = y.astype(x.dtype)[None]
    if x.shape[0] == 4:
        Y = np.concatenate([Y, x[3:4]], 0)
    return Y, np.stack([cb, cr]).astype(np.float32)


def quantise(v, bits):
    """moe_to_output's quantiser on float32 values: v * 2^bits, clamped to [0, 2^bits - 1], truncated, NaN = 0 -> uint8 / uint16."""
    if bits not in (8, 16):
        raise ValueError('bits must be 8 or 16, got {!r}'.format(bits))
    q = np.float32(1 << bits)
    with np.errstate(all='ignore'):
        v = np.fmin(np.fmax(np.asarray(v, np.float32) * q, np.float32(0)), q - np.float32(1))
    v = np.where(np.isnan(v), np.float32(0), v)
    return v.astype(np.int32).astype(np.uint8 if bits == 8 else np.uint16)


def lumaMerge(Y, C, matrix='bt709', order='rgb', bits=None):
    """Y (1 | 2, H, W) of T, C (2, H, W) float32 -> the canvas (3 | 4, H, W) of T, or with bits 8 | 16 the interleaved (H, W, 3 | 4) samples: each value rounded to T
    first, then through `quantise`."""
    Y = _image(Y, 'lumaMerge', (1, 2))
    C = np.asarray(C)
    if C.dtype != np.float32 or C.shape != (2,) + Y.shape[1:]:
        raise ValueError('lumaMerge: C must be float32 of shape {}, got {} {}'.format((2,) + Y.shape[1:], C.dtype, C.shape))
    k, (pr, pg, pb) = lumaCoefficients(matrix), _order(order)
    with np.errstate(all='ignore'):
        y, cb, cr = Y[0].astype(np.float32), C[0], C[1]
        planes = [None] * 3
        planes[pr] = y + k['er'] * cr
        planes[pb] = y + k['eb'] * cb
        planes[pg] = y - (k['gr'] * cr + k['gb'] * cb)
        out = np.stack(planes).astype(Y.dtype)
    if Y.shape[0] == 2:
        out = np.concatenate([out, Y[1:2]], 0)
    if bits is None:
        return out
    return np.ascontiguousarray(quantise(out.astype(np.float32), bits).transpose(1, 2, 0))
