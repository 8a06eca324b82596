"""The encoder's planar Y'CbCr 4:2:0 frames: the definition the device kernels (stitch_yuv_kernel, to_output_yuv_kernel) are held to, in numpy.  (Below it, the
definition of chains that run on such planes as they come from the decoder, with no conversion at all: planeShapes, toPlanes, fromPlanes.)

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
