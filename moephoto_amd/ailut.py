"""The AiLUT generator net, written down (numpy float64, on no hot path): the small net of the reference's "Retouch" that looks at a 256 x 256 thumbnail of a frame
and writes the frame's own 3D table and vertices (python/AiLUT.py: AiLUT.forward up to ailut_transform; the AiLUT_sRGB_3 / AiLUT_XYZ_3 rows of
python/dehaze.py:27-28).  It is the `tpami` backbone with extra_pooling, the LUT generator h and the interval generator g, from the modules' arithmetic:

  thumbnail  F.interpolate(.., (256, 256), 'bilinear', align_corners=False), no antialiasing, with integer source coordinates
  generate   five blocks Conv2d(3 x 3, stride 2, padding 1) -> LeakyReLU(0.2) -> InstanceNorm2d(affine; blocks 1 - 4 only), channels 3 -> 16 -> 32 -> 64 -> 128
             -> 128; Dropout is the identity; AdaptiveAvgPool2d(2) on the 8 x 8 map; the 512 features in the order c 4 + y 2 + x; the table = bank (W_h0 f + b_h0)
             as (3, d, d, d) -- the layout lut3d.check takes --; the vertices = [0, cumsum(softmax(W_g f + b_g))] per channel (Share-AdaInt is off)
  loadParams the reference's state-dict keys, checked

The device (moe_ailut_run, csrc/ailut.hip) computes the same in fp32; tests/test_gpu_ailut.py holds it to this file within four times the error of a float32 torch
forward of the same graph.  The reference runs the net under fp16 autocast; neither this file nor the device does.
"""
from collections import OrderedDict

import numpy as np

SIZE = 256                      # the thumbnail's side
CHANNELS = (3, 16, 32, 64, 128, 128)
SLOPE, EPS = 0.2, 1e-5
FEATURES = 512                  # 128 channels x 2 x 2 means
RANKS = (1, 8)
D = (2, 65)                     # lut3d.check's range
MODELS = {'AiLUT_sRGB_3': './model/AiLUT/AiLUT-FiveK-sRGB.pth', 'AiLUT_XYZ_3': './model/AiLUT/AiLUT-FiveK-XYZ.pth'}          # python/dehaze.py:27-28
NOT_HERE = {'AiLUT_sRGB_5': 'the res18 backbone is not in this change'}                                                          # python/dehaze.py:29
KEY_H0, KEY_BANK, KEY_G = 'lut_generator.weights_generator', 'lut_generator.basis_luts_bank', 'adaint.intervals_generator'


def axis(n, size=SIZE):
    """(i0, i1, frac) of the `size` outputs along an axis of n samples: num = (2 j + 1) n - size, a negative one 0; i0 = num // (2 size), frac = num % (2 size) /
    (2 size), i1 = min(i0 + 1, n - 1).  Integers: the device computes the same ones.  At n = size frac is 0 and i0 = j."""
    j = np.arange(size, dtype=np.int64)
    num = np.maximum((2 * j + 1) * int(n) - size, 0)
    i0 = num // (2 * size)
    return i0, np.minimum(i0 + 1, n - 1), (num % (2 * size)) / float(2 * size)


def thumbnail(samples, srcBits=16, order='bgr'):
    """(3, 256, 256) float64 RGB planes of an (H, W, 3) image of codes: x = code 2^-16 at 16 bits, code / 255 at 8; bilinear between the four neighbours."""
    a = np.asarray(samples)
    if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError('ailut: thumbnail takes an (H, W, 3) image, got shape {}'.format(a.shape))
    if srcBits not in (8, 16):
        raise ValueError('ailut: srcBits must be 8 or 16, got {!r}'.format(srcBits))
    if order not in ('bgr', 'rgb'):
        raise ValueError("ailut: 'order' {!r} is not supported (bgr, rgb)".format(order))
    x = a.astype(np.float64) / (65536.0 if srcBits == 16 else 255.0)
    if order == 'bgr':
        x = x[:, :, ::-1]
    y0, y1, fy = axis(a.shape[0])
    x0, x1, fx = axis(a.shape[1])
    top = x[y0][:, x0] + fx[None, :, None] * (x[y0][:, x1] - x[y0][:, x0])
    bot = x[y1][:, x0] + fx[None, :, None] * (x[y1][:, x1] - x[y1][:, x0])
    return np.ascontiguousarray((top + fy[:, None, None] * (bot - top)).transpose(2, 0, 1))


def conv(x, w, b):
    """Conv2d(3 x 3, stride 2, padding 1) on (C, H, W) with even H, W."""
    C, H, W = x.shape
    p = np.zeros((C, H + 2, W + 2), x.dtype)
    p[:, 1:-1, 1:-1] = x
    cols = np.stack([p[:, ky:ky + H:2, kx:kx + W:2] for ky in range(3) for kx in range(3)], 1)          # (C, 9, H / 2, W / 2)
    return np.tensordot(w.reshape(w.shape[0], -1), cols.reshape(C * 9, H // 2, W // 2), 1) + b[:, None, None]


def features(thumb, params, dtype=np.float64):
    """The 512 pooled features of a thumbnail, in the order c 4 + y 2 + x."""
    x = np.asarray(thumb, dtype)
    if x.shape != (3, SIZE, SIZE):
        raise ValueError('ailut: the thumbnail is (3, {0}, {0}), got shape {1}'.format(SIZE, x.shape))
    for i in range(5):
        x = conv(x, params['backbone.{}.0.weight'.format(i)].astype(dtype), params['backbone.{}.0.bias'.format(i)].astype(dtype))
        x = np.where(x >= 0, x, x * dtype(SLOPE))
        if i < 4:          # the norm comes after the activation; biased variance
            mu, var = x.mean((1, 2), keepdims=True), x.var((1, 2), keepdims=True)
            x = (x - mu) / np.sqrt(var + dtype(EPS)) * params['backbone.{}.2.weight'.format(i)].astype(dtype)[:, None, None] + params['backbone.{}.2.bias'.format(i)].astype(dtype)[:, None, None]
    return x.reshape(128, 2, 4, 2, 4).mean((2, 4)).reshape(FEATURES)


def heads(f, params, dtype=np.float64):
    """(table, vertices) of the 512 features."""
    d = params['d']
    w = params[KEY_H0 + '.weight'].astype(dtype) @ f + params[KEY_H0 + '.bias'].astype(dtype)
    table = (params[KEY_BANK + '.weight'].astype(dtype) @ w).reshape(3, d, d, d)
    z = (params[KEY_G + '.weight'].astype(dtype) @ f + params[KEY_G + '.bias'].astype(dtype)).reshape(3, d - 1)
    e = np.exp(z - z.max(1, keepdims=True))
    intervals = e / e.sum(1, keepdims=True)
    vertices = np.zeros((3, d), dtype)
    for j in range(d - 1):          # a sequential sum of non-negative terms: it cannot decrease, in any precision
        vertices[:, j + 1] = vertices[:, j] + intervals[:, j]
    return table, vertices


def generate(thumb, params):
    """(table (3, d, d, d), vertices (3, d)), float64, of a thumbnail and loadParams' dict."""
    return heads(features(thumb, params), params)


def paramShapes(d, ranks):
    """OrderedDict name -> shape of the state dict of a generator with d vertices and `ranks` basis tables, in the reference's order."""
    s = OrderedDict()
    for i in range(5):
        s['backbone.{}.0.weight'.format(i)] = (CHANNELS[i + 1], CHANNELS[i], 3, 3)
        s['backbone.{}.0.bias'.format(i)] = (CHANNELS[i + 1],)
        if i < 4:
            s['backbone.{}.2.weight'.format(i)] = (CHANNELS[i + 1],)
            s['backbone.{}.2.bias'.format(i)] = (CHANNELS[i + 1],)
    s[KEY_H0 + '.weight'], s[KEY_H0 + '.bias'] = (ranks, FEATURES), (ranks,)
    s[KEY_BANK + '.weight'] = (3 * d ** 3, ranks)
    s[KEY_G + '.weight'], s[KEY_G + '.bias'] = (3 * (d - 1), FEATURES), (3 * (d - 1),)
    return s


def loadParams(state_dict):
    """dict name -> float32 array (plus 'd' and 'ranks') of a state dict with the reference's key names.  n_ranks (1 .. 8) and d (2 .. 65) come from the shapes of
    lut_generator.weights_generator.weight and adaint.intervals_generator.weight.  ValueError naming the key: a missing key, a wrong shape, a value that is not
    finite, a basis_luts_bank whose row count is not 3 d^3 (and so a Share-AdaInt checkpoint, whose intervals generator has d - 1 rows for a bank of 3 d^3)."""
    def get(key):
        if key not in state_dict:
            raise ValueError("ailut: the state dict has no '{}'".format(key))
        return np.asarray(state_dict[key])
    h0, g = get(KEY_H0 + '.weight'), get(KEY_G + '.weight')
    if h0.ndim != 2 or h0.shape[1] != FEATURES or not RANKS[0] <= h0.shape[0] <= RANKS[1]:
        raise ValueError("ailut: '{}.weight' has shape {}, expected (n_ranks, {}) with n_ranks {} .. {}".format(KEY_H0, h0.shape, FEATURES, *RANKS))
    if g.ndim != 2 or g.shape[1] != FEATURES or g.shape[0] % 3 or not D[0] <= g.shape[0] // 3 + 1 <= D[1]:
        raise ValueError("ailut: '{}.weight' has shape {}, expected (3 (d - 1), {}) with d {} .. {}".format(KEY_G, g.shape, FEATURES, *D))
    ranks, d = int(h0.shape[0]), int(g.shape[0]) // 3 + 1
    bank = get(KEY_BANK + '.weight')
    if bank.ndim != 2 or bank.shape[0] != 3 * d ** 3:
        raise ValueError("ailut: '{}.weight' has {} rows, expected 3 d^3 = {} for the d = {} of '{}.weight'".format(
            KEY_BANK, bank.shape[0] if bank.ndim else 0, 3 * d ** 3, d, KEY_G))
    out = {}
    for key, shape in paramShapes(d, ranks).items():
        a = get(key)
        if tuple(a.shape) != shape:
            raise ValueError("ailut: '{}' has shape {}, expected {}".format(key, tuple(a.shape), shape))
        a = np.ascontiguousarray(a, np.float32)
        if not np.isfinite(a).all():
            raise ValueError("ailut: '{}' holds a value that is not finite".format(key))
        out[key] = a
    out['d'], out['ranks'] = d, ranks
    return out
