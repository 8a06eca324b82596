"""The 3D LUT colour step: the definition the device kernel (to_output_lut3d_kernel, csrc/lut3d.hip; moe_lut3d_run) is held to, in numpy.  It is on no hot path; it is
the comparator of the tests, as pixfmt.py, luma.py and quant.py are.

The transform is the reference's AiLUT op (site-packages/ailut/csrc/ailut_transform_cpu.cpp:20-113; its CUDA twin ailut_transform_cuda.cu): a per-pixel trilinear
lookup in a 3D table whose lattice has non-uniform ("adaptive") intervals, one row of d vertices per input channel.

    table       float32 (3, d, d, d), 2 <= d <= 65, indexed [c, b, g, r] -- red varies fastest: the reference's luts[0], flat index c d^3 + b d^2 + g d + r
    vertices    float32 (3, d), non-decreasing per row, finite: the reference's vertices[0]

Per pixel (r, g, b), every operation rounded to float32 on its own (no fused multiply-add), in the reference's order:

    i_c = clamp(lower_bound(v_c, x_c) - 1, 0, d - 2)             lower_bound: the first i with v_c[i] >= x_c (ailut_transform_cpu.cpp:20-40)
    t_c = (x_c - v_c[i]) / ((v_c[i + 1] - v_c[i]) + 1e-10f)      (:84-93)  a zero-width interval divides by 1e-10f: finite
    w000 = ((1 - t_r) (1 - t_g)) (1 - t_b)   w100 = (t_r (1 - t_g)) (1 - t_b)   ..   w111 = (t_r t_g) t_b          (:95-102)
    y_k = ((((((w000 L000 + w100 L100) + w010 L010) + w110 L110) + w001 L001) + w101 L101) + w011 L011) + w111 L111        (:105-111), L_rgb = table[k, i_b + b, i_g + g, i_r + r]

Values outside [v[0], v[d - 1]] extrapolate with the clamped index, as the reference does.  A NaN input takes index 0 and yields NaN; the quantiser turns NaN into 0.

apply() is the whole edge on samples: the chain's readers (code 2^-16 for 16-bit samples, code / 255 for 8-bit ones), the transform, RGBFilter's strength blend
 and quant.quantise with the thresholds at the pixel's coordinates.  A .cube file (parseCube) gives a table with uniform vertices."""
import numpy as np

from . import quant

D_MIN, D_MAX = 2, 65
EPS = np.float32(1e-10)
ORDERS = ('bgr', 'rgb')


def check(table, vertices):
    """(table, vertices) as contiguous float32 arrays, or ValueError naming what is wrong."""
    t, v = np.asarray(table), np.asarray(vertices)
    if t.dtype != np.float32 or v.dtype != np.float32:
        raise ValueError('lut: table and vertices must be float32, got {} and {}'.format(t.dtype, v.dtype))
    if t.ndim != 4 or t.shape[0] != 3 or not (t.shape[1] == t.shape[2] == t.shape[3]):
        raise ValueError("lut: 'table' must have the shape (3, d, d, d), got {}".format(t.shape))
    d = t.shape[1]
    if not D_MIN <= d <= D_MAX:
        raise ValueError("lut: 'table' has d = {} ({} to {})".format(d, D_MIN, D_MAX))
    if v.shape != (3, d):
        raise ValueError("lut: 'vertices' must have the shape (3, {}), got {}".format(d, v.shape))
    if not np.isfinite(t).all():
        raise ValueError("lut: 'table' holds a value that is not finite")
    if not np.isfinite(v).all():
        raise ValueError("lut: 'vertices' holds a value that is not finite")
    if (np.diff(v, axis=1) < 0).any():
        raise ValueError("lut: 'vertices' must not decrease along a row")
    return np.ascontiguousarray(t), np.ascontiguousarray(v)


def uniform(d, lo=0.0, hi=1.0):
    """The (3, d) vertices fl32(lo + (hi - lo) i / (d - 1)); lo / hi: a number or one per channel."""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), (3,)), np.broadcast_to(np.asarray(hi, np.float64), (3,))
    i = np.arange(d, dtype=np.float64)
    return np.ascontiguousarray((lo[:, None] + (hi - lo)[:, None] * i[None, :] / (d - 1)).astype(np.float32))


def identity(d, vertices=None):
    """The table that maps every lattice point to itself: table[c, b, g, r] = the vertex of channel c (uniform(d) unless given)."""
    v = uniform(d) if vertices is None else np.asarray(vertices, np.float32)
    t = np.empty((3, d, d, d), np.float32)
    t[0] = v[0][None, None, :]
    t[1] = v[1][None, :, None]
    t[2] = v[2][:, None, None]
    return t


def parseCube(text):
    """The text of a .cube file -> (table, vertices): TITLE, # comments, LUT_3D_SIZE N, DOMAIN_MIN / DOMAIN_MAX (uniform vertices per channel), then N^3 rows 'r g b', red
    fastest -- the table's own order.  ValueError naming the line for LUT_1D_SIZE, a size outside 2 .. 65, a row count that does not match, numbers that are not
    finite, DOMAIN_MIN >= DOMAIN_MAX and unknown keywords."""
    n, lo, hi, rows = None, [0.0] * 3, [1.0] * 3, []

    def numbers(parts, ln, what):
        try:
            vals = [float(p) for p in parts]
        except ValueError:
            raise ValueError('cube line {}: {} expected, got {!r}'.format(ln, what, ' '.join(parts)))
        if len(vals) != 3:
            raise ValueError('cube line {}: {} expected, got {} values'.format(ln, what, len(vals)))
        if not all(np.isfinite(vals)):
            raise ValueError('cube line {}: a number that is not finite'.format(ln))
        return vals
    for ln, line in enumerate(str(text).splitlines(), 1):
        line = line.strip()
        if not line or line.startswith('#'):
            continue
        parts = line.split()
        key = parts[0]
        if key == 'TITLE':
            continue
        if key == 'LUT_1D_SIZE':
            raise ValueError('cube line {}: LUT_1D_SIZE: 1D tables are not supported (LUT_3D_SIZE)'.format(ln))
        if key == 'LUT_3D_SIZE':
            try:
                n = int(parts[1]) if len(parts) == 2 else None
            except ValueError:
                n = None
            if n is None or not D_MIN <= n <= D_MAX:
                raise ValueError('cube line {}: LUT_3D_SIZE {} ({} to {})'.format(ln, ' '.join(parts[1:]), D_MIN, D_MAX))
            continue
        if key in ('DOMAIN_MIN', 'DOMAIN_MAX'):
            vals = numbers(parts[1:], ln, key + ' r g b')
            if key == 'DOMAIN_MIN':
                lo = vals
            else:
                hi = vals
            continue
        if key[0].isalpha() or key[0] == '_':
            raise ValueError('cube line {}: unknown keyword {}'.format(ln, key))
        if n is None:
            raise ValueError('cube line {}: a table row in front of LUT_3D_SIZE'.format(ln))
        rows.append(numbers(parts, ln, 'a row r g b'))
        if len(rows) > n ** 3:
            raise ValueError('cube line {}: more than the {} rows of LUT_3D_SIZE {}'.format(ln, n ** 3, n))
    if n is None:
        raise ValueError('cube: LUT_3D_SIZE is missing')
    if len(rows) != n ** 3:
        raise ValueError('cube line {}: {} rows, LUT_3D_SIZE {} needs {}'.format(ln, len(rows), n, n ** 3))
    for c in range(3):
        if not lo[c] < hi[c]:
            raise ValueError('cube: DOMAIN_MIN {} is not below DOMAIN_MAX {}'.format(lo[c], hi[c]))
    table = np.ascontiguousarray(np.asarray(rows, np.float64).reshape(n, n, n, 3).transpose(3, 0, 1, 2).astype(np.float32))
    return check(table, uniform(n, lo, hi))


def formatCube(table, title=None):
    """The text of a .cube file that holds `table` (uniform vertices on [0, 1]; 9 significant digits: parseCube returns the same float32 values)."""
    t = np.asarray(table, np.float32)
    d = t.shape[1]
    rows = t.transpose(1, 2, 3, 0).reshape(-1, 3)
    head = (['TITLE "{}"'.format(title)] if title else []) + ['LUT_3D_SIZE {}'.format(d)]
    return '\n'.join(head + ['{:.9g} {:.9g} {:.9g}'.format(*(float(x) for x in r)) for r in rows]) + '\n'


def cellIndex(x, v):
    """clamp(lower_bound(v, x) - 1, 0, d - 2) for every x (ailut_transform_cpu.cpp:20-40); NaN -> 0."""
    i = np.searchsorted(v, x, side='left').astype(np.int64) - 1
    i = np.where(np.isnan(x), 0, i)
    return np.clip(i, 0, len(v) - 2)


def transform(x, table, vertices):
    """x: float32 (H, W, 3) in (r, g, b) order -> float32 (H, W, 3), the expressions of the module's docstring."""
    table, vertices = check(table, vertices)
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 3 or x.shape[2] != 3:
        raise ValueError('lut: transform takes a float32 (H, W, 3) array, got {} {}'.format(x.dtype, x.shape))
    d = table.shape[1]
    one = np.float32(1)
    idx, t = [], []
    with np.errstate(all='ignore'):
        for c in range(3):
            v, xc = vertices[c], x[:, :, c]
            i = cellIndex(xc, v)
            v0, v1 = v[i], v[i + 1]
            t.append((xc - v0) / ((v1 - v0) + EPS))
            idx.append(i)
        (ir, ig, ib), (tr, tg, tb) = idx, t
        ur, ug, ub = one - tr, one - tg, one - tb
        flat = table.reshape(3, -1)
        base = ir + d * ig + d * d * ib
        corners = ((ur, ug, ub, 0), (tr, ug, ub, 1), (ur, tg, ub, d), (tr, tg, ub, d + 1),
                   (ur, ug, tb, d * d), (tr, ug, tb, d * d + 1), (ur, tg, tb, d * d + d), (tr, tg, tb, d * d + d + 1))
        y = np.empty(x.shape, np.float32)
        for k in range(3):
            acc = None
            for a, b, c, off in corners:
                p = ((a * b) * c) * flat[k][base + off]
                acc = p if acc is None else acc + p
            y[:, :, k] = acc
    return y


def read(samples, srcBits):
    """The chain's readers: code 2^-16 for uint16 samples, code / 255 for uint8 ones, as float32."""
    s = np.asarray(samples)
    if srcBits == 16 and s.dtype == np.uint16:
        return s.astype(np.float32) * np.float32(2.0 ** -16)
    if srcBits == 8 and s.dtype == np.uint8:
        return s.astype(np.float32) / np.float32(255)
    raise ValueError('lut: srcBits {!r} with {} samples (8 with uint8, 16 with uint16)'.format(srcBits, s.dtype))


def apply(samples, srcBits, table, vertices, bits, order='bgr', strength=1.0, dither=None):
    """(H, W, 3) uint8 / uint16 samples in `order` -> uint8 (bits 8) / uint16 (bits 16) samples in `order`: read, transform, blend with strength s != 1 as
    y = fl32(fl32(s y) + fl32(fl32(1 - s) x)), quant.quantise with quant.flags(dither, bits, 'rgb')."""
    if order not in ORDERS:
        raise ValueError("lut: 'order' {!r} is not supported ({})".format(order, ', '.join(ORDERS)))
    if bits not in (8, 16):
        raise ValueError('lut: bits {!r} (8 or 16)'.format(bits))
    s = np.asarray(samples)
    if s.ndim != 3 or s.shape[2] != 3:
        raise ValueError('lut: (H, W, 3) samples expected, got {}'.format(s.shape))
    x = read(s, srcBits)
    if order == 'bgr':
        x = x[:, :, ::-1]
    x = np.ascontiguousarray(x)
    y = transform(x, table, vertices)
    s32 = np.float32(strength)
    if not np.isfinite(s32):
        raise ValueError("lut: 'strength' {!r} is not finite".format(strength))
    if s32 != np.float32(1):
        with np.errstate(all='ignore'):
            y = s32 * y + (np.float32(1) - s32) * x
    mode = 'none' if dither is None else dither
    f = quant.flags(mode, bits, 'rgb')
    out = quant.quantise(np.ascontiguousarray(y.transpose(2, 0, 1)), bits, mode, bool(f & quant.Q_UNIT)).transpose(1, 2, 0)
    if order == 'bgr':
        out = out[:, :, ::-1]
    return np.ascontiguousarray(out)
