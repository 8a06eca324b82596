"""Fitted sizes without a device: the integer definition of the rational polyphase filter (pixfmt.fitTable / fitPlanes) -- its tables against
chromaTable at integer scales, its invariants, its distance from a float64 evaluation of the same formula with unrounded weights -- and every refusal of
moe_fit_create / moe_fit_run and of the output step's 'width' / 'height' / 'fit' keys that needs no device."""
import ctypes
import os
import re
from fractions import Fraction as Fr
from math import ceil, floor

import numpy as np
import pytest

from moephoto_amd import _lib, pixfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ('nearest', 'bilinear', 'bicubic')
LOCS = ('center', 'left')
ONE = 1 << 14


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('loc', LOCS)
def test_integer_scales_are_chromatables_taps(method, loc):
    """fitTable(method, n, n * scale, loc) has the same non-zero taps at the same source indices as chromaTable(method, scale, loc), for every scale."""
    for scale in range(1, 17):
        want_off, want = pixfmt.chromaTable(method, scale, loc)
        for n in (1, 3):
            off, coef = pixfmt.fitTable(method, n, n * scale, loc)
            assert len(off) == len(coef) == n * scale
            for o in range(n * scale):
                q, p = divmod(o, scale)
                got = {off[o] + j: c for j, c in enumerate(coef[o]) if c}
                assert got == {q + want_off[p] + j: c for j, c in enumerate(want[p]) if c}, (scale, n, o)


SIZES = ((64, 16), (68, 17), (37, 23), (23, 37), (41, 29), (29, 41), (5, 5), (1, 1), (1, 16), (2, 7), (719, 180), (100, 26), (1080, 720), (45, 67))


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('loc', LOCS)
def test_rows_sum_to_one_fit_int32_reach_the_plane_and_do_not_step_back(method, loc):
    for n, m in SIZES:
        off, coef = pixfmt.fitTable(method, n, m, loc)
        T = len(coef[0])
        assert len(off) == len(coef) == m and all(len(r) == T for r in coef) and 1 <= T <= 16
        for o in range(m):
            assert sum(coef[o]) == ONE, (n, m, o, coef[o])
            assert sum(abs(c) for c in coef[o]) <= 32767, (n, m, o, coef[o])
            # every row reaches the plane -- but for 'nearest' sited 'left' on a growing axis, whose last outputs round up to n (the clamp reads n - 1)
            assert off[o] + T - 1 >= 0 and off[o] <= (n if (method, loc) == ('nearest', 'left') and m > n else n - 1), (n, m, o, off[o])
        assert off == sorted(off), (n, m)


def test_tap_counts_at_the_downscale_limit():
    for n, m in ((64, 16), (68, 17), (4319, 1080), (101, 26), (7, 2)):
        for loc in LOCS:
            assert len(pixfmt.fitTable('nearest', n, m, loc)[1][0]) == 1
            assert len(pixfmt.fitTable('bilinear', n, m, loc)[1][0]) <= 8
            assert len(pixfmt.fitTable('bicubic', n, m, loc)[1][0]) <= 16
    assert len(pixfmt.fitTable('bicubic', 64, 16)[1][0]) == 16 and len(pixfmt.fitTable('bilinear', 64, 16)[1][0]) == 8


def test_table_refuses_what_it_does_not_know():
    for args in (('lanczos', 4, 6, 'center'), ('bicubic', 4, 6, 'top'), ('bicubic', 0, 6, 'center'), ('bicubic', 4, 0, 'center'), ('bicubic', -4, 6, 'center'),
                 ('bicubic', 4.0, 6, 'center'), ('bicubic', 4, True, 'center'), ('bicubic', 65, 16, 'center'), ('bilinear', 9, 2, 'left'), ('nearest', 1, 17, 'center'),
                 ('bicubic', 2, 33, 'left')):
        with pytest.raises(ValueError):
            pixfmt.fitTable(*args)
    pixfmt.fitTable('bicubic', 64, 16)          # (the limits themselves are inside)
    pixfmt.fitTable('bicubic', 2, 32, 'left')


def test_a_table_is_the_callers_to_change():
    off, coef = pixfmt.fitTable('bicubic', 37, 23)
    off[0], coef[0][0] = 99, 99
    again = pixfmt.fitTable('bicubic', 37, 23)
    assert again[0][0] != 99 and again[1][0][0] != 99


# ---- fitPlanes ------------------------------------------------------------------------------------------------------------------------------------
def _codes(seed, depth, C, h, w):
    return np.random.default_rng(seed).integers(0, 1 << depth, size=(C, h, w)).astype(np.uint8 if depth == 8 else '<u2')


@pytest.mark.parametrize('method', METHODS)
def test_same_size_is_the_identity_and_the_depth_shift(method):
    x = _codes(1, 8, 2, 37, 41)
    for loc in LOCS:          # (at n = m both sitings centre output o on source o)
        same = pixfmt.fitPlanes(x, 8, 8, 37, 41, method, loc)
        assert same.dtype == np.uint8 and (same == x).all()
        up = pixfmt.fitPlanes(x, 8, 10, 37, 41, method, loc)
        assert up.dtype == np.dtype('<u2') and (up == x.astype(np.int64) << 2).all()
    y = _codes(2, 16, 1, 9, 7)
    assert (pixfmt.fitPlanes(y, 16, 10, 9, 7, method) == y >> 6).all() and (pixfmt.fitPlanes(y, 16, 8, 9, 7, method) == y >> 8).all()


@pytest.mark.parametrize('method', METHODS)
@pytest.mark.parametrize('loc', LOCS)
def test_a_constant_plane_stays_constant(method, loc):
    for depth, code in ((10, 0), (10, 1023), (10, 513), (16, 65535), (8, 255), (12, 2048)):
        for (h, w), (oh, ow) in (((37, 41), (23, 29)), ((23, 29), (37, 41)), ((64, 68), (16, 17)), ((2, 2), (7, 5)), ((1, 1), (1, 1))):
            x = np.full((2, h, w), code, np.uint16)
            assert (pixfmt.fitPlanes(x, depth, depth, oh, ow, method, loc) == code).all(), (depth, code, h, w)


def test_nearest_is_index_selection():
    for (h, w), (oh, ow) in (((37, 41), (23, 29)), ((23, 29), (37, 41)), ((64, 68), (16, 17)), ((2, 2), (7, 5)), ((9, 5), (3, 80))):
        x = _codes(h + w, 10, 2, h, w)
        iy = [min(floor(Fr(2 * o + 1, 2) * h / oh), h - 1) for o in range(oh)]
        ix = [min(floor(Fr(2 * o + 1, 2) * w / ow), w - 1) for o in range(ow)]
        assert (pixfmt.fitPlanes(x, 10, 10, oh, ow, 'nearest') == x[:, iy][:, :, ix]).all(), (h, w, oh, ow)


def test_fitplanes_refuses_other_input():
    x = _codes(3, 10, 2, 6, 8)
    for bad in (lambda: pixfmt.fitPlanes(x, 9, 10, 4, 4, 'bicubic'), lambda: pixfmt.fitPlanes(x, 10, 11, 4, 4, 'bicubic'), lambda: pixfmt.fitPlanes(x[0], 10, 10, 4, 4, 'bicubic'),
                lambda: pixfmt.fitPlanes(x.astype(np.float32), 10, 10, 4, 4, 'bicubic'), lambda: pixfmt.fitPlanes(x, 10, 10, 1, 4, 'bicubic'),
                lambda: pixfmt.fitPlanes(x, 10, 10, 4, 4, 'lanczos'), lambda: pixfmt.fitPlanes(x, 10, 10, 4, 4, 'bicubic', 'top')):
        with pytest.raises(ValueError):
            bad()


def _float_axis(method, n, m, loc):
    """The same formula with unrounded weights: (m, n) float64 matrix of one axis, the edge sample repeated."""
    A = Fr(-3, 4)

    def k(x):
        x = abs(x)
        if method == 'bilinear':
            return max(1 - x, Fr(0))
        if x <= 1:
            return ((A + 2) * x - (A + 3)) * x * x + 1
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A if x < 2 else Fr(0)
    R = 1 if method == 'bilinear' else 2
    s = Fr(n, m)
    f = max(Fr(1), s)
    M = np.zeros((m, n))
    for o in range(m):
        c = (Fr(2 * o + 1) * s - 1) / 2 if loc == 'center' else o * s
        taps = range(floor(c - R * f) + 1, ceil(c + R * f))
        w = [k((i - c) / f) for i in taps]
        for i, v in zip(taps, w):
            M[o, min(max(i, 0), n - 1)] += float(v / sum(w))
    return M


@pytest.mark.parametrize('method', ('bilinear', 'bicubic'))
@pytest.mark.parametrize('loc', LOCS)
def test_distance_from_the_float64_evaluation_of_the_same_formula(method, loc):
    """Bound: every 14-bit coefficient is off its weight by at most 2^-15 and the deficit moves one of them by at most T 2^-15 more, so an axis' weights are off by at
    most T 2^-14 in sum; on codes below 2^Ds the two passes are off by (T_x + T_y) 2^-14 2^Ds, and the final rounding adds 1/2.  Observed maxima (random codes, both
    shapes, all four cases): 0.55 codes at Ds = 10 (bound 0.9 to 2.5) and 4.7 at Ds = 16 (bound 28 to 128.5)."""
    for (h, w), (oh, ow) in (((37, 41), (23, 29)), ((64, 68), (16, 17))):
        My, Mx = _float_axis(method, h, oh, 'center'), _float_axis(method, w, ow, loc)
        Tx, Ty = len(pixfmt.fitTable(method, w, ow, loc)[1][0]), len(pixfmt.fitTable(method, h, oh, 'center')[1][0])
        for Ds in (10, 16):
            x = _codes(Ds + h, Ds, 2, h, w)
            want = np.clip(np.einsum('oh,chw,pw->cop', My, x.astype(np.float64), Mx), 0, (1 << Ds) - 1)
            got = pixfmt.fitPlanes(x, Ds, Ds, oh, ow, method, loc).astype(np.float64)
            err = np.abs(got - want).max()
            print('{} {} {}x{} -> {}x{} Ds {}: max |integer - float64| = {:.3f} codes (T {} + {})'.format(method, loc, w, h, ow, oh, Ds, err, Tx, Ty))
            assert err <= (Tx + Ty) * 2.0 ** -14 * (1 << Ds) + 0.5, (h, w, Ds, err)


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------------
NEW = ('moe_fit_create', 'moe_fit_run', 'moe_fit_info', 'moe_fit_destroy')


def test_fit_exports_are_declared_bound_and_present():
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    declared = set(re.findall(r'\b(moe_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert sorted(_lib.EXPORTS) == sorted(declared)
    assert L.moe_abi_version() == _lib.ABI_VERSION == 4          # additions only: the version stays
    from moephoto_amd import build
    assert 'fit.hip' in build.SOURCES


def _tabs(method, n, m, loc='center'):
    off, coef = pixfmt.fitTable(method, n, m, loc)
    T = len(coef[0])
    return T, (ctypes.c_int16 * (m * T))(*[c for r in coef for c in r]), (ctypes.c_int32 * m)(*off)


def test_fit_entry_points_validate_their_arguments_without_a_device():
    L = _lib.lib()
    h, w, oh, ow = 12, 20, 7, 9
    tx, ty = _tabs('bicubic', w, ow, 'left'), _tabs('bicubic', h, oh)
    handle = ctypes.c_void_p()

    def create(planes=2, ds=10, dd=10, h=h, w=w, oh=oh, ow=ow, tx=tx, ty=ty, out=ctypes.byref(handle)):
        return L.moe_fit_create(planes, ds, h, w, dd, oh, ow, tx[0], tx[1], tx[2], ty[0], ty[1], ty[2], 0, out)

    def refused(rc, text):
        msg = L.moe_last_error()
        assert rc == _lib.EINVAL and text in msg and not handle.value, (rc, msg, text)
    for k in (1, 2):
        for axis in ('tx', 'ty'):
            bad = list(tx if axis == 'tx' else ty)
            bad[k] = None
            refused(create(**{axis: bad}), b'moe_fit_create: NULL')
    refused(create(out=None), b'NULL')
    for d in (0, 7, 9, 14, 17, -8):
        refused(create(ds=d), b'depth')
        refused(create(dd=d), b'depth')
    for p in (0, 5, -1):
        refused(create(planes=p), b'planes')
    for key in ('h', 'w', 'oh', 'ow'):
        for v in (0, -2):
            refused(create(**{key: v}), b'must be positive')
        refused(create(**{key: 1 << 31}), b'does not fit an int')
    for t in (0, 17, -1):
        refused(create(tx=(t,) + tx[1:]), b'taps')
        refused(create(ty=(t,) + ty[1:]), b'taps')
    for axis, name, tab, n, m in (('tx', b'horizontal', tx, w, ow), ('ty', b'vertical', ty, h, oh)):
        T = tab[0]
        for row in (0, m - 1):
            c = list(tab[1])
            c[row * T + T - 1] += 1
            refused(create(**{axis: (T, (ctypes.c_int16 * len(c))(*c), tab[2])}), name + b' coefficients of output ' + str(row).encode())
        c = list(tab[1])
        c[T:2 * T] = [-8193, 16385, 16385, -8193] + [0] * (T - 4)          # sums to 2^14, magnitudes 49156: the int32 bound is part of the contract
        refused(create(**{axis: (T, (ctypes.c_int16 * len(c))(*c), tab[2])}), b'magnitudes 49156')
        for row, value in ((m - 1, n), (0, -T), (m - 1, 1 << 30), (0, -(1 << 31))):
            o = list(tab[2])
            o[row] = value
            refused(create(**{axis: (T, tab[1], (ctypes.c_int32 * m)(*o))}), name + b' offset')
        o = list(tab[2])
        o[3] = o[2] - 1
        refused(create(**{axis: (T, tab[1], (ctypes.c_int32 * m)(*o))}), b'must not decrease')
    # offsets that are valid one by one but step so far that no tile's window fits the LDS
    far = (1, (ctypes.c_int16 * 4)(*[ONE] * 4), (ctypes.c_int32 * 4)(0, 2048, 4096, 6144))
    refused(create(h=8192, w=8192, oh=4, ow=4, tx=far, ty=far), b'bytes of LDS')
    buf = (ctypes.c_uint16 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.moe_fit_run(None, p, p, None) == _lib.EINVAL and b'moe_fit_run: NULL' in L.moe_last_error()
    assert L.moe_fit_info(None, (ctypes.c_int64 * 4)()) == _lib.EINVAL and b'moe_fit_info: NULL' in L.moe_last_error()
    L.moe_fit_destroy(None)          # (a no-op)


# ---- the builders -------------------------------------------------------------------------------------------------------------------------------
def test_builders_refuse_the_fit_keys_before_any_model_is_loaded():
    from moephoto_amd import imageProcess, procedure
    before = dict(imageProcess.modelCache)
    sr = lambda scale=2: {'op': 'SR', 'model': 'no such model', 'scale': scale}
    buf = lambda **kw: dict({'op': 'buffer', 'pixFmt': 'yuv420p10le'}, **kw)
    out = lambda **kw: dict({'op': 'output'}, **kw)
    cases = [(out(width=210), "'height' is missing"), (out(height=150), "'width' is missing"), (out(fit='bicubic'), "'fit' needs a size"),
             (out(width=210, height=150, fit='lanczos'), 'fit "lanczos"'), (out(width=210, height=150, fit=None), 'fit'),
             (out(width=211, height=150), "'width' must be a positive even int"), (out(width=210, height=151), "'height' must be a positive even int"),
             (out(width=0, height=150), "'width'"), (out(width=210, height=-150), "'height'"), (out(width=210.0, height=150), "'width'"),
             (out(width='210', height=150), "'width'"), (out(width=True, height=150), "'width'"), (out(width=210, height=None), "'height'")]
    for o, text in cases:
        for steps in ([buf(), sr(), o], [buf(chroma='bicubic', chromaLoc='left'), sr(), o], [buf(), sr(), dict(o, pixFmt='yuv420p')]):
            with pytest.raises(ValueError, match=text):
                procedure.genProcess(steps)
            with pytest.raises(ValueError, match=text):
                procedure.genFrameStream(steps, 140, 100, 2)
            with pytest.raises(ValueError, match=text):
                procedure._planeFormats(steps)
    # ratios against the chain's own output size (140 x 100 through a2: 280 x 200), known to the stream builder before a model is loaded
    for o, text in ((out(width=68, height=100), "'width' 68 shrinks"), (out(width=140, height=48), "'height' 48 shrinks"),
                    (out(width=4482, height=200), "'width' 4482 enlarges"), (out(width=280, height=3202), "'height' 3202 enlarges")):
        with pytest.raises(ValueError, match=text):
            procedure.genFrameStream([buf(), sr(), o], 140, 100, 2)
    with pytest.raises(ValueError, match="'width' 2242 enlarges the source's chroma"):          # luma-only: one pass from the 70 x 50 chroma planes
        procedure.genFrameStream([buf(chroma='bilinear'), sr(4), sr(2), out(width=2242, height=1600)], 140, 100, 2)
    assert procedure._planeFit([buf(), sr(), out(width=70, height=50)], 140, 100) == (70, 50, 'bicubic')          # (4 down exactly)
    assert procedure._planeFit([buf(), sr(), out(width=4480, height=3200, fit='nearest')], 140, 100) == (4480, 3200, 'nearest')          # (16 up exactly)
    assert procedure._planeFit([buf(), sr(), out(pixFmt='yuv420p')], 140, 100) is None and procedure._planeFit([buf(), sr()]) is None
    # a chain whose source is not planar has a resize step for this
    for k, v in (('width', 210), ('height', 150), ('fit', 'bicubic')):
        for src in ({'op': 'buffer', 'bitDepth': 16}, {'op': 'buffer', 'bitDepth': 8}):
            for extra in ({}, {'pixFmt': 'yuv420p'}):
                steps = [dict(src), sr(), dict(out(**{k: v}), **extra)]
                with pytest.raises(ValueError, match="output: '{}' applies to a chain on planar".format(k)):
                    procedure.genProcess(steps)
                with pytest.raises(ValueError, match="output: '{}' applies to a chain on planar".format(k)):
                    procedure.genFrameStream(steps, 140, 100, 2)
    with pytest.raises(ValueError, match='cannot hold a resize step'):          # (the refusals the planar chains already had are as they were)
        procedure.genProcess([buf(), sr(), {'op': 'resize', 'width': 210, 'height': 150, 'method': 'bicubic'}, out(width=210, height=150)])
    assert imageProcess.modelCache == before


def test_step_lists_without_the_new_keys_are_read_as_before():
    from moephoto_amd import procedure
    sr = {'op': 'SR', 'model': 'no such model', 'scale': 2}
    buf = lambda **kw: dict({'op': 'buffer', 'pixFmt': 'yuv420p10le'}, **kw)
    assert procedure._planeFormats([buf(), sr]) == ('yuv420p10le', 'yuv420p10le')
    assert procedure._planeFormats([buf(), sr, {'op': 'output', 'pixFmt': 'yuv420p'}], 140, 100) == ('yuv420p10le', 'yuv420p')
    assert procedure._planeFormats([buf(chroma='bicubic', chromaLoc='left'), sr, {'op': 'output'}]) == ('yuv420p10le', 'yuv420p10le')
    assert procedure._planeFormats([{'op': 'buffer', 'bitDepth': 16}, sr]) is None and procedure._planeFormats([]) is None
    # the size changes neither member of the result: the formats are the chain's
    assert procedure._planeFormats([buf(), sr, {'op': 'output', 'pixFmt': 'yuv420p', 'width': 210, 'height': 150}], 140, 100) == ('yuv420p10le', 'yuv420p')
    assert procedure._planeFormats([buf(), sr, {'op': 'output', 'width': 210, 'height': 150, 'fit': 'bilinear'}]) == ('yuv420p10le', 'yuv420p10le')
