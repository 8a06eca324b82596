"""The 3D LUT colour step without a device: the written definition (moephoto_amd/lut3d.py) -- .cube files, its distance from a float64
trilinear model, continuity, zero-width intervals, extrapolation, the identity, the channel order, the strength blend -- and every refusal of the moe_lut3d_* entry
points and of the builders' 'lut' step that needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from moephoto_amd import _lib, lut3d, quant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24          # the unit roundoff of float32


def random_lut(d, seed, uniform=True):
    rng = np.random.default_rng(seed)
    table = (rng.random((3, d, d, d)) * 1.4 - 0.2).astype(np.float32)
    if uniform:
        return table, lut3d.uniform(d)
    v = np.sort(rng.random((3, d)).astype(np.float32), axis=1)
    v[:, 0], v[:, -1] = 0, 1
    return table, v


# ---- .cube files ---------------------------------------------------------------------------------------------------------------------------------
def test_parse_cube_round_trips_and_maps_the_domain():
    table, _ = random_lut(5, 1)
    text = lut3d.formatCube(table, 'a look')
    t, v = lut3d.parseCube(text)
    assert t.dtype == v.dtype == np.float32 and (t == table).all() and (v == lut3d.uniform(5)).all()
    # rows are 'r g b', red fastest: row 1 is lattice point (r, g, b) = (1, 0, 0)
    rows = [l for l in text.splitlines() if l[0] in '-0123456789']
    assert [np.float32(x) for x in rows[1].split()] == [table[0, 0, 0, 1], table[1, 0, 0, 1], table[2, 0, 0, 1]]
    assert [np.float32(x) for x in rows[5].split()] == [table[0, 0, 1, 0], table[1, 0, 1, 0], table[2, 0, 1, 0]]
    assert [np.float32(x) for x in rows[25].split()] == [table[0, 1, 0, 0], table[1, 1, 0, 0], table[2, 1, 0, 0]]
    # comments, blank lines, a title and a domain
    body = '\n'.join(rows)
    t2, v2 = lut3d.parseCube('# made by a test\n\nTITLE "x y"\nLUT_3D_SIZE 5\nDOMAIN_MIN 0 -0.5 0.25\nDOMAIN_MAX 1 1.5 0.75\n' + body + '\n# the end\n')
    assert (t2 == table).all() and (v2 == lut3d.uniform(5, (0, -0.5, 0.25), (1, 1.5, 0.75))).all()
    assert v2[1, 0] == np.float32(-0.5) and v2[1, -1] == np.float32(1.5) and v2[2, 2] == np.float32(0.5)
    assert (lut3d.uniform(3, 0.1, 0.9) == np.float32([0.1, 0.5, 0.9])[None, :].repeat(3, 0)).all()


def test_parse_cube_refuses_by_line():
    rows = '\n'.join('0 0 0' for _ in range(8))
    for text, match in (('LUT_1D_SIZE 4\n', 'line 1: LUT_1D_SIZE'),
                        ('TITLE "t"\nLUT_3D_SIZE 1\n', 'line 2: LUT_3D_SIZE 1'),
                        ('LUT_3D_SIZE 66\n', 'line 1: LUT_3D_SIZE 66'),
                        ('LUT_3D_SIZE two\n', 'line 1: LUT_3D_SIZE two'),
                        ('LUT_3D_SIZE 2\n' + rows + '\n0 0 0\n', 'line 10: more than the 8 rows'),
                        ('LUT_3D_SIZE 2\n' + rows[:-6], 'line 8: 7 rows, LUT_3D_SIZE 2 needs 8'),
                        ('LUT_3D_SIZE 2\n0 0 nan\n', 'line 2: a number that is not finite'),
                        ('LUT_3D_SIZE 2\n0 inf 0\n', 'line 2: a number that is not finite'),
                        ('LUT_3D_SIZE 2\n0 0\n', 'line 2: a row r g b expected, got 2 values'),
                        ('LUT_3D_SIZE 2\n0 0 x\n', 'line 2: a row r g b expected'),
                        ('0 0 0\nLUT_3D_SIZE 2\n', 'line 1: a table row in front of LUT_3D_SIZE'),
                        ('LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 inf\n', 'line 2: a number that is not finite'),
                        ('LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 1\n' + rows, 'DOMAIN_MIN 1.0 is not below DOMAIN_MAX 1.0'),
                        ('LUT_3D_SIZE 2\nDOMAIN_MAX 1 -1 1\n' + rows, 'DOMAIN_MIN 0.0 is not below DOMAIN_MAX -1.0'),
                        ('LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 0 1\n', 'line 2: unknown keyword LUT_3D_INPUT_RANGE'),
                        (rows, 'line 1: a table row in front'),
                        ('# nothing\n', 'LUT_3D_SIZE is missing')):
        with pytest.raises(ValueError, match=re.escape(match)):
            lut3d.parseCube(text)


def test_check_refuses():
    t, v = random_lut(4, 2)
    assert all(a is not None for a in lut3d.check(t, v))
    for bad, match in (((t.astype(np.float64), v), 'float32'), ((t[:, :3], v), r'\(3, d, d, d\)'), ((t[:2], v[:2]), r'\(3, d, d, d\)'), ((t[:, :1, :1, :1], v[:, :1]), 'd = 1'),
                       ((np.zeros((3, 66, 66, 66), np.float32), lut3d.uniform(66)), 'd = 66'), ((t, v[:, :3]), r"'vertices' must have the shape \(3, 4\)")):
        with pytest.raises(ValueError, match=match):
            lut3d.check(*bad)
    for x in (np.inf, -np.inf, np.nan):
        t2, v2 = t.copy(), v.copy()
        t2[2, 3, 3, 3] = x
        v2[1, 2] = x
        with pytest.raises(ValueError, match="'table' holds"):
            lut3d.check(t2, v)
        with pytest.raises(ValueError, match="'vertices' holds"):
            lut3d.check(t, v2)
    v2 = v.copy()
    v2[2, 3] = v2[2, 2] - np.float32(1e-3)
    with pytest.raises(ValueError, match='must not decrease'):
        lut3d.check(t, v2)
    v2[2, 3] = v2[2, 2]          # (a repeated vertex is fine)
    lut3d.check(t, v2)


# ---- the transform ------------------------------------------------------------------------------------------------------------------------------
def model64(x, table, vertices):
    """The same trilinear expression in float64 on the same cells (the index search compares float32 values: it has no rounding), and the per-pixel quantities the
    bound below is made of.  -> (y, bound)"""
    d = table.shape[1]
    x64, eps = x.astype(np.float64), np.float64(np.float32(1e-10))
    idx, t = [], []
    for c in range(3):
        v = vertices[c].astype(np.float64)
        i = lut3d.cellIndex(x[:, :, c], vertices[c])
        t.append((x64[:, :, c] - v[i]) / ((v[i + 1] - v[i]) + eps))
        idx.append(i)
    flat = table.reshape(3, -1).astype(np.float64)
    base = idx[0] + d * idx[1] + d * d * idx[2]
    A = [np.abs(tc) + np.abs(1 - tc) for tc in t]
    W = A[0] * A[1] * A[2]
    slope = np.abs(t[0]) * A[1] * A[2] + np.abs(t[1]) * A[0] * A[2] + np.abs(t[2]) * A[0] * A[1]
    y, bound = np.empty(x.shape, np.float64), np.empty(x.shape, np.float64)
    for k in range(3):
        L = np.stack([flat[k][base + r + d * g + d * d * b] for b in (0, 1) for g in (0, 1) for r in (0, 1)])          # (8, H, W), index r + 2 g + 4 b
        acc = 0
        for b in (0, 1):
            for g in (0, 1):
                for r in (0, 1):
                    acc = acc + (t[0] if r else 1 - t[0]) * (t[1] if g else 1 - t[1]) * (t[2] if b else 1 - t[2]) * L[r + 2 * g + 4 * b]
        y[:, :, k] = acc
        M, V = np.abs(L).max(0), L.max(0) - L.min(0)
        bound[:, :, k] = 1.01 * U * (4.1 * V * slope + 11.2 * W * M) + 1e-12
    return y, bound


@pytest.mark.parametrize('uniform', (True, False))
@pytest.mark.parametrize('d', (2, 17, 33))
def test_transform_is_within_the_derived_bound_of_a_float64_trilinear_model(d, uniform):
    """With u = 2^-24, per channel c the fraction t_c = (x - v0) / ((v1 - v0) + eps) is three roundings in front of the quotient's own: t~ = t (1 + 4.1 u) at most.
    Moving t_c by e with 1 - t_c moving by -e keeps the weights' sum along that axis: the output moves by e times its slope along c, which is at most V A_c' A_c'',
    V = the spread of the cell's eight corner values and A_c = |t_c| + |1 - t_c| (1 inside the lattice, more where a value extrapolates).  Every term w_k L_k carries
    four more relative roundings (1 - t~, two products for the weight, the product with L): 4.1 u |w_k L_k| each, and sum |w_k| <= W = A_r A_g A_b, |L_k| <= M.  Seven
    additions of partial sums of at most W M: 7.1 u W M.  Together
        |y32 - y64| <= 1.01 u (4.1 V sum_c |t_c| A_c' A_c'' + 11.2 W M) + 1e-12
    (1.01: the second-order terms; 1e-12: the float64 model's own).  Inside the lattice, with |L| <= 1.2 and V <= 1.4: 31 u = 1.9e-6 at most."""
    table, vertices = random_lut(d, 10 * d + uniform, uniform)
    rng = np.random.default_rng(d)
    x = (rng.random((40, 50, 3)) * 1.2 - 0.1).astype(np.float32)          # (a tenth outside the vertices on either side)
    x[0, :d, 0] = vertices[0]                                             # the vertices themselves, and their float32 neighbours
    x[1, :d, 1] = np.nextafter(vertices[1], np.float32(2))
    x[2, :d, 2] = np.nextafter(vertices[2], np.float32(-2))
    y = lut3d.transform(x, table, vertices)
    want, bound = model64(x, table, vertices)
    assert y.dtype == np.float32 and y.shape == x.shape
    err = np.abs(y.astype(np.float64) - want)
    assert (err <= bound).all(), 'error {:.3e} where the bound is {:.3e}'.format(err[err > bound].max(), bound[err > bound].min())
    inside = ((x >= 0) & (x <= 1)).all(2)
    assert bound[inside].max() <= 31 * U * 1.02 and err.max() > 0          # (float32 is not float64: the test sees an error)


def test_continuous_across_cell_faces():
    """Either side of a vertex the two cells' expressions meet: the values at the float32 neighbours of a vertex differ by what the table's slope makes of two ulps,
    plus the bound above on each side."""
    d = 9
    table, vertices = random_lut(d, 3, False)
    rng = np.random.default_rng(4)
    x = rng.random((d - 2, 64, 3)).astype(np.float32)
    for c in range(3):
        lo, hi = x.copy(), x.copy()
        v = vertices[c][1:-1]
        lo[:, :, c], hi[:, :, c] = np.nextafter(v, np.float32(-1))[:, None], np.nextafter(v, np.float32(2))[:, None]
        a, b = lut3d.transform(lo, table, vertices), lut3d.transform(hi, table, vertices)
        width = np.diff(vertices[c]).min()
        jump = 1.4 * 2 * np.spacing(np.float32(1)) / width + 2 * 31 * U * 1.02          # spread / narrowest cell x the step, and both sides' rounding
        assert np.abs(a - b).max() <= jump, (c, np.abs(a - b).max(), jump)


def test_zero_width_intervals_stay_finite_and_extrapolation_is_the_clamped_cell():
    table = random_lut(2, 5)[0]
    v = np.float32([[0.5, 0.5]] * 3)
    x = np.float32([[[0.5, 0.5, 0.5], [0.25, 0.5, 1.0], [0.0, 1.0, 0.5]]])
    y = lut3d.transform(x, table, v)
    assert np.isfinite(y).all()
    assert (y[0, 0] == table[:, 0, 0, 0]).all()          # t = 0 / 1e-10 on every axis: the first corner
    table, vertices = random_lut(5, 6), None
    table, vertices = table
    inner = lut3d.uniform(5, 0.25, 0.75)
    # beyond the last vertex the last cell's plane goes on: on a table that is linear along red the value is that line's
    ramp = lut3d.identity(5, inner)
    x = np.float32([[[0.0, 0.5, 0.5], [1.0, 0.5, 0.5], [0.9, 0.3, 0.7], [0.1, 0.25, 0.75]]])
    assert (lut3d.cellIndex(x[0, :, 0], inner[0]) == [0, 3, 3, 0]).all()
    y = lut3d.transform(x, ramp, inner)
    assert np.abs(y - x).max() <= 8 * U          # the identity over [0.25, 0.75] extrapolates to the identity
    y = lut3d.transform(x, table, inner)
    assert np.isfinite(y).all() and not (y[0, 0] == lut3d.transform(np.float32([[[0.25, 0.5, 0.5]]]), table, inner)[0, 0]).all()          # (not clamped to the edge value)
    nan = lut3d.transform(np.float32([[[np.nan, 0.5, 0.5]]]), table, inner)
    assert np.isnan(nan).all() and lut3d.cellIndex(np.float32([np.nan]), inner[0])[0] == 0
    assert (lut3d.apply(np.uint16([[[1, 2, 3]]]), 16, np.full((3, 2, 2, 2), 0, np.float32) + np.float32(0.5), lut3d.uniform(2), 16) == 32768).all()


def test_identity_returns_every_16_bit_code():
    codes = np.arange(65536, dtype=np.uint16)
    im = np.ascontiguousarray(np.stack([codes, codes[::-1], np.roll(codes, 77)], -1).reshape(256, 256, 3))
    out = lut3d.apply(im, 16, lut3d.identity(33), lut3d.uniform(33), 16, dither='round')
    assert out.dtype == np.uint16 and (out == im).all()
    t = lut3d.identity(33)
    assert t[0, 5, 7, 9] == lut3d.uniform(33)[0, 9] and t[1, 5, 7, 9] == lut3d.uniform(33)[1, 7] and t[2, 5, 7, 9] == lut3d.uniform(33)[2, 5]


def test_order_only_permutes_and_strength_blends():
    table, vertices = random_lut(9, 7, False)
    rng = np.random.default_rng(8)
    for srcBits, dt in ((8, np.uint8), (16, np.uint16)):
        im = rng.integers(0, 1 << srcBits, (12, 20, 3)).astype(dt)
        for bits in (8, 16):
            for dither in (None, 'round', 'ordered'):
                a = lut3d.apply(im, srcBits, table, vertices, bits, 'rgb', 0.6, dither)
                b = lut3d.apply(np.ascontiguousarray(im[:, :, ::-1]), srcBits, table, vertices, bits, 'bgr', 0.6, dither)
                assert (a == b[:, :, ::-1]).all()
        # strength 0 under 'round': the input's codes (fl32(0 y) + fl32(1 x) = x for the finite y of a finite table)
        assert (lut3d.apply(im, srcBits, table, vertices, srcBits, 'bgr', 0.0, 'round') == im).all()
        # strength 1 is no blend at all; the blend's expression otherwise
        x = np.ascontiguousarray(lut3d.read(im, srcBits)[:, :, ::-1])
        y = lut3d.transform(x, table, vertices)
        s = np.float32(0.6)
        mixed = s * y + (np.float32(1) - s) * x
        want = quant.quantise(np.ascontiguousarray(mixed.transpose(2, 0, 1)), 16, 'round').transpose(1, 2, 0)[:, :, ::-1]
        assert (lut3d.apply(im, srcBits, table, vertices, 16, 'bgr', 0.6, 'round') == want).all()
        plain = quant.quantise(np.ascontiguousarray(y.transpose(2, 0, 1)), 8, 'ordered', True).transpose(1, 2, 0)[:, :, ::-1]          # (8 bits: the unit scale)
        assert (lut3d.apply(im, srcBits, table, vertices, 8, 'bgr', 1.0, 'ordered') == plain).all()
    for kw, match in ((dict(order='gbr'), "'order'"), (dict(strength=np.inf), "'strength'"), (dict(strength=np.nan), "'strength'"), (dict(dither='blue'), 'dither')):
        with pytest.raises(ValueError, match=match):
            lut3d.apply(im, 16, table, vertices, 16, **kw)
    with pytest.raises(ValueError, match='srcBits'):
        lut3d.apply(im, 8, table, vertices, 16)
    with pytest.raises(ValueError, match='bits 10'):
        lut3d.apply(im, 16, table, vertices, 10)


# ---- the library ---------------------------------------------------------------------------------------------------------------------------------
def test_the_exports_are_declared_and_listed():
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    declared = set(re.findall(r'\b(moe_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    for name, nargs in (('moe_lut3d_create', 5), ('moe_lut3d_run', 10), ('moe_lut3d_info', 2), ('moe_lut3d_destroy', 1)):
        assert name in declared and name in _lib.EXPORTS and len(getattr(L, name).argtypes) == nargs
    assert sorted(_lib.EXPORTS) == sorted(declared) and L.moe_abi_version() == _lib.ABI_VERSION == 4
    assert 'lut3d.py (transform' in hdr and 'ailut_transform_cpu.cpp:20-113' in hdr          # (the definition and the reference lines it replaces are cited)
    src = open(os.path.join(ROOT, 'moephoto_amd', 'lut3d.py')).read()
    assert 'ailut_transform_cpu.cpp:20-113' in src
    kernel = open(os.path.join(ROOT, 'moephoto_amd', 'csrc', 'lut3d.hip')).read()
    assert 'to_output_lut3d_kernel' in kernel and 'lut3d.py' in kernel


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    L = _lib.lib()
    table, vertices = random_lut(3, 9)
    h = ctypes.c_void_p()
    tp, vp = table.ctypes.data, vertices.ctypes.data

    def refused(rc, text):
        assert rc == _lib.EINVAL if hasattr(_lib, 'EINVAL') else rc == -1
        assert text in L.moe_last_error().decode()
    refused(L.moe_lut3d_create(3, None, vp, 0, ctypes.byref(h)), 'NULL')
    refused(L.moe_lut3d_create(3, tp, None, 0, ctypes.byref(h)), 'NULL')
    refused(L.moe_lut3d_create(3, tp, vp, 0, None), 'NULL')
    for d in (1, 66, 0, -3):
        refused(L.moe_lut3d_create(d, tp, vp, 0, ctypes.byref(h)), 'd = {}'.format(d))
    for x in (np.inf, np.nan):
        t2, v2 = table.copy(), vertices.copy()
        t2[2, 2, 2, 2] = x
        v2[2, 2] = x
        refused(L.moe_lut3d_create(3, t2.ctypes.data, vp, 0, ctypes.byref(h)), 'table value 26 of channel 2 is not finite')
        refused(L.moe_lut3d_create(3, tp, v2.ctypes.data, 0, ctypes.byref(h)), 'vertex 2 of channel 2 is not finite')
    v2 = vertices.copy()
    v2[1, 1] = 2
    refused(L.moe_lut3d_create(3, tp, v2.ctypes.data, 0, ctypes.byref(h)), 'vertex 2 of channel 1 decreases')
    assert not h.value
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    p += -p % 16
    fake, src, dst = ctypes.c_void_p(16), p + 512, p + 1024          # (every refusal comes before the handle is read)
    run = lambda *a: L.moe_lut3d_run(*a, None)
    refused(run(None, src, 16, 4, 6, dst, 16, 0, 1.0), 'NULL')
    refused(run(fake, None, 16, 4, 6, dst, 16, 0, 1.0), 'NULL')
    refused(run(fake, src, 16, 4, 6, None, 16, 0, 1.0), 'NULL')
    refused(run(fake, src, 10, 4, 6, dst, 16, 0, 1.0), 'src_bits 10')
    refused(run(fake, src, 16, 4, 6, dst, 12, 0, 1.0), 'bits 12')
    refused(run(fake, src, 16, 4, 6, dst, 16 | quant.Q_UNIT, 0, 1.0), 'MOE_Q_UNIT without')
    refused(run(fake, src, 16, 4, 6, dst, 16 | quant.Q_ROUND | quant.Q_ORDERED, 0, 1.0), 'both set')
    refused(run(fake, src, 16, 4, 6, dst, 16 | 0x800, 0, 1.0), 'unknown flags')
    refused(run(fake, src, 16, 0, 6, dst, 16, 0, 1.0), 'must be positive')
    refused(run(fake, src, 16, 4, -1, dst, 16, 0, 1.0), 'must be positive')
    refused(run(fake, src, 16, 1 << 15, 1 << 15, dst, 16, 0, 1.0), 'do not fit an int')
    refused(run(fake, src, 16, 4, 6, dst, 16, 2, 1.0), 'order 2')
    refused(run(fake, src, 16, 4, 6, dst, 16, 0, float('inf')), 'strength is not finite')
    refused(run(fake, src, 16, 4, 6, dst, 16, 0, float('nan')), 'strength is not finite')
    refused(run(fake, src + 1, 16, 4, 6, dst, 16, 0, 1.0), 'src is not 2-byte aligned')
    refused(run(fake, src, 16, 4, 6, dst + 1, 16, 0, 1.0), 'dst is not 2-byte aligned')
    refused(run(fake, src, 16, 4, 6, src + 142, 16, 0, 1.0), 'overlaps')
    refused(run(fake, src, 16, 4, 6, src - 142, 16, 0, 1.0), 'overlaps')
    info = (ctypes.c_int64 * 4)()
    refused(L.moe_lut3d_info(None, info), 'NULL')
    refused(L.moe_lut3d_info(fake, None), 'NULL')
    L.moe_lut3d_destroy(None)


def test_the_wrapper_refuses_before_it_needs_a_device():
    from moephoto_amd import imageProcess as ip
    table, vertices = random_lut(4, 11)
    with pytest.raises(ValueError, match='float32'):
        ip.lut3d(table.astype(np.float64), vertices)
    with pytest.raises(ValueError, match='must not decrease'):
        ip.lut3d(table, vertices[:, ::-1])
    for kw, match in ((dict(srcBits=10), 'srcBits'), (dict(bits=12), 'bits'), (dict(order='gbr'), "'order'"), (dict(strength=float('nan')), "'strength'"), (dict(dither='blue'), "'dither'")):
        with pytest.raises(ValueError, match=match):
            ip.lut3d(table, vertices, **kw)
    assert callable(ip.lut3d(table)) and callable(ip.lut3d(table, vertices, 8, 8, 'rgb', 0.5, 'ordered'))


# ---- the builders --------------------------------------------------------------------------------------------------------------------------------
def test_builders_refuse_before_a_model_is_loaded(monkeypatch, tmp_path):
    from moephoto_amd import procedure, runDN, runSR

    def no_model(*_a, **_k):
        raise AssertionError('a model was asked for before the chain was checked')
    monkeypatch.setattr(runSR, 'getOpt', no_model)
    monkeypatch.setattr(runDN, 'getOpt', no_model)
    table, vertices = random_lut(5, 12, False)
    cube = tmp_path / 'look.cube'
    cube.write_text(lut3d.formatCube(table))
    bad_cube = tmp_path / 'bad.cube'
    bad_cube.write_text('LUT_1D_SIZE 16\n')
    sr = {'op': 'SR', 'model': 'a', 'scale': 2}
    lut = lambda **kw: dict({'op': 'lut'}, **(kw or dict(table=table, vertices=vertices)))
    out = lambda **kw: dict({'op': 'output'}, **kw)
    rgb, planar = {'op': 'buffer', 'bitDepth': 16}, {'op': 'buffer', 'pixFmt': 'yuv420p10le'}
    builders = (lambda steps: procedure.genFrameStream(steps, 140, 100), procedure.genProcess)
    for build in builders:
        for buf, tail in ((rgb, []), (planar, [out(pixFmt='bgr48le')])):
            with pytest.raises(ValueError, match="'lut' step must be the last compute step"):
                build([buf, lut(), sr] + tail)
            with pytest.raises(ValueError, match="one 'lut' step at most, this one has 2"):
                build([buf, sr, lut(), lut()] + tail)
            with pytest.raises(ValueError, match="exactly one of 'file' and 'table' names the table, the step has both"):
                build([buf, sr, lut(file=str(cube), table=table)] + tail)
            with pytest.raises(ValueError, match="exactly one of 'file' and 'table' names the table, the step has neither"):
                build([buf, sr, lut(strength=0.5)] + tail)
            with pytest.raises(ValueError, match="'vertices' needs 'table'"):
                build([buf, sr, lut(file=str(cube), vertices=vertices)] + tail)
            for s in (float('inf'), float('nan'), 'nan'):
                with pytest.raises(ValueError, match="'strength' .* is not finite"):
                    build([buf, sr, lut(table=table, strength=s)] + tail)
            with pytest.raises(ValueError, match="'strength' 'much' is not a number"):
                build([buf, sr, lut(table=table, strength='much')] + tail)
            with pytest.raises(ValueError, match='must not decrease'):
                build([buf, sr, lut(table=table, vertices=vertices[:, ::-1])] + tail)
            with pytest.raises(ValueError, match='line 1: LUT_1D_SIZE'):
                build([buf, sr, lut(file=str(bad_cube))] + tail)
            with pytest.raises(AssertionError, match='a model was asked for'):          # (a chain nothing is wrong with reaches the model)
                build([buf, sr, lut()] + tail)
            with pytest.raises(AssertionError, match='a model was asked for'):
                build([buf, sr, lut(file=str(cube), strength='0.5')] + tail)
        # a planar Y'CbCr sink is not in this change: the message says so
        with pytest.raises(ValueError, match="planar Y'CbCr sink .'pixFmt': 'yuv420p10le'. behind a 'lut' step is not in this change"):
            build([planar, sr, lut()])
        with pytest.raises(ValueError, match="planar Y'CbCr sink .'pixFmt': 'yuv420p'. behind a 'lut' step is not in this change"):
            build([planar, sr, lut(), out(pixFmt='yuv420p')])
        with pytest.raises(ValueError, match="planar Y'CbCr sink .'pixFmt': 'yuv420p10le'. behind a 'lut' step is not in this change"):
            build([rgb, sr, lut(), out(pixFmt='yuv420p10le')])
        with pytest.raises(ValueError, match="'order' does not apply to a chain on planar frames"):
            build([planar, sr, lut(table=table, order='rgb'), out(pixFmt='bgr48le')])
        with pytest.raises(ValueError, match="'order' 'gbr'"):
            build([rgb, sr, lut(table=table, order='gbr')])
        # what is pinned stays refused, with its type and message
        with pytest.raises(NotImplementedError, match='op "dehaze" is not part of the SR/DN hot path'):
            build([rgb, {'op': 'dehaze', 'model': 'dehaze'}])
        with pytest.raises(NotImplementedError, match='op "dehaze" is not part of the SR/DN hot path'):
            build([rgb, {'op': 'dehaze', 'model': 'dehaze'}, lut()])
        with pytest.raises(NotImplementedError, match='op "slomo"'):
            build([rgb, {'op': 'slomo'}])
        with pytest.raises(NotImplementedError, match='op "dehaze"'):
            build([planar, {'op': 'dehaze'}, lut(), out(pixFmt='bgr24')])
        with pytest.raises(ValueError, match="'dither' does not apply"):
            build([rgb, sr, {'op': 'resize', 'width': 100, 'height': 80, 'fit': 'bicubic'}, lut(), out(dither='round')])
    with pytest.raises(ValueError, match="'lut' step must be the last"):
        procedure.genProcess([{'op': 'file'}, lut(), sr])
    with pytest.raises(ValueError, match="the chain's bitDepth is 10"):
        procedure.genProcess([sr, lut()], 10)
    got = procedure._lutStep([rgb, sr, lut(table=table)], None, 16)
    assert got['order'] == 'bgr' and got['strength'] == 1.0 and (got['vertices'] == lut3d.uniform(5)).all() and (got['table'] == table).all()
    assert procedure._lutStep([sr, lut(file=str(cube), strength=0.25)], None, 8)['order'] == 'rgb'
    assert procedure._lutStep([planar, sr, lut(), out(pixFmt='rgb24')], ('yuv420p10le', 'rgb24'))['order'] == 'rgb'
    assert procedure._lutStep([rgb, sr], None, 16) is None
    assert procedure._withoutLut([rgb, sr, lut()]) == [rgb, sr]
