"""lite's fp16 path against the oracle: the U branch as a table over the 65,536 fp16 bit patterns (option lite_lut; build_lite_lut in forward.cpp, forward_lite.cpp;
tail1sum_kernel / tail1sum_lut4_kernel in misc_kernels.hip).  Needs a HIP device: `pytest -m gpu`.

The reference is oracle.nets.forward in fp32 on the fp16-rounded input.  Bounds are those of lite's default arithmetic (fp16x3, split operands everywhere):
  fp32 output   2e-5
  fp16 output   2e-5 + half an fp16 ulp of the expected value (HALF_OUT for values up to 2, relative above that)
The table form must give the bits of the computed branch (lite_lut = 0) everywhere.

A plane that holds an inf or a NaN is NaN throughout in BOTH forms (the FRM gate pools the whole plane), so an image of every bit pattern in one plane compares only
where the NaNs sit; every pattern's own table entry is compared on one-pixel planes, one pattern per plane (test_every_fp16_pattern_one_per_plane).
"""
import ctypes

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd.weights import load_state_dict_file
from oracle import nets as onets, planner as oplanner, stitch as ostitch
from test_gpu_fullsize import _report
from test_gpu_parity import _opt_sr, dev, module_for  # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-3
X3 = 2e-5                 # lite's default arithmetic (fp16x3) against the oracle
HALF_OUT = 5e-4           # extra allowance when the caller asks for an fp16 result tensor (values up to 2: half an ulp = 4.9e-4)
KEYS = ['lite2', 'lite4', 'lite8']
_DT = {torch.float32: 0, torch.float16: 1}
_worst = {}


def _bound(want, half):
    """elementwise bound against the oracle: 2e-5, plus half an fp16 ulp of the expected value for an fp16 result (HALF_OUT up to 2, relative above)"""
    return X3 + (np.maximum(HALF_OUT, np.abs(want) * 2.0 ** -11) if half else 0.0)


def _check(got, want, half, what, classes=None):
    """got within _bound of want; records the worst error per input class (classes: name -> HR mask) under `what`"""
    got = got.float().cpu().numpy() if isinstance(got, torch.Tensor) else got
    err = np.abs(got.astype(np.float64) - want)
    bad = ~(err <= _bound(want, half))
    rec = _worst.setdefault(what, {})
    for name, mask in (classes or {'all': None}).items():
        e = err if mask is None else err[mask]
        if e.size:
            rec[name] = max(rec.get(name, 0.0), float(e.max()))
    _report('lite_fp16_worst', _worst)
    assert not bad.any(), (what, int(bad.sum()), float(err.max()), {k: '{:.3e}'.format(v) for k, v in rec.items()})


def _forward(m, x, y_dtype=torch.float32):
    """moe_net_forward on x as it lies in memory (its strides and storage offset), the result in y_dtype"""
    from moephoto_amd import _lib
    B, _, h, w = x.shape
    y = torch.empty((B, 1, h * m.scale, w * m.scale), dtype=y_dtype, device=x.device)
    sB, _, sH, sW = x.stride()
    _lib.check(_lib.lib().moe_net_forward(m._h, x.data_ptr(), _DT[x.dtype], B, h, w, sB, sH, sW, None, y.data_ptr(), _DT[y_dtype], None,
                                          torch.cuda.current_stream(x.device).cuda_stream))
    return y


def _both(m, x, y_dtype=torch.float32):
    """(table form, computed form) of one forward; lite_lut is back on afterwards"""
    try:
        y1 = _forward(m.set_option('lite_lut', 1), x, y_dtype)
        y0 = _forward(m.set_option('lite_lut', 0), x, y_dtype)
    finally:
        m.set_option('lite_lut', 1)
    return y1, y0


def _same_bits(a, b, what):
    """equal as bit patterns, except that NaNs only have to sit at the same positions"""
    assert a.dtype == b.dtype and a.shape == b.shape
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), (what, 'NaN positions', int(na.sum()), int(nb.sum()))
    it = torch.int16 if a.dtype == torch.float16 else torch.int32
    diff = (a.view(it) != b.view(it)) & ~na
    assert not diff.any(), (what, int(diff.sum()), float((a.float() - b.float())[diff].abs().max()))


def _oracle(key, sd, x):
    return onets.forward(gd.MODELS[key][0], sd, np.ascontiguousarray(x, dtype=np.float32)).numpy()


# ---- 1. fp16 frames through doCrop -----------------------------------------------------------------------------------------------------------------------------------
# Tiles of 256 px, pad 5.  Which summing kernel a plan's tiles get is decided per plan: tail1sum_lut4_kernel needs every output plane's offset in the tile pool to be a
# multiple of 8 (and the HR width a multiple of 4) -- true of the product's align 8 -- and tail1sum_kernel takes the whole plan otherwise: align 1 gives ragged tiles
# of odd extent (1079 x 1917: 85-row and 185-column tiles) at odd pool offsets.  lite8's frames are smaller (its canvas alone is 64 x the input).
FRAME = {('lite2', 8): (3, 1080, 1920), ('lite4', 8): (3, 1080, 1920), ('lite8', 8): (3, 533, 647), ('lite2', 1): (3, 1079, 1917)}


def _frame_opt(key, x, align=1):
    from moephoto_amd import imageProcess as ip
    opt = _opt_sr('lite', gd.MODELS[key][2], 256, fp16_io=True)
    opt.align = align
    return opt, ip._plan_for(opt, x.shape)


def _vec_sum(plan, C):
    """True when the plan's tiles are summed by tail1sum_lut4_kernel (every output plane 8-element aligned in the pool, HR widths multiples of 4)"""
    off = plan.tile_offsets(C)
    sizes = [(t[1] - t[0]) * (t[3] - t[2]) * plan.sc * plan.sc for t in plan.tiles]
    return all((o + c * n) % 8 == 0 for o, n in zip(off, sizes) for c in range(C)) and all((t[3] - t[2]) * plan.sc % 4 == 0 for t in plan.tiles)


def _run_plan(opt, plan, xp):
    """moe_run_plan_ex: the canvas (fp16) and the tile pool (fp32) of one doCrop"""
    from moephoto_amd import _lib
    C = xp.shape[0]
    pool = torch.zeros(plan.pool_elems(C), dtype=torch.float32, device=xp.device)
    out = torch.empty((C, plan.outH, plan.outW), dtype=torch.float16, device=xp.device)
    sC, sH, sW = xp.stride()
    _lib.check(_lib.lib().moe_run_plan_ex(opt.modelCached._h, plan._h, xp.data_ptr(), _lib.F16, sC, sH, sW, out.data_ptr(), _lib.F16, 0,
                                          ctypes.c_void_p(pool.data_ptr()), 0, 1, 1, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out, pool


def _four_tiles(plan):
    """indices of an interior tile, the ragged right and bottom ones of its row / column, and the corner"""
    i, j, I, J = 1, 1, plan.stepH - 1, plan.stepW - 1
    assert plan.stepH >= 3 and plan.stepW >= 3
    return {'interior': i * plan.stepW + j, 'right': i * plan.stepW + J, 'bottom': I * plan.stepW + j, 'corner': I * plan.stepW + J}


def _pool_tile(pool, off, plan, k, C):
    t = plan.tiles[k]
    sc = plan.sc
    n = C * (t[1] - t[0]) * sc * (t[3] - t[2]) * sc
    return pool[off[k]:off[k] + n].reshape(C, 1, (t[1] - t[0]) * sc, (t[3] - t[2]) * sc)


def _docrop_checks(key, x, what, pick, planes=None, align=1):
    """the whole canvas table == computed; the tiles pick(plan) names (name -> index) of the pool within the bound of the oracle; the canvas within 1e-6 (+ the fp16
    rounding) of the oracle's closed-form fold of the engine's own tiles.  Returns (opt, plan, xp, pool, oracle results by tile)."""
    from moephoto_amd import imageProcess as ip
    opt, plan = _frame_opt(key, x, align)
    m = opt.modelCached
    sd = gd.state_dict_for(key, load_state_dict_file)
    sc, C = gd.MODELS[key][2], x.shape[0]
    xp = plan.padImage(x)
    try:
        out1, pool = _run_plan(opt, plan, xp)
        assert torch.equal(out1, ip.doCrop(opt, x)), what
        m.set_option('lite_lut', 0)
        out0, _ = _run_plan(opt, plan, xp)
    finally:
        m.set_option('lite_lut', 1)
    _same_bits(out1, out0, (key, what, 'canvas'))
    assert not torch.isnan(out1).any()
    off = plan.tile_offsets(C)
    wants = {}
    tiles = pick(plan)
    for name, k in tiles.items():
        top, bottom, left, right = plan.tiles[k][:4]
        got = _pool_tile(pool, off, plan, k, C).cpu().numpy()
        ps = list(range(C)) if planes is None or (bottom - top) * (right - left) < 40000 else planes
        want = _oracle(key, sd, xp[ps][:, None, top:bottom, left:right].float().cpu().numpy())
        wants[name] = (ps, want)
        _check(got[ps], want, False, '{} {} tile fp32'.format(key, what))
    pl = oplanner.prepare(tuple(x.shape), 1 << 40, 1e-3, opt.padding, sc, align, 256)
    assert [tuple(t[:4]) for t in pl.tiles] == [tuple(t[:4]) for t in plan.tiles]
    hp = pool.cpu().numpy()
    res = [_pool_tile(hp, off, plan, k, C)[:, 0] for k in range(plan.n_tiles)]
    fold = ostitch.fold_stitch(res, pl, sc)
    err = np.abs(out1.float().cpu().numpy() - fold)
    assert (err <= 1e-6 + (np.abs(fold) + 1e-6) * 2.0 ** -11).all(), (key, what, float(err.max()))
    return opt, plan, xp, pool, wants


@pytest.mark.parametrize('key,align', list(FRAME))
def test_fp16_frames_through_docrop(key, align, dev):
    """A natural frame in fp16 through the device doCrop (config.fp16, 256-px tiles, default arithmetic) -- the path behind the headline lite figures (1080p, align 8:
    the vector summing kernel), and for lite2 a frame of odd tile extents (align 1: the scalar one): the whole canvas with the table equals the computed branch bit for
    bit; an interior, the ragged right, the ragged bottom and the corner tile of the fp32 tile pool are within 2e-5 of the oracle; the stitched fp16 canvas is the
    oracle's fold of the engine's own tiles."""
    x = torch.from_numpy(gd.natural_image(201, FRAME[key, align])).to(dev).half()
    _, plan, _, _, _ = _docrop_checks(key, x, 'natural frame align {}'.format(align), _four_tiles, planes=[0, 2] if key == 'lite8' else None, align=align)
    assert _vec_sum(plan, 3) == (align == 8)


def test_fp16_frame_through_the_reference_tile_loop(dev):
    """The reference's own tile loop (python/imageProcess.py:157-172; test_dropin_protocol_reference_loop's form): one forward of the module per tile on a slice view
    of the padded fp16 frame (moe_net_forward_ex, consecutive calls on one storage), blended into an fp16 canvas.  The canvas with the table equals the computed branch
    bit for bit; every tile is the doCrop pool's tile rounded to fp16 (a tile's bits do not depend on its launch set); the four tiles are within the bound of the oracle."""
    from moephoto_amd import imageProcess as ip
    key = 'lite2'
    x = torch.from_numpy(gd.natural_image(203, (3, 611, 823))).to(dev).half()
    opt, plan, xp, pool, wants = _docrop_checks(key, x, 'loop frame', _four_tiles)
    tiles = _four_tiles(plan)
    off = plan.tile_offsets(3)
    ramp = torch.from_numpy(plan.ramp).to(dev).half()
    xu = xp.unsqueeze(1)
    m = opt.modelCached

    def loop():
        out = torch.zeros((3, plan.outH, plan.outW), dtype=torch.float16, device=dev)
        rs = []
        for t in plan.tiles:
            r = opt(xu[..., t[0]:t[1], t[2]:t[3]]).squeeze(1)
            ip.blendTile(r, out, t, plan.sc, plan.padSc, ramp)
            rs.append(r)
        torch.cuda.synchronize()
        return out, rs
    try:
        out1, rs = loop()
        assert m._last_flag == 1          # (the calls overlapped: slices of one storage)
        m.set_option('lite_lut', 0)
        out0, _ = loop()
    finally:
        m.set_option('lite_lut', 1)
    _same_bits(out1, out0, 'reference loop canvas')
    for k, r in enumerate(rs):
        assert torch.equal(r, _pool_tile(pool, off, plan, k, 3)[:, 0].half()), k
    for name, k in tiles.items():
        ps, want = wants[name]
        _check(rs[k][ps][:, None], want, True, 'lite2 reference loop tile fp16')


# ---- 2. the whole fp16 range -----------------------------------------------------------------------------------------------------------------------------------------
PAT = np.arange(65536, dtype=np.uint16)


def _layouts(bits, dev):
    """one plane of 256 x 256 fp16 values from `bits` (65,536 patterns) in three memory layouts, none of them the table's: a fixed permutation (contiguous), its
    transpose (a view, unit stride along the rows), a view with column stride 2 at an odd element offset inside a larger tensor"""
    img = torch.from_numpy(bits.view(np.float16).reshape(256, 256).copy()).to(dev)
    big = torch.zeros((1, 1, 260, 515), dtype=torch.float16, device=dev)
    view = big[:, :, 2:258, 1:513:2]
    view.copy_(img[None, None])
    assert view.storage_offset() % 2 == 1 and view.stride()[-1] == 2
    return {'permuted': img[None, None].contiguous(), 'transposed': img.t()[None, None], 'strided': view}


def _classes(xl, r):
    """HR masks of the input classes, by the value of the LR pixel"""
    v = np.repeat(np.repeat(xl.float().cpu().numpy()[:, 0], r, -2), r, -1)[:, None]
    b = np.repeat(np.repeat(xl.contiguous().view(torch.int16).cpu().numpy()[:, 0], r, -2), r, -1)[:, None]
    sub = (np.abs(v) < 2.0 ** -14) & (v != 0)
    return {'negative': (v < 0) & ~sub, '-0': b == np.int16(-32768), 'subnormal': sub, '[0,1]': (v >= 0) & (v <= 1) & ~sub & (b != np.int16(-32768)),
            '(1,4]': v > 1}


@pytest.mark.parametrize('key', KEYS)
def test_every_fp16_pattern_in_one_plane(key, dev):
    """Images of ALL 65,536 bit patterns (inf, NaN, the largest values included) in three layouts: the table form equals the computed branch as bit patterns, NaNs at
    the same places, with fp32 and fp16 results.  (Such a plane is NaN throughout: see the module docstring.)"""
    m = module_for(key)
    perm = np.random.default_rng(11).permutation(65536)
    for name, xl in _layouts(PAT[perm], dev).items():
        for yd in (torch.float32, torch.float16):
            y1, y0 = _both(m, xl, yd)
            _same_bits(y1, y0, (key, name, yd))


@pytest.mark.parametrize('key', KEYS)
def test_every_fp16_pattern_one_per_plane(key, dev):
    """Every bit pattern alone in a one-pixel plane (65,536 planes in a fixed permuted order, four forwards of 16,384): each plane's result is the r x r phases of
    one table entry, and the R branch of a plane holding a moderate value is finite -- so the table form must equal the computed branch bit for bit on every pattern
    whose result is not NaN, and be NaN where it is."""
    m = module_for(key)
    perm = np.random.default_rng(12).permutation(65536)
    x = torch.from_numpy(PAT[perm].view(np.float16).copy()).to(dev).view(65536, 1, 1, 1)
    fin = torch.from_numpy(np.abs(PAT[perm].view(np.float16).astype(np.float32)) <= 4).to(dev)
    for c in range(0, 65536, 16384):
        for yd in (torch.float32, torch.float16):
            y1, y0 = _both(m, x[c:c + 16384], yd)
            _same_bits(y1, y0, (key, 'one per plane', c, yd))
            assert not torch.isnan(y1[fin[c:c + 16384]]).any(), key


@pytest.mark.parametrize('key', KEYS)
def test_finite_fp16_patterns_up_to_4_vs_oracle(key, dev):
    """Every finite pattern with |x| <= 4 -- negatives, -0, subnormals, values above 1 (what a DN step hands to SR in a chain) -- in one-plane images of three layouts:
    the table form equals the computed branch bit for bit and is within the bound of the oracle, with fp32 and fp16 results.  The worst error per input class is recorded."""
    m = module_for(key)
    sd = gd.state_dict_for(key, load_state_dict_file)
    r = gd.MODELS[key][2]
    v = PAT.view(np.float16).astype(np.float32)
    fin = PAT[np.abs(v) <= 4]
    assert fin.size == 2 * 17409
    rng = np.random.default_rng(13)
    bits = np.concatenate([fin[rng.permutation(fin.size)], fin[rng.permutation(fin.size)][:65536 - fin.size]])
    for name, xl in _layouts(bits, dev).items():
        want = _oracle(key, sd, xl.float().cpu().numpy())
        cls = _classes(xl, r)
        for yd in (torch.float32, torch.float16):
            y1, y0 = _both(m, xl, yd)
            _same_bits(y1, y0, (key, name, yd))
            _check(y1, want, yd == torch.float16, '{} all finite |x| <= 4 {}'.format(key, 'fp16' if yd == torch.float16 else 'fp32'), cls)


@pytest.mark.parametrize('key', KEYS)
def test_signed_and_above_one_frame_through_docrop(key, dev):
    """The signed / above-1 input classes through the device doCrop as well: a frame of values in [-4, 4] (fp16): canvas table == computed, an interior and the corner
    tile within the bound of the oracle, the canvas the fold of the engine's tiles."""
    x = torch.from_numpy((gd.natural_image(207, (2, 523, 541)) - np.float32(0.5)) * np.float32(8)).to(dev).half()
    assert float(x.min()) < -1 and float(x.max()) > 1
    _docrop_checks(key, x, 'signed frame', lambda plan: {k: v for k, v in _four_tiles(plan).items() if k in ('interior', 'corner')}, planes=[1] if key == 'lite8' else None)


# ---- 3. the table's lifetime ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', ['lite2', 'lite8'])
def test_table_lifetime(key, dev):
    """After each change below, the next fp16 forward equals the computed branch bit for bit and matches the oracle of the weights loaded at that point: a perturbed
    checkpoint loaded on the same module and the original again; the fp16 precision and back; fuse_tail, up_fuse2, conv1x1 and lite_lut off and on; the first fp16
    forward inside a graph capture (no table is built there: the replay and the eager forward after it are the computed branch's bits)."""
    from moephoto_amd import models
    r = gd.MODELS[key][2]
    sd0 = gd.state_dict_for(key, load_state_dict_file)
    rng = np.random.default_rng(5)
    sd1 = {k: (v * np.float32(1.1) + (rng.standard_normal(v.shape).astype(np.float32) * np.float32(0.1 * np.sqrt(np.mean(v ** 2))) if v.ndim == 4 else 0)).astype(np.float32)
           for k, v in sd0.items()}
    m = models.Net(r)
    x = torch.from_numpy(gd.natural_image(211, (2, 40, 56))).to(dev).half()[:, None]
    xn = x.float().cpu().numpy()

    def load(sd):
        m.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(v)) for n, v in sd.items()})
        m.to(dtype=torch.float16, device=dev)

    def step(what, sd, tol=None):
        y = _forward(m, x)                      # the next fp16 forward (fills the table when there is none)
        y0 = _both(m, x)[1]
        _same_bits(y, y0, (key, what))
        want = _oracle(key, sd, xn)
        if tol is None:
            _check(y, want, False, '{} lifetime'.format(key))
        else:
            assert np.abs(y.cpu().numpy() - want).max() <= tol, (key, what)
        assert torch.equal(_forward(m, x), y), (key, what)      # (with the table of this state)
        return y

    load(sd0)
    ya = step('first', sd0)
    load(sd1)
    yb = step('perturbed checkpoint', sd1)
    assert not torch.equal(ya, yb)
    load(sd0)
    assert torch.equal(step('original again', sd0), ya)
    try:
        m.set_precision('fp16')
        step('precision fp16', sd0, tol=6e-3)       # (the documented bound of the forced fp16 mode for lite: test_net_forward_fast_mode_documented_error)
    finally:
        m.set_precision('auto')
    assert torch.equal(step('precision auto', sd0), ya)
    for opt in ('fuse_tail', 'up_fuse2', 'conv1x1', 'lite_lut'):
        try:
            m.set_option(opt, 0)
            step(opt + ' off', sd0)
        finally:
            m.set_option(opt, 1)
        assert torch.equal(step(opt + ' on', sd0), ya), opt
    # the first fp16 forward inside a capture.  The toggle drops the table; fp32 forwards (which build none) grow the workspace beforehand to what this shape and the
    # table's own 256 x 256 forward need -- the captured launches hold its address, and the table built after the capture must not move it
    m.set_option('lite_lut', 0)
    m.set_option('lite_lut', 1)
    xs = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(torch.zeros((1, 1, 256, 256), device=dev))
        m(xs.float())
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yg = m(xs)[-1]
    x2 = torch.from_numpy(gd.noise_image(212, (2, 40, 56))).to(dev).half()[:, None]
    xs.copy_(x2)
    g.replay()
    torch.cuda.synchronize()
    got = yg.clone()
    y_eager = m(x2)[-1]                        # (fills the table)
    want2 = _both(m, x2, torch.float16)[1]
    _same_bits(got, want2, (key, 'graph replay'))
    _same_bits(y_eager, want2, (key, 'eager after the capture'))


# ---- 4. launch-set edges ----------------------------------------------------------------------------------------------------------------------------------------------
def test_launch_set_edges_lite8(dev):
    """lite8 at 256 x 256: bmax planes per launch set from max_tile_pixels().  fp16 batches of bmax and bmax + 1 planes, up_fuse2 on and off: every plane equals the
    same plane run in a batch of three; the first and last plane of each launch set within the bound of the oracle.  And the batch whose last upsampler stage sits
    exactly at the 32-bit offset limit of conv1x1 (B h w = 32 x 255 x 257: 128 B x 16 B h w = 2^32 - 2^16) with up_fuse2 off: that stage falls back to the two-part
    tail, where the table cannot be used -- the U branch is computed (it returned MOE_EINVAL once), bit for bit the computed form."""
    key = 'lite8'
    m = module_for(key)
    sd = gd.state_dict_for(key, load_state_dict_file)
    bmax = m.max_tile_pixels() // (256 * 256)
    assert bmax == 31
    x = torch.from_numpy(gd.natural_image(221, (bmax + 2, 256, 256))).to(dev).half()[:, None]
    want = {b: _oracle(key, sd, x[b:b + 1].float().cpu().numpy()) for b in (0, bmax - 1, bmax)}
    try:
        for uf in (1, 0):
            m.set_option('up_fuse2', uf)
            ref = torch.cat([m(x[b:b + 3])[-1] for b in range(0, bmax + 2, 3)])      # (33 planes: eleven batches of three)
            for n in (bmax, bmax + 1):
                y = m(x[:n])[-1]
                assert torch.equal(y, ref[:n]), (uf, n, [b for b in range(n) if not torch.equal(y[b], ref[b])])
                for b in (0, bmax - 1, bmax):
                    if b < n:
                        _check(y[b:b + 1], want[b], True, 'lite8 launch sets fp16')
        m.set_option('up_fuse2', 0)
        xe = torch.from_numpy(gd.natural_image(223, (32, 255, 257))).to(dev).half()[:, None]
        assert 128 * 16 * xe.shape[0] * 255 * 257 == (1 << 32) - (1 << 16) and m.max_tile_pixels() // (255 * 257) == 32
        y1, y0 = _both(m, xe, torch.float16)
        _same_bits(y1, y0, 'two-part tail')
        for b in (0, 31):
            _check(y1[b:b + 1], _oracle(key, sd, xe[b:b + 1].float().cpu().numpy()), True, 'lite8 two-part tail fp16')
    finally:
        m.set_option('up_fuse2', 1)


# ---- 5. the forward's entry ---------------------------------------------------------------------------------------------------------------------------------------------
def _fresh(key, dev):
    from moephoto_amd import models
    m = models.Net(gd.MODELS[key][2])
    m.load_state_dict({n: torch.from_numpy(v) for n, v in gd.state_dict_for(key, load_state_dict_file).items()})
    return m.to(dtype=torch.float16, device=dev)


def test_refused_first_fp16_call_then_a_valid_one(dev):
    """A fresh lite net's first fp16 call with a bad shape or a bad dtype is refused (MOE_EINVAL) and builds no table; the next valid call equals the computed branch."""
    from moephoto_amd import _lib
    L = _lib.lib()
    x = torch.from_numpy(gd.natural_image(231, (2, 24, 40))).to(dev).half()[:, None].contiguous()
    st = torch.cuda.current_stream().cuda_stream
    for bad in ((0, 24, 40, _lib.F16), (2, 0, 40, _lib.F16), (2, 24, 40, _lib.U8)):
        m = _fresh('lite4', dev)
        y = torch.empty((2, 1, 96, 160), dtype=torch.float32, device=dev)
        B, h, w, yd = bad
        assert L.moe_net_forward(m._h, x.data_ptr(), _lib.F16, B, h, w, 960, 40, 1, None, y.data_ptr(), yd, None, st) == _lib.EINVAL, bad
        y1, y0 = _both(m, x)
        _same_bits(y1, y0, bad)
        _check(y1, _oracle('lite4', gd.state_dict_for('lite4', load_state_dict_file), x.float().cpu().numpy()), False, 'lite4 after a refused call')


@pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2, reason='needs two visible devices')
def test_table_built_on_the_nets_device(dev):
    """The net lives on device 0 while the caller's current device is 1: the table is built on device 0, the result equals the computed branch."""
    m = _fresh('lite2', dev)
    x = torch.from_numpy(gd.natural_image(233, (2, 24, 40))).to(dev).half()[:, None].contiguous()
    with torch.cuda.device(1):
        y1 = m(x)[-1]
        torch.cuda.synchronize(0)
    y0 = _both(m, x, torch.float16)[1]
    _same_bits(y1, y0, 'device 1 current')


def test_every_family_under_inference_mode(dev):
    """EngineModule.forward under torch.inference_mode() (inference tensors keep no version counter) equals the plain forward, for every family; two calls on slices of
    one image as the reference's tile loop makes them."""
    for key in ('a2', 'a3', 'a4', 'dn_lite5', 'l25', 'lite2', 'lite4', 'lite8'):
        for dt in ((torch.float32, torch.float16) if key.startswith('lite') else (torch.float32,)):
            m = module_for(key)
            img = torch.from_numpy(gd.natural_image(241, (2, 48, 40))).to(dev).to(dt)[:, None]
            want = [m(img[..., :24, :])[-1].clone(), m(img[..., 24:, :])[-1].clone()]
            with torch.inference_mode():
                xi = img.clone()
                got = [m(xi[..., :24, :])[-1], m(xi[..., 24:, :])[-1]]
            for a, b in zip(got, want):
                assert torch.equal(a, b), (key, dt)
