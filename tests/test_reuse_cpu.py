"""The frame stream's reuse without a device: the region bookkeeping of moephoto_amd/reuse.py against brute force on pixels, the resize rule
against torch's CPU F.interpolate, the fallbacks, and every refusal of moe_changed_blocks, moe_run_plan_subset and genFrameStream(reuse=..) that needs no device."""
import ctypes
import os

import numpy as np
import pytest

import golden_defs as gd
from moephoto_amd import _lib, reuse
from moephoto_amd.imageProcess import TilePlan

CELL = 16


def _tiny_last():
    z = np.load(os.path.join(gd.GOLDEN, 'stitch_only', 's2_tiny_last.npz'))
    return tuple(int(v) for v in z['shape']), int(z['pad']), int(z['sc']), int(z['align']), int(z['crop'])


# name -> (shape, pad, sc, align, crop)
PLANS = {'rgb_100x140_c48_p5_x2': ((3, 100, 140), 5, 2, 8, 48),
         'rgb_100x140_c48_p7_x1': ((3, 100, 140), 7, 1, 8, 48),
         'one_tile_axis_30x140': ((1, 30, 140), 5, 2, 8, 48),            # 30 rows padded to 32: two reflected rows
         'reflect_and_zeros_3x50': ((1, 3, 50), 5, 2, 8, 48),            # 3 rows padded to 8: two reflected rows, three rows of zeros
         's2_tiny_last': _tiny_last()}


def _plan(name):
    shape, pad, sc, align, crop = PLANS[name]
    return TilePlan(shape, 1 << 40, 1e-3, pad, sc, align, crop)


def _padded_index(pl):
    """padImage's rule on an image whose pixel (i, j) holds i * W + j + 1: reflection with the edge not repeated, up to len - 1 samples, zeros behind."""
    _, H, W = pl.shape
    a = np.arange(1, H * W + 1, dtype=np.int64).reshape(H, W)
    for axis, to in ((1, pl.padWTo), (0, pl.padHTo)):
        n = a.shape[axis]
        if not to or to <= n:
            continue
        refl = min(n - 1, to - n)
        width = [(0, 0), (0, 0)]
        if refl > 0:
            width[axis] = (0, refl)
            a = np.pad(a, width, mode='reflect')
        if to - n - refl > 0:
            width[axis] = (0, to - n - refl)
            a = np.pad(a, width)
    return a


def _seen(pl):
    """Per tile the boolean H x W mask of the source pixels it reads."""
    _, H, W = pl.shape
    padded = _padded_index(pl)
    out = []
    for t in pl.tiles:
        ids = np.unique(padded[t[0]:t[1], t[2]:t[3]])
        m = np.zeros(H * W, bool)
        m[ids[ids > 0] - 1] = True
        out.append(m.reshape(H, W))
    return out


def _cells_of(mask):
    """The cells an H x W pixel mask touches."""
    H, W = mask.shape
    ch, cw = reuse.cells(H, W)
    p = np.zeros((ch * CELL, cw * CELL), bool)
    p[:H, :W] = mask
    return p.reshape(ch, CELL, cw, CELL).any(axis=(1, 3))


def _pixels_of(region, h, w):
    """The pixels of an h x w image the True cells of a region cover."""
    return np.repeat(np.repeat(region, CELL, axis=0), CELL, axis=1)[:h, :w]


@pytest.mark.parametrize('name', sorted(PLANS))
def test_support_of_a_tile_against_brute_force(name):
    pl = _plan(name)
    _, H, W = pl.shape
    if name == 'one_tile_axis_30x140':
        assert pl.padHTo == 32 and pl.stepH == 1
    if name == 'reflect_and_zeros_3x50':
        assert pl.padHTo == 8
    reg = reuse.PlanRegions(pl)
    seen = _seen(pl)
    assert reg.n_tiles == pl.n_tiles == len(seen)
    for k in range(pl.n_tiles):
        assert seen[k].any()
        as_cells = reuse.markRects(H, W, reg.support[k])
        assert (as_cells | ~_cells_of(seen[k])).all(), (name, k)                      # the support, as cells, contains what the tile sees
        px = np.zeros((H, W), bool)
        for r0, r1, c0, c1 in reg.support[k]:
            assert 0 <= r0 < r1 <= H and 0 <= c0 < c1 <= W
            px[r0:r1, c0:c1] = True
        assert np.array_equal(px, seen[k]), (name, k)                                 # and as pixels it is what the tile sees, no more
    rng = np.random.default_rng(11)
    touched = [_cells_of(m) for m in seen]
    some = 0
    for _ in range(200):
        changed = rng.random(reuse.cells(H, W)) < rng.choice([0.0, 0.01, 0.03, 0.1])
        want = np.array([1 if (changed & t).any() else 0 for t in touched], np.uint8)
        got = reuse.runSet(reg, changed)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, changed.sum())
        some += int(0 < want.sum() < len(want))
    assert some > 20 or pl.n_tiles < 3


def test_all_equal_and_all_changed_maps():
    for name in PLANS:
        pl = _plan(name)
        reg = reuse.PlanRegions(pl)
        _, H, W = pl.shape
        zero, ones = reuse.runSet(reg, reuse.none(H, W)), reuse.runSet(reg, reuse.full(H, W))
        assert zero.sum() == 0 and ones.sum() == pl.n_tiles
        assert not reuse.outRegion(reg, zero).any() and reuse.outRegion(reg, ones).all()
        with pytest.raises(ValueError):
            reuse.runSet(reg, reuse.none(H + 16, W))


# ---- chains: the stream's walk against a restatement of the rules on pixels ----------------------------------------------------------------
def _restated(plans_or_sizes, changed_cells, H, W):
    """DESIGN.md section 14 on pixel masks: a tile runs iff a pixel it sees lies in a changed cell; a step's output differs at most inside the HR extents
    [top sc, bsc) x [left sc, rsc) of the tiles that ran; the next step sees that through its own cells.  -> per tiled step the run set."""
    px = _pixels_of(changed_cells, H, W)
    runs = []
    for step in plans_or_sizes:
        if not isinstance(step, TilePlan):
            break                                                   # (the chains here end with their resize: nothing behind it has tiles)
        cellpx = _pixels_of(_cells_of(px), *px.shape)
        run = [bool((m & cellpx).any()) for m in _seen(step)]
        runs.append(np.array(run, np.uint8))
        out = np.zeros((step.outH, step.outW), bool)
        for t, r in zip(step.tiles, run):
            if r:
                out[t[0] * step.sc:t[6], t[2] * step.sc:t[7]] = True
        px = out
    return runs


def _chain(name):
    sr = lambda shape: TilePlan(shape, 1 << 40, 1e-3, 5, 2, 8, 48)
    dn = lambda shape: TilePlan(shape, 1 << 40, 1e-3, 7, 1, 8, 48)
    s = (3, 100, 140)
    return {'sr2': [sr(s)], 'dn_sr2': [dn(s), sr(s)], 'sr2_resize_100x90_bilinear': [sr(s), ((90, 100), 'bilinear')],
            'sr2_resize_bicubic_up': [sr(s), ((250, 333), 'bicubic')]}[name]


@pytest.mark.parametrize('name', ['sr2', 'dn_sr2', 'sr2_resize_100x90_bilinear', 'sr2_resize_bicubic_up'])
def test_chain_run_sets_equal_the_restated_rules(name):
    chain = _chain(name)
    steps = [('tiles', s) if isinstance(s, TilePlan) else ('resize',) + s for s in chain]
    H, W = 100, 140
    tr = reuse.Tracker()
    masks, region = reuse.walk(tr, 'rgb', steps, reuse.none(H, W), (H, W))               # the first frame: no plan has run yet, whatever the map says
    assert all(m is None or m.all() for m in masks) and (region is None or region.all())
    rng = np.random.default_rng(5)
    partial = 0
    for trial in range(60):
        changed = rng.random(reuse.cells(H, W)) < rng.choice([0.0, 0.01, 0.02, 0.05])
        masks, region = reuse.walk(tr, 'rgb', steps, changed, (H, W))
        want = _restated(chain, changed, H, W)
        tiled = [m for m in masks if m is not None]
        assert len(tiled) == len(want)
        for i, (g, w_) in enumerate(zip(tiled, want)):
            assert np.array_equal(g, w_), (name, trial, i, g, w_)
        partial += int(0 < tiled[-1].sum() < len(tiled[-1]))
        last = chain[-1]
        oh, ow = (last.outH, last.outW) if isinstance(last, TilePlan) else last[0]
        assert region.shape == reuse.cells(oh, ow)
        if not changed.any():
            assert not region.any()
    assert partial > 10


# ---- the resize rule is a superset ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['nearest', 'bilinear', 'bicubic'])
@pytest.mark.parametrize('sizes', [((60, 84), (90, 100)), ((60, 84), (23, 31)), ((60, 84), (151, 200)), ((61, 83), (60, 84)), ((40, 40), (7, 130))],
                         ids=lambda s: '{0[0]}x{0[1]}_to_{1[0]}x{1[1]}'.format(*s))
def test_resize_rule_is_a_superset(mode, sizes):
    import torch
    import torch.nn.functional as F
    (H, W), (h, w) = sizes
    rng = np.random.default_rng(H * w)
    rects = [(0, 1, 0, 1), (H - 1, H, W - 1, W), (0, H, 0, 1), (H - 1, H, 0, W), (17, 18, 29, 30), (16, 32, 16, 32)]
    rects += [tuple(int(v) for v in (r0, r0 + dr, c0, c0 + dc)) for r0, dr, c0, dc in
              zip(rng.integers(0, H - 8, 12), rng.integers(1, 9, 12), rng.integers(0, W - 8, 12), rng.integers(1, 9, 12))]
    a = torch.from_numpy(rng.random((2, H, W), dtype=np.float32))
    fa = F.interpolate(a[None], size=(h, w), mode=mode, **({} if mode == 'nearest' else {'align_corners': False}))[0]
    for rect in rects:
        r0, r1, c0, c1 = rect
        b = a.clone()
        b[:, r0:r1, c0:c1] += 1.0
        fb = F.interpolate(b[None], size=(h, w), mode=mode, **({} if mode == 'nearest' else {'align_corners': False}))[0]
        diff = (fa != fb).any(0).numpy()
        o = reuse.resizeRect(rect, (H, W), (h, w), mode)
        inside = np.zeros((h, w), bool)
        inside[o[0]:o[1], o[2]:o[3]] = True
        assert (inside | ~diff).all(), (mode, sizes, rect, o, np.argwhere(diff & ~inside)[:4])
        region = reuse.resizeRegion(reuse.markRects(H, W, [rect]), (H, W), (h, w), mode)
        assert region.shape == reuse.cells(h, w) and (_pixels_of(region, h, w) | ~diff).all(), (mode, sizes, rect)
    assert not reuse.resizeRegion(reuse.none(H, W), (H, W), (h, w), mode).any()
    with pytest.raises(ValueError):
        reuse.resizeRegion(reuse.none(H, W), (H, W), (h, w), 'area')


# ---- fallbacks ----------------------------------------------------------------------------------------------------------------------------------
def test_a_step_without_a_rule_runs_everything_and_marks_everything():
    pl = _plan('rgb_100x140_c48_p5_x2')
    tr = reuse.Tracker()
    steps = [('tiles', pl, False)]                                    # an SR with ensemble = 3: the module has no rule for it
    for changed in (reuse.none(100, 140), reuse.none(100, 140), None):
        masks, region = reuse.walk(tr, 'rgb', steps, changed, (100, 140))
        assert masks[0].all() and len(masks[0]) == pl.n_tiles and region.all() and region.shape == reuse.cells(200, 280)
    masks, region = reuse.walk(tr, 'rgb', [('opaque',), ('tiles', pl)], reuse.none(100, 140), (100, 140))      # behind a step the walk cannot see through: unknown input
    assert masks[0] is None and masks[1].all() and region.all()
    masks, region = reuse.walk(tr, 'rgb', [('opaque',), ('tiles', pl)], reuse.none(100, 140), (100, 140))
    assert masks[1].all() and region.all()


def test_a_changed_plan_object_runs_everything():
    a, b = _plan('rgb_100x140_c48_p5_x2'), _plan('rgb_100x140_c48_p5_x2')
    tr = reuse.Tracker()
    quiet = reuse.none(100, 140)
    assert tr.step('k', a, quiet)[0].all()                            # the first frame
    m, r = tr.step('k', a, quiet)
    assert m.sum() == 0 and not r.any()
    m, r = tr.step('k', b, quiet)                                     # a re-plan / an eviction from the plan cache: an equal plan, another object
    assert m.all() and r.all()
    assert tr.step('k', b, quiet)[0].sum() == 0
    assert tr.step('other', b, quiet)[0].all()                        # another step of the chain keeps its own memory
    tr.forget('k')
    assert tr.step('k', b, quiet)[0].all()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_changed_blocks_refuses_bad_arguments_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    cb = lambda cur, prev, n, rows, rb, br, bb, m: L.moe_changed_blocks(cur, prev, n, rows, rb, br, bb, m, 0, None)
    for args in ((None, p + 1024, 1, 4, 16, 2, 8, p + 2048), (p, None, 1, 4, 16, 2, 8, p + 2048), (p, p + 1024, 1, 4, 16, 2, 8, None)):
        assert cb(*args) == _lib.EINVAL and b'moe_changed_blocks: NULL' in L.moe_last_error()
    for n, rows, rb in ((0, 4, 16), (-1, 4, 16), (1, 0, 16), (1, -4, 16), (1, 4, 0), (1, 4, -16)):
        assert cb(p, p + 1024, n, rows, rb, 2, 8, p + 2048) == _lib.EINVAL and b'must be 1 at least' in L.moe_last_error(), (n, rows, rb)
    for br, bb in ((0, 8), (-2, 8), (2, 0), (2, -8)):
        assert cb(p, p + 1024, 1, 4, 16, br, bb, p + 2048) == _lib.EINVAL and b'blocks of' in L.moe_last_error(), (br, bb)
    assert cb(p, p, 1, 4, 16, 2, 8, p + 2048) == _lib.EINVAL and b'same buffer' in L.moe_last_error()
    for cur, prev in ((p, p + 63), (p + 63, p), (p, p + 1), (p + 100, p + 40)):                 # 64 bytes each
        assert cb(cur, prev, 1, 4, 16, 2, 8, p + 2048) == _lib.EINVAL and b'overlap' in L.moe_last_error(), (cur - p, prev - p)
    assert cb(p, p + 127, 2, 4, 16, 2, 8, p + 2048) == _lib.EINVAL and b'overlap' in L.moe_last_error()      # two matrices: 128 bytes each
    assert cb(p, p + 1024, 1 << 30, 1 << 30, 1 << 40, 2, 8, p + 2048) == _lib.EINVAL and b'63 bits' in L.moe_last_error()
    assert cb(p, p + (1 << 45), 1, 1 << 20, 1 << 20, 1, 1, p + 2048) == _lib.EINVAL and b'cells' in L.moe_last_error()


def test_run_plan_subset_refuses_bad_arguments_without_a_device():
    L = _lib.lib()
    pl = _plan('rgb_100x140_c48_p5_x2')
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    run = (ctypes.c_uint8 * pl.n_tiles)(*([1] * pl.n_tiles))
    net = ctypes.c_void_p()
    _lib.check(L.moe_net_create(_lib.ARCH_NET2X, 2, ctypes.byref(net)))
    try:
        sub = lambda n, plan, img, r, pool: L.moe_run_plan_subset(n, plan, img, _lib.F32, 14000, 140, 1, r, pool, 0, None)
        for args in ((None, pl._h, p, run, p), (net, None, p, run, p), (net, pl._h, None, run, p), (net, pl._h, p, None, p), (net, pl._h, p, run, None)):
            assert sub(*args) == _lib.EINVAL and b'moe_run_plan_subset: NULL' in L.moe_last_error()
        assert sub(net, pl._h, p, run, p) == _lib.ESTATE and b'moe_run_plan_subset: net is not finalized' in L.moe_last_error()
    finally:
        L.moe_net_destroy(net)
    assert 'moe_changed_blocks' in _lib.EXPORTS and 'moe_run_plan_subset' in _lib.EXPORTS and L.moe_abi_version() == 4


def test_genframestream_refuses_a_reuse_that_is_not_a_bool_before_any_model_is_loaded():
    from moephoto_amd import imageProcess, procedure
    before = dict(imageProcess.modelCache)
    sr = {'op': 'SR', 'model': 'no such model', 'scale': 2}
    for bad in (1, 0, 'yes', None, 1.0):
        for steps in ([{'op': 'buffer', 'bitDepth': 16}, sr], [{'op': 'buffer', 'pixFmt': 'yuv420p10le'}, sr],
                      [{'op': 'buffer', 'bitDepth': 8}, sr, {'op': 'output', 'pixFmt': 'yuv420p'}]):
            with pytest.raises(ValueError, match='reuse must be True or False'):
                procedure.genFrameStream(steps, 140, 100, 2, reuse=bad)
    # the refusals the stream already had still come first
    with pytest.raises(ValueError, match='first step'):
        procedure.genFrameStream([sr], 140, 100, 2, reuse='x')
    with pytest.raises(ValueError, match='depth must be 1..4'):
        procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 16}, sr], 140, 100, 9, reuse='x')
    with pytest.raises(ValueError, match='bitDepth must be 8 or 16'):
        procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 12}, sr], 140, 100, 2, reuse='x')
    with pytest.raises(ValueError, match='depth must be 1..4'):
        procedure.genFrameStream([{'op': 'buffer', 'pixFmt': 'yuv420p'}, sr], 140, 100, 0, reuse='x')
    with pytest.raises(ValueError):
        procedure.genFrameStream([{'op': 'buffer', 'pixFmt': 'yuv420p'}, sr], 141, 100, 2, reuse='x')             # an odd width
    with pytest.raises(ValueError, match='pixFmt'):
        procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 8}, sr, {'op': 'output', 'pixFmt': 'nv12'}], 140, 100, 2, reuse='x')
    assert imageProcess.modelCache == before
