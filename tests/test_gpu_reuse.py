"""The frame stream's reuse on the device (`pytest -m gpu`):

  moe_changed_blocks                     against  numpy on the same bytes
  moe_run_plan_subset                    against  moe_run_plan_ex(do_stitch = 0), bit for bit, tile by tile
  genFrameStream(reuse=True)             against  genFrameStream(reuse=False), byte for byte per frame, and its counters against the CPU rule (moephoto_amd/reuse.py)
  one frame after a partial update       against  the oracle's doCrop (tests/test_gpu_planes.py's input kind and bound)

Equality is the bar everywhere but in the last."""
import ctypes

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import pixfmt, reuse

pytestmark = pytest.mark.gpu
W, H = 140, 100
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}
DN = {'op': 'DN', 'model': 'lite5', 'strength': 0.6}


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _st():
    return torch.cuda.current_stream().cuda_stream


def _configure(fp16, crop=48):
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, fp16
    config.crop_sr = config.crop_dn = config.crop_dns = crop
    config.ensembleSR = 0


# ---- 1. the change map ----------------------------------------------------------------------------------------------------------------------
def _np_map(cur, prev, n, rows, row_bytes, br, bb):
    """moe_changed_blocks' definition on host bytes."""
    d = (np.frombuffer(cur, np.uint8) != np.frombuffer(prev, np.uint8)).reshape(n, rows, row_bytes).any(0)
    nr, nc = -(-rows // br), -(-row_bytes // bb)
    p = np.zeros((nr * br, nc * bb), bool)
    p[:rows, :row_bytes] = d
    return p.reshape(nr, br, nc, bb).any(axis=(1, 3)).astype(np.uint8)


def _matrices(kind, w, h, es):
    """The calls a frame of this kind takes: (byte offset, n, rows, row_bytes, block_rows, block_bytes) each, and the frame's bytes."""
    if kind == 'interleaved':
        return [(0, 1, h, w * 3 * es, 16, 48 * es)], w * h * 3 * es
    return [(0, 1, h, w * es, 16, 16 * es), (w * h * es, 2, h // 2, w // 2 * es, 16, 16 * es)], w * h * 3 // 2 * es


# (136 x 40 at 16 bits, 176 x 48 planar at 10 bits: rows of a multiple of 16 bytes -- the 16-byte path on an aligned base, with a ragged last block row and column)
MAP_CASES = [('interleaved', 140, 100, 2), ('interleaved', 140, 100, 1), ('interleaved', 37, 19, 2), ('interleaved', 37, 19, 1), ('interleaved', 136, 40, 2),
             ('planar', 140, 100, 1), ('planar', 140, 100, 2), ('planar', 2, 2, 1), ('planar', 2, 2, 2), ('planar', 176, 48, 2)]


@pytest.mark.parametrize('case', MAP_CASES, ids=lambda c: '{}_{}x{}_{}B'.format(*c))
def test_changed_blocks_against_numpy(case, dev):
    from moephoto_amd import _lib
    L = _lib.lib()
    kind, w, h, es = case
    calls, nbytes = _matrices(kind, w, h, es)
    rng = np.random.default_rng(w * h + es)
    base = rng.integers(0, 256, nbytes, dtype=np.uint8)
    off, n, rows, rb, br, bb = calls[-1]
    o0, _, rows0, rb0, br0, _ = calls[0]
    variants = {'equal': [], 'first_byte': [0], 'last_byte': [nbytes - 1],
                'end_of_the_first_block_row': [o0 + min(rows0, br0) * rb0 - 1],        # its last column: ragged where row_bytes is no multiple of block_bytes
                'end_of_the_last_block_row': [o0 + rows0 * rb0 - 1],                   # ragged where rows is no multiple of block_rows
                'sparse': list(rng.integers(0, nbytes, 7)), 'all': None}
    if kind == 'planar':
        variants['only_in_cr'] = [off + rows * rb + (rows * rb) // 2]   # inside the second chroma matrix
    took_vec = False
    for lead in (0, 1):                                                 # an aligned base, and one byte behind a 16-byte boundary, between sentinels
        for name, where in variants.items():
            prev = base.copy()
            cur = base.copy()
            if where is None:
                cur = (base + rng.integers(1, 256, nbytes, dtype=np.uint8)).astype(np.uint8)
            else:
                for i in where:
                    cur[i] ^= 0x40
            dc = torch.full((lead + nbytes + 32,), 0xA5, dtype=torch.uint8, device=dev)
            dp = torch.full((lead + nbytes + 32,), 0x5A, dtype=torch.uint8, device=dev)
            assert dc.data_ptr() % 16 == 0 and dp.data_ptr() % 16 == 0
            dc[lead:lead + nbytes] = torch.from_numpy(cur).to(dev)
            dp[lead:lead + nbytes] = torch.from_numpy(prev).to(dev)
            sizes = [(-(-c[2] // c[4])) * (-(-c[3] // c[5])) for c in calls]
            dm = torch.full((sum(sizes) + 8,), 0x77, dtype=torch.uint8, device=dev)
            at = 0
            for (o, n_, rows_, rb_, br_, bb_), size in zip(calls, sizes):
                took_vec |= lead == 0 and o % 16 == 0 and rb_ % 16 == 0 and bb_ % 16 == 0
                _lib.check(L.moe_changed_blocks(dc.data_ptr() + lead + o, dp.data_ptr() + lead + o, n_, rows_, rb_, br_, bb_, dm.data_ptr() + at, 0, _st()))
                at += size
            got, hc, hp = dm.cpu().numpy(), dc.cpu().numpy(), dp.cpu().numpy()
            at = 0
            for (o, n_, rows_, rb_, br_, bb_), size in zip(calls, sizes):
                m = n_ * rows_ * rb_
                want = _np_map(cur[o:o + m].tobytes(), prev[o:o + m].tobytes(), n_, rows_, rb_, br_, bb_)
                assert np.array_equal(got[at:at + size].reshape(want.shape), want), (case, lead, name, o)
                if name == 'equal':
                    assert not want.any()
                elif name == 'all':
                    assert want.all()
                elif name != 'sparse':
                    assert want.sum() == (1 if o <= where[0] < o + m else 0)
                at += size
            assert (got[at:] == 0x77).all()                              # the map ends where it should
            assert np.array_equal(hp[lead:lead + nbytes], cur), (case, lead, name)                  # prev retains cur
            assert np.array_equal(hc[lead:lead + nbytes], cur)
            assert (hp[:lead] == 0x5A).all() and (hp[lead + nbytes:] == 0x5A).all() and (hc[:lead] == 0xA5).all() and (hc[lead + nbytes:] == 0xA5).all()
    assert took_vec == (case in (('interleaved', 136, 40, 2), ('planar', 176, 48, 2))), 'which cases take the 16-byte path is part of what this test covers'


# ---- 2. the subset runner -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def a2(dev):
    """a2 with 48-pixel tiles on a 3 x 100 x 140 image: 12 tiles; the reference pool of moe_run_plan_ex(do_stitch = 0), computed once."""
    from moephoto_amd import _lib, imageProcess as ip, runSR
    from moephoto_amd.config import config
    _configure(True)
    opt = runSR.getOpt(dict(SR))
    x = torch.from_numpy(gd.noise_image(31, (3, H, W))).to(dev).to(config.dtype())
    plan = ip._plan_for(opt, x.shape)
    xp = plan.padImage(x).contiguous()
    assert plan.n_tiles == 12
    want = _run_ex(opt.modelCached, plan, xp, dev)
    return opt.modelCached, plan, xp, want.cpu().numpy()


def _run_ex(model, plan, xp, dev):
    from moephoto_amd import _lib
    from moephoto_amd.imageProcess import _DT
    pool = torch.full((plan.pool_elems(xp.shape[0]),), -3.0, dtype=torch.float32, device=dev)
    sC, sH, sW = xp.stride()
    _lib.check(_lib.lib().moe_run_plan_ex(model._h, plan._h, xp.data_ptr(), _DT[xp.dtype], sC, sH, sW, None, _lib.F32, 0, pool.data_ptr(), 0, 1, 0, _st()))
    return pool


def _run_subset(model, plan, xp, mask, pool):
    from moephoto_amd import _lib
    from moephoto_amd.imageProcess import _DT
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    sC, sH, sW = xp.stride()
    _lib.check(_lib.lib().moe_run_plan_subset(model._h, plan._h, xp.data_ptr(), _DT[xp.dtype], sC, sH, sW, m.ctypes.data, pool.data_ptr(), 0, _st()))


def _tile_spans(plan, C):
    off = plan.tile_offsets(C)
    return [(off[k], off[k] + C * (t[1] - t[0]) * plan.sc * (t[3] - t[2]) * plan.sc) for k, t in enumerate(plan.tiles)]


def _check_pool(got, want, spans, mask, fill, what):
    covered = np.zeros(got.size, bool)
    for (a, b), m in zip(spans, mask):
        covered[a:b] = True
        if m:
            assert np.array_equal(got[a:b].view(np.uint32), want[a:b].view(np.uint32)), '{}: a tile that ran differs'.format(what)
        else:
            assert (got[a:b] == fill).all(), '{}: a tile that did not run was written'.format(what)
    assert (got[~covered] == fill).all()


def test_run_plan_subset_with_every_tile_equals_run_plan_ex(a2, dev):
    model, plan, xp, want = a2
    pool = torch.full((want.size,), -3.0, dtype=torch.float32, device=dev)
    _run_subset(model, plan, xp, np.ones(plan.n_tiles, np.uint8), pool)
    assert np.array_equal(pool.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_run_plan_subset_with_a_mask_touches_only_its_tiles(a2, dev):
    model, plan, xp, want = a2
    spans = _tile_spans(plan, 3)
    rng = np.random.default_rng(3)
    for mask in (rng.integers(0, 2, plan.n_tiles), np.eye(plan.n_tiles, dtype=np.uint8)[plan.n_tiles - 1], np.zeros(plan.n_tiles, np.uint8), 7 * np.eye(plan.n_tiles, dtype=np.uint8)[0]):
        pool = torch.full((want.size,), 123.0, dtype=torch.float32, device=dev)
        _run_subset(model, plan, xp, mask, pool)
        _check_pool(pool.cpu().numpy(), want, spans, mask, 123.0, mask)


def test_forty_masks_in_a_row_equal_fresh_plans(a2, dev):
    """More calls than the table ring has buffers, none of them waited for: every mask's tiles are those a fresh plan computes, nothing else is written."""
    from moephoto_amd.imageProcess import TilePlan
    model, plan, xp, want = a2
    spans = _tile_spans(plan, 3)
    rng = np.random.default_rng(17)
    masks = [rng.integers(0, 2, plan.n_tiles).astype(np.uint8) for _ in range(40)]
    assert len({m.tobytes() for m in masks}) > 32
    pools = [torch.full((want.size,), 9.0, dtype=torch.float32, device=dev) for _ in masks]
    for m, p in zip(masks, pools):
        _run_subset(model, plan, xp, m, p)
    torch.cuda.synchronize()
    for i, (m, p) in enumerate(zip(masks, pools)):
        got = p.cpu().numpy()
        _check_pool(got, want, spans, m, 9.0, 'mask {}'.format(i))
        if i % 8 == 0:
            fresh = TilePlan(plan.shape, 1 << 40, 1e-3, plan.pad, plan.sc, plan.align, 48)
            assert fresh.tiles == plan.tiles
            q = torch.full((want.size,), 9.0, dtype=torch.float32, device=dev)
            _run_subset(model, fresh, xp, m, q)
            assert np.array_equal(q.cpu().numpy().view(np.uint32), got.view(np.uint32)), i


def test_the_tile_table_cache_still_serves_run_plan_tiles(a2, dev):
    """moe_run_plan_tiles with more destination tables than its cache keeps, subset calls in between: both as before."""
    from moephoto_amd import _lib
    from moephoto_amd.imageProcess import _DT
    model, plan, xp, want = a2
    spans, off = _tile_spans(plan, 3), plan.tile_offsets(3)
    sC, sH, sW = xp.stride()
    rng = np.random.default_rng(23)
    for i in range(20):
        mask = rng.integers(0, 2, plan.n_tiles).astype(np.uint8)
        mask[i % plan.n_tiles] = 1
        dst = (ctypes.c_int64 * plan.n_tiles)(*[o if m else -1 for o, m in zip(off, mask)])
        pool = torch.full((want.size,), 5.0, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().moe_run_plan_tiles(model._h, plan._h, xp.data_ptr(), _DT[xp.dtype], 0, sC, sH, sW, 1, pool.data_ptr(), dst, 0, _st()))
        _check_pool(pool.cpu().numpy(), want, spans, mask, 5.0, 'tiles {}'.format(i))
        pool2 = torch.full((want.size,), 5.0, dtype=torch.float32, device=dev)
        _run_subset(model, plan, xp, 1 - mask, pool2)
        _check_pool(pool2.cpu().numpy(), want, spans, 1 - mask, 5.0, 'subset {}'.format(i))


# ---- 3. streams -----------------------------------------------------------------------------------------------------------------------------
def _interleaved_frames(bits, seed=5):
    """random; one 8 x 8 patch changed inside a tile's interior; a duplicate; wholly new; one pixel changed inside an overlap band; the last pixel of the last row."""
    rng = np.random.default_rng(seed)
    new, top = (lambda: rng.integers(0, 1 << bits, (H, W, 3), dtype=np.uint16)), 1 << (bits - 1)      # (a change of half the range: no rounding can hide it)
    f1 = new()
    f2 = f1.copy()
    f2[8:16, 8:16] ^= top
    f4 = new()
    f5 = f4.copy()
    f5[20, 45, 1] ^= top
    f6 = f5.copy()
    f6[H - 1, W - 1, 2] ^= top
    dt = np.uint8 if bits == 8 else np.dtype('<u2')
    return [f.astype(dt).tobytes() for f in (f1, f2, f2, f4, f5, f6)]


def _planar_frames(fmt, seed=5):
    depth = pixfmt.FORMATS[fmt]
    rng = np.random.default_rng(seed)
    ny = W * H
    new, top = (lambda: rng.integers(0, 1 << depth, ny * 3 // 2, dtype=np.uint16)), 1 << (depth - 1)
    f1 = new()
    f2 = f1.copy()
    y = f2[:ny].reshape(H, W)
    y[8:16, 8:16] ^= top
    cb = f2[ny:ny + ny // 4].reshape(H // 2, W // 2)
    cb[4:8, 4:8] ^= top
    f4 = new()
    f5 = f4.copy()
    f5[20 * W + 45] ^= top
    f6 = f5.copy()
    f6[ny - 1] ^= top
    f6[-1] ^= top                                                        # the last Cr sample
    dt = np.uint8 if depth == 8 else np.dtype('<u2')
    return [f.astype(dt).tobytes() for f in (f1, f2, f2, f4, f5, f6)]


# name -> (source step, the steps behind it, edge, the first tiled step's plan parameters (pad, scale) or None when the chain has no rule)
STREAMS = {'sr_a2_16bit': ({'op': 'buffer', 'bitDepth': 16}, [dict(SR)], 'crop', (5, 2)),
           'sr_a2_yuv_out': ({'op': 'buffer', 'bitDepth': 16}, [dict(SR), {'op': 'output', 'pixFmt': 'yuv420p10le'}], 'crop', (5, 2)),
           'dn_0.6': ({'op': 'buffer', 'bitDepth': 16}, [dict(DN)], 'filter', (7, 1)),
           'dn_0.6_sr_a2': ({'op': 'buffer', 'bitDepth': 8}, [dict(DN), dict(SR)], 'crop', (7, 1)),
           'sr_a2_resize': ({'op': 'buffer', 'bitDepth': 8}, [dict(SR), {'op': 'resize', 'width': 100, 'height': 90, 'method': 'bilinear'}], 'quantise', (5, 2)),
           'sr_a2_ensemble_1': ({'op': 'buffer', 'bitDepth': 16}, [dict(SR, ensemble=1)], 'quantise', None),
           'planar_sr_a2': ({'op': 'buffer', 'pixFmt': 'yuv420p10le'}, [dict(SR)], 'crop', (5, 2)),
           'planar_sr_a2_dn_0.6': ({'op': 'buffer', 'pixFmt': 'yuv420p10le'}, [dict(SR), dict(DN)], 'quantise', (5, 2))}


def _frames_of(source):
    return _planar_frames(source['pixFmt']) if 'pixFmt' in source else _interleaved_frames(source['bitDepth'])


def _run(steps, frames, depth, reuse_):
    from moephoto_amd import procedure
    stream = procedure.genFrameStream([dict(s) for s in steps], W, H, depth, reuse=reuse_)
    out = []
    for f in frames:
        out += stream.push(f)
    out += stream.flush()
    stats = stream.reuse
    edge, nodes = stream.edge, stream.nodes
    stream.close()
    return out, stats, edge, nodes


def _first_step_counts(source, frames, first):
    """What the CPU rule gives for the first tiled step of each image: per frame {image: tiles run}, from the cell maps of consecutive raw frames."""
    from moephoto_amd.imageProcess import TilePlan
    pad, sc = first
    planar = 'pixFmt' in source
    es = 1 if (pixfmt.FORMATS[source['pixFmt']] if planar else source['bitDepth']) == 8 else 2
    calls, _ = _matrices('planar' if planar else 'interleaved', W, H, es)
    shapes = [('y', (1, H, W)), ('c', (2, H // 2, W // 2))] if planar else [('rgb', (3, H, W))]
    out = []
    for k in range(1, len(frames)):
        counts = {}
        for (image, shape), (o, n, rows, rb, br, bb) in zip(shapes, calls):
            pl = TilePlan(shape, 1 << 40, 1e-3, pad, sc, 8, 48)
            m = n * rows * rb
            changed = _np_map(frames[k][o:o + m], frames[k - 1][o:o + m], n, rows, rb, br, bb) != 0
            counts[image] = (pl.n_tiles, int(reuse.runSet(reuse.PlanRegions(pl), changed).sum()))
        out.append(counts)
    return out


@pytest.mark.parametrize('name', sorted(STREAMS))
def test_reuse_stream_equals_the_plain_stream(name, dev):
    _configure(True)
    source, work, edge, first = STREAMS[name]
    steps = [source] + work
    frames = _frames_of(source)
    assert frames[1] == frames[2] and len(set(frames)) == 5
    want, none_, edge0, nodes0 = _run(steps, frames, 2, False)
    assert none_ is None and edge0 == edge and len(want) == 6 and want[1] == want[2] and len(set(want)) == 5
    for depth in (1, 2, 3):
        got, stats, edge1, nodes1 = _run(steps, frames, depth, True)
        assert edge1 == edge and nodes1 == nodes0 and len(got) == 6
        for k, (g, w_) in enumerate(zip(got, want)):
            assert len(g) == len(w_)
            assert g == w_, '{} ring depth {} frame {}: {} bytes differ'.format(name, depth, k, int((np.frombuffer(g, np.uint8) != np.frombuffer(w_, np.uint8)).sum()))
        per_frame = list(stats['frames'])
        assert len(per_frame) == 6
        if first is None:                                             # no rule: the step runs as it is, nothing is counted
            assert all(not f for f in per_frame) and stats['pixels_planned'] == 0
            continue
        keys = sorted(per_frame[0])
        assert keys and all(sorted(f) == keys for f in per_frame)
        for k in (0, 3):                                              # the first frame and the wholly new one: everything runs
            assert all(run == planned and planned > 1 for planned, run in per_frame[k].values()), (name, depth, k, per_frame[k])
        assert all(run == 0 for _, run in per_frame[2].values()), (name, depth, per_frame[2])       # the duplicate: nothing runs, in any step
        rule = _first_step_counts(source, frames, first)
        for k in (1, 2, 4, 5):
            for image, (planned, run) in rule[k - 1].items():
                assert per_frame[k][(0, image)] == (planned, run), (name, depth, k, image, per_frame[k], rule[k - 1])
        if 'pixFmt' not in source:
            assert rule[0]['rgb'][1] == 1 and rule[3]['rgb'][1] >= 2 and 1 <= rule[4]['rgb'][1] < rule[4]['rgb'][0]      # one tile's interior; both neighbours of a band; the corner
        for k in (1, 4, 5):                                           # a partial update stays partial in every step
            assert all(run < planned for planned, run in per_frame[k].values()), (name, depth, k, per_frame[k])
        tiles = stats['tiles']
        assert sorted(tiles) == keys and all(tiles[key] == [sum(f[key][0] for f in per_frame), sum(f[key][1] for f in per_frame)] for key in keys)
        assert 0 < stats['pixels_run'] < stats['pixels_planned']


def test_a_frame_after_a_partial_update_against_the_oracle(dev):
    """tests/test_gpu_planes.py's oracle case -- fp32 images, a planar 10-bit frame of noise over the format's codes, |code - clamp(oracle * 2^D)| <= 1e-3 * 2^D + 1 --
    on the SECOND frame of a reuse stream: most of its tiles are the first frame's, kept in the pool."""
    from moephoto_amd import procedure
    from moephoto_amd.weights import load_state_dict_file
    from oracle import nets as onets, planner as oplanner, stitch as ostitch
    _configure(False)
    D, fmt = 10, 'yuv420p10le'
    a = np.random.default_rng(77).integers(0, 1 << D, W * H * 3 // 2, dtype=np.uint16)
    b = a.copy()
    b[:W * H].reshape(H, W)[50:58, 60:68] ^= 0x155
    b[W * H:W * H + W * H // 4].reshape(H // 2, W // 2)[25:29, 30:34] ^= 0x155
    stream = procedure.genFrameStream([{'op': 'buffer', 'pixFmt': fmt}, dict(SR)], W, H, 1, reuse=True)
    got = stream.push(a.astype('<u2').tobytes()) + stream.push(b.astype('<u2').tobytes()) + stream.flush()
    second = dict(list(stream.reuse['frames'])[1])
    stream.close()
    assert len(got) == 2 and all(0 < run < planned for planned, run in second.values()), second
    codes = np.frombuffer(got[1], '<u2').astype(np.float64)
    model = onets.model_fn('net2x', gd.state_dict_for('a2', load_state_dict_file))
    planes = []
    for p in pixfmt.toPlanes(b.astype('<u2').tobytes(), fmt, W, H, np.float32):
        pl = oplanner.prepare(p.shape, 1 << 40, 1e-3, 5, 2, 8, 48)
        planes.append(ostitch.do_crop(p, pl, 2, model).astype(np.float64).reshape(-1))
    want = np.clip(np.concatenate(planes) * (1 << D), 0, (1 << D) - 1)
    err = float(np.abs(codes - want).max())
    print('reuse stream, frame 2 of planar a2 140x100 at {} bits: max |code - oracle| = {:.3f} codes (bound {:.3f}); tiles run {}'.format(D, err, 1e-3 * (1 << D) + 1, second))
    assert codes.size == want.size and err <= 1e-3 * (1 << D) + 1, err


# ---- 4. failure handling --------------------------------------------------------------------------------------------------------------------
def test_a_stream_closed_in_flight_leaves_nothing_behind_for_the_next(dev):
    from moephoto_amd import procedure
    _configure(True)
    steps = [{'op': 'buffer', 'bitDepth': 16}, dict(DN), dict(SR)]
    frames = _interleaved_frames(16, seed=9)
    want, _, _, _ = _run(steps, frames, 2, False)
    first = procedure.genFrameStream([dict(s) for s in steps], W, H, 3, reuse=True)
    assert first.push(frames[3]) == [] and first.push(frames[4]) == []          # two frames in flight
    first.close()
    with pytest.raises(RuntimeError):
        first.push(frames[0])
    got, stats, _, _ = _run(steps, frames, 3, True)                              # the state is the stream's: the next one starts from nothing
    assert got == want
    assert all(run == planned for planned, run in list(stats['frames'])[0].values())


def test_an_exception_in_a_stage_closes_a_reuse_stream(dev):
    from moephoto_amd import procedure
    _configure(True)
    frames = _interleaved_frames(16)
    stream = procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 16}, dict(SR)], W, H, 2, reuse=True)
    assert stream.push(frames[0]) == []

    def boom(*a, **k):
        raise RuntimeError('boom')
    stream.backend.edge = boom
    with pytest.raises(RuntimeError, match='boom'):
        stream.push(frames[1])
    assert stream.closed
    with pytest.raises(RuntimeError, match='closed'):
        stream.push(frames[2])
    stream.close()
