"""The streamed frame path on the device, byte for byte against the serial path it replaces (`pytest -m gpu`):

  moe_stitch_out                        against  moe_stitch -> fp32 -> moe_to_output
  imageProcess.doCropOut                against  toOutput(bits)(toFloat(doCrop(opt, x)))
  genFrameStream + runFramesStreamed    against  genProcess + runFrames

Both sides of every comparison run in this process on the same fp32 tile values through the same stitch_pixel and the same quantiser arithmetic: equality is the bar,
there is no tolerance anywhere in this file."""
import ctypes
import glob
import io
import os

import numpy as np
import pytest
import torch

import golden_defs as gd

pytestmark = pytest.mark.gpu
G = gd.GOLDEN


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------
def _golden_plans():
    """The nine plans of tests/golden/stitch_only, read for their parameters only: multi-tile grids, one-tile reflect-padded axes, the 8-pixel last tile."""
    for p in sorted(glob.glob(os.path.join(G, 'stitch_only', '*.npz'))):
        z = np.load(p)
        yield os.path.basename(p)[:-4], (tuple(int(v) for v in z['shape']), int(z['sc']), int(z['pad']), int(z['align']), int(z['crop']))


PLANS = dict(_golden_plans())
PLANS.update({'one_tile_odd_width_x3': ((3, 37, 45), 3, 9, 8, 0),        # out_w = 135: no run of eight ends the row, unaligned stores
              'rgb_100x140_c48': ((3, 100, 140), 2, 5, 8, 48), 'gray_100x140_c48': ((1, 100, 140), 2, 5, 8, 48), 'rgba_100x140_c48': ((4, 100, 140), 2, 5, 8, 48)})
_OUT = {8: (torch.uint8, 2), 16: (torch.int16, 3)}       # bits -> (storage, library dtype MOE_U8 / MOE_U16)


def _plan_and_pool(params, dev, order=None):
    """TilePlan + a pool seeded per tile as in test_stitch_kernel_golden, but drawn from [-0.25, 1.25): both clamps are hit.  order: the tiles' order in the pool."""
    from moephoto_amd.imageProcess import TilePlan
    shape, sc, pad, align, crop = params
    pl = TilePlan(shape, 1 << 40, 1e-3, pad, sc, align, crop)
    C = shape[0]
    sizes = [C * (t[1] - t[0]) * sc * (t[3] - t[2]) * sc for t in pl.tiles]
    if order is None:
        off = pl.tile_offsets(C)
    else:
        off, at = [0] * pl.n_tiles, 0
        for k in order:
            off[k] = at
            at += sizes[k]
    pool = np.empty(pl.pool_elems(C), np.float32)
    for k in range(pl.n_tiles):
        r = np.random.default_rng(9000 + k).random(sizes[k], dtype=np.float32) * np.float32(1.5) - np.float32(0.25)
        pool[off[k]:off[k] + sizes[k]] = r
    return pl, C, torch.from_numpy(pool).to(dev), off


def _three_passes(pl, C, pool_d, host_off, canvas_dt, bits, dev):
    """Today's path: the stitch into a canvas of canvas_dt, its fp32 copy, the quantiser."""
    from moephoto_amd import _lib
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    canvas = torch.empty((C, pl.outH, pl.outW), dtype=canvas_dt, device=dev)
    off = (ctypes.c_int64 * pl.n_tiles)(*host_off) if host_off is not None else None
    _lib.check(L.moe_stitch(pl._h, 0, pool_d.data_ptr(), off, C, canvas.data_ptr(), _lib.F16 if canvas_dt == torch.float16 else _lib.F32, st))
    f32 = canvas.float()
    want = torch.empty((pl.outH, pl.outW, C), dtype=_OUT[bits][0], device=dev)
    _lib.check(L.moe_to_output(f32.data_ptr(), _lib.F32, pl.outH, pl.outW, C, bits, want.data_ptr(), _OUT[bits][1], 0, st))
    return want


def _stitch_out(pl, C, pool_d, off_d, canvas_dt, bits, dev):
    from moephoto_amd import _lib
    got = torch.full((pl.outH, pl.outW, C), 77, dtype=_OUT[bits][0], device=dev)
    _lib.check(_lib.lib().moe_stitch_out(pl._h, 0, pool_d.data_ptr(), off_d.data_ptr() if off_d is not None else None, C,
                                         _lib.F16 if canvas_dt == torch.float16 else _lib.F32, bits, got.data_ptr(), _OUT[bits][1], torch.cuda.current_stream().cuda_stream))
    return got


@pytest.mark.parametrize('name', sorted(PLANS))
def test_stitch_out_equals_stitch_float_quantise(name, dev):
    pl, C, pool_d, _ = _plan_and_pool(PLANS[name], dev)
    for canvas_dt in (torch.float16, torch.float32):
        for bits in (8, 16):
            want = _three_passes(pl, C, pool_d, None, canvas_dt, bits, dev)
            got = _stitch_out(pl, C, pool_d, None, canvas_dt, bits, dev)
            torch.cuda.synchronize()
            samples = want.to(torch.int32) & 0xFFFF                     # (uint16 samples live in int16 storage)
            assert samples.min().item() == 0 and samples.max().item() == (1 << bits) - 1, 'the pool does not reach both clamps'
            bad = int((got != want).sum().item())
            assert bad == 0, '{} canvas {} bits {}: {} of {} samples differ'.format(name, canvas_dt, bits, bad, want.numel())


def test_stitch_out_with_a_permuted_pool_layout(dev):
    params = PLANS['rgb_100x140_c48']
    n = _plan_and_pool(params, dev)[0].n_tiles
    order = list(reversed(range(n)))
    pl, C, pool_d, off = _plan_and_pool(params, dev, order)
    assert n > 4 and off != pl.tile_offsets(C)
    off_d = torch.tensor(off, dtype=torch.int64, device=dev)
    want = _three_passes(pl, C, pool_d, off, torch.float16, 16, dev)
    got = _stitch_out(pl, C, pool_d, off_d, torch.float16, 16, dev)
    plain = _stitch_out(*_plan_and_pool(params, dev)[:3], None, torch.float16, 16, dev)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(got, plain)


def _stitch(pl, C, pool_d, dt, dev, out=None):
    from moephoto_amd import _lib
    if out is None:
        out = torch.empty((C, pl.outH, pl.outW), dtype=dt, device=dev)
    _lib.check(_lib.lib().moe_stitch(pl._h, 0, pool_d.data_ptr(), None, C, out.data_ptr(), _lib.F16 if dt == torch.float16 else _lib.F32, torch.cuda.current_stream().cuda_stream))
    return out


@pytest.mark.parametrize('width', [1100, 1104])
def test_stitch_of_more_than_64_tile_columns(width, dev):
    """92 tile columns x 2 tile rows (the column table of a block no longer has a size): the canvas against the oracle's fold, the fp16 canvas and the samples against
    the fp32 canvas.  Width 1100 ends every row on a ragged run of four pixels, 1104 on a whole run of eight."""
    from oracle import planner as oplanner, stitch as ostitch
    params = ((2, 24, width), 1, 2, 8, 16)
    pl, C, pool_d, off = _plan_and_pool(params, dev)
    opl = oplanner.prepare(params[0], 1 << 40, 1e-3, 2, 1, 8, 16)
    assert pl.stepW > 64 and (pl.stepW, pl.stepH, pl.n_tiles) == (92, 2, 184) and (opl.step_w, opl.step_h) == (92, 2) and pl.outW % 8 == width % 8
    f32 = _stitch(pl, C, pool_d, torch.float32, dev)
    f16 = _stitch(pl, C, pool_d, torch.float16, dev)
    want = _three_passes(pl, C, pool_d, None, torch.float16, 16, dev)
    got = _stitch_out(pl, C, pool_d, None, torch.float16, 16, dev)
    torch.cuda.synchronize()
    hp = pool_d.cpu().numpy()
    tiles = [hp[off[k]:off[k] + C * (t[1] - t[0]) * (t[3] - t[2])].reshape(C, t[1] - t[0], t[3] - t[2]) for k, t in enumerate(pl.tiles)]
    err = float(np.abs(f32.cpu().numpy() - ostitch.fold_stitch(tiles, opl, 1)).max())
    print('width {}: max abs error against the oracle fold {:.3e}'.format(width, err))
    assert err <= 1e-6
    assert torch.equal(f16, f32.half())
    assert torch.equal(got, want)


@pytest.mark.parametrize('name', sorted(PLANS))
def test_stitch_fp16_canvas_is_the_rounded_fp32_canvas_dense_and_unaligned(name, dev):
    """The canvas edge on every width and base: the fp16 canvas is the fp32 canvas rounded, written into a dense tensor and into one that starts one element past a
    16-byte boundary (no row of it can take a vector store); the elements in front of and behind the canvas stay as they were."""
    pl, C, pool_d, _ = _plan_and_pool(PLANS[name], dev)
    want = _stitch(pl, C, pool_d, torch.float32, dev).half()
    dense = _stitch(pl, C, pool_d, torch.float16, dev)
    n = C * pl.outH * pl.outW
    flat = torch.full((n + 2,), 7.0, dtype=torch.float16, device=dev)
    assert flat.data_ptr() % 16 == 0
    shifted = _stitch(pl, C, pool_d, torch.float16, dev, out=flat[1:n + 1].view(C, pl.outH, pl.outW))
    torch.cuda.synchronize()
    assert shifted.data_ptr() % 16 == 2
    assert torch.equal(dense, want)
    assert torch.equal(shifted, want)
    assert flat[0].item() == 7.0 and flat[n + 1].item() == 7.0


# ---- 2. doCropOut -------------------------------------------------------------------------------------------------------------------------
def _configure(fp16, crop):
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, fp16
    config.crop_sr = config.crop_dn = config.crop_dns = crop
    config.ensembleSR = 0


@pytest.mark.parametrize('case', ['a2_fp16', 'a2_fp32', 'dn_lite5', 'lite2'])
def test_docropout_equals_docrop_float_output(case, dev):
    from moephoto_amd import imageProcess as ip, runDN, runSR
    from moephoto_amd.config import config
    _configure(case != 'a2_fp32', 48)
    if case.startswith('a2'):
        opt, shape = runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}), (3, 100, 140)
    elif case == 'lite2':
        opt, shape = runSR.getOpt({'op': 'SR', 'model': 'lite', 'scale': 2, 'ensemble': 0}), (3, 72, 88)
    else:
        opt, shape = runDN.getOpt({'op': 'DN', 'model': 'lite5'}), (3, 72, 88)
    x = torch.from_numpy(gd.noise_image(31, shape)).to(dev).to(config.dtype())
    canvas = ip.doCrop(opt, x)
    assert canvas.dtype == config.dtype() and ip._plan_for(opt, x.shape).n_tiles > 1
    for bits in (8, 16):
        want = ip.toOutput(bits)(ip.toFloat(canvas))
        got = ip.doCropOut(opt, x, bits)
        assert got.device.type == 'cuda' and got.dtype == _OUT[bits][0] and tuple(got.shape) == want.shape
        got = got.cpu().numpy().view(want.dtype)
        bad = int((got != want).sum())
        assert bad == 0, '{} bits {}: {} of {} samples differ'.format(case, bits, bad, want.size)
    with pytest.raises(ValueError):
        ip.doCropOut(opt, x, 12)
    with pytest.raises(ValueError):
        ip.doCropOut(opt, x, 8, out=torch.empty((4, 4, 3), dtype=torch.uint8, device=dev))


# ---- 3. the stream ------------------------------------------------------------------------------------------------------------------------
H, W = 72, 88
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}


def _raw_frames(n, bits, seed=5):
    rng = np.random.default_rng(seed)
    return b''.join(rng.integers(0, 1 << bits, (H, W, 3), dtype=np.uint16).astype(np.uint8 if bits == 8 else np.uint16).tobytes() for _ in range(n))


def _both_ways(steps, raw, depth, **kw):
    from moephoto_amd import procedure
    bits = steps[0]['bitDepth']
    process, nodes = procedure.genProcess(steps, bitDepth=bits)
    want, got = [], []
    n0 = procedure.runFrames(process, io.BytesIO(raw).read, want.append, W, H, bitDepth=bits, **kw)
    stream = procedure.genFrameStream(steps, W, H, depth)
    assert stream.nodes == nodes
    n1 = procedure.runFramesStreamed(stream, io.BytesIO(raw).read, got.append, **kw)
    assert n1 == n0 == len(want) == len(got)
    assert len(set(want)) == len(want)                                   # distinct frames: a slot mix-up cannot hide
    for k, (g, w_) in enumerate(zip(got, want)):
        assert len(g) == len(w_)
        assert g == w_, 'frame {}: {} bytes differ'.format(k, int((np.frombuffer(g, np.uint8) != np.frombuffer(w_, np.uint8)).sum()))
    return stream, n1


@pytest.mark.parametrize('depth,kw', [(1, {}), (2, {}), (3, {}), (2, dict(start=1, stop=5))], ids=['depth1', 'depth2', 'depth3', 'depth2_start1_stop5'])
def test_streamed_sr_frames_equal_serial(depth, kw, dev):
    _configure(not kw, 64)                                               # (the windowed case runs with fp32 I/O, the others with the default fp16)
    stream, n = _both_ways([{'op': 'buffer', 'bitDepth': 16}, dict(SR)], _raw_frames(7, 16), depth, **kw)
    assert n == (5 if kw else 7)
    stream.close()
    with pytest.raises(RuntimeError):
        stream.push(_raw_frames(1, 16))


def test_streamed_unfused_edge_after_resize(dev):
    _configure(True, 64)
    steps = [{'op': 'buffer', 'bitDepth': 8}, {'op': 'DN', 'model': 'lite5', 'strength': 0.6}, dict(SR), {'op': 'resize', 'width': 100, 'height': 90, 'method': 'bilinear'}]
    stream, n = _both_ways(steps, _raw_frames(4, 8), 2)
    assert n == 4 and [d['op'] for d in stream.nodes] == ['DN', 'SR', 'resize']
    stream.close()


def test_streamed_ensemble(dev):
    _configure(True, 64)
    stream, n = _both_ways([{'op': 'buffer', 'bitDepth': 16}, dict(SR, ensemble=1)], _raw_frames(3, 16), 2)
    assert n == 3
    stream.close()


# ---- 4. nothing is allocated in steady state -----------------------------------------------------------------------------------------------
def test_stream_allocates_nothing_after_the_second_frame(dev):
    from moephoto_amd import procedure
    _configure(True, 64)
    raw = _raw_frames(7, 16)
    nb = len(raw) // 7
    stream = procedure.genFrameStream([{'op': 'buffer', 'bitDepth': 16}, dict(SR)], W, H, 2)
    out = []
    for k in range(2):
        out += stream.push(raw[k * nb:(k + 1) * nb])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    for k in range(2, 7):
        out += stream.push(raw[k * nb:(k + 1) * nb])
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated(dev)
    out += stream.flush()
    stream.close()
    assert len(out) == 7 and after <= before, (before, after)


def test_stream_stage_times(dev):
    """timing=True (tools/frame_stream_bench.py): the ring's events take timestamps and `stats` sums the stages of the collected frames; the bytes are the same."""
    from moephoto_amd import procedure
    _configure(True, 64)
    steps = [{'op': 'buffer', 'bitDepth': 16}, dict(SR)]
    raw = _raw_frames(4, 16)
    plain, timed = [], []
    a = procedure.genFrameStream(steps, W, H, 2)
    assert procedure.runFramesStreamed(a, io.BytesIO(raw).read, plain.append) == 4
    a.close()
    b = procedure.genFrameStream(steps, W, H, 2, timing=True)
    assert procedure.runFramesStreamed(b, io.BytesIO(raw).read, timed.append) == 4
    st = dict(b.backend.stats)
    b.close()
    assert timed == plain and st['frames'] == 4
    assert all(st[k] >= 0 for k in ('memcpy_ms', 'h2d_ms', 'compute_ms', 'd2h_ms', 'tobytes_ms')) and st['compute_ms'] > 0 and st['d2h_ms'] > 0
