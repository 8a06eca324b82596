"""The encoder's Y'CbCr 4:2:0 frames on the device (`pytest -m gpu`).  The comparator is always moephoto_amd.pixfmt.fromSamples16 -- the written definition, integer
arithmetic in numpy -- applied to the 16-bit samples of a path that exists without this feature:

  moe_stitch_yuv                        against  moe_stitch_out(bits = 16)
  moe_to_yuv                            against  moe_to_output(bits = 16)
  imageProcess.doCropYuv                against  doCropOut(.., 16)
  genFrameStream with an output step    against  genProcess + runFrames with the same step, and against the bgr48le stream's own bytes

Equality is the bar: there is no tolerance anywhere in this file."""
import io

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import pixfmt

pytestmark = pytest.mark.gpu
FMT = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le', 16: 'yuv420p16le'}


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _dt(t):
    from moephoto_amd import _lib
    return _lib.F16 if t == torch.float16 else _lib.F32


def _differ(got, want):
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    return 'sizes {} / {}'.format(g.size, w.size) if g.size != w.size else '{} of {} bytes differ, the first at {}'.format(int((g != w).sum()), g.size, int(np.argmax(g != w)))


# ---- 1. the fold's edge ---------------------------------------------------------------------------------------------------------------------
PLANS = {'even_3x4_tiles': ((3, 100, 140), 2, 5, 8, 48),             # out 200 x 280
         'odd_111x135_one_tile': ((3, 37, 45), 3, 9, 8, 0),          # both odd, no whole run of eight ends a row
         'odd_61x75_3x3_tiles': ((3, 61, 75), 1, 7, 8, 32),          # tile origins and blend bands at odd rows and columns
         'wide_172_tile_columns': ((3, 24, 2060), 1, 2, 8, 16)}      # a second block column, a ragged end of four
EXTRAS = 'odd_61x75_3x3_tiles'


def _plan_and_pool(params, dev, order=None):
    """TilePlan + a pool seeded per tile and drawn from [-0.25, 1.25): both clamps are hit.  order: the tiles' order in the pool."""
    from moephoto_amd.imageProcess import TilePlan
    shape, sc, pad, align, crop = params
    pl = TilePlan(shape, 1 << 40, 1e-3, pad, sc, align, crop)
    sizes = [3 * (t[1] - t[0]) * sc * (t[3] - t[2]) * sc for t in pl.tiles]
    if order is None:
        off = pl.tile_offsets(3)
    else:
        off, at = [0] * pl.n_tiles, 0
        for k in order:
            off[k] = at
            at += sizes[k]
    pool = np.empty(pl.pool_elems(3), np.float32)
    for k in range(pl.n_tiles):
        pool[off[k]:off[k] + sizes[k]] = np.random.default_rng(4200 + k).random(sizes[k], dtype=np.float32) * np.float32(1.5) - np.float32(0.25)
    return pl, torch.from_numpy(pool).to(dev), off


def _samples16(pl, pool_d, off_d, canvas_dt, dev):
    """moe_stitch_out(bits = 16) as an (H, W, 3) uint16 array."""
    from moephoto_amd import _lib
    out = torch.empty((pl.outH, pl.outW, 3), dtype=torch.int16, device=dev)
    _lib.check(_lib.lib().moe_stitch_out(pl._h, 0, pool_d.data_ptr(), off_d.data_ptr() if off_d is not None else None, 3, _dt(canvas_dt), 16,
                                         out.data_ptr(), _lib.U16, torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy().view(np.uint16)


def _stitch_yuv(pl, pool_d, off_d, canvas_dt, depth, dev, matrix='bt709', order='bgr', dst=None):
    from moephoto_amd import _lib
    n = pixfmt.frameBytes(FMT[depth], pl.outW, pl.outH)
    if dst is None:
        dst = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
    assert dst.numel() == n
    _lib.check(_lib.lib().moe_stitch_yuv(pl._h, 0, pool_d.data_ptr(), off_d.data_ptr() if off_d is not None else None, _dt(canvas_dt), depth,
                                         pixfmt.MATRICES[matrix], pixfmt.ORDERS[order], dst.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return dst.cpu().numpy().tobytes()


@pytest.fixture(scope='module')
def extras(dev):
    pl, pool_d, off = _plan_and_pool(PLANS[EXTRAS], dev)
    return pl, pool_d, off, _samples16(pl, pool_d, None, torch.float16, dev)


@pytest.mark.parametrize('name', sorted(PLANS))
def test_stitch_yuv_equals_the_definition_on_stitch_out_samples(name, dev):
    pl, pool_d, _ = _plan_and_pool(PLANS[name], dev)
    if name == 'wide_172_tile_columns':
        assert pl.stepW == 172 and pl.outW == 2060 and pl.outW > 2048 and pl.outW % 8 == 4
    if name == 'odd_61x75_3x3_tiles':
        assert (pl.stepH, pl.stepW) == (3, 3) and (pl.outH, pl.outW) == (61, 75)
    for canvas_dt in (torch.float16, torch.float32):
        s16 = _samples16(pl, pool_d, None, canvas_dt, dev)
        assert s16.min() == 0 and s16.max() == 65535, 'the pool does not reach both clamps'
        for depth in (8, 10, 16):
            got = _stitch_yuv(pl, pool_d, None, canvas_dt, depth, dev)
            want = pixfmt.fromSamples16(s16, FMT[depth])
            assert got == want, '{} canvas {} depth {}: {}'.format(name, canvas_dt, depth, _differ(got, want))


@pytest.mark.parametrize('order', ['bgr', 'rgb'])
@pytest.mark.parametrize('matrix', ['bt709', 'bt601', 'bt2020nc'])
def test_stitch_yuv_matrices_and_orders(matrix, order, extras, dev):
    pl, pool_d, _, s16 = extras
    for depth in (8, 12):
        got = _stitch_yuv(pl, pool_d, None, torch.float16, depth, dev, matrix, order)
        want = pixfmt.fromSamples16(s16, FMT[depth], matrix, order)
        assert got == want, '{} {} depth {}: {}'.format(matrix, order, depth, _differ(got, want))


def test_stitch_yuv_with_a_permuted_pool_layout(extras, dev):
    pl0, _, off0, s16 = extras
    order = list(reversed(range(pl0.n_tiles)))
    pl, pool_d, off = _plan_and_pool(PLANS[EXTRAS], dev, order)
    assert pl.n_tiles > 4 and off != off0
    off_d = torch.tensor(off, dtype=torch.int64, device=dev)
    assert np.array_equal(_samples16(pl, pool_d, off_d, torch.float16, dev), s16)
    got = _stitch_yuv(pl, pool_d, off_d, torch.float16, 10, dev)
    want = pixfmt.fromSamples16(s16, FMT[10])
    assert got == want, _differ(got, want)


@pytest.mark.parametrize('depth', [8, 10])
def test_stitch_yuv_into_an_unaligned_frame_leaves_its_neighbours_alone(depth, extras, dev):
    pl, pool_d, _, s16 = extras
    n = pixfmt.frameBytes(FMT[depth], pl.outW, pl.outH)
    flat = torch.full((n + 50,), 0xA5, dtype=torch.uint8, device=dev)
    assert flat.data_ptr() % 16 == 0
    dst = flat[18:18 + n]
    assert dst.data_ptr() % 16 == 2
    got = _stitch_yuv(pl, pool_d, None, torch.float16, depth, dev, dst=dst)
    want = pixfmt.fromSamples16(s16, FMT[depth])
    assert got == want, _differ(got, want)
    host = flat.cpu().numpy()
    assert (host[:18] == 0xA5).all() and (host[18 + n:] == 0xA5).all()


# ---- 2. the unfused form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('shape', [(3, 111, 135), (3, 144, 176)], ids=['111x135', '144x176'])
def test_to_yuv_equals_the_definition_on_to_output_samples(shape, dtype, dev):
    from moephoto_amd import _lib
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    _, H, W = shape
    a = np.random.default_rng(H).random(shape, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)
    flat = a.reshape(-1)
    flat[3::97] = np.float32(-3.5)
    flat[5::101] = np.float32(7.25)
    flat[7::211] = np.inf
    flat[11::223] = -np.inf
    flat[13::227] = np.nan
    flat[-1] = np.nan
    flat[W - 1] = np.inf           # (the odd last column of the first row)
    x = torch.from_numpy(a).to(dev).to(dtype)
    s16_d = torch.empty((H, W, 3), dtype=torch.int16, device=dev)
    _lib.check(L.moe_to_output(x.data_ptr(), _dt(dtype), H, W, 3, 16, s16_d.data_ptr(), _lib.U16, 0, st))
    s16 = s16_d.cpu().numpy().view(np.uint16)
    assert s16.min() == 0 and s16.max() == 65535
    for depth in (8, 10, 12, 16):
        for matrix, order in (('bt709', 'bgr'), ('bt601', 'rgb')):
            n = pixfmt.frameBytes(FMT[depth], W, H)
            flat_d = torch.full((n + 4,), 0xA5, dtype=torch.uint8, device=dev)
            _lib.check(L.moe_to_yuv(x.data_ptr(), _dt(dtype), H, W, depth, pixfmt.MATRICES[matrix], pixfmt.ORDERS[order], flat_d[2:].data_ptr(), 0, st))
            host = flat_d.cpu().numpy()
            got, want = host[2:2 + n].tobytes(), pixfmt.fromSamples16(s16, FMT[depth], matrix, order)
            assert got == want, '{} {} depth {} {} {}: {}'.format(shape, dtype, depth, matrix, order, _differ(got, want))
            assert (host[:2] == 0xA5).all() and (host[2 + n:] == 0xA5).all()


# ---- 3. doCropYuv ---------------------------------------------------------------------------------------------------------------------------
def _configure(fp16, crop):
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, fp16
    config.crop_sr = config.crop_dn = config.crop_dns = crop
    config.ensembleSR = 0


@pytest.mark.parametrize('case', ['a2_fp16', 'a2_fp32', 'dn_lite5', 'a3'])
def test_docropyuv_equals_the_definition_on_docropout_samples(case, dev, tmp_path, monkeypatch):
    from moephoto_amd import imageProcess as ip, runDN, runSR
    from moephoto_amd.config import config
    from moephoto_amd.weights import load_state_dict_file, save_state_dict_file
    if case.startswith('a2'):
        _configure(case != 'a2_fp32', 48)
        opt, shape = runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}), (3, 100, 140)
    elif case == 'a3':
        _configure(True, 48)
        path = str(tmp_path / 'a3.pth')                                  # (the zoo has no x3 weights: the synthetic ones of golden_defs)
        save_state_dict_file(gd.synth_state_dict('a3', load_state_dict_file), path)
        monkeypatch.setitem(runSR.mode_switch, 'a3', (path, runSR.mode_switch['a3'][1]))
        monkeypatch.delitem(ip.modelCache, 'SRa3', raising=False)
        opt, shape = runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': 3, 'ensemble': 0}), (3, 37, 45)
    else:
        _configure(True, 32)
        opt, shape = runDN.getOpt({'op': 'DN', 'model': 'lite5'}), (3, 61, 75)
    x = torch.from_numpy(gd.noise_image(31, shape)).to(dev).to(config.dtype())
    s16 = ip.doCropOut(opt, x, 16).cpu().numpy().view(np.uint16)
    plan = ip._plan_for(opt, x.shape)
    assert s16.shape == (plan.outH, plan.outW, 3) and (case == 'a3' or plan.n_tiles > 1)
    for fmt, matrix, order in (('yuv420p', 'bt709', 'bgr'), ('yuv420p10le', 'bt709', 'bgr'), ('yuv420p16le', 'bt2020nc', 'rgb')):
        got = ip.doCropYuv(opt, x, fmt, matrix=matrix, order=order)
        assert got.device.type == 'cuda' and got.dtype == torch.uint8 and got.dim() == 1
        got, want = got.cpu().numpy().tobytes(), pixfmt.fromSamples16(s16, fmt, matrix, order)
        assert got == want, '{} {}: {}'.format(case, fmt, _differ(got, want))
    out = torch.empty((pixfmt.frameBytes('yuv420p10le', plan.outW, plan.outH),), dtype=torch.uint8, device=dev)
    assert ip.doCropYuv(opt, x, 'yuv420p10le', out=out) is out
    assert out.cpu().numpy().tobytes() == pixfmt.fromSamples16(s16, 'yuv420p10le')
    with pytest.raises(ValueError):
        ip.doCropYuv(opt, x, 'yuv420p10le', out=out[:-2])
    with pytest.raises(ValueError):
        ip.doCropYuv(opt, x, 'nv12')


# ---- 4. the stream --------------------------------------------------------------------------------------------------------------------------
H, W = 72, 88
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}


def _raw_frames(n, bits, seed=5):
    rng = np.random.default_rng(seed)
    return b''.join(rng.integers(0, 1 << bits, (H, W, 3), dtype=np.uint16).astype(np.uint8 if bits == 8 else np.uint16).tobytes() for _ in range(n))


def _both_ways(steps, raw, depth, edge, out_wh):
    from moephoto_amd import procedure
    bits = steps[0]['bitDepth']
    req = procedure._outputFormat(steps)
    process, nodes = procedure.genProcess(steps, bitDepth=bits)
    want, got = [], []
    n0 = procedure.runFrames(process, io.BytesIO(raw).read, want.append, W, H, bitDepth=bits)
    stream = procedure.genFrameStream(steps, W, H, depth)
    assert stream.nodes == nodes and stream.edge == edge
    n1 = procedure.runFramesStreamed(stream, io.BytesIO(raw).read, got.append)
    stream.close()
    assert n1 == n0 == len(want) == len(got)
    assert len(set(want)) == len(want)                                   # distinct frames: a slot mix-up cannot hide
    for k, (g, w_) in enumerate(zip(got, want)):
        assert len(g) == len(w_) == pixfmt.frameBytes(req[0], *out_wh)
        assert g == w_, 'frame {}: {}'.format(k, _differ(g, w_))
    return got


@pytest.mark.parametrize('depth', [1, 2, 3])
def test_streamed_yuv_frames_equal_serial_and_the_bgr48_stream(depth, dev):
    from moephoto_amd import procedure
    _configure(True, 64)
    raw = _raw_frames(5, 16)
    buf = {'op': 'buffer', 'bitDepth': 16}
    got = _both_ways([buf, dict(SR), {'op': 'output', 'pixFmt': 'yuv420p10le', 'matrix': 'bt709'}], raw, depth, 'crop', (2 * W, 2 * H))
    assert len(got) == 5
    if depth == 2:        # the same frames as bgr48le, converted by the definition
        plain = []
        stream = procedure.genFrameStream([buf, dict(SR)], W, H, depth)
        assert procedure.runFramesStreamed(stream, io.BytesIO(raw).read, plain.append) == 5
        stream.close()
        for k, (g, p) in enumerate(zip(got, plain)):
            want = pixfmt.fromSamples16(np.frombuffer(p, np.uint16).reshape(2 * H, 2 * W, 3), 'yuv420p10le', 'bt709', 'bgr')
            assert g == want, 'frame {}: {}'.format(k, _differ(g, want))


def test_streamed_yuv_behind_a_blended_dn(dev):
    _configure(True, 64)
    steps = [{'op': 'buffer', 'bitDepth': 8}, {'op': 'DN', 'model': 'lite5', 'strength': 0.6}, {'op': 'output', 'pixFmt': 'yuv420p'}]
    assert len(_both_ways(steps, _raw_frames(4, 8), 2, 'filter', (W, H))) == 4


def test_streamed_yuv_behind_a_resize(dev):
    _configure(True, 64)
    steps = [{'op': 'buffer', 'bitDepth': 8}, dict(SR), {'op': 'resize', 'width': 100, 'height': 90, 'method': 'bilinear'},
             {'op': 'output', 'pixFmt': 'yuv420p16le', 'matrix': 'bt601', 'order': 'rgb'}]
    assert len(_both_ways(steps, _raw_frames(4, 8), 2, 'quantise', (100, 90))) == 4
