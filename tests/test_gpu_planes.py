"""Chains on the decoder's own Y'CbCr 4:2:0 planes on the device (`pytest -m gpu`).  The comparators are the written definition (moephoto_amd.pixfmt: toPlanes /
fromPlanes, numpy) and paths that exist without this feature:

  moe_planes_to_float                    against  pixfmt.toPlanes
  moe_stitch_planes                      against  moe_stitch -> moe_to_output(C = 1, bits = depth), and for one plane at 8 / 16 bits moe_stitch_out
  imageProcess.doCropPlanes              against  doCrop, quantised by moe_to_output and by pixfmt.fromPlanes
  genFrameStream with a planar source    against  pixfmt.fromPlanes(doCrop(Y), doCrop(C)) on pixfmt.toPlanes' planes, and against genProcess + runFrames
  one frame through a2                   against  the oracle's doCrop of the same planes

Equality is the bar everywhere but in the last: there the bound is the project's 1e-3 of full scale plus one code for the quantiser's truncation."""
import io

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import pixfmt
from test_gpu_yuv import PLANS

pytestmark = pytest.mark.gpu
FMT = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le', 16: 'yuv420p16le'}
NP_DT = {torch.float16: np.float16, torch.float32: np.float32}


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _dt(t):
    from moephoto_amd import _lib
    return _lib.F16 if t == torch.float16 else _lib.F32


def _udt(depth):
    from moephoto_amd import _lib
    return _lib.U8 if depth == 8 else _lib.U16


def _es(depth):
    return 1 if depth == 8 else 2


def _differ(got, want):
    g, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    return 'sizes {} / {}'.format(g.size, w.size) if g.size != w.size else '{} of {} bytes differ, the first at {}'.format(int((g != w).sum()), g.size, int(np.argmax(g != w)))


def _frame(seed, depth, w, h):
    """A planar frame of random codes below 2^depth; the 16-bit containers of 10 and 12 bits also get a few codes with high bits set (they are not masked)."""
    n = w * h * 3 // 2
    a = np.random.default_rng(seed).integers(0, 1 << depth, n, dtype=np.uint32)
    a[:2] = (0, (1 << depth) - 1)
    if depth in (10, 12):
        a[2::61] |= 0x8000
        a[3] = 65535
    return a.astype(np.uint8 if depth == 8 else np.dtype('<u2')).tobytes()


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---- 1. the source edge -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('wh', [(2, 2), (16, 2), (18, 10), (140, 100)], ids='{0[0]}x{0[1]}'.format)
def test_planes_to_float_equals_the_definition(wh, dtype, dev):
    from moephoto_amd import _lib
    L = _lib.lib()
    w, h = wh
    ny, nc = w * h, w * h // 2
    for depth in (8, 10, 12, 16):
        frame = _frame(w + depth, depth, w, h)
        wantY, wantC = pixfmt.toPlanes(frame, FMT[depth], w, h, NP_DT[dtype])
        es = _es(depth)
        for lead in (0, es):                      # an aligned source, and one a single sample behind a 16-byte boundary, between sentinel bytes
            flat = torch.full((lead + len(frame) + 16,), 0xA5, dtype=torch.uint8, device=dev)
            assert flat.data_ptr() % 16 == 0
            flat[lead:lead + len(frame)] = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).to(dev)
            y = torch.full((ny + 16,), -7.0, dtype=dtype, device=dev)
            c = torch.full((nc + 16,), -7.0, dtype=dtype, device=dev)
            _lib.check(L.moe_planes_to_float(flat[lead:].data_ptr(), depth, h, w, y[8:].data_ptr(), c[8:].data_ptr(), _dt(dtype), 0, _st()))
            gy, gc = y.cpu().numpy(), c.cpu().numpy()
            bits = np.uint16 if dtype == torch.float16 else np.uint32
            assert np.array_equal(gy[8:8 + ny].view(bits), wantY.reshape(-1).view(bits)), (wh, depth, lead, 'Y')
            assert np.array_equal(gc[8:8 + nc].view(bits), wantC.reshape(-1).view(bits)), (wh, depth, lead, 'C')
            assert (gy[:8] == -7).all() and (gy[8 + ny:] == -7).all() and (gc[:8] == -7).all() and (gc[8 + nc:] == -7).all()
            assert (flat.cpu().numpy()[lead + len(frame):] == 0xA5).all()


def test_fromplanes_wrapper(dev):
    from moephoto_amd import imageProcess as ip
    w, h = 18, 10
    frame = _frame(3, 10, w, h)
    raw = torch.from_numpy(np.frombuffer(frame, np.uint8).copy()).to(dev)
    for dtype in (torch.float16, torch.float32):
        f = ip.fromPlanes('yuv420p10le', w, h, dtype)
        Y, C = f(raw)
        wantY, wantC = pixfmt.toPlanes(frame, 'yuv420p10le', w, h, NP_DT[dtype])
        assert tuple(Y.shape) == (1, h, w) and tuple(C.shape) == (2, h // 2, w // 2) and Y.dtype == C.dtype == dtype
        assert np.array_equal(Y.cpu().numpy(), wantY) and np.array_equal(C.cpu().numpy(), wantC)
        oy, oc = torch.empty_like(Y), torch.empty_like(C)
        y2, c2 = f(raw, oy, oc)
        assert y2 is oy and c2 is oc and torch.equal(oy, Y) and torch.equal(oc, C)
        with pytest.raises(ValueError):
            f(raw[:-2])
        with pytest.raises(ValueError):
            f(raw, oc, oy)


# ---- 2. the fold's edge ---------------------------------------------------------------------------------------------------------------------
def _plan_and_pool(params, C, dev, order=None):
    """TilePlan + a pool of C planes per tile, seeded per tile and drawn from [-0.25, 1.25) with NaN and both infinities planted.  order: the tiles' order in the pool."""
    from moephoto_amd.imageProcess import TilePlan
    shape, sc, pad, align, crop = params
    pl = TilePlan(shape, 1 << 40, 1e-3, pad, sc, align, crop)
    sizes = [C * (t[1] - t[0]) * sc * (t[3] - t[2]) * sc for t in pl.tiles]
    if order is None:
        off = pl.tile_offsets(C)
    else:
        off, at = [0] * pl.n_tiles, 0
        for k in order:
            off[k] = at
            at += sizes[k]
    pool = np.zeros(max(pl.pool_elems(C), sum(sizes)), np.float32)
    for k in range(pl.n_tiles):
        t = np.random.default_rng(4200 + k).random(sizes[k], dtype=np.float32) * np.float32(1.5) - np.float32(0.25)
        t[5::97] = np.nan
        t[11::193] = np.inf
        t[17::211] = -np.inf
        pool[off[k]:off[k] + sizes[k]] = t
    return pl, torch.from_numpy(pool).to(dev), off


def _canvas(pl, pool_d, off_d, C, canvas_dt, dev):
    from moephoto_amd import _lib
    out = torch.empty((C, pl.outH, pl.outW), dtype=canvas_dt, device=dev)
    if off_d is None:
        _lib.check(_lib.lib().moe_stitch(pl._h, 0, pool_d.data_ptr(), None, C, out.data_ptr(), _dt(canvas_dt), _st()))
    else:
        _lib.check(_lib.lib().moe_stitch_dev(pl._h, 0, pool_d.data_ptr(), off_d.data_ptr(), C, out.data_ptr(), _dt(canvas_dt), _st()))
    return out


def _quantised(canvas, depth, dev):
    """moe_to_output(H = C * h, W = w, C = 1, bits = depth) on a dense canvas: its bytes."""
    from moephoto_amd import _lib
    C, H, W = canvas.shape
    out = torch.empty((C * H * W * _es(depth),), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().moe_to_output(canvas.data_ptr(), _dt(canvas.dtype), C * H, W, 1, depth, out.data_ptr(), _udt(depth), 0, _st()))
    return out.cpu().numpy().tobytes()


def _stitch_planes(pl, pool_d, off_d, C, canvas_dt, depth, dev, dst=None):
    from moephoto_amd import _lib
    n = C * pl.outH * pl.outW * _es(depth)
    if dst is None:
        dst = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
    assert dst.numel() == n
    _lib.check(_lib.lib().moe_stitch_planes(pl._h, 0, pool_d.data_ptr(), off_d.data_ptr() if off_d is not None else None, C, _dt(canvas_dt), depth,
                                            dst.data_ptr(), _st()))
    return dst.cpu().numpy().tobytes()


@pytest.mark.parametrize('C', [1, 2, 3])
@pytest.mark.parametrize('name', sorted(PLANS))
def test_stitch_planes_equals_stitch_then_to_output(name, C, dev):
    from moephoto_amd import _lib
    pl, pool_d, _ = _plan_and_pool(PLANS[name], C, dev)
    if name == 'wide_172_tile_columns':
        assert pl.stepW == 172 and pl.outW == 2060 and pl.outW % 8 == 4
    for canvas_dt in (torch.float16, torch.float32):
        canvas = _canvas(pl, pool_d, None, C, canvas_dt, dev)
        for depth in (8, 10, 12, 16):
            got, want = _stitch_planes(pl, pool_d, None, C, canvas_dt, depth, dev), _quantised(canvas, depth, dev)
            codes = np.frombuffer(want, np.uint8 if depth == 8 else np.uint16)
            assert codes.min() == 0 and codes.max() == (1 << depth) - 1, 'the pool does not reach both clamps'
            assert got == want, '{} C {} canvas {} depth {}: {}'.format(name, C, canvas_dt, depth, _differ(got, want))
            if C == 1 and depth in (8, 16):
                out = torch.empty((pl.outH, pl.outW, 1), dtype=torch.uint8 if depth == 8 else torch.int16, device=dev)
                _lib.check(_lib.lib().moe_stitch_out(pl._h, 0, pool_d.data_ptr(), None, 1, _dt(canvas_dt), depth, out.data_ptr(), _udt(depth), _st()))
                assert got == out.cpu().numpy().tobytes(), '{} canvas {} depth {} against moe_stitch_out'.format(name, canvas_dt, depth)


EXTRAS = 'odd_61x75_3x3_tiles'


def test_stitch_planes_with_a_permuted_pool_layout(dev):
    pl0, pool0, off0 = _plan_and_pool(PLANS[EXTRAS], 2, dev)
    want = _quantised(_canvas(pl0, pool0, None, 2, torch.float16, dev), 10, dev)
    order = list(reversed(range(pl0.n_tiles)))
    pl, pool_d, off = _plan_and_pool(PLANS[EXTRAS], 2, dev, order)
    assert pl.n_tiles > 4 and off != off0
    off_d = torch.tensor(off, dtype=torch.int64, device=dev)
    got = _stitch_planes(pl, pool_d, off_d, 2, torch.float16, 10, dev)
    assert got == want, _differ(got, want)


@pytest.mark.parametrize('depth', [8, 10])
@pytest.mark.parametrize('name', [EXTRAS, 'even_3x4_tiles'])
def test_stitch_planes_at_an_odd_offset_leaves_its_neighbours_alone(name, depth, dev):
    pl, pool_d, _ = _plan_and_pool(PLANS[name], 2, dev)
    want = _quantised(_canvas(pl, pool_d, None, 2, torch.float32, dev), depth, dev)
    n, lead = len(want), 16 + _es(depth)                              # one sample behind a 16-byte boundary
    flat = torch.full((n + lead + 30,), 0xA5, dtype=torch.uint8, device=dev)
    assert flat.data_ptr() % 16 == 0
    got = _stitch_planes(pl, pool_d, None, 2, torch.float32, depth, dev, dst=flat[lead:lead + n])
    assert got == want, _differ(got, want)
    host = flat.cpu().numpy()
    assert (host[:lead] == 0xA5).all() and (host[lead + n:] == 0xA5).all()


# ---- 3. doCropPlanes ------------------------------------------------------------------------------------------------------------------------
def _configure(fp16, crop):
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, fp16
    config.crop_sr = config.crop_dn = config.crop_dns = crop
    config.ensembleSR = 0


@pytest.mark.parametrize('shape', [(1, 100, 140), (2, 50, 70)], ids=['1x100x140', '2x50x70'])
@pytest.mark.parametrize('case', ['a2_fp16', 'a2_fp32', 'dn_lite5'])
def test_docropplanes_equals_the_quantised_docrop(case, shape, dev):
    from moephoto_amd import imageProcess as ip, runDN, runSR
    from moephoto_amd.config import config
    _configure(case != 'a2_fp32', 48)
    if case.startswith('a2'):
        opt = runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0})
    else:
        opt = runDN.getOpt({'op': 'DN', 'model': 'lite5'})
    x = torch.from_numpy(gd.noise_image(31, shape)).to(dev).to(config.dtype())
    canvas = ip.doCrop(opt, x)
    plan = ip._plan_for(opt, x.shape)
    C = shape[0]
    assert tuple(canvas.shape) == (C, plan.outH, plan.outW) and plan.n_tiles > 1
    host = canvas.cpu().numpy()
    for depth in (8, 10, 12, 16):
        got = ip.doCropPlanes(opt, x, depth)
        assert got.device.type == 'cuda' and got.dtype == torch.uint8 and got.dim() == 1
        got = got.cpu().numpy().tobytes()
        want = ip.toPlanes(depth)(canvas).cpu().numpy().tobytes()
        assert got == want, '{} {} depth {}: {}'.format(case, shape, depth, _differ(got, want))
        q = np.float32(1 << depth)                                    # the definition's quantiser on the canvas
        ref = np.fmin(np.fmax(host.astype(np.float32) * q, np.float32(0)), q - np.float32(1)).astype(np.int64).astype(np.uint8 if depth == 8 else np.dtype('<u2')).tobytes()
        assert got == ref, '{} {} depth {} against numpy: {}'.format(case, shape, depth, _differ(got, ref))
    n = C * plan.outH * plan.outW * 2
    frame = torch.full((n + 6,), 0xA5, dtype=torch.uint8, device=dev)
    view = frame[2:2 + n]                                             # a view into a frame: 2-byte aligned, no more
    assert ip.doCropPlanes(opt, x, 10, out=view) is view
    hostf = frame.cpu().numpy()
    assert hostf[2:2 + n].tobytes() == ip.toPlanes(10)(canvas).cpu().numpy().tobytes() and (hostf[:2] == 0xA5).all() and (hostf[2 + n:] == 0xA5).all()
    with pytest.raises(ValueError):
        ip.doCropPlanes(opt, x, 10, out=view[:-2])
    with pytest.raises(ValueError):
        ip.doCropPlanes(opt, x, 10, out=frame[1:1 + n])               # an odd address for uint16 samples
    with pytest.raises(ValueError):
        ip.doCropPlanes(opt, x, 9)


# ---- 4. the stream --------------------------------------------------------------------------------------------------------------------------
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}
# name -> (source format, compute / output steps, output format, edge, scale).  The edge is the rule's: 'crop' when the LAST step is an SR without
# ensemble or a DN of strength 1, else 'quantise'.  So a blended DN in front of a plain SR is still a 'crop' chain (its blend runs in RGBFilter, the SR's folds
# write the frame); the blended DN as the last step and the ensemble are the 'quantise' chains.
CHAINS = {'sr_a2': ('yuv420p10le', [dict(SR)], 'yuv420p10le', 'crop', 2),
          'sr_a2_8_to_10': ('yuv420p', [dict(SR), {'op': 'output', 'pixFmt': 'yuv420p10le'}], 'yuv420p10le', 'crop', 2),
          'dn_0.6_sr_a2': ('yuv420p10le', [{'op': 'DN', 'model': 'lite5', 'strength': 0.6}, dict(SR)], 'yuv420p10le', 'crop', 2),
          'blended_dn_last': ('yuv420p', [dict(SR), {'op': 'DN', 'model': 'lite5', 'strength': 0.6}], 'yuv420p', 'quantise', 2),
          'sr_a2_ensemble_1': ('yuv420p16le', [dict(SR, ensemble=1)], 'yuv420p16le', 'quantise', 2)}


def _frames(n, fmt, w, h, seed=5):
    return [_frame(seed + k, pixfmt.FORMATS[fmt], w, h) for k in range(n)]


@pytest.mark.parametrize('wh', [(140, 100), (48, 32)], ids='{0[0]}x{0[1]}'.format)
@pytest.mark.parametrize('chain', sorted(CHAINS))
def test_streamed_planar_frames_equal_serial_and_the_definition(chain, wh, dev):
    from moephoto_amd import imageProcess as ip, procedure, runSR
    from moephoto_amd.config import config
    _configure(True, 48)
    src, work, dst, edge, scale = CHAINS[chain]
    w, h = wh
    steps = [{'op': 'buffer', 'pixFmt': src}] + [dict(s) for s in work]
    frames = _frames(5, src, w, h)
    raw = b''.join(frames)
    nbytes = pixfmt.frameBytes(src, w, h)
    process, nodes = procedure.genProcess(steps)
    want = []
    assert procedure.runFrames(process, io.BytesIO(raw).read, want.append, w, h, frameBytes=nbytes) == 5
    assert len(set(want)) == 5                                        # distinct frames: a slot mix-up cannot hide
    assert all(len(f) == pixfmt.frameBytes(dst, w * scale, h * scale) for f in want)
    if chain in ('sr_a2', 'sr_a2_8_to_10'):                           # the definition: toPlanes, doCrop on each image, fromPlanes
        opt = runSR.getOpt(dict(SR))
        for k, f in enumerate(frames):
            Y, C = pixfmt.toPlanes(f, src, w, h, np.float16)
            oy, oc = (ip.doCrop(opt, torch.from_numpy(p.copy()).to(dev)).cpu().numpy() for p in (Y, C))
            if k == 0:
                py, pc = ip._plan_for(opt, Y.shape), ip._plan_for(opt, C.shape)
                assert (py.n_tiles, pc.stepH, pc.stepW) == ((12, 2, 2) if wh == (140, 100) else (1, 1, 1))
            ref = pixfmt.fromPlanes(oy, oc, dst)
            assert want[k] == ref, 'frame {} against the definition: {}'.format(k, _differ(want[k], ref))
    for depth in (1, 2, 3):
        stream = procedure.genFrameStream(steps, w, h, depth)
        assert stream.nodes == nodes and stream.edge == edge and stream.frameBytes == nbytes
        got = []
        assert procedure.runFramesStreamed(stream, io.BytesIO(raw).read, got.append) == 5
        stream.close()
        for k, (g, w_) in enumerate(zip(got, want)):
            assert g == w_, '{} ring depth {} frame {}: {}'.format(chain, depth, k, _differ(g, w_))


# ---- 5. against the oracle --------------------------------------------------------------------------------------------------------------------
def test_a_planar_frame_through_a2_against_the_oracle(dev):
    """fp32 images, so that the comparison sees the engine's own error and the quantiser's truncation only.  Per code: |code - clamp(oracle * 2^D)| <= 1e-3 * 2^D + 1
    (the clamp to [0, 2^D - 1] is the quantiser's and moves no pair of values apart)."""
    from moephoto_amd import procedure
    from moephoto_amd.weights import load_state_dict_file
    from oracle import nets as onets, planner as oplanner, stitch as ostitch
    _configure(False, 48)
    w, h, D, fmt = 140, 100, 10, 'yuv420p10le'
    frame = np.random.default_rng(77).integers(0, 1 << D, w * h * 3 // 2, dtype=np.uint16).astype('<u2').tobytes()      # noise over the format's own codes: values in [0, 1)
    stream = procedure.genFrameStream([{'op': 'buffer', 'pixFmt': fmt}, dict(SR)], w, h, 1)
    got = stream.push(frame) + stream.flush()
    stream.close()
    assert stream.edge == 'crop' and len(got) == 1 and len(got[0]) == pixfmt.frameBytes(fmt, 2 * w, 2 * h)
    codes = np.frombuffer(got[0], '<u2').astype(np.float64)
    model = onets.model_fn('net2x', gd.state_dict_for('a2', load_state_dict_file))
    planes = []
    for p in pixfmt.toPlanes(frame, fmt, w, h, np.float32):
        pl = oplanner.prepare(p.shape, 1 << 40, 1e-3, 5, 2, 8, 48)
        planes.append(ostitch.do_crop(p, pl, 2, model).astype(np.float64).reshape(-1))
    want = np.clip(np.concatenate(planes) * (1 << D), 0, (1 << D) - 1)
    assert codes.size == want.size
    err = float(np.abs(codes - want).max())
    print('planar a2 140x100 at {} bits: max |code - oracle| = {:.3f} codes (bound {:.3f})'.format(D, err, 1e-3 * (1 << D) + 1))
    assert err <= 1e-3 * (1 << D) + 1, err
