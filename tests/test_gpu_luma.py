"""Luma-only steps on RGB sources on the device (`pytest -m gpu`).  The comparators are the written definition (moephoto_amd.luma, numpy) and
paths that exist without this feature:

  moe_luma_split, moe_luma_merge          against  luma.lumaSplit / luma.lumaMerge, bit for bit (NaN against NaN: IEEE leaves a NaN's payload open)
  moe_stitch_luma                         against  moe_stitch -> moe_luma_merge, byte for byte
  imageProcess.doCropLuma (fused)         against  lumaSplit -> doCrop -> resize -> lumaMerge, byte for byte, and against luma.lumaMerge on doCrop's Y'
  one image through a2                    against  the definition with the oracle's doCrop on Y
  genFrameStream                          against  genProcess + runFrames, and against the definition applied step by step with the unfused pieces

Equality is the bar everywhere but against the oracle: there each output plane carries Y' 's error with coefficient 1 and the chroma path is exact against the
definition, so the bound is the engine's own 1e-3 on Y' plus 1e-6 for the merge's fp32 rounding."""
import io

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import luma
from test_gpu_planes import _canvas, _differ, _dt, _plan_and_pool, _st

pytestmark = pytest.mark.gpu
NP_DT = {torch.float16: np.float16, torch.float32: np.float32}
MATRICES = ('bt709', 'bt601', 'bt2020nc')
SIZES = [(1, 1), (2, 3), (7, 9), (8, 16), (100, 140)]


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _ids(matrix, order):
    from moephoto_amd import pixfmt
    return pixfmt.MATRICES[matrix], pixfmt.ORDERS[order]


def _udt(bits):
    from moephoto_amd import _lib
    return _lib.U8 if bits == 8 else _lib.U16


def _same(got, want):
    """Bit equality of two float arrays, a NaN standing for any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    ng, nw = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(ng, nw) and np.array_equal(np.where(ng, 0, got).astype(got.dtype).view(bits), np.where(nw, 0, want).astype(want.dtype).view(bits)))


def _values(seed, shape, dtype, lo=-0.25, hi=1.25):
    """Values below 0 and above 1 with NaN and both infinities planted (where the array is large enough to keep plain values too)."""
    v = (np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(hi - lo) + np.float32(lo)).reshape(-1)
    if v.size >= 12:
        v[5::97] = np.nan
        v[7::193] = np.inf
        v[11::211] = -np.inf
    return v.reshape(shape).astype(NP_DT[dtype] if isinstance(dtype, torch.dtype) else dtype)


# ---- 1. the split and merge kernels ------------------------------------------------------------------------------------------------------------
def _split(x, matrix, order, lead, dev):
    """moe_luma_split on the device tensor x (any strides) into buffers whose payload starts `lead` elements behind a 16-byte boundary, between sentinels."""
    from moephoto_amd import _lib
    C, H, W = x.shape
    ny, nc = (C - 2) * H * W, 2 * H * W
    y = torch.full((lead + ny + 16,), -7.0, dtype=x.dtype, device=dev)
    c = torch.full((lead + nc + 16,), -7.0, dtype=torch.float32, device=dev)
    assert y.data_ptr() % 16 == 0 and c.data_ptr() % 16 == 0
    mat, ordr = _ids(matrix, order)
    _lib.check(_lib.lib().moe_luma_split(x.data_ptr(), _dt(x.dtype), C, x.stride(0), x.stride(1), x.stride(2), H, W, mat, ordr, y[lead:].data_ptr(), c[lead:].data_ptr(), 0, _st()))
    hy, hc = y.cpu().numpy(), c.cpu().numpy()
    assert (hy[:lead] == -7).all() and (hy[lead + ny:] == -7).all() and (hc[:lead] == -7).all() and (hc[lead + nc:] == -7).all(), 'a sentinel was overwritten'
    return hy[lead:lead + ny].reshape(C - 2, H, W), hc[lead:lead + nc].reshape(2, H, W)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('hw', SIZES, ids='{0[0]}x{0[1]}'.format)
def test_split_equals_the_definition(hw, dtype, dev):
    H, W = hw
    for C in (3, 4):
        host = _values(H * W + C, (C, H + 3, (W + 13 + 7) // 8 * 8), dtype)          # (a row pitch of whole 16-byte vectors)
        big = torch.from_numpy(host).to(dev)
        views = {'slice': (big[:, 1:1 + H, 5:5 + W], host[:, 1:1 + H, 5:5 + W]), 'dense': (big[:, :H, :W].contiguous(), host[:, :H, :W]),
                 'aligned rows': (big[:, 2:2 + H, 8:8 + W], host[:, 2:2 + H, 8:8 + W])}      # (base and row pitch multiples of 16 bytes: the vector path on a view)
        for name, (x, hx) in views.items():
            for matrix in MATRICES:
                for order in ('rgb', 'bgr'):
                    wantY, wantC = luma.lumaSplit(hx, matrix, order)
                    for lead in (16, 17):          # an aligned destination, and one a single sample behind a 16-byte boundary
                        gotY, gotC = _split(x, matrix, order, lead, dev)
                        assert _same(gotY, wantY), (hw, C, name, matrix, order, lead, 'Y')
                        assert _same(gotC, wantC), (hw, C, name, matrix, order, lead, 'C')


def _merge(Y, C, matrix, order, bits, lead, dev):
    """moe_luma_merge on dense device tensors into a buffer whose payload starts `lead` elements behind a 16-byte boundary, between sentinels."""
    from moephoto_amd import _lib
    P, H, W = Y.shape
    n = (P + 2) * H * W
    o_dt = Y.dtype if bits is None else (torch.uint8 if bits == 8 else torch.int16)
    out = torch.full((lead + n + 16,), 90, dtype=o_dt, device=dev)
    assert out.data_ptr() % 16 == 0
    mat, ordr = _ids(matrix, order)
    _lib.check(_lib.lib().moe_luma_merge(Y.data_ptr(), _dt(Y.dtype), C.data_ptr(), P + 2, H, W, mat, ordr, bits or 0, out[lead:].data_ptr(),
                                         _dt(Y.dtype) if bits is None else _udt(bits), 0, _st()))
    h = out.cpu().numpy()
    assert (h[:lead] == 90).all() and (h[lead + n:] == 90).all(), 'a sentinel was overwritten'
    h = h[lead:lead + n]
    return h.reshape(P + 2, H, W) if bits is None else (h.view(np.uint16) if bits == 16 else h).reshape(H, W, P + 2)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('hw', SIZES, ids='{0[0]}x{0[1]}'.format)
def test_merge_equals_the_definition(hw, dtype, dev):
    H, W = hw
    for P in (1, 2):
        hY, hC = _values(H + W + P, (P, H, W), dtype), _values(H * W + P, (2, H, W), np.float32, -0.6, 0.6)
        Y, C = torch.from_numpy(hY).to(dev), torch.from_numpy(hC).to(dev)
        for matrix in MATRICES:
            for order in ('rgb', 'bgr'):
                for bits in (None, 8, 16):
                    want = luma.lumaMerge(hY, hC, matrix, order, bits)
                    for lead in (16, 17):
                        got = _merge(Y, C, matrix, order, bits, lead, dev)
                        ok = _same(got, want) if bits is None else np.array_equal(got, want)
                        assert ok, (hw, P, matrix, order, bits, lead)
                    if bits and H * W >= 100:
                        assert want.min() == 0 and want.max() == (1 << bits) - 1, 'the values do not reach both clamps'


def test_split_then_merge_wrappers(dev):
    from moephoto_amd import imageProcess as ip
    host = _values(3, (4, 21, 37), np.float16, 0.0, 1.0)
    host[np.isnan(host) | np.isinf(host)] = 0.25
    x = torch.from_numpy(host).to(dev)
    Y, C = ip.lumaSplit('bt601', 'bgr')(x[:, 1:, 2:])
    wantY, wantC = luma.lumaSplit(host[:, 1:, 2:], 'bt601', 'bgr')
    assert Y.dtype == torch.float16 and C.dtype == torch.float32 and Y.is_contiguous() and C.is_contiguous()
    assert _same(Y.cpu().numpy(), wantY) and _same(C.cpu().numpy(), wantC)
    merge = ip.lumaMerge('bt601', 'bgr')
    assert _same(merge(Y, C).cpu().numpy(), luma.lumaMerge(wantY, wantC, 'bt601', 'bgr'))
    out = torch.empty((20, 35, 4), dtype=torch.int16, device=dev)
    assert merge(Y, C, 16, out) is out and np.array_equal(out.cpu().numpy().view(np.uint16), luma.lumaMerge(wantY, wantC, 'bt601', 'bgr', 16))
    assert np.array_equal(merge(Y, C, 8).cpu().numpy(), luma.lumaMerge(wantY, wantC, 'bt601', 'bgr', 8))
    with pytest.raises(ValueError):
        merge(Y, C[:, :-1])
    with pytest.raises(ValueError):
        merge(Y, C, 16, out[:-1])
    with pytest.raises(ValueError):
        ip.lumaSplit()(x[:2])


# ---- 2. the fold's edge ---------------------------------------------------------------------------------------------------------------------
PADS = {1: 7, 2: 5, 3: 9}
PLANS = {'{}x{}_x{}'.format(h, w, sc): ((1, h, w), sc, PADS[sc], 8, 48) for h, w in ((2, 2), (48, 48), (100, 140)) for sc in (1, 2, 3)}
PLANS['wide_172_tile_columns'] = ((1, 24, 2060), 1, 2, 8, 16)          # a second block column, a ragged end of four (tests/test_gpu_yuv.py)


def _chroma(pl, seed, dev):
    return torch.from_numpy(_values(seed, (2, pl.outH, pl.outW), np.float32, -0.6, 0.6)).to(dev)


def _stitch_luma(pl, pool_d, off_d, P, canvas_dt, c, matrix, order, bits, dev, lead=0):
    from moephoto_amd import _lib
    n = (P + 2) * pl.outH * pl.outW
    o_dt = canvas_dt if bits is None else (torch.uint8 if bits == 8 else torch.int16)
    out = torch.full((lead + n + 16,), 90, dtype=o_dt, device=dev)
    mat, ordr = _ids(matrix, order)
    _lib.check(_lib.lib().moe_stitch_luma(pl._h, 0, pool_d.data_ptr(), off_d.data_ptr() if off_d is not None else None, P, _dt(canvas_dt), c.data_ptr(), mat, ordr, bits or 0,
                                          out[lead:].data_ptr(), _dt(canvas_dt) if bits is None else _udt(bits), _st()))
    h = out.cpu().numpy()
    assert (h[:lead] == 90).all() and (h[lead + n:] == 90).all(), 'a sentinel was overwritten'
    return h[lead:lead + n].tobytes()


def _stitch_then_merge(pl, pool_d, off_d, P, canvas_dt, c, matrix, order, bits, dev):
    canvas = _canvas(pl, pool_d, off_d, P, canvas_dt, dev)
    return _merge(canvas, c, matrix, order, bits, 16, dev).tobytes()


@pytest.mark.parametrize('name', sorted(PLANS))
def test_stitch_luma_equals_stitch_then_merge(name, dev):
    shape, sc, pad, align, crop = PLANS[name]
    for P in (1, 2):
        pl, pool_d, _ = _plan_and_pool(((P,) + shape[1:], sc, pad, align, crop), P, dev)
        if name == 'wide_172_tile_columns':
            assert pl.stepW == 172 and pl.outW == 2060 and pl.outW % 8 == 4
        if name == '100x140_x2':
            assert pl.n_tiles == 12
        c = _chroma(pl, 17 + P, dev)
        for canvas_dt in (torch.float16, torch.float32):
            for bits in (None, 8, 16):
                matrix, order = MATRICES[(P + (bits or 0)) % 3], ('rgb', 'bgr')[(P + (bits or 1)) % 2]
                got = _stitch_luma(pl, pool_d, None, P, canvas_dt, c, matrix, order, bits, dev)
                want = _stitch_then_merge(pl, pool_d, None, P, canvas_dt, c, matrix, order, bits, dev)
                assert got == want, '{} P {} canvas {} bits {}: {}'.format(name, P, canvas_dt, bits, _differ(got, want))


@pytest.mark.parametrize('order', ['rgb', 'bgr'])
@pytest.mark.parametrize('matrix', MATRICES)
def test_stitch_luma_matrices_and_orders(matrix, order, dev):
    pl, pool_d, _ = _plan_and_pool(PLANS['100x140_x2'], 1, dev)
    c = _chroma(pl, 5, dev)
    for bits in (None, 16):
        got = _stitch_luma(pl, pool_d, None, 1, torch.float16, c, matrix, order, bits, dev)
        want = _stitch_then_merge(pl, pool_d, None, 1, torch.float16, c, matrix, order, bits, dev)
        assert got == want, _differ(got, want)


def test_stitch_luma_with_a_permuted_pool_and_an_unaligned_destination(dev):
    params = ((2, 61, 75), 1, 7, 8, 32)
    pl0, pool0, off0 = _plan_and_pool(params, 2, dev)
    c = _chroma(pl0, 9, dev)
    order = list(reversed(range(pl0.n_tiles)))
    pl, pool_d, off = _plan_and_pool(params, 2, dev, order)
    assert pl.n_tiles > 4 and off != off0
    off_d = torch.tensor(off, dtype=torch.int64, device=dev)
    for bits in (None, 8, 16):
        want = _stitch_then_merge(pl0, pool0, None, 2, torch.float16, c, 'bt709', 'bgr', bits, dev)
        for lead in (16, 17):          # one sample behind a 16-byte boundary: the sentinels in front and behind survive (_stitch_luma)
            got = _stitch_luma(pl, pool_d, off_d, 2, torch.float16, c, 'bt709', 'bgr', bits, dev, lead)
            assert got == want, 'bits {} lead {}: {}'.format(bits, lead, _differ(got, want))


# ---- 3. doCropLuma ------------------------------------------------------------------------------------------------------------------------------
def _configure(fp16, crop=48):
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, fp16
    config.crop_sr = config.crop_dn = config.crop_dns = crop
    config.ensembleSR = 0


CROPS = {'a2_noise': (True, 'SR', 2, (3, 100, 140), 'noise', 'bicubic'), 'a2_smooth': (True, 'SR', 2, (3, 100, 140), 'smooth', 'bilinear'),
         'a2_fp32_alpha': (False, 'SR', 2, (4, 100, 140), 'noise', 'bicubic'), 'dn_lite5': (True, 'DN', 1, (3, 100, 140), 'noise', 'nearest'),
         'a3': (True, 'SR', 3, (3, 60, 52), 'noise', 'bicubic')}


@pytest.mark.parametrize('case', sorted(CROPS))
def test_docropluma_equals_the_unfused_composition(case, dev, tmp_path, monkeypatch):
    from moephoto_amd import imageProcess as ip, runDN, runSR
    from moephoto_amd.config import config
    from moephoto_amd.weights import load_state_dict_file, save_state_dict_file
    fp16, op, scale, shape, kind, method = CROPS[case]
    _configure(fp16)
    if case == 'a3':
        path = str(tmp_path / 'a3.pth')                                  # (the zoo has no x3 weights: the synthetic ones of golden_defs)
        save_state_dict_file(gd.synth_state_dict('a3', load_state_dict_file), path)
        monkeypatch.setitem(runSR.mode_switch, 'a3', (path, runSR.mode_switch['a3'][1]))
        monkeypatch.delitem(ip.modelCache, 'SRa3', raising=False)
    opt = runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': scale, 'ensemble': 0}) if op == 'SR' else runDN.getOpt({'op': 'DN', 'model': 'lite5'})
    host = gd.noise_image(41, shape) if kind == 'noise' else gd.smooth_image(shape)
    x = torch.from_numpy(host).to(dev).to(config.dtype())
    matrix, order = 'bt601', 'bgr'
    Y, C = ip.lumaSplit(matrix, order)(x)
    Yo = ip.doCrop(opt, Y)
    plan = ip._plan_for(opt, Y.shape)
    assert plan.n_tiles > 1 and tuple(Yo.shape) == (shape[0] - 2, shape[1] * scale, shape[2] * scale)
    Co = ip.lumaChroma(C, plan.outH, plan.outW, method)
    assert (Co is C) == (scale == 1) and Co.dtype == torch.float32
    merge = ip.lumaMerge(matrix, order)
    for bits in (None, 8, 16):
        want = merge(Yo, Co, bits)
        got = ip.doCropLuma(opt, x, method, matrix, order, bits)
        assert got.shape == want.shape and got.dtype == want.dtype
        g, w = got.cpu().numpy(), want.cpu().numpy()
        assert g.tobytes() == w.tobytes(), '{} bits {}: {}'.format(case, bits, _differ(g.tobytes(), w.tobytes()))
        ref = luma.lumaMerge(Yo.cpu().numpy(), Co.cpu().numpy(), matrix, order, bits)          # the definition on the device's own Y' and C'
        assert np.array_equal(g.view(np.uint16) if bits == 16 else g, ref), '{} bits {} against numpy'.format(case, bits)
    out = torch.empty((plan.outH, plan.outW, shape[0]), dtype=torch.int16, device=dev)
    assert ip.doCropLuma(opt, x, method, matrix, order, 16, out) is out and torch.equal(out, merge(Yo, Co, 16))
    with pytest.raises(ValueError):
        ip.doCropLuma(opt, x, method, matrix, order, 16, out[:-1])
    # fewer than three planes: nothing to set aside, the call is doCrop's
    assert torch.equal(ip.doCropLuma(opt, x[:1], method, matrix, order), ip.doCrop(opt, x[:1]))


def test_an_image_through_a2_against_the_oracle(dev):
    """fp32 I/O, a2's real weights, 100 x 140 noise.  The definition in numpy with the oracle's doCrop on Y; the chroma planes are the definition's own, resized by the
    existing moe_resize (held to the oracle's resize by its own tests), so the chroma path is exact and every output plane carries Y' 's error with coefficient 1:
    the bound is the engine's 1e-3 on Y' plus 1e-6 for the merge's fp32 rounding.  Measured: profiles/luma/summary.md."""
    from moephoto_amd import imageProcess as ip, runSR
    from moephoto_amd.weights import load_state_dict_file
    from oracle import nets as onets, planner as oplanner, stitch as ostitch
    _configure(False)
    host = gd.noise_image(77, (3, 100, 140))
    opt = runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0})
    got = ip.doCropLuma(opt, torch.from_numpy(host).to(dev), 'bicubic', 'bt709', 'rgb').cpu().numpy()
    Y, C = luma.lumaSplit(host, 'bt709', 'rgb')
    model = onets.model_fn('net2x', gd.state_dict_for('a2', load_state_dict_file))
    Yo = ostitch.do_crop(Y, oplanner.prepare(Y.shape, 1 << 40, 1e-3, 5, 2, 8, 48), 2, model).astype(np.float32).reshape(1, 200, 280)
    Co = ip.resizeByTorch(torch.from_numpy(C).to(dev), 280, 200, 'bicubic').cpu().numpy()
    want = luma.lumaMerge(Yo, Co, 'bt709', 'rgb')
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print('luma-only a2 100x140 fp32: max |engine - definition on the oracle\'s Y\'| = {:.3e} (bound {:.3e})'.format(err, 1e-3 + 1e-6))
    assert got.shape == (3, 200, 280) and err <= 1e-3 + 1e-6, err


# ---- 4. the builders ------------------------------------------------------------------------------------------------------------------------------
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0, 'chroma': 'bicubic'}
DN = {'op': 'DN', 'model': 'lite5', 'chroma': 'bilinear'}
# name -> (compute / output steps, the stream's edge)
CHAINS = {'sr': ([dict(SR)], 'crop'),
          'dn_sr': ([dict(DN), dict(SR)], 'crop'),
          'sr_ensemble_1': ([dict(SR, ensemble=1)], 'quantise'),
          'dn_0.6_nearest': ([{'op': 'DN', 'model': 'lite5', 'strength': 0.6, 'chroma': 'nearest'}], 'quantise'),
          'sr_to_yuv': ([dict(SR, chromaMatrix='bt601'), {'op': 'output', 'pixFmt': 'yuv420p10le'}], 'quantise')}
W, H = 140, 100


def _bgr48(seed):
    return np.random.default_rng(seed).integers(0, 65536, (H, W, 3), dtype=np.uint16)


def _by_the_definition(work, frame, dev):
    """One frame through the chain, step by step, with the unfused pieces: toTorch, per step lumaSplit -> the step on Y -> resize of C -> lumaMerge, then the output edge."""
    from moephoto_amd import imageProcess as ip, runDN, runSR
    x = ip.toTorch(16)(frame)
    yuv = None
    for s in work:
        if s['op'] == 'output':
            yuv = s['pixFmt']
            continue
        split, merge = ip.lumaSplit(s.get('chromaMatrix', 'bt709'), 'bgr'), ip.lumaMerge(s.get('chromaMatrix', 'bt709'), 'bgr')
        Y, C = split(x)
        if s['op'] == 'SR':
            Yo = runSR.sr(runSR.getOpt({k: v for k, v in s.items() if k != 'chroma' and k != 'chromaMatrix'}))(Y)
        else:
            Yo = ip.RGBFilter(runDN.getOpt({k: v for k, v in s.items() if k != 'chroma'}))(Y)
        x = merge(Yo, C if Yo.shape[-2:] == C.shape[-2:] else ip.resizeByTorch(C, Yo.shape[-1], Yo.shape[-2], s['chroma']))
    if yuv:
        return ip.toYuv(yuv)(x).cpu().numpy().tobytes()
    return ip.toOutput(16)(ip.toFloat(x)).tobytes()


@pytest.mark.parametrize('chain', sorted(CHAINS))
def test_streamed_frames_equal_serial_and_the_definition(chain, dev):
    from moephoto_amd import procedure
    _configure(True)
    work, edge = CHAINS[chain]
    steps = [{'op': 'buffer', 'bitDepth': 16}] + [dict(s) for s in work]
    frames = [_bgr48(60 + k) for k in range(3)]
    raw = b''.join(f.tobytes() for f in frames)
    process, nodes = procedure.genProcess(steps)
    want = []
    assert procedure.runFrames(process, io.BytesIO(raw).read, want.append, W, H, 16) == 3 and len(set(want)) == 3
    for k in (0, 2):
        ref = _by_the_definition(work, frames[k], dev)
        assert want[k] == ref, '{} frame {} against the definition: {}'.format(chain, k, _differ(want[k], ref))
    for depth in (1, 2, 3):
        stream = procedure.genFrameStream(steps, W, H, depth)
        assert stream.nodes == nodes and stream.edge == edge
        got = []
        assert procedure.runFramesStreamed(stream, io.BytesIO(raw).read, got.append) == 3
        stream.close()
        for k, (g, w_) in enumerate(zip(got, want)):
            assert g == w_, '{} ring depth {} frame {}: {}'.format(chain, depth, k, _differ(g, w_))


@pytest.mark.parametrize('chain', ['sr', 'dn_sr', 'dn_0.6_nearest'])
def test_reuse_stream_equals_the_plain_stream(chain, dev):
    from moephoto_amd import procedure
    _configure(True)
    steps = [{'op': 'buffer', 'bitDepth': 16}] + [dict(s) for s in CHAINS[chain][0]]
    a = _bgr48(3)
    b = a.copy()
    b[20:40, 30:70] = _bgr48(4)[20:40, 30:70]          # a partial update: rows 20 .. 40, columns 30 .. 70
    c = b.copy()
    c[90:, 120:] ^= 0x0100
    frames = [f.tobytes() for f in (a, a, b, b, c, a)]

    def run(reuse):
        stream = procedure.genFrameStream([dict(s) for s in steps], W, H, 2, reuse=reuse)
        out = []
        for f in frames:
            out += stream.push(f)
        out += stream.flush()
        stats = stream.reuse
        stream.close()
        return out, stats
    want, none = run(False)
    got, stats = run(True)
    assert none is None and len(got) == len(want) == 6
    for k, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, '{} frame {}: {}'.format(chain, k, _differ(g, w_))
    per = [dict(f) for f in stats['frames']]
    assert all(run == planned for planned, run in per[0].values())                      # the first frame runs everything
    assert all(run == 0 for planned, run in per[1].values())                            # a frame shown twice runs nothing
    assert all(0 < run <= planned for planned, run in per[2].values()), per[2]          # a partial update runs some tiles: of the chain's first tiled step a part
    assert 0 < per[2][(0, 'rgb')][1] < per[2][(0, 'rgb')][0], per[2]                    # (a later step sees the HR extents of the tiles that ran: here up to all of it)
    assert stats['pixels_run'] < stats['pixels_planned']


def test_four_plane_images_through_genprocess(dev):
    """An RGBA image: the SR step sends Y' and alpha through the net (two planes instead of four); the DN step splits alpha off first, as RGBFilter does."""
    from moephoto_amd import imageProcess as ip, procedure, runDN, runSR
    _configure(True)
    im = gd.noise_u8(9, (60, 52, 4))
    x = ip.toTorch(8)(im)
    process, _ = procedure.genProcess([dict(SR)])
    got = process(im)
    Y, C = ip.lumaSplit('bt709', 'rgb')(x)
    assert Y.shape[0] == 2
    Yo = ip.doCrop(runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}), Y)
    want = ip.toOutput8(ip.toFloat(ip.lumaMerge('bt709', 'rgb')(Yo, ip.resizeByTorch(C, 104, 120, 'bicubic'))))
    assert got.shape == (120, 104, 4) and got.dtype == np.uint8 and np.array_equal(got, want)
    process, _ = procedure.genProcess([{'op': 'DN', 'model': 'lite5', 'strength': 0.6, 'chroma': 'nearest', 'chromaMatrix': 'bt2020nc'}])
    got = process(im)
    Y, C = ip.lumaSplit('bt2020nc', 'rgb')(x[:3])
    Yo = ip.RGBFilter(runDN.getOpt({'op': 'DN', 'model': 'lite5', 'strength': 0.6}))(Y)
    want = ip.toOutput8(ip.toFloat(torch.cat([ip.lumaMerge('bt2020nc', 'rgb')(Yo, C), x[3:]], 0)))
    assert got.shape == im.shape and np.array_equal(got, want)
    assert np.array_equal(got[..., 3], ip.toOutput8(ip.toFloat(x[3:]))[..., 0])          # alpha: the plane as it was uploaded, through the output edge alone
    # a grey image: the key is a no-op
    grey = gd.noise_u8(10, (60, 52, 1))
    plain, _ = procedure.genProcess([{'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}])
    keyed, _ = procedure.genProcess([dict(SR)])
    assert np.array_equal(keyed(grey), plain(grey))
