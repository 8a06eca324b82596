"""Rounding and ordered dither in the quantising edges on the device (`pytest -m gpu`).  Every comparison is equality.  The comparators are the
written definition (moephoto_amd.quant, numpy) and, for each fused edge, its unfused composition:

  moe_to_output (flagged)                 against  quant.quantiseHWC
  moe_stitch_out / _planes / _mix / _luma against  moe_stitch -> [blend | merge] -> flagged moe_to_output, and against quant.py on moe_stitch's canvas
  moe_stitch_yuv, moe_to_yuv              against  quant.yuvFromSamples16 on the 16-bit samples of moe_stitch_out / moe_to_output
  genProcess + runFrames, genFrameStream  against  each other at ring depths 1 - 3, and against the definition applied step by step

Without the feature every flagged call is refused (an unknown bits / depth value) and the builders ignore the key."""
import io

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import luma, pixfmt, quant
from test_gpu_planes import _canvas, _differ, _dt, _es, _plan_and_pool, _st, _udt

pytestmark = pytest.mark.gpu
NP_DT = {torch.float16: np.float16, torch.float32: np.float32}
DITHERS = ('round', 'ordered')
FMT = {8: 'yuv420p', 10: 'yuv420p10le', 12: 'yuv420p12le', 16: 'yuv420p16le'}
FLAG = {'round': quant.Q_ROUND, 'ordered': quant.Q_ORDERED}


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


def _values(seed, shape, dtype):
    """[-0.25, 1.25) with values far outside [0, 1], NaN and both infinities planted (where the array is large enough to keep plain values too)."""
    v = (np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).reshape(-1)
    if v.size >= 12:
        v[3::89] = np.float32(-3.5)
        v[4::83] = np.float32(7.25)
        v[5::97] = np.nan
        v[7::193] = np.inf
        v[11::211] = -np.inf
    return v.reshape(shape).astype(NP_DT[dtype])


def _to_output(x, bits, flags, dev, lead=0):
    """Flagged moe_to_output on a dense (C, H, W) device tensor -> (H, W, C) codes; the destination starts `lead` samples behind a 16-byte boundary, between sentinels."""
    from moephoto_amd import _lib
    C, H, W = x.shape
    n = C * H * W
    out = torch.full((lead + n + 16,), 90, dtype=torch.uint8 if bits <= 8 else torch.int16, device=dev)
    assert out.data_ptr() % 16 == 0
    _lib.check(_lib.lib().moe_to_output(x.data_ptr(), _dt(x.dtype), H, W, C, bits | flags, out[lead:].data_ptr(), _udt(8 if bits <= 8 else 16), 0, _st()))
    h = out.cpu().numpy()
    assert (h[:lead] == 90).all() and (h[lead + n:] == 90).all(), 'a sentinel was overwritten'
    h = h[lead:lead + n]
    return (h if bits <= 8 else h.view(np.uint16)).reshape(H, W, C)


# ---- 1. moe_to_output -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('hw', [(1, 1), (7, 9), (100, 140)], ids='{0[0]}x{0[1]}'.format)
def test_to_output_equals_the_definition(hw, dtype, dev):
    H, W = hw
    for C in (1, 3, 4):
        host = _values(H * W + C, (C, H, W), dtype)
        x = torch.from_numpy(host).to(dev)
        for bits in (8, 16) + ((10, 12) if C == 1 else ()):
            for mode in DITHERS:
                for unit in (False, True):
                    want = quant.quantiseHWC(host, bits, mode, unit)
                    if H * W >= 100:
                        assert want.min() == 0 and want.max() == (1 << bits) - 1, 'the values do not reach both clamps'
                    for lead in (0, 1):          # C = 3 on 100 x 140, aligned: the eight-pixels-per-thread form; one sample off: the per-element form
                        got = _to_output(x, bits, FLAG[mode] | (quant.Q_UNIT if unit else 0), dev, lead)
                        assert np.array_equal(got, want), (hw, C, bits, mode, unit, lead, int((got != want).sum()))
    # the flags change something: the modes differ from the truncating quantiser and from each other
    plain = _to_output(x, 8, 0, dev)
    assert np.array_equal(plain, quant.quantiseHWC(host, 8))
    if H * W >= 100:
        assert not np.array_equal(plain, _to_output(x, 8, quant.Q_ROUND, dev)) and not np.array_equal(_to_output(x, 8, quant.Q_ORDERED, dev), _to_output(x, 8, quant.Q_ROUND, dev))


def test_to_output_fixed_points_on_the_device(dev):
    """Every 8-bit code c / 255 at every threshold of the matrix comes back under unit scale, from fp32 in both modes and from fp16 under 'round'."""
    codes = np.arange(256, dtype=np.float32) / np.float32(255)
    img = np.broadcast_to(codes.reshape(16, 16)[:, None, :, None], (16, 8, 16, 8)).reshape(1, 128, 128).copy()
    want = np.broadcast_to(np.arange(256).reshape(16, 16)[:, None, :, None], (16, 8, 16, 8)).reshape(128, 128, 1)
    for mode in DITHERS:
        assert np.array_equal(_to_output(torch.from_numpy(img).to(dev), 8, FLAG[mode] | quant.Q_UNIT, dev), want), mode
    assert np.array_equal(_to_output(torch.from_numpy(img.astype(np.float16)).to(dev), 8, quant.Q_ROUND | quant.Q_UNIT, dev), want)


# ---- 2. the fused edges ---------------------------------------------------------------------------------------------------------------------------
# (shape without planes, scale, pad, align, crop)
PLANS = {'one_tile_odd_37x45': ((37, 45), 1, 7, 8, 0),
         '2x2_tiles_ragged_140': ((100, 140), 1, 7, 8, 80),          # seams on both axes, 140 = 8 * 17 + 4
         'x2_2x2_tiles': ((50, 70), 2, 5, 8, 48),
         'narrow_172_tile_columns': ((24, 2060), 1, 2, 8, 16)}       # a second block column, a ragged end of four


def _plan(name, C, dev):
    shape, sc, pad, align, crop = PLANS[name]
    pl, pool_d, _ = _plan_and_pool(((C,) + shape, sc, pad, align, crop), C, dev)
    if name == '2x2_tiles_ragged_140':
        assert (pl.stepH, pl.stepW) == (2, 2) and pl.outW % 8 == 4
    if name == 'narrow_172_tile_columns':
        assert pl.stepW == 172 and pl.outW == 2060
    if name == 'one_tile_odd_37x45':
        assert pl.n_tiles == 1
    return pl, pool_d


def _stitch_out(pl, pool_d, C, canvas_dt, bits, flags, dev):
    from moephoto_amd import _lib
    out = torch.empty((pl.outH, pl.outW, C), dtype=torch.uint8 if bits == 8 else torch.int16, device=dev)
    _lib.check(_lib.lib().moe_stitch_out(pl._h, 0, pool_d.data_ptr(), None, C, _dt(canvas_dt), bits | flags, out.data_ptr(), _udt(bits), _st()))
    h = out.cpu().numpy()
    return h if bits == 8 else h.view(np.uint16)


@pytest.mark.parametrize('name', sorted(PLANS))
def test_stitch_out_equals_stitch_then_to_output_and_the_definition(name, dev):
    for C in ((3,) if name == 'narrow_172_tile_columns' else (1, 3, 4)):
        pl, pool_d = _plan(name, C, dev)
        for canvas_dt in (torch.float16, torch.float32):
            canvas = _canvas(pl, pool_d, None, C, canvas_dt, dev)
            host = canvas.cpu().numpy()
            for bits, mode, unit in ((8, 'ordered', True), (8, 'round', True), (8, 'ordered', False), (16, 'ordered', False), (16, 'round', True)):
                flags = FLAG[mode] | (quant.Q_UNIT if unit else 0)
                got = _stitch_out(pl, pool_d, C, canvas_dt, bits, flags, dev)
                assert np.array_equal(got, _to_output(canvas, bits, flags, dev)), (name, C, canvas_dt, bits, mode, unit, 'against moe_stitch -> moe_to_output')
                assert np.array_equal(got, quant.quantiseHWC(host, bits, mode, unit)), (name, C, canvas_dt, bits, mode, unit, 'against the definition')


def _stitch_planes(pl, pool_d, C, canvas_dt, depth, flags, dev, lead=0):
    from moephoto_amd import _lib
    n = C * pl.outH * pl.outW * _es(depth)
    flat = torch.full((lead + n + 30,), 0xA5, dtype=torch.uint8, device=dev)
    assert flat.data_ptr() % 16 == 0
    _lib.check(_lib.lib().moe_stitch_planes(pl._h, 0, pool_d.data_ptr(), None, C, _dt(canvas_dt), depth | flags, flat[lead:].data_ptr(), _st()))
    h = flat.cpu().numpy()
    assert (h[:lead] == 0xA5).all() and (h[lead + n:] == 0xA5).all(), 'a neighbour was overwritten'
    return h[lead:lead + n].tobytes()


def _planes_by_to_output(canvas, depth, flags, dev):
    """One flagged moe_to_output per plane: a sample's coordinates are its own plane's."""
    return b''.join(_to_output(canvas[c:c + 1].contiguous(), depth, flags, dev).astype(np.uint8 if depth == 8 else np.dtype('<u2')).tobytes() for c in range(canvas.shape[0]))


def _planes_by_the_definition(host, depth, mode, unit=False):
    return quant.quantise(host, depth, mode, unit).astype(np.uint8 if depth == 8 else np.dtype('<u2')).tobytes()


@pytest.mark.parametrize('name', sorted(PLANS))
def test_stitch_planes_equals_stitch_then_to_output_and_the_definition(name, dev):
    for C in (1, 2):
        pl, pool_d = _plan(name, C, dev)
        for canvas_dt in (torch.float16, torch.float32):
            canvas = _canvas(pl, pool_d, None, C, canvas_dt, dev)
            host = canvas.cpu().numpy()
            for depth in (8, 10, 12, 16):
                mode = DITHERS[(depth // 2 + C) % 2] if canvas_dt == torch.float16 else 'ordered'
                for lead in (0, 16 + _es(depth)):          # an aligned plane base, and one a single sample behind a 16-byte boundary
                    got = _stitch_planes(pl, pool_d, C, canvas_dt, depth, FLAG[mode], dev, lead)
                    want = _planes_by_the_definition(host, depth, mode)
                    assert got == want, '{} C {} {} depth {} {} lead {}: {}'.format(name, C, canvas_dt, depth, mode, lead, _differ(got, want))
                assert got == _planes_by_to_output(canvas, depth, FLAG[mode], dev), (name, C, canvas_dt, depth, mode)
            got = _stitch_planes(pl, pool_d, C, canvas_dt, 8, quant.Q_ROUND | quant.Q_UNIT, dev)
            assert got == _planes_by_the_definition(host, 8, 'round', True)


def test_stitch_planes_four_rows_per_thread_on_a_tall_narrow_canvas(dev):
    """64 x 1400, three planes: 350 four-row workgroups per plane, 1050 in all -- the four-rows-per-thread form (smaller canvases take one row per thread)."""
    pl, pool_d, _ = _plan_and_pool(((3, 1400, 64), 1, 7, 8, 512), 3, dev)
    assert pl.n_tiles == 3 and ((pl.outW + 7) // 8 + 255) // 256 * ((pl.outH + 3) // 4) * 3 >= 1024
    for canvas_dt in (torch.float16, torch.float32):
        host = _canvas(pl, pool_d, None, 3, canvas_dt, dev).cpu().numpy()
        for depth, mode in ((8, 'ordered'), (10, 'ordered'), (16, 'round')):
            got = _stitch_planes(pl, pool_d, 3, canvas_dt, depth, FLAG[mode], dev)
            want = _planes_by_the_definition(host, depth, mode)
            assert got == want, '{} depth {} {}: {}'.format(canvas_dt, depth, mode, _differ(got, want))


def _stitch_mix(pl, pool_d, C, inp, alpha, s, bits, flags, dev):
    from moephoto_amd import _lib
    planes = C + (alpha is not None)
    got = torch.full((pl.outH, pl.outW, planes), 77, dtype=torch.uint8 if bits == 8 else torch.int16, device=dev)
    sC, sH, sW = inp.stride()
    aH, aW = alpha.stride() if alpha is not None else (0, 0)
    _lib.check(_lib.lib().moe_stitch_mix(pl._h, 0, pool_d.data_ptr(), None, C, inp.data_ptr(), _dt(inp.dtype), sC, sH, sW, alpha.data_ptr() if alpha is not None else None, aH, aW,
                                         float(s), bits | flags, got.data_ptr(), _udt(bits), _st()))
    h = got.cpu().numpy()
    return h if bits == 8 else h.view(np.uint16)


MIX_PLANS = dict((k, v) for k, v in PLANS.items() if v[1] == 1)
MIX_PLANS['tall_4098x72_four_rows_per_thread'] = ((4098, 72), 1, 7, 8, 512)


@pytest.mark.parametrize('name', sorted(MIX_PLANS))
def test_stitch_mix_equals_stitch_blend_cat_quantise(name, dev):
    shape, sc, pad, align, crop = MIX_PLANS[name]
    C = 3 if name != 'tall_4098x72_four_rows_per_thread' else 2
    pl, pool_d, _ = _plan_and_pool(((C,) + shape, sc, pad, align, crop), C, dev)
    if name.startswith('tall'):
        assert (pl.outH + 3) // 4 >= 1024
    for dt in (torch.float16, torch.float32):
        pool_clean = torch.nan_to_num(pool_d, nan=0.5, posinf=2.0, neginf=-2.0)          # (what torch's blend makes of a NaN is its own business: tests/test_gpu_filter.py)
        canvas = _canvas(pl, pool_clean, None, C, dt, dev)
        inp = torch.from_numpy(_values(41, (C, pl.outH, pl.outW), torch.float32)).to(dev)
        inp = torch.nan_to_num(inp, nan=0.25, posinf=3.0, neginf=-3.0).to(dt)
        alpha = torch.from_numpy(np.random.default_rng(42).random((pl.outH, pl.outW), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).to(dev).to(dt)
        for s in (0.6, 1.0):
            y = canvas if s == 1 else s * canvas + (1 - s) * inp
            y = torch.cat([y, alpha.unsqueeze(0)], 0).contiguous()
            host = y.cpu().numpy()
            for bits, mode, unit in ((8, 'ordered', True), (16, 'round', False), (8, 'round', False)):
                flags = FLAG[mode] | (quant.Q_UNIT if unit else 0)
                got = _stitch_mix(pl, pool_clean, C, inp, alpha, s, bits, flags, dev)
                assert np.array_equal(got, _to_output(y, bits, flags, dev)), (name, dt, s, bits, mode, unit, 'against the passes')
                assert np.array_equal(got, quant.quantiseHWC(host, bits, mode, unit)), (name, dt, s, bits, mode, unit, 'against the definition')


def _stitch_luma(pl, pool_d, P, canvas_dt, c, matrix, order, bits, flags, dev):
    from moephoto_amd import _lib
    out = torch.full((pl.outH, pl.outW, P + 2), 90, dtype=torch.uint8 if bits == 8 else torch.int16, device=dev)
    _lib.check(_lib.lib().moe_stitch_luma(pl._h, 0, pool_d.data_ptr(), None, P, _dt(canvas_dt), c.data_ptr(), pixfmt.MATRICES[matrix], pixfmt.ORDERS[order], bits | flags,
                                          out.data_ptr(), _udt(bits), _st()))
    h = out.cpu().numpy()
    return h if bits == 8 else h.view(np.uint16)


def _luma_merge(Y, c, matrix, order, bits, flags, dev):
    from moephoto_amd import _lib
    P, H, W = Y.shape
    out = torch.full((H, W, P + 2), 90, dtype=torch.uint8 if bits == 8 else torch.int16, device=dev)
    _lib.check(_lib.lib().moe_luma_merge(Y.data_ptr(), _dt(Y.dtype), c.data_ptr(), P + 2, H, W, pixfmt.MATRICES[matrix], pixfmt.ORDERS[order], bits | flags, out.data_ptr(),
                                         _udt(bits), 0, _st()))
    h = out.cpu().numpy()
    return h if bits == 8 else h.view(np.uint16)


@pytest.mark.parametrize('name', sorted(MIX_PLANS) + ['x2_2x2_tiles'])
def test_stitch_luma_equals_stitch_then_merge_and_the_definition(name, dev):
    shape, sc, pad, align, crop = (MIX_PLANS.get(name) or PLANS[name])
    for P in (1, 2):
        pl, pool_d, _ = _plan_and_pool(((P,) + shape, sc, pad, align, crop), P, dev)
        c_host = (np.random.default_rng(17 + P).random((2, pl.outH, pl.outW), dtype=np.float32) * np.float32(1.2) - np.float32(0.6))
        c_host.reshape(-1)[5::97] = np.nan
        c = torch.from_numpy(c_host).to(dev)
        for canvas_dt in (torch.float16, torch.float32):
            canvas = _canvas(pl, pool_d, None, P, canvas_dt, dev)
            merged = luma.lumaMerge(canvas.cpu().numpy(), c_host, 'bt601', 'bgr')          # (the canvas form: T values; a NaN quantises to 0 whatever its payload)
            for bits, mode, unit in ((8, 'ordered', True), (16, 'ordered', False), (8, 'round', True)):
                flags = FLAG[mode] | (quant.Q_UNIT if unit else 0)
                got = _stitch_luma(pl, pool_d, P, canvas_dt, c, 'bt601', 'bgr', bits, flags, dev)
                assert np.array_equal(got, _luma_merge(canvas, c, 'bt601', 'bgr', bits, flags, dev)), (name, P, canvas_dt, bits, mode, 'against moe_stitch -> moe_luma_merge')
                assert np.array_equal(got, quant.quantiseHWC(merged, bits, mode, unit)), (name, P, canvas_dt, bits, mode, 'against the definition')


YUV_PLANS = {'even_3x4_tiles': ((3, 100, 140), 2, 5, 8, 48), 'odd_101x141': ((3, 101, 141), 1, 7, 8, 64), 'odd_111x135_one_tile': ((3, 37, 45), 3, 9, 8, 0),
             'narrow_172_tile_columns': ((3, 24, 2060), 1, 2, 8, 16)}


@pytest.mark.parametrize('name', sorted(YUV_PLANS))
def test_stitch_yuv_equals_to_yuv_equals_the_definition(name, dev):
    from moephoto_amd import _lib
    L = _lib.lib()
    pl, pool_d, _ = _plan_and_pool(YUV_PLANS[name], 3, dev)
    if name == 'odd_101x141':
        assert (pl.outH, pl.outW) == (101, 141) and pl.n_tiles > 1
    for canvas_dt in (torch.float16, torch.float32):
        canvas = _canvas(pl, pool_d, None, 3, canvas_dt, dev)
        s16 = _stitch_out(pl, pool_d, 3, canvas_dt, 16, 0, dev)
        for depth in (8, 10):
            n = pixfmt.frameBytes(FMT[depth], pl.outW, pl.outH)
            for mode in DITHERS:
                matrix, order = ('bt709', 'bgr') if mode == 'ordered' else ('bt601', 'rgb')
                want = quant.yuvFromSamples16(s16, FMT[depth], matrix, order, mode)
                flat = torch.full((n + 50,), 0xA5, dtype=torch.uint8, device=dev)
                _lib.check(L.moe_stitch_yuv(pl._h, 0, pool_d.data_ptr(), None, _dt(canvas_dt), depth | FLAG[mode], pixfmt.MATRICES[matrix], pixfmt.ORDERS[order],
                                            flat[18:].data_ptr(), _st()))
                h = flat.cpu().numpy()
                got = h[18:18 + n].tobytes()
                assert (h[:18] == 0xA5).all() and (h[18 + n:] == 0xA5).all(), 'a neighbour was overwritten'
                assert got == want, '{} {} depth {} {}: {}'.format(name, canvas_dt, depth, mode, _differ(got, want))
                out = torch.full((n + 4,), 0xA5, dtype=torch.uint8, device=dev)
                _lib.check(L.moe_to_yuv(canvas.data_ptr(), _dt(canvas_dt), pl.outH, pl.outW, depth | FLAG[mode], pixfmt.MATRICES[matrix], pixfmt.ORDERS[order], out[2:].data_ptr(), 0, _st()))
                h = out.cpu().numpy()
                assert h[2:2 + n].tobytes() == want and (h[:2] == 0xA5).all() and (h[2 + n:] == 0xA5).all(), (name, canvas_dt, depth, mode, 'moe_to_yuv')
                if mode == 'round':
                    assert want == pixfmt.fromSamples16(s16, FMT[depth], matrix, order)
                else:
                    assert want != pixfmt.fromSamples16(s16, FMT[depth], matrix, order)


# ---- 3. the chains --------------------------------------------------------------------------------------------------------------------------------
W, H = 140, 100
SR = {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}
DN06 = {'op': 'DN', 'model': 'lite5', 'strength': 0.6}


def _configure(fp16=True, crop=48):
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, fp16
    config.crop_sr = config.crop_dn = config.crop_dns = crop
    config.ensembleSR = 0


def _bgr24(seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _serial_and_streamed(steps, raw, n, edge, w=W, h=H, bits=8, frameBytes=None):
    """genProcess + runFrames -> the frames; genFrameStream at ring depths 1 - 3 gives the same."""
    from moephoto_amd import procedure
    process, nodes = procedure.genProcess(steps)
    want = []
    assert procedure.runFrames(process, io.BytesIO(raw).read, want.append, w, h, bits, frameBytes=frameBytes) == n and len(set(want)) == n
    for depth in (1, 2, 3):
        stream = procedure.genFrameStream(steps, w, h, depth)
        assert stream.nodes == nodes and stream.edge == edge
        got = []
        assert procedure.runFramesStreamed(stream, io.BytesIO(raw).read, got.append) == n
        stream.close()
        for k, (g, w_) in enumerate(zip(got, want)):
            assert g == w_, 'ring depth {} frame {}: {}'.format(depth, k, _differ(g, w_))
    return want


def _opt(step):
    from moephoto_amd import runDN, runSR
    return (runSR if step['op'] == 'SR' else runDN).getOpt(dict(step))


RGB_CHAINS = {'a2_ordered': ([dict(SR)], 'ordered', 'crop'), 'dn_lite5_0.6_round': ([dict(DN06)], 'round', 'filter'), 'dn_lite5_0.6_ordered': ([dict(DN06)], 'ordered', 'filter'),
              'a2_ensemble_1_ordered': ([dict(SR, ensemble=1)], 'ordered', 'quantise')}


@pytest.mark.parametrize('chain', sorted(RGB_CHAINS))
def test_bgr24_chains_stream_serial_and_definition(chain, dev):
    from moephoto_amd import imageProcess as ip, runSR
    _configure()
    work, mode, edge = RGB_CHAINS[chain]
    steps = [{'op': 'buffer', 'bitDepth': 8}] + work + [{'op': 'output', 'dither': mode}]
    frames = [_bgr24(60 + k) for k in range(3)]
    want = _serial_and_streamed(steps, b''.join(f.tobytes() for f in frames), 3, edge)
    plain = _serial_and_streamed([s for s in steps if s['op'] != 'output'], frames[0].tobytes(), 1, edge)
    assert plain[0] != want[0], 'the key changed nothing'
    for k in (0, 2):          # step by step: the reader's / 255, the step's canvas, the definition at unit scale
        x = ip.toTorch(8)(frames[k])
        y = runSR.sr(_opt(work[0]))(x) if work[0]['op'] == 'SR' else ip.RGBFilter(_opt(work[0]))(x)
        ref = quant.quantiseHWC(y.cpu().numpy(), 8, mode, unit=True).tobytes()
        assert want[k] == ref, '{} frame {} against the definition: {}'.format(chain, k, _differ(want[k], ref))


def test_a2_to_yuv420p_ordered(dev):
    from moephoto_amd import imageProcess as ip
    _configure()
    steps = [{'op': 'buffer', 'bitDepth': 8}, dict(SR), {'op': 'output', 'pixFmt': 'yuv420p', 'dither': 'ordered'}]
    frames = [_bgr24(70 + k) for k in range(3)]
    want = _serial_and_streamed(steps, b''.join(f.tobytes() for f in frames), 3, 'crop')
    for k in (0, 2):
        y = ip.doCrop(_opt(SR), ip.toTorch(8)(frames[k]))
        ref = quant.yuvFromSamples16(quant.quantiseHWC(y.cpu().numpy(), 16), 'yuv420p', 'bt709', 'bgr', 'ordered')
        assert want[k] == ref, 'frame {}: {}'.format(k, _differ(want[k], ref))
        assert want[k] != pixfmt.fromSamples16(quant.quantiseHWC(y.cpu().numpy(), 16), 'yuv420p')


def _planar_frames(n, fmt, seed=5):
    from test_gpu_planes import _frame
    return [_frame(seed + k, pixfmt.FORMATS[fmt], W, H) for k in range(n)]


def test_planar_10_to_8_chroma_net_ordered(dev):
    from moephoto_amd import imageProcess as ip
    _configure()
    src, dst = 'yuv420p10le', 'yuv420p'
    steps = [{'op': 'buffer', 'pixFmt': src}, dict(SR), {'op': 'output', 'pixFmt': dst, 'dither': 'ordered'}]
    frames = _planar_frames(3, src)
    want = _serial_and_streamed(steps, b''.join(frames), 3, 'crop', frameBytes=pixfmt.frameBytes(src, W, H))
    opt = _opt(SR)
    for k in (0, 2):          # the definition: toPlanes, doCrop on each image, each plane quantised at its own coordinates
        Y, C = pixfmt.toPlanes(frames[k], src, W, H, np.float16)
        oy, oc = (ip.doCrop(opt, torch.from_numpy(p.copy()).to(dev)).cpu().numpy() for p in (Y, C))
        ref = quant.quantise(oy, 8, 'ordered').tobytes() + quant.quantise(oc, 8, 'ordered').tobytes()
        assert want[k] == ref, 'frame {}: {}'.format(k, _differ(want[k], ref))
    # the unfused edge (an ensemble: toPlanes plane by plane) gives the definition's bytes too
    steps[1] = dict(SR, ensemble=1)
    ens = _serial_and_streamed(steps, frames[0], 1, 'quantise', frameBytes=pixfmt.frameBytes(src, W, H))
    from moephoto_amd import runSR
    Y, C = pixfmt.toPlanes(frames[0], src, W, H, np.float16)
    oy, oc = (runSR.sr(_opt(steps[1]))(torch.from_numpy(p.copy()).to(dev)).cpu().numpy() for p in (Y, C))
    assert ens[0] == quant.quantise(oy, 8, 'ordered').tobytes() + quant.quantise(oc, 8, 'ordered').tobytes()


def test_planar_luma_only_chain_dithers_luma_alone(dev):
    from moephoto_amd import imageProcess as ip
    _configure()
    src, dst = 'yuv420p10le', 'yuv420p'
    source = {'op': 'buffer', 'pixFmt': src, 'chroma': 'bicubic'}
    frames = _planar_frames(3, src, 9)
    raw, nb = b''.join(frames), pixfmt.frameBytes(src, W, H)
    want = _serial_and_streamed([source, dict(SR), {'op': 'output', 'pixFmt': dst, 'dither': 'ordered'}], raw, 3, 'crop', frameBytes=nb)
    plain = _serial_and_streamed([source, dict(SR), {'op': 'output', 'pixFmt': dst}], raw, 3, 'crop', frameBytes=nb)
    cb = pixfmt.planeOffsets(dst, 2 * W, 2 * H)[1]
    opt = _opt(SR)
    for k in range(3):
        assert want[k][cb:] == plain[k][cb:], 'frame {}: the chroma planes come from the integer filter and do not change'.format(k)
        Y, _ = pixfmt.toPlanes(frames[k], src, W, H, np.float16)
        ref = quant.quantise(ip.doCrop(opt, torch.from_numpy(Y.copy()).to(dev)).cpu().numpy(), 8, 'ordered').tobytes()
        assert want[k][:cb] == ref and want[k][:cb] != plain[k][:cb], 'frame {}: {}'.format(k, _differ(want[k][:cb], ref))


def test_luma_only_rgb_step(dev):
    from moephoto_amd import imageProcess as ip
    _configure()
    step = dict(SR, chroma='bicubic')
    steps = [{'op': 'buffer', 'bitDepth': 8}, step, {'op': 'output', 'dither': 'ordered'}]
    frames = [_bgr24(80 + k) for k in range(3)]
    want = _serial_and_streamed(steps, b''.join(f.tobytes() for f in frames), 3, 'crop')
    for k in (0, 2):
        x = ip.toTorch(8)(frames[k])
        Y, C = ip.lumaSplit('bt709', 'bgr')(x)
        Yo = ip.doCrop(_opt(SR), Y)
        merged = ip.lumaMerge('bt709', 'bgr')(Yo, ip.resizeByTorch(C, 2 * W, 2 * H, 'bicubic'))
        ref = quant.quantiseHWC(merged.cpu().numpy(), 8, 'ordered', unit=True).tobytes()
        assert want[k] == ref, 'frame {}: {}'.format(k, _differ(want[k], ref))
    # the unfused merge (an ensemble in front of it) writes the same definition
    steps[1] = dict(step, ensemble=1)
    _serial_and_streamed(steps, frames[0].tobytes(), 1, 'quantise')


@pytest.mark.parametrize('chain', ['a2_ordered', 'dn_lite5_0.6_ordered', 'a2_yuv420p', 'planar_net'])
def test_reuse_stream_equals_the_plain_dithered_stream(chain, dev):
    from moephoto_amd import procedure
    _configure()
    out = {'op': 'output', 'dither': 'ordered'}
    if chain == 'planar_net':
        steps, a = [{'op': 'buffer', 'pixFmt': 'yuv420p'}, dict(SR), out], np.frombuffer(_planar_frames(1, 'yuv420p')[0], np.uint8).copy()
        b = a.copy()
        b[20 * W + 30:20 * W + 70] ^= 0x10          # a few luma samples of row 20
    else:
        steps = [{'op': 'buffer', 'bitDepth': 8}] + RGB_CHAINS.get(chain, ([dict(SR)],))[0] + [dict(out, pixFmt='yuv420p') if chain == 'a2_yuv420p' else out]
        a = _bgr24(3)
        b = a.copy()
        b[20:40, 30:70] = _bgr24(4)[20:40, 30:70]
    frames = [f.tobytes() for f in (a, a, b, b, a)]

    def run(reuse):
        stream = procedure.genFrameStream([dict(s) for s in steps], W, H, 2, reuse=reuse, views=reuse)
        got = []
        for f in frames:
            got += [bytes(v) for v in stream.push(f)]
        got += [bytes(v) for v in stream.flush()]
        stats = stream.reuse
        stream.close()
        return got, stats
    want, _ = run(False)
    got, stats = run(True)
    assert len(got) == len(want) == 5 and want[0] != want[2]
    for k, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, '{} frame {}: {}'.format(chain, k, _differ(g, w_))
    per = [dict(f) for f in stats['frames']]
    assert all(r == 0 for _, r in per[1].values()) and stats['pixels_run'] < stats['pixels_planned']


def test_an_8_bit_still_image_through_genprocess(dev):
    from moephoto_amd import imageProcess as ip, procedure
    _configure()
    im = gd.noise_u8(9, (60, 52, 3))
    for mode in DITHERS:
        process, _ = procedure.genProcess([dict(SR), {'op': 'output', 'dither': mode}])
        got = process(im)
        y = ip.doCrop(_opt(SR), ip.toTorch(8)(im))
        want = quant.quantiseHWC(y.cpu().numpy(), 8, mode, unit=True)
        assert got.shape == (120, 104, 3) and got.dtype == np.uint8 and np.array_equal(got, want), mode
    plain, _ = procedure.genProcess([dict(SR)])
    assert not np.array_equal(plain(im), got)
    none, _ = procedure.genProcess([dict(SR), {'op': 'output', 'dither': 'none'}])
    assert np.array_equal(none(im), plain(im))
