"""The DN step's edge on the device, bit for bit against the passes it replaces (`pytest -m gpu`):

  moe_stitch_mix                        against  moe_stitch -> torch s * c + (1 - s) * inp -> torch.cat(alpha) [-> fp32 -> moe_to_output]
  imageProcess._RGBFilter, flag on      against  the same with config.filterOnDevice = False (the torch expressions)
  imageProcess.filterOut                against  toOutput(bits)(toFloat(_RGBFilter(opt, img))) with the flag off
  genFrameStream + runFramesStreamed    against  genProcess + runFrames, on the 'filter' edge

Both sides of every comparison run in this process on the same fp32 tile values: equality is the bar, there is no tolerance anywhere in this file."""
import ctypes
import io

import numpy as np
import pytest
import torch

import golden_defs as gd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------
# (shape, scale, pad, align, crop): a multi-tile grid with seams on both axes; one plane; one tile with reflect-padded axes, an odd width and unaligned rows; 2 x 2 tiles
PLANS = {'rgb_100x140_c48': ((3, 100, 140), 1, 7, 8, 48), 'gray_100x140_c48': ((1, 100, 140), 1, 7, 8, 48),
         'one_tile_odd_37x45': ((3, 37, 45), 1, 7, 8, 0), 'rgb_72x88_c32': ((3, 72, 88), 1, 7, 8, 32)}
STRENGTHS = (0.0, 0.3, 0.6, 1.25, 1.0)
_OUT = {8: (torch.uint8, 2), 16: (torch.int16, 3)}       # bits -> (storage, library dtype MOE_U8 / MOE_U16)


def _lib_dt(dt):
    from moephoto_amd import _lib
    return _lib.F16 if dt == torch.float16 else _lib.F32


def _plan_and_pool(params, dev, order=None):
    """TilePlan + a pool seeded per tile, drawn from [-0.25, 1.25): both clamps of the quantiser are within reach.  order: the tiles' order in the pool."""
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


def _image(shape, seed, dt, dev):
    """Values of [-0.25, 1.25) in dtype dt."""
    a = np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)
    return torch.from_numpy(a).to(dev).to(dt)


def _stitch(pl, C, pool_d, host_off, dt, dev):
    from moephoto_amd import _lib
    canvas = torch.empty((C, pl.outH, pl.outW), dtype=dt, device=dev)
    off = (ctypes.c_int64 * pl.n_tiles)(*host_off) if host_off is not None else None
    _lib.check(_lib.lib().moe_stitch(pl._h, 0, pool_d.data_ptr(), off, C, canvas.data_ptr(), _lib_dt(dt), torch.cuda.current_stream().cuda_stream))
    return canvas


def _quantise(y, bits, dev):
    """toFloat's fp32 copy and the quantiser, as the serial path runs them."""
    from moephoto_amd import _lib
    C, H, W = y.shape
    f32 = y.float().contiguous()
    want = torch.empty((H, W, C), dtype=_OUT[bits][0], device=dev)
    _lib.check(_lib.lib().moe_to_output(f32.data_ptr(), _lib.F32, H, W, C, bits, want.data_ptr(), _OUT[bits][1], 0, torch.cuda.current_stream().cuda_stream))
    return want


def _passes(canvas, inp, alpha, s):
    """The passes behind the stitch: strengthOp's expression as torch evaluates it on the device, then mergeAlpha's concatenation."""
    y = canvas if s == 1 else s * canvas + (1 - s) * inp
    return torch.cat([y, alpha.unsqueeze(0)], 0) if alpha is not None else y


def _stitch_mix(pl, C, pool_d, off_d, inp, alpha, s, bits, dev):
    from moephoto_amd import _lib
    planes = C + (alpha is not None)
    if bits == 0:
        got = torch.full((planes, pl.outH, pl.outW), 77, dtype=inp.dtype, device=dev)
        dst_dt = _lib_dt(inp.dtype)
    else:
        got = torch.full((pl.outH, pl.outW, planes), 77, dtype=_OUT[bits][0], device=dev)
        dst_dt = _OUT[bits][1]
    sC, sH, sW = inp.stride()
    aH, aW = alpha.stride() if alpha is not None else (0, 0)
    _lib.check(_lib.lib().moe_stitch_mix(pl._h, 0, pool_d.data_ptr(), off_d.data_ptr() if off_d is not None else None, C, inp.data_ptr(), _lib_dt(inp.dtype), sC, sH, sW,
                                         alpha.data_ptr() if alpha is not None else None, aH, aW, float(s), bits, got.data_ptr(), dst_dt,
                                         torch.cuda.current_stream().cuda_stream))
    return got


def _same(got, want):
    """Bit equality, NaNs included."""
    if got.dtype == torch.float16:
        got, want = got.view(torch.int16), want.view(torch.int16)
    elif got.dtype == torch.float32:
        got, want = got.view(torch.int32), want.view(torch.int32)
    return got.shape == want.shape and int((got != want).sum().item()) == 0


def _check_all_forms(tag, pl, C, pool_d, off_d, canvas, inp, alpha, s, dev, clamps=True):
    want = _passes(canvas, inp, alpha, s)
    assert want.dtype == canvas.dtype
    got = _stitch_mix(pl, C, pool_d, off_d, inp, alpha, s, 0, dev)
    assert _same(got, want), '{}: canvas form, {} of {} values differ'.format(tag, int((got != want).sum().item()), want.numel())
    for bits in (8, 16):
        wq = _quantise(want, bits, dev)
        gq = _stitch_mix(pl, C, pool_d, off_d, inp, alpha, s, bits, dev)
        if clamps:
            samples = wq.to(torch.int32) & 0xFFFF                     # (uint16 samples live in int16 storage)
            assert samples.min().item() == 0 and samples.max().item() == (1 << bits) - 1, '{}: the blend does not reach both clamps'.format(tag)
        assert _same(gq, wq), '{}: {} bits, {} of {} samples differ'.format(tag, bits, int((gq != wq).sum().item()), wq.numel())


@pytest.mark.parametrize('name', sorted(PLANS))
def test_stitch_mix_equals_stitch_blend_cat_quantise(name, dev):
    from moephoto_amd import _lib
    pl, C, pool_d, _ = _plan_and_pool(PLANS[name], dev)
    assert (pl.outH, pl.outW) == PLANS[name][0][1:]
    for dt in (torch.float16, torch.float32):
        canvas = _stitch(pl, C, pool_d, None, dt, dev)
        inp = _image((C, pl.outH, pl.outW), 41, dt, dev)
        alpha = _image((pl.outH, pl.outW), 42, dt, dev)
        for s in STRENGTHS:
            for al in (None, alpha):
                if al is not None and C == 4:
                    continue
                _check_all_forms('{} {} s={} alpha={}'.format(name, dt, s, al is not None), pl, C, pool_d, None, canvas, inp, al, s, dev)
        # strength 1 is the plain stitch, canvas and samples
        assert _same(_stitch_mix(pl, C, pool_d, None, inp, None, 1.0, 0, dev), canvas)
        for bits in (8, 16):
            plain = torch.empty((pl.outH, pl.outW, C), dtype=_OUT[bits][0], device=dev)
            _lib.check(_lib.lib().moe_stitch_out(pl._h, 0, pool_d.data_ptr(), None, C, _lib_dt(dt), bits, plain.data_ptr(), _OUT[bits][1], torch.cuda.current_stream().cuda_stream))
            assert _same(_stitch_mix(pl, C, pool_d, None, inp, None, 1.0, bits, dev), plain)


def test_stitch_mix_strength_one_keeps_the_stitch_nans(dev):
    pl, C, pool_d, _ = _plan_and_pool(PLANS['rgb_72x88_c32'], dev)
    pool_d[::97] = float('nan')
    pool_d[5::101] = float('inf')
    for dt in (torch.float16, torch.float32):
        canvas = _stitch(pl, C, pool_d, None, dt, dev)
        assert torch.isnan(canvas).any()
        inp = _image((C, pl.outH, pl.outW), 41, dt, dev)
        assert _same(_stitch_mix(pl, C, pool_d, None, inp, None, 1.0, 0, dev), canvas)


def test_stitch_mix_reads_a_strided_view(dev):
    """inp = every second column of a wider tensor (sW = 2), alpha likewise, and an unaligned plane base: the scalar path."""
    pl, C, pool_d, _ = _plan_and_pool(PLANS['rgb_100x140_c48'], dev)
    for dt in (torch.float16, torch.float32):
        canvas = _stitch(pl, C, pool_d, None, dt, dev)
        wide = _image((C + 1, pl.outH, 2 * pl.outW), 43, dt, dev)
        inp, alpha = wide[:C, :, ::2], wide[C, :, 1::2]
        assert inp.stride(2) == 2 and alpha.stride(1) == 2 and not inp.is_contiguous()
        _check_all_forms('strided {}'.format(dt), pl, C, pool_d, None, canvas, inp, alpha, 0.6, dev)
        rows = _image((C, pl.outH + 1, pl.outW + 3), 44, dt, dev)[:, 1:, 3:]      # unit column stride, rows that start off a 16-byte boundary
        assert rows.stride(2) == 1 and rows.data_ptr() % 16 != 0
        _check_all_forms('unaligned rows {}'.format(dt), pl, C, pool_d, None, canvas, rows, None, 0.3, dev)


def test_stitch_mix_four_rows_per_thread_on_a_tall_canvas(dev):
    """Canvases of 1024 four-row workgroups and more take the four-rows-per-thread form (smaller ones one row per thread): 4098 rows, the last workgroup ragged."""
    pl, C, pool_d, _ = _plan_and_pool(((2, 4098, 72), 1, 7, 8, 512), dev)
    assert pl.n_tiles > 4 and (pl.outH + 3) // 4 >= 1024
    for dt in (torch.float16, torch.float32):
        canvas = _stitch(pl, C, pool_d, None, dt, dev)
        inp, alpha = _image((C, pl.outH, pl.outW), 41, dt, dev), _image((pl.outH, pl.outW), 42, dt, dev)
        _check_all_forms('tall {}'.format(dt), pl, C, pool_d, None, canvas, inp, alpha, 0.3, dev)
        _check_all_forms('tall {} no alpha'.format(dt), pl, C, pool_d, None, canvas, inp, None, 0.6, dev)


def test_stitch_mix_with_a_permuted_pool_layout(dev):
    params = PLANS['rgb_100x140_c48']
    n = _plan_and_pool(params, dev)[0].n_tiles
    order = list(reversed(range(n)))
    pl, C, pool_d, off = _plan_and_pool(params, dev, order)
    assert n > 4 and off != pl.tile_offsets(C)
    off_d = torch.tensor(off, dtype=torch.int64, device=dev)
    canvas = _stitch(pl, C, pool_d, off, torch.float16, dev)
    plain = _stitch(*_plan_and_pool(params, dev)[:3], None, torch.float16, dev)
    assert _same(canvas, plain)
    inp, alpha = _image((C, pl.outH, pl.outW), 41, torch.float16, dev), _image((pl.outH, pl.outW), 42, torch.float16, dev)
    _check_all_forms('permuted', pl, C, pool_d, off_d, canvas, inp, alpha, 0.6, dev)


# ---- 2. the roundings, on every finite fp16 value ------------------------------------------------------------------------------------------
def test_blend_rounds_as_torch_on_every_finite_half(dev):
    """One tile of 248 x 256 = 63,488 pixels whose pool holds every finite fp16 value once (exact in fp32, so the fold's value is that value), blended with the same
    values in a seeded permutation: a fused multiply-add or a product rounded once to fp16 instead of fp32-then-fp16 shows here (the ensemble's closing average found
    its tie cases the same way)."""
    from moephoto_amd.imageProcess import TilePlan
    bits = np.concatenate([np.arange(0, 0x7C00), np.arange(0x8000, 0xFC00)]).astype(np.uint16)
    vals = bits.view(np.float16)
    assert vals.size == 63488 and np.isfinite(vals.astype(np.float32)).all()
    pl = TilePlan((1, 248, 256), 1 << 40, 1e-3, 7, 1, 8, 0)
    assert pl.n_tiles == 1 and (pl.outH, pl.outW) == (248, 256) and pl.pool_elems(1) == vals.size
    pool_d = torch.from_numpy(vals.astype(np.float32)).to(dev)
    c16 = torch.from_numpy(vals.copy()).to(dev).view(1, 248, 256)
    assert _same(_stitch(pl, 1, pool_d, None, torch.float16, dev), c16)
    inp = torch.from_numpy(vals[np.random.default_rng(63488).permutation(vals.size)].copy()).to(dev).view(1, 248, 256)
    for s in (0.3, 0.6, 1 / 3):
        want = s * c16 + (1 - s) * inp
        got = _stitch_mix(pl, 1, pool_d, None, inp, None, s, 0, dev)
        bad = int((got.view(torch.int16) != want.view(torch.int16)).sum().item())
        assert bad == 0, 'strength {}: {} of {} values differ'.format(s, bad, want.numel())
        assert _same(_stitch_mix(pl, 1, pool_d, None, inp, None, s, 16, dev), _quantise(want, 16, dev))
        # the same values behind a strided view: torch serves it with another kernel, whose products are rounded once (stitch_mix_kernel's comment)
        wide = torch.zeros((1, 248, 512), dtype=torch.float16, device=dev)
        wide[..., ::2] = inp
        view = wide[..., ::2]
        want = s * c16 + (1 - s) * view
        got = _stitch_mix(pl, 1, pool_d, None, view, None, s, 0, dev)
        bad = int((got.view(torch.int16) != want.view(torch.int16)).sum().item())
        assert bad == 0, 'strength {}, strided input: {} of {} values differ'.format(s, bad, want.numel())


# ---- 3. _RGBFilter ------------------------------------------------------------------------------------------------------------------------
def _configure(fp16, crop):
    from moephoto_amd.config import config
    config.modelRoot, config.deviceId, config.fp16 = gd.ZOO, 0, fp16
    config.crop_sr = config.crop_dn = config.crop_dns = crop
    config.ensembleSR = 0


def _flag_off(f):
    from moephoto_amd.config import config
    assert config.filterOnDevice is True
    config.filterOnDevice = False
    try:
        return f()
    finally:
        config.filterOnDevice = True


@pytest.mark.parametrize('fp16', [True, False], ids=['fp16', 'fp32'])
@pytest.mark.parametrize('planes', [3, 4])
def test_rgbfilter_on_device_equals_the_torch_expressions(planes, fp16, dev):
    from moephoto_amd import imageProcess as ip, runDN
    from moephoto_amd.config import config
    _configure(fp16, 48)
    opt = runDN.getOpt({'op': 'DN', 'model': 'lite5', 'strength': 0.6})
    x = torch.from_numpy(gd.noise_image(31, (planes, 72, 88))).to(dev).to(config.dtype())
    want = _flag_off(lambda: ip._RGBFilter(opt, x))
    got = ip._RGBFilter(opt, x)
    assert ip._plan_for(opt, (3, 72, 88)).n_tiles > 1
    assert got.dtype == want.dtype == config.dtype() and tuple(got.shape) == (planes, 72, 88)
    assert torch.equal(got, want)
    if planes == 4:
        assert torch.equal(got[3], x[3])
    # strength 1: without alpha the step is doCrop itself; with alpha the plane still rides in the fold
    opt.strength = 1.0
    one = ip._RGBFilter(opt, x)
    assert torch.equal(one[:3], ip.doCrop(opt, x[:3])) and torch.equal(one, _flag_off(lambda: ip._RGBFilter(opt, x)))
    assert not torch.equal(one[:3], got[:3])


# ---- 4. filterOut -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', [3, 4])
def test_filterout_equals_rgbfilter_float_output(planes, dev):
    from moephoto_amd import imageProcess as ip, runDN
    from moephoto_amd.config import config
    _configure(True, 48)
    opt = runDN.getOpt({'op': 'DN', 'model': 'lite5', 'strength': 0.6})
    x = torch.from_numpy(gd.noise_image(31, (planes, 72, 88))).to(dev).to(config.dtype())
    canvas = _flag_off(lambda: ip._RGBFilter(opt, x))
    for bits in (8, 16):
        want = ip.toOutput(bits)(ip.toFloat(canvas))
        got = ip.filterOut(opt, x, bits)
        assert got.device.type == 'cuda' and got.dtype == _OUT[bits][0] and tuple(got.shape) == want.shape == (72, 88, planes)
        got = got.cpu().numpy().view(want.dtype)
        bad = int((got != want).sum())
        assert bad == 0, '{} planes, {} bits: {} of {} samples differ'.format(planes, bits, bad, want.size)
    out = torch.empty((72, 88, planes), dtype=torch.uint8, device=dev)
    assert ip.filterOut(opt, x, 8, out=out) is out
    with pytest.raises(ValueError):
        ip.filterOut(opt, x, 12)
    with pytest.raises(ValueError):
        ip.filterOut(opt, x, 8, out=torch.empty((4, 4, planes), dtype=torch.uint8, device=dev))


# ---- 5. the stream ------------------------------------------------------------------------------------------------------------------------
H, W = 72, 88


def test_streamed_dn_frames_take_the_filter_edge_and_equal_serial(dev):
    from moephoto_amd import procedure
    _configure(True, 48)
    steps = [{'op': 'buffer', 'bitDepth': 16}, {'op': 'DN', 'model': 'lite5', 'strength': 0.6}]
    rng = np.random.default_rng(5)
    raw = b''.join(rng.integers(0, 1 << 16, (H, W, 3), dtype=np.uint16).tobytes() for _ in range(5))
    process, nodes = procedure.genProcess(steps, bitDepth=16)
    want, got = [], []
    n0 = procedure.runFrames(process, io.BytesIO(raw).read, want.append, W, H, bitDepth=16)
    stream = procedure.genFrameStream(steps, W, H, 2)
    try:
        assert stream.edge == 'filter' and stream.nodes == nodes
        n1 = procedure.runFramesStreamed(stream, io.BytesIO(raw).read, got.append)
    finally:
        stream.close()
    assert n1 == n0 == len(want) == len(got) == 5 and len(set(want)) == 5
    for k, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, 'frame {}: {} bytes differ'.format(k, int((np.frombuffer(g, np.uint8) != np.frombuffer(w_, np.uint8)).sum()))
    # the other edges keep their names: strength 1 folds straight into the samples, the flag off leaves the blend to torch and the quantiser
    for st, flag, name in ((1.0, True, 'crop'), (0.6, False, 'quantise')):
        f = lambda: procedure.genFrameStream([steps[0], dict(steps[1], strength=st)], W, H, 2)
        s2 = f() if flag else _flag_off(f)
        try:
            assert s2.edge == name
        finally:
            s2.close()
