"""Parity of the HIP path (through the C ABI) against the oracle and the reference's golden vectors.
Needs a HIP device: `pytest -m gpu`.

ONE tolerance for the product's default arithmetic (precision 'auto'), on every input class and every golden:

    TOL = 1e-3 max-abs, compared in fp32        (north star: 1e-3 vs the reference's PyTorch-CPU fp32 path)

'auto' resolves to 'mixed' for Net2x/3x/4x and NetDN (fp16 MFMA operands, hi+lo trunk stream, split operands on the few
error-setting layers: DESIGN.md section 5, tests/emu_precision.py), 'fp16' for SEDN, 'fp16x3' for lite*.  Other bounds
in this file belong to explicitly forced, non-default modes and are written where they are used:
  'fp16x3' forced (hi/lo split operands everywhere)   2e-5   (observed ~1e-6)
  'fp16' forced (= the arithmetic of the reference's own GPU fp16 mode)   documented per family in
      test_net_forward_fast_mode_documented_error
  stitch kernel alone (fp32 in/out): 1e-6 (the ramp's sigmoid differs from torch's by <= 1 ulp)
  fp16 OUTPUT dtype requested by the caller (config.fp16): + 5e-4, the rounding of a value in [1, 2) to half
"""
import glob
import os

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd.weights import load_state_dict_file
from oracle import imageio as oio, nets as onets, planner as oplanner, stitch as ostitch
from tests_util import oracle_ensemble

pytestmark = pytest.mark.gpu
G = gd.GOLDEN
TOL = 1e-3
HALF_OUT = 5e-4           # extra allowance when the caller asks for an fp16 result tensor (values up to 2: half an ulp = 4.9e-4)


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    return torch.device('cuda:0')


_models = {}


def module_for(key, precision='auto', dtype=torch.float32):
    from moephoto_amd import models
    ctor = {'net2x': models.Net2x, 'net3x': models.Net3x, 'net4x': models.Net4x, 'netdn': models.NetDN, 'sedn': models.SEDN,
            'lite2': lambda: models.Net(2), 'lite4': lambda: models.Net(4), 'lite8': lambda: models.Net(8)}[gd.MODELS[key][0]]
    k = (key, precision)
    if k not in _models:
        m = ctor()
        m.load_state_dict({n: torch.from_numpy(v) for n, v in gd.state_dict_for(key, load_state_dict_file).items()})
        m.eval()
        m.precision = precision
        _models[k] = m
    return _models[k].to(dtype=dtype, device='cuda:0')


NET_KEYS = [os.path.basename(p)[:-4] for p in sorted(glob.glob(os.path.join(G, 'nets', '*.npz')))]


@pytest.mark.parametrize('key', NET_KEYS)
def test_net_forward_vs_reference_golden(key, dev):
    """Single-tile forward of every net family on the seeded inputs of tests/golden/nets (reference outputs)."""
    z = np.load(os.path.join(G, 'nets', key + '.npz'))
    h, w = [int(v) for v in z['hw']]
    seed = int(z['seed'])
    m = module_for(key)
    for kind in ('natural', 'noise'):
        x = gd.natural_image(seed, (3, h, w))[:, None] if kind == 'natural' else gd.noise_image(seed, (3, 1, h, w))
        y = m(torch.from_numpy(x).to(dev))[-1].float().cpu().numpy()
        err = np.abs(y - z['y_' + kind]).max()
        assert err <= TOL, '{} {} ({}): {:.3e}'.format(key, kind, m.resolved_precision(), err)


@pytest.mark.parametrize('key', NET_KEYS)
def test_net_forward_fast_mode_documented_error(key, dev):
    """Forced single-pass fp16 operands: what fp16 activation/weight rounding costs per family (documented bound)."""
    z = np.load(os.path.join(G, 'nets', key + '.npz'))
    h, w = [int(v) for v in z['hw']]
    seed = int(z['seed'])
    arch = gd.MODELS[key][0]
    tol_nat = 1.5e-3 if arch in ('net2x', 'net3x', 'net4x', 'sedn') else (2.5e-3 if arch == 'netdn' else 6e-3)
    m = module_for(key, 'fp16')
    for kind, tol in (('natural', tol_nat), ('noise', 1e-2)):
        x = gd.natural_image(seed, (3, h, w))[:, None] if kind == 'natural' else gd.noise_image(seed, (3, 1, h, w))
        y = m(torch.from_numpy(x).to(dev))[-1].float().cpu().numpy()
        err = np.abs(y - z['y_' + kind]).max()
        assert err <= tol, '{} {}: {:.3e}'.format(key, kind, err)


@pytest.mark.parametrize('key', ['a2', 'a4', 'dn_lite5', 'l25', 'lite2'])
def test_net_forward_exact_mode_noise(key, dev):
    z = np.load(os.path.join(G, 'nets', key + '.npz'))
    h, w = [int(v) for v in z['hw']]
    m = module_for(key, 'fp16x3')
    x = gd.noise_image(int(z['seed']), (3, 1, h, w))
    y = m(torch.from_numpy(x).to(dev))[-1].float().cpu().numpy()
    assert np.abs(y - z['y_noise']).max() <= 2e-5      # far inside the 1e-3 bar


@pytest.mark.parametrize('key', ['a2', 'dn_lite10', 'l25', 'lite4'])
def test_layer_by_layer(key, dev):
    """Named intermediates (debug taps) against the oracle's, to localise a failing kernel."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    x = gd.natural_image(3, (2, 24, 40))[:, None]
    taps = {}
    onets.forward(arch, sd, x, 'torch', taps)
    m = module_for(key).set_debug(True)
    m(torch.from_numpy(x).to(dev))
    torch.cuda.synchronize()
    for name, want in taps.items():
        got = m.debug_tap(name)
        want = want.numpy()
        scale = max(1.0, float(np.abs(want).max()))      # intermediates are not normalised to [0, 1]: the bound is relative to their swing
        assert got.shape == want.shape, name
        tol = (2e-3 if arch == 'sedn' else 1e-3) * scale      # SEDN: fp16 operands through 16 blocks (its OUTPUT is held to TOL elsewhere)
        assert np.abs(got - want).max() <= tol, '{} {}: {:.3e} (swing {:.2f})'.format(key, name, np.abs(got - want).max(), scale)
    m.set_debug(False)


def test_ragged_and_tiny_tiles(dev):
    """Edge tiles the planner produces: 8x16 up to non-multiples of the 8x32 patch; strided slice views; fp16 and
    fp32 I/O.  Run with split operands so that the bound (2e-5) is tight enough to expose any indexing slip."""
    sd = gd.state_dict_for('a2', load_state_dict_file)
    mx = module_for('a2', 'fp16x3')
    for (h, w) in ((8, 16), (8, 8), (16, 88), (40, 33 * 8), (88, 192), (24, 24), (9, 35)):
        big = gd.natural_image(9, (3, h + 6, w + 10))
        xs = torch.from_numpy(big).to(dev)[:, None, 3:3 + h, 5:5 + w]            # non-contiguous slice view, like doCrop's
        want = onets.forward('net2x', sd, np.ascontiguousarray(big[:, None, 3:3 + h, 5:5 + w])).numpy()
        y = mx(xs)[-1]
        assert y.shape == (3, 1, 2 * h, 2 * w) and y.dtype == torch.float32
        assert np.abs(y.cpu().numpy() - want).max() <= 2e-5, (h, w)
    mf = module_for('a2')                             # the default arithmetic (fused tail kernel, hi+lo stream)
    x = gd.natural_image(9, (3, 40, 264))[:, None]    # the busiest tile of the sweep: 1.3-1.4e-3 with plain fp16 operands
    y = mf(torch.from_numpy(x).to(dev))[-1].cpu().numpy()
    assert np.abs(y - onets.forward('net2x', sd, x).numpy()).max() <= TOL
    for (h, w) in ((9, 35), (24, 52), (16, 42), (8, 16), (88, 192)):      # fused-tail kernel: widths that are odd / 4-aligned only / 2-aligned (fallback paths)
        for kind in ('natural', 'noise'):
            x = (gd.natural_image(11, (3, h, w)) if kind == 'natural' else gd.noise_image(11, (3, h, w)))[:, None]
            y = mf(torch.from_numpy(x).to(dev))[-1].cpu().numpy()
            assert np.abs(y - onets.forward('net2x', sd, x).numpy()).max() <= TOL, (h, w, kind)
    m16 = module_for('a2', dtype=torch.float16)
    x = gd.natural_image(9, (4, 40, 48))[:, None]                                 # 4 planes: RGBA through SR
    x16 = torch.from_numpy(x).half()
    y = m16(x16.to(dev))[-1]
    assert y.dtype == torch.float16
    want = onets.forward('net2x', sd, x16.float().numpy()).numpy()                # same fp16-quantised input
    assert np.abs(y.float().cpu().numpy() - want).max() <= TOL + HALF_OUT


def test_sedn_fused_block_tail_shapes(dev):
    """SEDN's fused block tail (per-plane effective weights, gate from shifted-window sums of the block input) on ragged and
    tiny tiles and on more planes than one tile has; the unfused form (MOE_SEDN_FUSE=0 is an environment switch, so the split
    precision mode is used here) must agree with the oracle as well."""
    sd = gd.state_dict_for('l25', load_state_dict_file)
    mf = module_for('l25', 'fp16')
    for (bn, h, w) in ((3, 8, 16), (3, 24, 56), (5, 88, 40), (12, 16, 64)):
        x = gd.natural_image(13, (bn, h, w))[:, None]
        want = onets.forward('sedn', sd, x).numpy()
        got = mf(torch.from_numpy(x).to(dev))[-1].cpu().numpy()
        assert np.abs(got - want).max() <= TOL, (bn, h, w, float(np.abs(got - want).max()))
    # the gate's sums two ways: totals from rblock.2's epilogue + the border visited by sedn_fmean (default), and the full pass of sedn_xsum (pool_fuse = 0): both forms
    # within the tolerance of the oracle (they differ from each other at the level of this mode's own fp16 rounding, 4.5e-4 here: another gate bit, another fp16 W_eff)
    x = gd.natural_image(17, (3, 88, 72))[:, None]
    xd = torch.from_numpy(x).to(dev)
    want = onets.forward('sedn', sd, x).numpy()
    try:
        y0 = mf.set_option('pool_fuse', 0)(xd)[-1].cpu().numpy()
    finally:
        mf.set_option('pool_fuse', 1)
    y1 = mf(xd)[-1].cpu().numpy()
    assert np.abs(y0 - want).max() <= TOL and np.abs(y1 - want).max() <= TOL, (float(np.abs(y0 - want).max()), float(np.abs(y1 - want).max()), float(np.abs(y0 - y1).max()))
    mx = module_for('l25', 'fp16x3')
    x = gd.natural_image(13, (3, 24, 56))[:, None]
    assert np.abs(mx(torch.from_numpy(x).to(dev))[-1].cpu().numpy() - onets.forward('sedn', sd, x).numpy()).max() <= 2e-5


def test_config5_512px_tiles(dev):
    """BASELINE config 5 in miniature (8K -> 32K with 512-px overlapped tiles): a 1100x1100 RGB image, a4, crop_sr = 512
    -> 3x3 = 9 tiles (four full 512x512 ones = 2048x2048 outputs per plane, ragged last row / column).  The whole
    device doCrop runs; one full tile and the ragged corner tile are compared with the oracle, and the stitched 4400x4400 canvas
    with the oracle's closed-form fold of the engine's own tile results."""
    import ctypes
    from moephoto_amd import _lib, imageProcess as ip
    opt = _opt_sr('a', 4, 512)
    x = gd.natural_image(55, (3, 1100, 1100))
    xd = torch.from_numpy(x).to(dev)
    plan = ip._plan_for(opt, xd.shape)
    assert plan.n_tiles == 9 and plan.tiles[0][:4] == (0, 512, 0, 512)
    pool = torch.zeros(plan.pool_elems(3), dtype=torch.float32, device=dev)
    out = torch.empty((3, plan.outH, plan.outW), dtype=torch.float32, device=dev)
    sC, sH, sW = xd.stride()
    _lib.check(_lib.lib().moe_run_plan_ex(opt.modelCached._h, plan._h, xd.data_ptr(), _lib.F32, sC, sH, sW, out.data_ptr(), _lib.F32, 0,
                                          ctypes.c_void_p(pool.data_ptr()), 0, 1, 1, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(out, ip.doCrop(opt, xd))
    off = plan.tile_offsets(3)
    sd = gd.state_dict_for('a4', load_state_dict_file)
    for k in (4, 8):           # the interior 512x512 tile and the ragged bottom-right corner
        top, bottom, left, right = plan.tiles[k][:4]
        want = onets.forward('net4x', sd, np.ascontiguousarray(x[:, None, top:bottom, left:right])).numpy()[:, 0]
        got = pool[off[k]:off[k] + want.size].reshape(want.shape).cpu().numpy()
        assert np.abs(got - want).max() <= TOL, (k, float(np.abs(got - want).max()))
    pl = oplanner.prepare((3, 1100, 1100), 1 << 40, 1e-3, 5, 4, 8, 512)
    hp = pool.cpu().numpy()
    tiles = [hp[off[k]:off[k] + 3 * (t[1] - t[0]) * (t[3] - t[2]) * 16].reshape(3, (t[1] - t[0]) * 4, (t[3] - t[2]) * 4) for k, t in enumerate(pl.tiles)]
    assert np.abs(out.cpu().numpy() - ostitch.fold_stitch(tiles, pl, 4)).max() <= 1e-6


STITCH_ONLY = [os.path.basename(p)[:-4] for p in sorted(glob.glob(os.path.join(G, 'stitch_only', '*.npz')))]


@pytest.mark.parametrize('name', STITCH_ONLY)
def test_stitch_kernel_golden(name, dev):
    """moe_stitch alone: seeded tile results in, the reference's stitched canvas out."""
    import ctypes
    from moephoto_amd import _lib
    from moephoto_amd.imageProcess import TilePlan
    z = np.load(os.path.join(G, 'stitch_only', name + '.npz'))
    shape = tuple(int(v) for v in z['shape'])
    sc = int(z['sc'])
    pl = TilePlan(shape, 1 << 40, 1e-3, int(z['pad']), sc, int(z['align']), int(z['crop']))
    C = shape[0]
    pool = np.empty(pl.pool_elems(C), np.float32)
    off = pl.tile_offsets(C)
    for k, t in enumerate(pl.tiles):
        r = np.random.default_rng(9000 + k).random((C, 1, (t[1] - t[0]) * sc, (t[3] - t[2]) * sc), dtype=np.float32)
        pool[off[k]:off[k] + r.size] = r.reshape(-1)
    pool_d = torch.from_numpy(pool).to(dev)
    out = torch.empty((C, pl.outH, pl.outW), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().moe_stitch(pl._h, 0, pool_d.data_ptr(), None, C, out.data_ptr(), _lib.F32, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert np.abs(out.cpu().numpy() - z['y']).max() <= 1e-6


def _opt_sr(model, scale, crop, ensemble=0, precision='auto', fp16_io=False):
    from moephoto_amd import imageProcess as ip, runSR
    from moephoto_amd.config import config
    config.modelRoot, config.crop_sr, config.fp16, config.deviceId = gd.ZOO, crop, fp16_io, 0
    key = model + str(scale)
    ip.modelCache.pop('SR' + key, None)
    if gd.MODELS[key][1] is None:      # a3 / a4: synthetic weights, written in the zoo's own format
        from moephoto_amd.weights import save_state_dict_file
        path = os.path.join('/tmp', 'moe_synth_{}.pth'.format(key))
        save_state_dict_file(gd.synth_state_dict(key, load_state_dict_file), path)
        runSR.mode_switch[key] = (path, runSR.mode_switch[key][1])
    opt = runSR.getOpt({'op': 'SR', 'model': model, 'scale': scale, 'ensemble': ensemble})
    opt.modelCached.set_precision(precision)
    return opt


STITCHED = [('a2_natural', 'a', 2, TOL), ('a2_noise', 'a', 2, TOL), ('a4_natural', 'a', 4, TOL),
            ('lite2_natural', 'lite', 2, TOL), ('a2_onetile_pad', 'a', 2, TOL)]


@pytest.mark.parametrize('name,model,scale,tol', STITCHED)
def test_docrop_vs_reference_golden(name, model, scale, tol, dev):
    """The whole device-resident doCrop (plugin table -> zoo file -> tile gather -> net -> stitch) on the
    reference's multi-tile goldens."""
    from moephoto_amd import runSR
    z = np.load(os.path.join(G, 'stitched', name + '.npz'))
    shape = tuple(int(v) for v in z['shape'])
    x = gd.noise_image(101, shape) if str(z['kind']) == 'noise' else gd.natural_image(101, shape)
    opt = _opt_sr(model, scale, int(z['crop']))
    y = runSR.sr(opt)(torch.from_numpy(x).to(dev))
    assert tuple(y.shape) == z['y'].shape
    assert np.abs(y.float().cpu().numpy() - z['y']).max() <= tol
    # and with split operands the north-star bar holds on every input, with two orders of magnitude to spare
    opt = _opt_sr(model, scale, int(z['crop']), precision='fp16x3')
    y = runSR.sr(opt)(torch.from_numpy(x).to(dev))
    assert np.abs(y.float().cpu().numpy() - z['y']).max() <= 2e-5


def test_ensemble_golden(dev):
    from moephoto_amd import runSR
    z = np.load(os.path.join(G, 'stitched', 'a2_ens3.npz'))
    x = gd.natural_image(101, (3, 60, 72))
    opt = _opt_sr('a', 2, 48, ensemble=3)
    y = runSR.sr(opt)(torch.from_numpy(x).to(dev))
    assert np.abs(y.float().cpu().numpy() - z['y']).max() <= TOL
    z = np.load(os.path.join(G, 'stitched', 'a2_ens7.npz'))
    x = gd.noise_image(101, (3, 52, 60))
    opt = _opt_sr('a', 2, 48, ensemble=7)          # eight passes over white noise, default arithmetic
    y = runSR.sr(opt)(torch.from_numpy(x).to(dev))
    assert np.abs(y.float().cpu().numpy() - z['y']).max() <= TOL


def test_dn_rgbfilter_golden(dev):
    from moephoto_amd import imageProcess as ip, runDN
    from moephoto_amd.config import config
    config.modelRoot, config.crop_dn, config.crop_dns, config.fp16 = gd.ZOO, 48, 48, False
    ip.modelCache.clear()
    z = np.load(os.path.join(G, 'stitched', 'dn5_rgba_s06.npz'))
    x = gd.natural_image(101, (4, 64, 80))
    opt = runDN.getOpt({'op': 'DN', 'model': 'lite5', 'strength': 0.6})
    y = ip.RGBFilter(opt)(torch.from_numpy(x).to(dev))
    assert tuple(y.shape) == (4, 64, 80)
    assert np.abs(y.float().cpu().numpy() - z['y']).max() <= TOL
    z = np.load(os.path.join(G, 'stitched', 'dn10_noise.npz'))
    opt = runDN.getOpt({'op': 'DN', 'model': 'lite10'})
    y = ip.RGBFilter(opt)(torch.from_numpy(gd.noise_image(101, (3, 100, 140))).to(dev))
    assert np.abs(y.float().cpu().numpy() - z['y']).max() <= TOL     # white noise through NetDN in the default ('mixed') arithmetic
    # SEDN (l25, synthetic weights written in the zoo format)
    from moephoto_amd.weights import save_state_dict_file
    path = '/tmp/moe_synth_l25.pth'
    save_state_dict_file(gd.synth_state_dict('l25', load_state_dict_file), path)
    runDN.mode_switch['25'] = (path,) + tuple(runDN.mode_switch['25'][1:])
    z = np.load(os.path.join(G, 'stitched', 'l25_natural.npz'))
    opt = runDN.getOpt({'op': 'DN', 'model': '25'})
    y = ip.RGBFilter(opt)(torch.from_numpy(gd.natural_image(101, (3, 60, 72))).to(dev))
    assert np.abs(y.float().cpu().numpy() - z['y']).max() <= TOL


def test_e2e_uint8_config1(dev):
    """Config 1: 256x256 RGB uint8 -> toTorch -> a2 x2 -> toFloat -> toOutput -> uint8, vs the reference's bytes."""
    from moephoto_amd import imageProcess as ip, runSR
    z = np.load(os.path.join(G, 'e2e', 'a2_256_natural.npz'))
    img = gd.to_u8(gd.natural_image(7, (3, 256, 256)))
    opt = _opt_sr('a', 2, 0)
    x = ip.toTorch(8, torch.float32, dev)(img)
    assert np.array_equal(x.cpu().numpy(), oio.to_float_image(img))              # the /255 edge is bit exact
    y = runSR.sr(opt)(x)
    out = ip.toOutput(8)(ip.toFloat(y))
    assert out.dtype == np.uint8 and out.shape == (512, 512, 3)
    d = np.abs(out.astype(np.int32) - z['out'].astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 0.1                                  # 1e-3 * 256 < 1 level
    assert np.array_equal(out, oio.to_output(oio.to_hwc(y.float().cpu().numpy())))  # the quantiser itself is exact
    v = torch.tensor([[[0.998, 0.5, -0.2, 1.7, 0.00390625, 0.0039]]], device=dev)
    assert ip.toOutput(8)(v).reshape(-1).tolist() == [255, 128, 0, 255, 1, 0]


def test_step_chain_dn_then_sr_config3(dev, tmp_path):
    """BASELINE config 3 in miniature: denoise (dn_lite5, pad 7) then x2 SR (a2, pad 5) as one device-resident chain built by
    procedure.genProcess from a MoePhoto step list, uint8 PNG file in -> uint8 out; against the oracle chain."""
    from PIL import Image
    from moephoto_amd import imageProcess as ip, procedure
    from moephoto_amd.config import config
    config.modelRoot, config.crop_sr, config.crop_dn, config.fp16, config.deviceId = gd.ZOO, 64, 64, False, 0
    ip.modelCache.clear()
    img = gd.to_u8(gd.natural_image(33, (3, 120, 150)))
    src = tmp_path / 'in.png'
    Image.fromarray(img).save(src)
    process, nodes = procedure.genProcess([{'op': 'file'}, {'op': 'DN', 'model': 'lite5', 'strength': '0.8'},
                                           {'op': 'SR', 'model': 'a', 'scale': '2', 'ensemble': 0}])
    assert [n['op'] for n in nodes] == ['DN', 'SR']
    out = process(str(src))
    assert out.dtype == np.uint8 and out.shape == (240, 300, 3)
    x = oio.to_float_image(img)
    sd_dn, sd_sr = gd.state_dict_for('dn_lite5', load_state_dict_file), gd.state_dict_for('a2', load_state_dict_file)
    pl = oplanner.prepare((3, 120, 150), 1 << 40, 1e-3, 7, 1, 8, 64)
    d = ostitch.do_crop(x, pl, 1, onets.model_fn('netdn', sd_dn))
    d = np.float32(0.8) * d + np.float32(1 - 0.8) * x
    pl = oplanner.prepare((3, 120, 150), 1 << 40, 1e-3, 5, 2, 8, 64)
    y = ostitch.do_crop(d, pl, 2, onets.model_fn('net2x', sd_sr))
    want = oio.to_output(oio.to_hwc(y))
    diff = np.abs(out.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= 1 and (diff > 0).mean() < 0.1          # 1e-3 * 256 < 1 grey level
    with pytest.raises(NotImplementedError):
        procedure.genProcess([{'op': 'slomo', 'sf': 2}])


def test_video_frame_buffer_chain_16bit(dev):
    """The video path's contract (python/video.py:23,349-360; procedure.py:141-142): a raw bgr48le frame goes through
    toNumPy -> toTorch(16) -> SR -> toFloat -> toOutput(16) -> toBuffer and comes back as raw 16-bit samples."""
    from moephoto_amd import imageProcess as ip, procedure
    from moephoto_amd.config import config
    config.modelRoot, config.crop_sr, config.fp16, config.deviceId = gd.ZOO, 64, False, 0
    ip.modelCache.clear()
    h, w = 72, 88
    img16 = (gd.natural_image(21, (3, h, w)).transpose(1, 2, 0) * 65535.0).astype(np.uint16)
    process, nodes = procedure.genProcess([{'op': 'buffer', 'bitDepth': 16}, {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}], bitDepth=16)
    assert [n['op'] for n in nodes] == ['SR']
    out = []
    assert procedure.runFrames(process, __import__('io').BytesIO(img16.tobytes() * 2).read, out.append, w, h, bitDepth=16) == 2
    assert out[0] == out[1] and len(out[0]) == 2 * h * 2 * w * 3 * 2
    got = np.frombuffer(out[0], np.uint16).reshape(2 * h, 2 * w, 3)
    x = oio.to_float_image(img16, 16)
    pl = oplanner.prepare((3, h, w), 1 << 40, 1e-3, 5, 2, 8, 64)
    y = ostitch.do_crop(x, pl, 2, onets.model_fn('net2x', gd.state_dict_for('a2', load_state_dict_file)))
    want = oio.to_output(oio.to_hwc(y), 16).astype(np.int64)
    diff = np.abs(got.astype(np.int64) - want)
    assert diff.max() <= TOL * 65536 + 1, diff.max()
    assert process((b'', h, w)) == []


def test_dropin_protocol_reference_loop(dev):
    """The reference's own doCrop loop (imageProcess.py:157-172) restated here with torch ops, calling the
    engine-backed module exactly like Option.__call__ does: per tile, on a slice view, list result."""
    from moephoto_amd.imageProcess import Option, initModel
    from moephoto_amd.models import Net2x
    from moephoto_amd.config import config
    config.fp16, config.deviceId = False, 0
    sd = gd.state_dict_for('a2', load_state_dict_file)
    opt = Option()
    opt.modelDef = Net2x
    opt.modelCached = initModel(opt, {k: torch.from_numpy(v) for k, v in sd.items()})
    z = np.load(os.path.join(G, 'stitched', 'a2_natural.npz'))
    x = torch.from_numpy(gd.natural_image(101, (3, 100, 140))).to(dev)
    pl = oplanner.prepare((3, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    ramp = torch.from_numpy(oplanner.blend_ramp(pl.pad_sc)).to(dev)
    out = torch.full((3, 200, 280), float('nan'), device=dev)
    xu = x.unsqueeze(1)

    def blend(r, ex, lt, pad, dim, b):
        l = r.shape[dim]
        lt = l + lt if lt < 0 else lt
        if lt < 1:
            return r, ex
        st = lt - pad
        rb, rc = r.narrow(dim, st, pad), r.narrow(dim, lt, l - lt)
        eb = ex.narrow(dim, st, pad)
        return torch.cat([eb + b * (rb - eb), rc], dim), ex.narrow(dim, st, l - st)
    for (top, bottom, left, right, tt, lt, bsc, rsc) in pl.tiles:
        s = xu[..., top:bottom, left:right]
        r = opt(s).squeeze(1)
        t = out[..., top * 2:bsc, left * 2:rsc]
        q, t2 = blend(r, t, tt, pl.pad_sc, -2, ramp.view(-1, 1))
        q, _ = blend(q, t2, lt, pl.pad_sc, -1, ramp.view(1, -1))
        hh, ww = q.shape[-2:]
        out[..., bsc - hh:bsc, rsc - ww:rsc] = q
    assert np.abs(out.cpu().numpy() - z['y']).max() <= TOL


def test_blend_tile_kernel_equals_the_reference_blend_expression(dev):
    """moe_blend_tile (imageProcess.blendTile): the two blend() calls + the slice-assign of the reference's loop body (python/imageProcess.py:120-131,167-170)
    as one kernel, for a maintainer who keeps that loop.  Held against the reference's own expression `bx + blend * (b - bx)` evaluated by
    torch in the canvas dtype, BIT FOR BIT, over every tile of plans with ragged last tiles, a reflect-padded single-tile axis (unpad), scale 2 / 3 / 4 windows that are
    and are not 4-element aligned, in fp16 (the reference's GPU path: ramp and canvas in half) and fp32; and end to end through the real net against the golden."""
    from moephoto_amd import imageProcess as ip

    def blend(r, ex, lt, pad, dim, b):
        l = r.shape[dim]
        lt = l + lt if lt < 0 else lt
        if lt < 1:
            return r, ex
        st = lt - pad
        rb, rc = r.narrow(dim, st, pad), r.narrow(dim, lt, l - lt)
        eb = ex.narrow(dim, st, pad)
        return torch.cat([eb + b * (rb - eb), rc], dim), ex.narrow(dim, st, l - st)
    rng = np.random.default_rng(11)
    for (shape, crop, pad, sc) in (((3, 100, 140), 48, 5, 2), ((2, 37, 150), 64, 5, 4), ((4, 90, 75), 40, 9, 3), ((3, 130, 61), 56, 7, 1)):
        pl = oplanner.prepare(shape, 1 << 40, 1e-3, pad, sc, 8, crop)
        outh, outw = pl.out_shape[-2:]
        for dt in (torch.float16, torch.float32):
            ramp = ((torch.arange(pl.pad_sc, dtype=dt, device=dev) / pl.pad_sc - .5) * 9).sigmoid().view(1, -1)      # prepare(), python/imageProcess.py:109
            want = torch.from_numpy(rng.random((shape[0], outh, outw), dtype=np.float32)).to(dev).to(dt)            # (new_empty in the reference: stale values the bands read)
            got = want.clone()
            for (top, bottom, left, right, tt, lt, bsc, rsc) in pl.tiles:
                r = torch.from_numpy(rng.standard_normal((shape[0], (bottom - top) * sc, (right - left) * sc)).astype(np.float32)).to(dev).to(dt)
                t = want[..., top * sc:bsc, left * sc:rsc]
                q, t2 = blend(r[..., :outh, :outw], t, tt, pl.pad_sc, -2, ramp.t())
                q, _ = blend(q, t2, lt, pl.pad_sc, -1, ramp)
                hh, ww = q.shape[-2:]
                want[..., bsc - hh:bsc, rsc - ww:rsc] = q
                # the forms the reference's loop hands over: (C, h, w) into (C, H, W); the net's own (C, 1, h, w) result; tmp_image as (1, C, H, W) (opt.oShape) -- ADVICE r05:
                # singleton axes are dropped by the wrapper, the kernel always sees (plane, row) strides
                form = (top // 8 + left // 8 + len(pl.tiles)) % 3
                ip.blendTile(r.unsqueeze(1) if form == 1 else r, got.unsqueeze(0) if form == 2 else got, (top, bottom, left, right, tt, lt, bsc, rsc), sc, pl.pad_sc, ramp)
            assert torch.equal(got, want), (shape, dt, float((got.float() - want.float()).abs().max()))
    # the loop of test_dropin_protocol_reference_loop with the fused kernel in place of the two blends
    from moephoto_amd.imageProcess import Option, initModel
    from moephoto_amd.models import Net2x
    from moephoto_amd.config import config
    config.fp16, config.deviceId = False, 0
    opt = Option()
    opt.modelDef = Net2x
    opt.modelCached = initModel(opt, {k: torch.from_numpy(v) for k, v in gd.state_dict_for('a2', load_state_dict_file).items()})
    z = np.load(os.path.join(G, 'stitched', 'a2_natural.npz'))
    xu = torch.from_numpy(gd.natural_image(101, (3, 100, 140))).to(dev).unsqueeze(1)
    pl = oplanner.prepare((3, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    ramp = torch.from_numpy(oplanner.blend_ramp(pl.pad_sc)).to(dev)
    out = torch.full((3, 200, 280), float('nan'), device=dev)
    for tile in pl.tiles:
        ip.blendTile(opt(xu[..., tile[0]:tile[1], tile[2]:tile[3]]), out, tile, 2, pl.pad_sc, ramp)
    assert np.abs(out.cpu().numpy() - z['y']).max() <= TOL


def test_run_plan_frames_owner_sharding(dev):
    """moe_run_plan_frames (the multi-GPU step of dist.run_frames): three frames in one call, tiles of different frames share
    launches.  With one owner, and with the work split over three owners (each computing (f * n_tiles + k) % 3 == i), every
    frame's pool and stitched result equal the frame-by-frame doCrop, bit for bit."""
    import ctypes
    from moephoto_amd import _lib, imageProcess as ip
    opt = _opt_sr('a', 2, 64)
    frames = torch.stack([torch.from_numpy(gd.natural_image(70 + f, (3, 150, 200))) for f in range(3)]).to(dev)
    plan = ip._plan_for(opt, frames[0].shape)
    L, model = _lib.lib(), opt.modelCached
    stream = torch.cuda.current_stream().cuda_stream
    pe = plan.pool_elems(3)
    sC, sH, sW = frames[0].stride()

    def run(owners):
        pools = torch.zeros((3, pe), dtype=torch.float32, device=dev)
        for i in range(owners):
            _lib.check(L.moe_run_plan_frames(model._h, plan._h, frames.data_ptr(), _lib.F32, frames.stride(0), sC, sH, sW, 3,
                                             ctypes.c_void_p(pools.data_ptr()), pe, i, owners, 3, stream))
        outs = []
        for f in range(3):
            y = torch.empty((3, plan.outH, plan.outW), dtype=torch.float32, device=dev)
            _lib.check(L.moe_stitch(plan._h, 0, pools[f].data_ptr(), None, 3, y.data_ptr(), _lib.F32, stream))
            outs.append(y)
        torch.cuda.synchronize()
        return pools, outs
    p1, o1 = run(1)
    p3, o3 = run(3)
    assert torch.equal(p1, p3)
    for f in range(3):
        want = ip.doCrop(opt, frames[f])
        assert torch.equal(o1[f], want) and torch.equal(o3[f], want), f
    with pytest.raises(RuntimeError):
        _lib.check(L.moe_run_plan_frames(model._h, plan._h, frames.data_ptr(), _lib.F32, frames.stride(0), sC, sH, sW, 3,
                                         ctypes.c_void_p(p1.data_ptr()), pe - 8, 0, 1, 3, stream))      # pool stride too small


_runner_case = {}


def _plan_runner_case(dev):
    """The shape of test_run_plan_frames_owner_sharding (a2, 3 x 150 x 200 fp32, cropsize 64: twelve tiles in four groups, ragged edge tiles included), computed
    once for the runner tests below: the image, its plan, doCrop's canvas, the tile pool in the plan's own layout and the tiles' sizes in that pool."""
    import ctypes
    from moephoto_amd import _lib, imageProcess as ip
    if not _runner_case:
        opt = _opt_sr('a', 2, 64)
        x = torch.from_numpy(gd.natural_image(70, (3, 150, 200))).to(dev)
        plan = ip._plan_for(opt, x.shape)
        assert plan.padImage(x).shape == x.shape and plan.n_tiles == 12
        want = ip.doCrop(opt, x)
        pool = torch.zeros(plan.pool_elems(3), dtype=torch.float32, device=dev)
        sC, sH, sW = x.stride()
        _lib.check(_lib.lib().moe_run_plan_ex(opt.modelCached._h, plan._h, x.data_ptr(), _lib.F32, sC, sH, sW, None, _lib.F32, 0,
                                              ctypes.c_void_p(pool.data_ptr()), 0, 1, 0, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        sizes = [3 * (t[1] - t[0]) * (t[3] - t[2]) * 4 for t in plan.tiles]
        _runner_case.update(opt=opt, x=x, plan=plan, want=want, pool=pool, sizes=sizes)
    c = _runner_case
    return c['opt'], c['x'], c['plan'], c['want'], c['pool'], c['sizes']


def _shuffled_layout(sizes, seed):
    """Pool offsets of the tiles packed in a shuffled order: (offsets by tile, the order)"""
    order = [int(k) for k in np.random.RandomState(seed).permutation(len(sizes))]
    offs, at = [0] * len(sizes), 0
    for k in order:
        offs[k] = at
        at += sizes[k]
    return offs, tuple(order)


def test_run_plan_ex_into_a_pool_equals_run_plan_tiles_with_one_frame(dev):
    """moe_run_plan_ex into a caller's pool without the stitch is moe_run_plan_tiles with one frame and the plan's own offsets as the destination table; its
    shard i of n is that table with the other tiles' entries at -1.  The pools are bit-equal."""
    import ctypes
    from moephoto_amd import _lib
    opt, x, plan, _, pool_ref, sizes = _plan_runner_case(dev)
    L, model = _lib.lib(), opt.modelCached
    stream = torch.cuda.current_stream().cuda_stream
    sC, sH, sW = x.stride()
    off = plan.tile_offsets(3)
    for si, scnt in ((0, 1), (1, 3)):
        a = torch.zeros_like(pool_ref)
        b = torch.zeros_like(pool_ref)
        _lib.check(L.moe_run_plan_ex(model._h, plan._h, x.data_ptr(), _lib.F32, sC, sH, sW, None, _lib.F32, 0, ctypes.c_void_p(a.data_ptr()), si, scnt, 0, stream))
        dst = (ctypes.c_int64 * plan.n_tiles)(*[o if k % scnt == si else -1 for k, o in enumerate(off)])
        _lib.check(L.moe_run_plan_tiles(model._h, plan._h, x.data_ptr(), _lib.F32, 0, sC, sH, sW, 1, ctypes.c_void_p(b.data_ptr()), dst, 0, stream))
        torch.cuda.synchronize()
        assert torch.equal(a, b), (si, scnt)
        mine = torch.zeros_like(pool_ref, dtype=torch.bool)
        for k, o in enumerate(off):
            if k % scnt == si:
                mine[o:o + sizes[k]] = True
        assert torch.equal(a[mine], pool_ref[mine]) and not a[~mine].any(), (si, scnt)


def test_run_plan_with_more_input_layouts_than_the_plan_caches(dev):
    """One plan, 18 distinct input layouts (row pitches: the image as a slice of wider tensors) -- more than the plan keeps device tables for -- with a
    moe_stitch between the runs, then the first layout again: every canvas is bit-equal to doCrop of the contiguous image."""
    from moephoto_amd import _lib
    opt, x, plan, want, pool_ref, _ = _plan_runner_case(dev)
    L, model = _lib.lib(), opt.modelCached
    stream = torch.cuda.current_stream().cuda_stream
    views = []
    for i in range(18):
        wide = torch.full((3, 150, 208 + 8 * i), float('nan'), dtype=torch.float32, device=dev)
        wide[:, :, 3:203] = x
        views.append(wide[:, :, 3:203])
    assert len({v.stride() for v in views}) == 18
    for v in views + [views[0]]:
        y = torch.empty_like(want)
        sC, sH, sW = v.stride()
        _lib.check(L.moe_run_plan(model._h, plan._h, v.data_ptr(), _lib.F32, sC, sH, sW, y.data_ptr(), _lib.F32, 0, stream))
        y2 = torch.empty_like(want)
        _lib.check(L.moe_stitch(plan._h, 0, pool_ref.data_ptr(), None, 3, y2.data_ptr(), _lib.F32, stream))
        torch.cuda.synchronize()
        assert torch.equal(y, want) and torch.equal(y2, want), v.stride()


def test_stitch_of_a_permuted_pool_host_table_device_table_and_default_layout(dev):
    """The tiles at shuffled offsets in the pool: moe_stitch with the offsets passed from the host, moe_stitch_dev with the same table on the device and
    moe_stitch of the plan's own layout give one canvas, bit for bit -- for 18 distinct permutations on one plan (more than the uploaded tables it keeps)."""
    import ctypes
    from moephoto_amd import _lib
    opt, _, plan, want, pool_ref, sizes = _plan_runner_case(dev)
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    off = plan.tile_offsets(3)
    canvas0 = torch.empty_like(want)
    _lib.check(L.moe_stitch(plan._h, 0, pool_ref.data_ptr(), None, 3, canvas0.data_ptr(), _lib.F32, stream))
    seen = set()
    for seed in range(18):
        offs, order = _shuffled_layout(sizes, 100 + seed)
        seen.add(order)
        pool = torch.full_like(pool_ref, float('nan'))
        for k in range(plan.n_tiles):
            pool[offs[k]:offs[k] + sizes[k]] = pool_ref[off[k]:off[k] + sizes[k]]
        host = (ctypes.c_int64 * plan.n_tiles)(*offs)
        tab = torch.tensor(offs, dtype=torch.int64, device=dev)
        ya, yb = torch.empty_like(want), torch.empty_like(want)
        _lib.check(L.moe_stitch(plan._h, 0, pool.data_ptr(), ctypes.c_void_p(ctypes.addressof(host)), 3, ya.data_ptr(), _lib.F32, stream))
        _lib.check(L.moe_stitch_dev(plan._h, 0, pool.data_ptr(), ctypes.c_void_p(tab.data_ptr()), 3, yb.data_ptr(), _lib.F32, stream))
        torch.cuda.synchronize()
        assert torch.equal(ya, canvas0) and torch.equal(yb, canvas0), seed
    assert len(seen) == 18 and torch.equal(canvas0, want)


def test_run_plan_tiles_with_more_destination_tables_than_the_plan_caches(dev):
    """moe_run_plan_tiles with 10 distinct destination tables on one plan (each a shuffled packing of the pool), each stitched through moe_stitch_dev with its
    table: every canvas is bit-equal to doCrop."""
    import ctypes
    from moephoto_amd import _lib
    opt, x, plan, want, pool_ref, sizes = _plan_runner_case(dev)
    L, model = _lib.lib(), opt.modelCached
    stream = torch.cuda.current_stream().cuda_stream
    sC, sH, sW = x.stride()
    seen = set()
    for seed in range(10):
        offs, order = _shuffled_layout(sizes, 200 + seed)
        seen.add(order)
        pool = torch.full_like(pool_ref, float('nan'))
        dst = (ctypes.c_int64 * plan.n_tiles)(*offs)
        _lib.check(L.moe_run_plan_tiles(model._h, plan._h, x.data_ptr(), _lib.F32, 0, sC, sH, sW, 1, ctypes.c_void_p(pool.data_ptr()), dst, 0, stream))
        tab = torch.tensor(offs, dtype=torch.int64, device=dev)
        y = torch.empty_like(want)
        _lib.check(L.moe_stitch_dev(plan._h, 0, pool.data_ptr(), ctypes.c_void_p(tab.data_ptr()), 3, y.data_ptr(), _lib.F32, stream))
        torch.cuda.synchronize()
        assert torch.equal(y, want), seed
    assert len(seen) == 10


def test_full_size_properties_config2(dev):
    """BASELINE config 2 at full size (1080p -> 7680x4320, a4-synth, 256-px tiles, 40 tiles), checked through
    properties that do not need a full CPU run:
      * two full-size tiles (an interior 256x256 one and the ragged 88x192 corner) against the oracle,
      * the stitched canvas equals the oracle's closed-form fold of the engine's OWN tile results,
      * batching invariance: 1 tile per launch == 4 tiles per launch, bit for bit,
      * sharding invariance: tiles computed as 3 shards land in the same pool, bit for bit."""
    import ctypes
    from moephoto_amd import _lib, imageProcess as ip
    from moephoto_amd.config import config
    opt = _opt_sr('a', 4, 256)
    x = gd.natural_image(0, (3, 1080, 1920))
    xd = torch.from_numpy(x).to(dev)
    plan = ip._plan_for(opt, xd.shape)
    assert plan.n_tiles == 40
    L, model = _lib.lib(), opt.modelCached
    stream = torch.cuda.current_stream().cuda_stream
    sC, sH, sW = xd.stride()

    def run(per_batch, shards=1):
        pool = torch.zeros(plan.pool_elems(3), dtype=torch.float32, device=dev)
        out = torch.empty((3, plan.outH, plan.outW), dtype=torch.float32, device=dev)
        for si in range(shards):
            _lib.check(L.moe_run_plan_ex(model._h, plan._h, xd.data_ptr(), _lib.F32, sC, sH, sW, out.data_ptr(), _lib.F32, per_batch,
                                         ctypes.c_void_p(pool.data_ptr()), si, shards, 1 if si == shards - 1 else 0, stream))
        torch.cuda.synchronize()
        return pool, out
    pool4, out4 = run(4)
    pool1, out1 = run(1)
    assert torch.equal(pool1, pool4) and torch.equal(out1, out4)
    pool3, out3 = run(4, shards=3)
    assert torch.equal(pool3, pool4) and torch.equal(out3, out4)
    off = plan.tile_offsets(3)
    sd = gd.state_dict_for('a4', load_state_dict_file)
    for k in (9, 39):
        top, bottom, left, right = plan.tiles[k][:4]
        want = onets.forward('net4x', sd, np.ascontiguousarray(x[:, None, top:bottom, left:right])).numpy()[:, 0]
        got = pool4[off[k]:off[k] + want.size].reshape(want.shape).cpu().numpy()
        assert np.abs(got - want).max() <= TOL, k
    pl = oplanner.prepare((3, 1080, 1920), 1 << 40, 1e-3, 5, 4, 8, 256)
    hp = pool4.cpu().numpy()
    tiles = [hp[off[k]:off[k] + 3 * (t[1] - t[0]) * (t[3] - t[2]) * 16].reshape(3, (t[1] - t[0]) * 4, (t[3] - t[2]) * 4) for k, t in enumerate(pl.tiles)]
    want = ostitch.fold_stitch(tiles, pl, 4)
    assert np.abs(out4.cpu().numpy() - want).max() <= 1e-6


def test_step_chain_config3_l25_then_a2(dev, tmp_path):
    """BASELINE config 3 as written, at test size: [{'op':'DN','model':'25'}, {'op':'SR','model':'a','scale':2}] through
    procedure.genProcess on an image that needs a 2x2 tile grid in BOTH steps (SEDN l25 with pad 7, then Net2x a2 with pad 5),
    uint8 file in -> uint8 out, against the oracle chain (sequential doCrop of each step)."""
    from PIL import Image
    from moephoto_amd import imageProcess as ip, procedure, runDN
    from moephoto_amd.config import config
    from moephoto_amd.weights import save_state_dict_file
    config.modelRoot, config.crop_sr, config.crop_dn, config.crop_dns, config.fp16, config.deviceId = gd.ZOO, 64, 64, 64, False, 0
    ip.modelCache.clear()
    path = '/tmp/moe_synth_l25.pth'
    save_state_dict_file(gd.synth_state_dict('l25', load_state_dict_file), path)
    runDN.mode_switch['25'] = (path,) + tuple(runDN.mode_switch['25'][1:])
    img = gd.to_u8(gd.natural_image(34, (3, 96, 104)))
    src = tmp_path / 'in.png'
    Image.fromarray(img).save(src)
    process, nodes = procedure.genProcess([{'op': 'file'}, {'op': 'DN', 'model': '25'}, {'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}])
    assert [(n['op'], n['model']) for n in nodes] == [('DN', '25'), ('SR', 'a')]
    out = process(str(src))
    assert out.dtype == np.uint8 and out.shape == (192, 208, 3)
    x = oio.to_float_image(img)
    sd_dn, sd_sr = gd.state_dict_for('l25', load_state_dict_file), gd.state_dict_for('a2', load_state_dict_file)
    pl = oplanner.prepare((3, 96, 104), 1 << 40, 1e-3, 7, 1, 8, 64)
    assert len(pl.tiles) == 4
    d = ostitch.do_crop(x, pl, 1, onets.model_fn('sedn', sd_dn))
    pl = oplanner.prepare((3, 96, 104), 1 << 40, 1e-3, 5, 2, 8, 64)
    assert len(pl.tiles) == 4
    y = ostitch.do_crop(d, pl, 2, onets.model_fn('net2x', sd_sr))
    want = oio.to_output(oio.to_hwc(y))
    diff = np.abs(out.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= 1 and (diff > 0).mean() < 0.1          # 1e-3 * 256 < 1 grey level
    # and the float result of the chain itself, before quantisation
    dev_x = ip.toTorch(8, torch.float32, dev)(img)
    from moephoto_amd import runSR
    dd = ip.RGBFilter(runDN.getOpt({'op': 'DN', 'model': '25'}))(dev_x)
    assert np.abs(dd.cpu().numpy() - d).max() <= TOL                      # step 1 against the oracle's step 1
    yd = runSR.sr(runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}))(dd)
    # step 2 against the oracle's step 2 ON THE SAME INPUT (the engine's denoised image): each step is held to TOL; a2 amplifies
    # an input perturbation ~2.5x, so the end-to-end float difference may reach ~2.5 TOL (the uint8 result above is within one level)
    y2 = ostitch.do_crop(dd.cpu().numpy(), pl, 2, onets.model_fn('net2x', sd_sr))
    assert np.abs(yd.cpu().numpy() - y2).max() <= TOL
    assert np.abs(yd.cpu().numpy() - y).max() <= 3 * TOL


def test_config4_frames_over_8_owners(dev):
    """BASELINE config 4 at test size: two 1080p frames, a4, 256-px tiles (2 x 40 tiles), the (frame, tile) pairs dealt
    round-robin to 8 owners exactly as on 8 GPUs (each owner computes its tenth-ish with cross-frame batching through
    moe_run_plan_frames); pools and stitched frames must equal the frame-by-frame doCrop bit for bit."""
    import ctypes
    from moephoto_amd import _lib, imageProcess as ip
    opt = _opt_sr('a', 4, 256, fp16_io=True)
    frames = torch.stack([torch.from_numpy(gd.natural_image(80 + f, (3, 1080, 1920))) for f in range(2)]).to(dev).half()
    plan = ip._plan_for(opt, frames[0].shape)
    assert plan.n_tiles == 40
    L, model = _lib.lib(), opt.modelCached
    stream = torch.cuda.current_stream().cuda_stream
    pe = plan.pool_elems(3)
    sC, sH, sW = frames[0].stride()
    pools = torch.zeros((2, pe), dtype=torch.float32, device=dev)
    for i in range(8):
        _lib.check(L.moe_run_plan_frames(model._h, plan._h, frames.data_ptr(), _lib.F16, frames.stride(0), sC, sH, sW, 2,
                                         ctypes.c_void_p(pools.data_ptr()), pe, i, 8, 0, stream))
    for f in range(2):
        y = torch.empty((3, plan.outH, plan.outW), dtype=torch.float16, device=dev)
        _lib.check(L.moe_stitch(plan._h, 0, pools[f].data_ptr(), None, 3, y.data_ptr(), _lib.F16, stream))
        torch.cuda.synchronize()
        assert torch.equal(y, ip.doCrop(opt, frames[f])), f


@pytest.mark.parametrize('model,scale', [('a', 2), ('a', 3), ('a', 4)])
def test_auto_cropsize_whole_frame_tiles(model, scale, dev):
    """cropsize 'auto' on a 288-GB part plans a 1080p frame as ONE tile: three planes of 1080x1920 through every kernel
    (the fused tail's tap planes alone are 36 B per output pixel).  The frame must run -- batches are split so that no launch
    leaves the kernels' 32-bit addressing range -- and its top-left corner must match the oracle of that corner's receptive
    field (a whole-frame oracle run would take minutes)."""
    from moephoto_amd import imageProcess as ip
    opt = _opt_sr(model, scale, 0)
    x = gd.natural_image(60 + scale, (3, 1080, 1920))
    xd = torch.from_numpy(x).to(dev)
    plan = ip._plan_for(opt, xd.shape)
    assert plan.n_tiles == 1, plan.n_tiles
    y = ip.doCrop(opt, xd)
    assert tuple(y.shape) == (3, 1080 * scale, 1920 * scale)
    key = model + str(scale)
    sd = gd.state_dict_for(key, load_state_dict_file)
    # outputs within 96 px of the corner depend on inputs within 96 + ~25 px (19 conv layers, the last ones at higher resolution)
    want = onets.forward(gd.MODELS[key][0], sd, np.ascontiguousarray(x[:, None, :160, :160])).numpy()[:, 0, :96 * scale, :96 * scale]
    assert np.abs(y[:, :96 * scale, :96 * scale].cpu().numpy() - want).max() <= TOL
    want = onets.forward(gd.MODELS[key][0], sd, np.ascontiguousarray(x[:, None, -160:, -160:])).numpy()[:, 0, -96 * scale:, -96 * scale:]
    assert np.abs(y[:, -96 * scale:, -96 * scale:].cpu().numpy() - want).max() <= TOL


def test_large_batches_are_split(dev):
    """40 tiles (120 planes of 256x256) in ONE requested batch exceed the fast kernel's 32-bit addressing range for Net4x
    (576 B per pixel-plane): the engine runs them as several launch sets with results identical to 4-tile batches."""
    import ctypes
    from moephoto_amd import _lib, imageProcess as ip
    opt = _opt_sr('a', 4, 256)
    xd = torch.from_numpy(gd.natural_image(0, (3, 1080, 1920))).to(dev)
    plan = ip._plan_for(opt, xd.shape)
    sC, sH, sW = xd.stride()
    outs = []
    for per in (4, 40):
        out = torch.empty((3, plan.outH, plan.outW), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().moe_run_plan(opt.modelCached._h, plan._h, xd.data_ptr(), _lib.F32, sC, sH, sW, out.data_ptr(), _lib.F32, per,
                                           torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])


def test_exact_blocks_knob(dev):
    """'mixed' precision: more split-operand ARSBs can only tighten the result; every setting stays within TOL on white noise
    for Net4x (Net2x's default is 4 blocks, the full-frame sweep in test_gpu_fullsize.py holds it to 1e-3)."""
    z = np.load(os.path.join(G, 'nets', 'a4.npz'))
    h, w = [int(v) for v in z['hw']]
    x = torch.from_numpy(gd.noise_image(int(z['seed']), (3, 1, h, w))).to(dev)
    m = module_for('a4', 'mixed')
    errs = []
    for nb in (0, 1, 3, 6):
        m.set_exact_blocks(nb)
        errs.append(float(np.abs(m(x)[-1].cpu().numpy() - z['y_noise']).max()))
    m.set_exact_blocks(-1)
    assert max(errs) <= TOL and errs[-1] <= errs[0] + 1e-4, errs
    with pytest.raises(RuntimeError):
        m.set_exact_blocks(9)
    from moephoto_amd import models
    with pytest.raises(RuntimeError):                    # 'mixed' is defined for the ARSB nets only
        from moephoto_amd import _lib
        net = models.SEDN()
        net.load_state_dict({n: torch.from_numpy(v) for n, v in gd.state_dict_for('l25', load_state_dict_file).items()})
        _lib.check(_lib.lib().moe_net_finalize(net._h, 0, _lib.PREC_MIXED))


def test_rccl_path_world1(dev):
    """The collective path of dist.run_frames on the real RCCL backend (`nccl` on ROCm) with one rank: process group on the
    device, weight broadcast on device tensors, the all-to-all issued even though nothing crosses ranks
    (dist.FORCE_COLLECTIVE), stitch from the exchange buffer.  Result == single-process doCrop, bit for bit."""
    import socket
    import torch.distributed as dist
    from moephoto_amd import dist as mdist, imageProcess as ip
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1')
    dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    try:
        sd = {k: torch.from_numpy(v) for k, v in gd.state_dict_for('a2', load_state_dict_file).items()}
        got = mdist.broadcast_state_dict(sd, src=0, device=dev)
        assert list(got.keys()) == list(sd.keys()) and all(torch.equal(got[k], sd[k]) for k in sd)
        opt = _opt_sr('a', 2, 64, fp16_io=True)
        frames = [torch.from_numpy(gd.natural_image(90 + f, (3, 150, 200))).to(dev).half() for f in range(3)]
        mdist.FORCE_COLLECTIVE = True
        for rep in range(2):          # second call: cached layout, same buffer
            out = mdist.run_frames(opt, frames, out_dtype=torch.float16)
            torch.cuda.synchronize()
            assert sorted(out) == [0, 1, 2]
            for f, y in out.items():
                assert torch.equal(y, ip.doCrop(opt, frames[f])), (rep, f)
        # the grouped form with ASYNCHRONOUS all-to-alls on RCCL's stream (groups of one frame here), two exchange buffers
        out = mdist.run_frames_overlapped(opt, frames, out_dtype=torch.float16)
        torch.cuda.synchronize()
        assert sorted(out) == [0, 1, 2]
        for f, y in out.items():
            assert torch.equal(y, ip.doCrop(opt, frames[f])), f
        # ... and they really run BESIDE the next group's convolutions (RCCL refuses two ranks on one device -- test_dist_two_ranks_on_one_gpu_over_rccl
        # records the refusal -- so one rank is where this can be observed): with frames large enough that a group computes for milliseconds, the host sees every group's
        # exchange complete while an event behind the NEXT group's kernels is still pending
        big = [torch.from_numpy(gd.natural_image(95 + f, (3, 600, 800))).to(dev).half() for f in range(4)]
        probe = []
        out = mdist.run_frames_overlapped(opt, big, out_dtype=torch.float16, probe=probe)
        torch.cuda.synchronize()
        assert len(probe) == 3 and all(p['exchange_done_while_computing'] for p in probe), probe
        assert torch.equal(out[2], ip.doCrop(opt, big[2]))
    finally:
        mdist.FORCE_COLLECTIVE = False
        dist.destroy_process_group()


def test_fused_arsb_matches_two_launch_form(dev):
    """arsb32c.hip (32x32x16 MFMAs, waves in lock-step, vertical continuation: ten rows per patch, a workgroup walks a column of patches and keeps the last
    two m rows for the patch below; the earlier forms arsb_fused.hip / arsb32.hip were retired in round 4).
    The fused ARSB kernel (conv_1 -> PReLU -> conv_2 -> + x in one launch, weights in registers) against the two-launch form of
    the same arithmetic (option arsb_fuse = 0) and the oracle: ragged shapes (patches are 8 x 30 outputs), 48- and 64-channel nets,
    with and without the hi+lo stream."""
    cases = [('a2', (3, 8, 16)), ('a2', (3, 24, 40)), ('a2', (2, 40, 264)), ('a2', (3, 9, 35)), ('a2', (5, 88, 64)), ('a2', (2, 131, 61)), ('dn_lite5', (3, 16, 64)), ('dn_lite5', (3, 33, 31)), ('dn_lite5', (2, 57, 128))]
    touched = []
    try:
        for key, shape in cases:
            arch = gd.MODELS[key][0]
            sd = gd.state_dict_for(key, load_state_dict_file)
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(17, shape) if kind == 'natural' else gd.noise_image(17, shape))[:, None]
                want = onets.forward(arch, sd, x).numpy()
                xd = torch.from_numpy(x).to(dev)
                for prec, nb in (('fp16', -1), ('mixed', 0), ('mixed', -1)):
                    m = module_for(key, prec).set_exact_blocks(nb)
                    touched.append(m)
                    y0 = m.set_option('arsb_fuse', 0)(xd)[-1].cpu().numpy()
                    y1 = m.set_option('arsb_fuse', 1)(xd)[-1].cpu().numpy()
                    m.set_exact_blocks(-1)
                    # same operands, same rounding points; only the fp32 summation order inside a conv differs, which flips an fp16 rounding
                    # of conv_1's output now and then -- and, in 'fp16' mode, of the stream itself (one ulp of a value near 1 is 5e-4,
                    # amplified ~2x by the upsampler).  The trunk taps of the two forms agree to four digits (tools/diag_arsb.py).
                    # On natural images the two forms agree to 2.5e-4.  White noise drives a2 to +-1.9 and every flipped rounding is
                    # amplified, so there each form is held against the ORACLE with the bound of its arithmetic (fp16: the documented
                    # 1e-2 on noise; mixed with nb = 0: 2e-3; the default is asserted at TOL below) instead of against the other.
                    if kind == 'natural':
                        assert np.abs(y1 - y0).max() <= 2.5e-4, (key, shape, prec, nb, float(np.abs(y1 - y0).max()))
                    else:
                        for y in (y0, y1):
                            assert np.abs(y - want).max() <= (1e-2 if prec == 'fp16' else 2e-3), (key, shape, prec, nb, float(np.abs(y - want).max()))
                    if prec == 'mixed' and nb == -1:
                        assert np.abs(y1 - want).max() <= TOL, (key, shape, kind, float(np.abs(y1 - want).max()))
                    if arch == 'netdn':      # the 48-channel nets leave the all-zero fourth k-slice out: not a bit may change
                        y3 = m.set_exact_blocks(nb).set_option('k48', 0)(xd)[-1].cpu().numpy()
                        m.set_option('k48', 1).set_exact_blocks(-1)
                        assert np.array_equal(y3, y1), (key, shape, prec, nb, float(np.abs(y3 - y1).max()))
                    # few persistent workgroups: every workgroup walks several patches (v2 hands output row 3 of a patch over to the next
                    # patch's first row steps); a conv is a pure function of its patch, so the result must not change by a bit
                    if shape[1] * shape[2] >= 40 * 64:
                        y2 = m.set_exact_blocks(nb).set_option('max_groups', 16)(xd)[-1].cpu().numpy()
                        m.set_option('max_groups', 0).set_exact_blocks(-1)
                        assert np.array_equal(y2, y1), (key, shape, prec, nb, float(np.abs(y2 - y1).max()))
    finally:
        for m in touched:
            m.set_option('arsb_fuse', 1).set_option('max_groups', 0).set_option('k48', 1).set_exact_blocks(-1)


@pytest.mark.parametrize('key', ['a2', 'a4', 'dn_lite5'])
def test_exact_layers_with_fp8_corrections(key, dev):
    """Option x3_impl = q8 (conv64_q8.hip): the split-operand layers with their two correction products on fp8 operands -- the corrections carry 2^-11 of
    the result, so the output must stay inside the product's tolerance against the oracle and move by a small fraction of it against the fp16 form
    (tests/emu_precision.py corr8 predicts +-1e-4 on noise)."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    try:
        for shape in ((3, 24, 40), (2, 40, 264), (3, 9, 35), (2, 88, 64)):
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(23, shape) if kind == 'natural' else gd.noise_image(23, shape))[:, None]
                want = onets.forward(arch, sd, x).numpy()
                xd = torch.from_numpy(x).to(dev)
                y3 = m.set_option('x3_impl', 'x3')(xd)[-1].cpu().numpy()
                y8 = m.set_option('x3_impl', 'q8')(xd)[-1].cpu().numpy()
                assert np.isfinite(y8).all(), (key, shape, kind)
                assert np.abs(y8 - want).max() <= TOL, (key, shape, kind, float(np.abs(y8 - want).max()), float(np.abs(y3 - want).max()))
                assert np.abs(y8 - y3).max() <= 8e-4, (key, shape, kind, float(np.abs(y8 - y3).max()))      # (pointwise, noise; the error against the oracle moves by ~1e-4)
                y8b = m(xd)[-1].cpu().numpy()
                assert np.array_equal(y8, y8b), (key, shape, kind)      # (same launch twice: the conversions' half-register writes once raced)
        # activations beyond the fp8 range (1856 = 4 x 464): the conversions saturate, the corrections of those pixels lose their meaning (2^-11 of the value) and
        # nothing else happens -- in particular no NaN, which is what the conversion instruction produces when MODE.FP16_OVFL is off
        x = gd.noise_image(29, (3, 40, 72))[:, None] * 6000.0
        xd = torch.from_numpy(x).to(dev)
        y3 = m.set_option('x3_impl', 'x3')(xd)[-1].cpu().numpy()
        y8 = m.set_option('x3_impl', 'q8')(xd)[-1].cpu().numpy()
        assert np.isfinite(y3).all() and np.abs(y3).max() > 1856.0, (key, float(np.abs(y3).max()))
        assert np.isfinite(y8).all(), key
        assert np.abs(y8 - y3).max() <= 2e-3 * np.abs(y3).max(), (key, float(np.abs(y8 - y3).max()), float(np.abs(y3).max()))
    finally:
        m.set_option('x3_impl', 'auto')


@pytest.mark.parametrize('key,blocks', [('a2', -1), ('a4', -1), ('a3', -1), ('a2', 6), ('a4', 3)])
def test_fp8_low_part_chain(key, blocks, dev):
    """Option lo8 (default on): between the conv64_q8 layers of a net the low parts of the activations travel as the fp8 words the correction products
    read (64 instead of 128 bytes a pixel; the last conv_2 of the chain writes fp16 low parts for the fused ARSB kernels).  The convolutions see the same
    operands either way; the residual additions see ~15 instead of 22 bits of the stream: the outputs agree to a small fraction of the tolerance, both
    hold the tolerance against the oracle, ragged shapes included, and a launch repeated gives the same bits."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    try:
        m.set_exact_blocks(blocks)
        for shape in ((3, 24, 40), (2, 40, 264), (3, 9, 35), (1, 88, 64), (2, 33, 31)):
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(37, shape) if kind == 'natural' else gd.noise_image(37, shape))[:, None]
                want = onets.forward(arch, sd, x).numpy()
                xd = torch.from_numpy(x).to(dev)
                y16 = m.set_option('x3_impl', 'q8').set_option('lo8', 'off')(xd)[-1].cpu().numpy()
                y8 = m.set_option('lo8', 'on')(xd)[-1].cpu().numpy()
                y8b = m(xd)[-1].cpu().numpy()
                assert np.isfinite(y8).all(), (key, shape, kind)
                assert np.array_equal(y8, y8b), (key, shape, kind)
                assert np.abs(y8 - want).max() <= TOL, (key, shape, kind, float(np.abs(y8 - want).max()), float(np.abs(y16 - want).max()))
                assert 0 < np.abs(y8 - y16).max() <= 6e-4, (key, shape, kind, float(np.abs(y8 - y16).max()), float(np.abs(y8 - want).max()), float(np.abs(y16 - want).max()))      # (pointwise, noise: 3e-4 .. 4.3e-4, as tests/emu_precision.py lo8 predicts; the error against the oracle moves by < 1e-4 either way, fullsize sweep)
    finally:
        m.set_option('x3_impl', 'auto').set_option('lo8', 'on').set_exact_blocks(-1)


def test_fp8_corrections_default_by_family(dev):
    """x3_impl = auto: the SR nets AND (since round 6: the stem writes the fp8 words beside its fp16 low part) the DN nets run their exact layers through the fp8-correction
    kernels (bit-equal to the explicit setting 'q8', not to 'x3')."""
    for key, same_as in (('a2', 'q8'), ('dn_lite5', 'q8')):
        m = module_for(key)
        try:
            xd = torch.from_numpy(gd.noise_image(31, (2, 40, 72))[:, None]).to(dev)
            ya = m.set_option('x3_impl', 'auto')(xd)[-1]
            for impl in ('x3', 'q8'):
                yi = m.set_option('x3_impl', impl)(xd)[-1]
                assert torch.equal(ya, yi) == (impl == same_as), (key, impl)
        finally:
            m.set_option('x3_impl', 'auto')


RESIZE = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(G, 'resize', '*.npz')) if 'scale_factors' not in p)


@pytest.mark.parametrize('name', RESIZE)
def test_resize_kernel_vs_reference_golden(name, dev):
    """moe_resize (the `resize` step, python/imageProcess.py:555-556) against the reference's outputs: fp32 I/O to 3e-6 (the index
    arithmetic is not contracted, so neighbours and weights are the reference's), fp16 I/O to half an ulp of the result."""
    from moephoto_amd import imageProcess as ip
    z = np.load(os.path.join(G, 'resize', name + '.npz'))
    shape = tuple(int(v) for v in z['shape'])
    h, w = [int(v) for v in z['hw']]
    x = gd.natural_image(77, shape) if str(z['kind']) == 'natural' else gd.noise_image(77, shape)
    y = ip.resizeByTorch(torch.from_numpy(x).to(dev), w, h, str(z['method']))
    assert tuple(y.shape) == z['y'].shape and y.dtype == torch.float32
    assert np.abs(y.cpu().numpy() - z['y']).max() <= 3e-6
    y16 = ip.resizeByTorch(torch.from_numpy(x).to(dev).half(), w, h, str(z['method']))
    assert y16.dtype == torch.float16
    from oracle import resize as oresize
    want16 = oresize.resize(x.astype(np.float16).astype(np.float32), w, h, str(z['method']))
    assert np.abs(y16.float().cpu().numpy() - want16).max() <= 1e-3          # fp16 result: half an ulp of values up to 2


def test_resize_step_in_chain(dev, tmp_path):
    """§8(f)3: the step chain [SR, resize] through procedure.genProcess -- the reference's `resize` closure with scale factors
    (target size rounded like python/imageProcess.py:185-186), device resident between upload and download."""
    from moephoto_amd import imageProcess as ip, procedure
    from moephoto_amd.config import config
    from oracle import resize as oresize
    z = np.load(os.path.join(G, 'resize', 'scale_factors.npz'))
    x = gd.natural_image(78, (3, 33, 47))
    f = ip.resize({'scaleH': 1.7, 'scaleW': 0.6}, {'source': False})
    y = f(torch.from_numpy(x).to(dev))
    assert tuple(y.shape) == z['y'].shape == (3, 56, 28)
    assert np.abs(y.cpu().numpy() - z['y']).max() <= 3e-6
    config.modelRoot, config.crop_sr, config.fp16, config.deviceId = gd.ZOO, 64, False, 0
    ip.modelCache.clear()
    img = gd.to_u8(gd.natural_image(35, (3, 72, 88)))
    process, nodes = procedure.genProcess([{'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 0}, {'op': 'resize', 'width': '100', 'height': '90', 'method': 'bilinear'}])
    assert [n['op'] for n in nodes] == ['SR', 'resize']
    out = process(img)
    assert out.shape == (90, 100, 3) and out.dtype == np.uint8
    xf = oio.to_float_image(img)
    pl = oplanner.prepare((3, 72, 88), 1 << 40, 1e-3, 5, 2, 8, 64)
    sr = ostitch.do_crop(xf, pl, 2, onets.model_fn('net2x', gd.state_dict_for('a2', load_state_dict_file)))
    want = oio.to_output(oio.to_hwc(oresize.resize(sr, 100, 90, 'bilinear')))
    d = np.abs(out.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 0.1
    with pytest.raises(ValueError):
        ip.resizeByTorch(torch.from_numpy(x).to(dev), 10, 10, 'area')


def test_p2_through_plugin_table(dev):
    """`p2` (the second real Net2x weight file of the zoo) through runSR's table: {'model': 'p', 'scale': 2} -> ./model/p2/model_new.pth."""
    from moephoto_amd import runSR
    opt = _opt_sr('p', 2, 48)
    x = gd.natural_image(103, (3, 60, 72))
    y = runSR.sr(opt)(torch.from_numpy(x).to(dev)).cpu().numpy()
    sd = gd.state_dict_for('p2', load_state_dict_file)
    pl = oplanner.prepare((3, 60, 72), 1 << 40, 1e-3, 5, 2, 8, 48)
    want = ostitch.do_crop(x, pl, 2, onets.model_fn('net2x', sd))
    assert np.abs(y - want).max() <= TOL


def test_kernel_forms_agree(dev):
    """The alternative forms of the hot kernels, switched in-process: the register-resident-weights upsampler conv (conv3x3_rw.hip; default
    for PReLU epilogues, option sp_impl = rw also for the fused tail, = sp not at all) and lite's 1x1 kernel (conv1x1.hip, option conv1x1 = 0:
    generic kernel).  Forms of one layer use the same operands and rounding points: outputs agree to fp32 summation order, and every
    form is inside the tolerance of its arithmetic against the oracle."""
    def with_opt(m, name, value, default):
        try:
            return m.set_option(name, value)(xd)[-1].cpu().numpy()
        finally:
            m.set_option(name, default)
    for key, shape, prec in (('a4', (3, 24, 72), 'mixed'), ('a4', (2, 41, 35), 'fp16'), ('a3', (3, 16, 40), 'mixed'), ('a2', (1, 9, 33), 'mixed')):
        arch, sd = gd.MODELS[key][0], gd.state_dict_for(key, load_state_dict_file)
        x = gd.natural_image(23, shape)[:, None]
        want = onets.forward(arch, sd, x).numpy()
        xd = torch.from_numpy(x).to(dev)
        m = module_for(key, prec)
        ys = {'ps4': m.set_option('up_impl', 'ps4')(xd)[-1].cpu().numpy()}      # the default: conv3x3_ps4.hip for every x2 upsampler stage (x3 nets: the forms below)
        m.set_option('up_impl', 'rw')                                           # ... and round 3's per-phase kernels behind it
        ys.update({impl: with_opt(m, 'sp_impl', impl, 'auto') for impl in ('auto', 'sp', 'rw')})
        # the fused tail's per-phase output forms: nine tap planes per phase (conv3x3_sp + tapsum2/3) vs phase-class sums + aprons (conv3x3_rw + tapsum4, x2 stages)
        ys['planes'] = with_opt(m, 'tail_form', 'planes', 'sums')
        ys['planes+sp'] = with_opt(m.set_option('tail_form', 'planes'), 'sp_impl', 'sp', 'auto')
        m.set_option('tail_form', 'sums').set_option('up_impl', 'ps4')
        for impl, y in ys.items():
            assert np.abs(y - ys['sp']).max() <= 2.5e-4, (key, shape, prec, impl, float(np.abs(y - ys['sp']).max()))
            if prec == 'mixed':
                assert np.abs(y - want).max() <= TOL, (key, shape, impl, float(np.abs(y - want).max()))
    for key, shape in (('lite2', (3, 24, 40)), ('lite4', (2, 16, 72)), ('lite8', (1, 9, 35))):
        arch, sd = gd.MODELS[key][0], gd.state_dict_for(key, load_state_dict_file)
        x = gd.noise_image(29, shape)[:, None]
        want = onets.forward(arch, sd, x).numpy()
        xd = torch.from_numpy(x).to(dev)
        for prec in ('fp16x3', 'fp16'):
            m = module_for(key, prec)
            y1 = with_opt(m, 'conv1x1', 1, 1)
            y0 = with_opt(m, 'conv1x1', 0, 1)
            assert np.abs(y1 - y0).max() <= (2e-5 if prec == 'fp16x3' else 1e-3), (key, prec, float(np.abs(y1 - y0).max()))
            if prec == 'fp16x3':
                assert np.abs(y1 - want).max() <= 2e-5, (key, float(np.abs(y1 - want).max()))


def test_fused_tail_sums_vs_planes(dev):
    """The two forms of the fused 64->1 tail compute the same nine products per HR pixel and differ only in the association of their fp32 sum
    (tests/tailsum_model.py): phase-class sums + aprons (conv3x3_rw EPI 3 / 7 + tapsum4) against nine tap planes (conv3x3_sp EPI 3 / 7 + tapsum2) on
    shapes that put patch seams, ragged last patches (H % 8, W % 32 != 0: the masked kernel variant), single-patch images and several planes
    into play, with and without the activation split of the R branch.  The main convs of the two forms (conv3x3_rw / conv3x3_sp) accumulate in different
    orders, which flips an fp16 rounding of an activation now and then (one ulp of it times a tail weight): the forms agree to ~1e-4, a misplaced apron
    would show as 1e-2."""
    cases = [('a2', (3, 8, 32)), ('a2', (2, 20, 44)), ('a2', (1, 72, 136)), ('a2', (5, 16, 64)), ('a2', (3, 12, 100)), ('a2', (1, 8, 8)),
             ('a4', (3, 8, 16)), ('a4', (2, 20, 44)), ('a4', (1, 40, 72)), ('a4', (3, 24, 36))]
    for key, shape in cases:
        arch, sd = gd.MODELS[key][0], gd.state_dict_for(key, load_state_dict_file)
        for kind in ('natural', 'noise'):
            x = (gd.natural_image(41, shape) if kind == 'natural' else gd.noise_image(41, shape))[:, None]
            xd = torch.from_numpy(x).to(dev)
            want = onets.forward(arch, sd, x).numpy()
            for prec, split in (('mixed', 'r'), ('mixed', '0'), ('fp16', 'r')):
                m = module_for(key, prec)
                try:
                    m.set_option('tail_split', split)
                    ys = m.set_option('tail_form', 'sums')(xd)[-1].cpu().numpy()
                    yp = m.set_option('tail_form', 'planes')(xd)[-1].cpu().numpy()
                finally:
                    m.set_option('tail_form', 'sums').set_option('tail_split', 'r')
                scale = max(1.0, float(np.abs(want).max()))
                assert np.abs(ys - yp).max() <= (2.5e-4 if kind == 'natural' else 6e-4) * scale, (key, shape, kind, prec, split, float(np.abs(ys - yp).max()))
                if prec == 'mixed' and split == 'r':
                    assert np.abs(ys - want).max() <= TOL, (key, shape, kind, float(np.abs(ys - want).max()))


def test_split_operand_conv_single_launch(dev):
    """conv64_x3.hip (the three split-operand products of a 3x3 64->64 layer in one launch, both weight parts in registers) against the
    three-launch form (option x3_fuse = 0) and the oracle: every epilogue (plain = conv_input2, PReLU = conv_1, residual = conv_2), ragged
    shapes, 48- and 64-channel nets.  With all six ARSBs split the trunk is ~fp32: the taps must agree with the oracle to ~1e-6."""
    m = None
    try:
        for key, shape in (('a2', (3, 8, 16)), ('a2', (3, 24, 40)), ('a2', (2, 40, 264)), ('a2', (3, 9, 35)), ('dn_lite5', (3, 33, 31)), ('dn_lite5', (5, 88, 64))):
            arch = gd.MODELS[key][0]
            sd = gd.state_dict_for(key, load_state_dict_file)
            x = gd.noise_image(19, shape)[:, None]
            taps = {}
            want = onets.forward(arch, sd, x, 'torch', taps).numpy()
            xd = torch.from_numpy(x).to(dev)
            m = module_for(key, 'mixed').set_exact_blocks(6).set_debug(True).set_option('x3_impl', 'x3')      # (conv64_q8's fp8 corrections have their own test)
            res = {}
            for fuse in ('0', '1'):
                y = m.set_option('x3_fuse', fuse)(xd)[-1].cpu().numpy()
                res[fuse] = (y, {k: m.debug_tap(k) for k in ('input2', 'arsb1', 'arsb6')})
            m.set_debug(False).set_exact_blocks(-1)
            for k in ('input2', 'arsb1', 'arsb6'):
                w = taps[k].numpy()
                scale = max(1.0, float(np.abs(w).max()))
                assert np.abs(res['1'][1][k] - w).max() <= 2e-6 * scale, (key, shape, k, float(np.abs(res['1'][1][k] - w).max()))
                assert np.abs(res['1'][1][k] - res['0'][1][k]).max() <= 2e-6 * scale, (key, shape, k)
            assert np.abs(res['1'][0] - want).max() <= TOL
    finally:
        if m is not None:
            m.set_option('x3_fuse', 1).set_option('x3_impl', 'auto').set_debug(False).set_exact_blocks(-1)


@pytest.mark.parametrize('key', ['a2', 'a4'])
def test_upconv_all_phases_in_one_workgroup_vs_per_phase_form(key, dev):
    """Option up_impl = ps4 (default; conv3x3_ps4.hip: every x2 upsampler stage with all four pixel-shuffle phases in one workgroup, rows streamed down a
    32-pixel column; the last stage carries the 64 -> 1 tail conv and leaves one fp32 plane + column aprons per branch, added by tailadd) against round 3's
    form (up_impl = rw: one phase per workgroup, phase-class sums, tapsum4).  The conv sums are the same MFMAs in the same order (bit-identical); the tail's
    nine products per output pixel are associated differently in fp32: the outputs agree to a few 1e-7 -- on shapes that are ragged against the 4-row blocks
    and 32-pixel columns, with several planes and strips -- both hold the tolerance against the oracle, a launch repeated gives the same bits, and the
    result does not depend on how the column-major ranges are cut (7 workgroups instead of one per CU: the rows above / below a range are recomputed)."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    shapes = ((3, 8, 8), (3, 24, 40), (2, 40, 264), (3, 16, 72), (1, 88, 64), (3, 64, 64)) if key == 'a4' else ((3, 24, 40), (2, 40, 264), (3, 8, 36), (1, 88, 64), (3, 128, 96), (4, 256, 256))
    try:
        for shape in shapes:
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(31, shape) if kind == 'natural' else gd.noise_image(31, shape))[:, None]
                xd = torch.from_numpy(x).to(dev)
                y_rw = m.set_option('up_impl', 'rw')(xd)[-1].cpu().numpy()
                y_ps = m.set_option('up_impl', 'ps4')(xd)[-1].cpu().numpy()
                y_again = m(xd)[-1].cpu().numpy()
                y_cut = m.set_option('max_groups', 7)(xd)[-1].cpu().numpy()
                m.set_option('max_groups', 0)
                assert np.isfinite(y_ps).all(), (key, shape, kind)
                assert np.abs(y_ps - y_rw).max() <= 2e-6, (key, shape, kind, float(np.abs(y_ps - y_rw).max()))
                assert np.array_equal(y_ps, y_again), (key, shape, kind)
                assert np.array_equal(y_ps, y_cut), (key, shape, kind, float(np.abs(y_ps - y_cut).max()))
                if shape[1] * shape[2] <= 128 * 128:
                    want = onets.forward(arch, sd, x).numpy()
                    assert np.abs(y_ps - want).max() <= TOL, (key, shape, kind, float(np.abs(y_ps - want).max()))
        # an fp16 result tensor (the drop-in path's dtype): tailadd rounds once
        x = gd.noise_image(7, (3, 24, 40))[:, None]
        m16 = module_for(key, dtype=torch.float16)
        y16 = m16(torch.from_numpy(x).to(dev).half())[-1].float().cpu().numpy()
        m32 = module_for(key)
        y32 = m32(torch.from_numpy(x.astype(np.float16).astype(np.float32)).to(dev))[-1].cpu().numpy()
        assert np.abs(y16 - y32).max() <= HALF_OUT * max(1.0, float(np.abs(y32).max()) / 2), (key, float(np.abs(y16 - y32).max()))
    finally:
        m.set_option('up_impl', 'ps4').set_option('max_groups', 0)


def test_x3_upconv_phase_rows_vs_per_phase_form(dev):
    """Net3x's upsampler stage on conv3x3_ps9.hip (option up_impl = ps4, the default: a workgroup = the three phases of one phase row, rows streamed down a
    32-pixel column, the 64 -> 1 tail's horizontal sums closed in the workgroup, three fp32 planes S[dy] + column aprons per branch, tailadd3) against round 2's
    form (up_impl = rw: conv3x3_sp per phase, nine tap planes, tapsum<3>).  The two main convs accumulate in different orders (an fp16 rounding of an activation
    flips now and then: the forms agree to ~1e-4, a misplaced apron or phase would show as 1e-2); both hold the tolerance against the oracle; a launch repeated
    gives the same bits; the result does not depend on how the ranges are cut (7 workgroups = 2 ranges instead of 80) -- on shapes ragged against the 32-pixel
    columns (the masked variant), with several planes, strips and columns, with and without the activation split of the R branch."""
    key = 'a3'
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    shapes = ((3, 8, 8), (3, 24, 40), (2, 40, 264), (3, 16, 72), (1, 88, 64), (3, 64, 96), (4, 128, 128), (3, 256, 256))
    try:
        for shape in shapes:
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(37, shape) if kind == 'natural' else gd.noise_image(37, shape))[:, None]
                xd = torch.from_numpy(x).to(dev)
                want = onets.forward(arch, sd, x).numpy() if (shape[1] * shape[2] <= 128 * 128 or (shape == (3, 256, 256) and kind == 'noise')) else None      # (one full-size tile against the oracle)
                for split in ('r', '0'):
                    m.set_option('tail_split', split)
                    y_sp = m.set_option('up_impl', 'rw')(xd)[-1].cpu().numpy()
                    y_ps = m.set_option('up_impl', 'ps4')(xd)[-1].cpu().numpy()
                    y_again = m(xd)[-1].cpu().numpy()
                    y_cut = m.set_option('max_groups', 7)(xd)[-1].cpu().numpy()
                    y_one = m.set_option('max_groups', 3)(xd)[-1].cpu().numpy()
                    m.set_option('max_groups', 0)
                    assert np.isfinite(y_ps).all(), (shape, kind, split)
                    scale = max(1.0, float(np.abs(y_sp).max()))
                    assert np.abs(y_ps - y_sp).max() <= (2.5e-4 if kind == 'natural' else 6e-4) * scale, (shape, kind, split, float(np.abs(y_ps - y_sp).max()))
                    assert np.array_equal(y_ps, y_again), (shape, kind, split)
                    assert np.array_equal(y_ps, y_cut), (shape, kind, split, float(np.abs(y_ps - y_cut).max()))
                    assert np.array_equal(y_ps, y_one), (shape, kind, split, float(np.abs(y_ps - y_one).max()))
                    if want is not None and split == 'r':
                        assert np.abs(y_ps - want).max() <= TOL, (shape, kind, float(np.abs(y_ps - want).max()))
        # an fp16 result tensor (the drop-in path's dtype): tailadd3 rounds once
        x = gd.noise_image(7, (3, 24, 40))[:, None]
        m16 = module_for(key, dtype=torch.float16)
        y16 = m16(torch.from_numpy(x).to(dev).half())[-1].float().cpu().numpy()
        m32 = module_for(key)
        y32 = m32(torch.from_numpy(x.astype(np.float16).astype(np.float32)).to(dev))[-1].cpu().numpy()
        assert np.abs(y16 - y32).max() <= HALF_OUT * max(1.0, float(np.abs(y32).max()) / 2), float(np.abs(y16 - y32).max())
    finally:
        m.set_option('up_impl', 'ps4').set_option('max_groups', 0).set_option('tail_split', 'r')


@pytest.mark.parametrize('key', ['a3', 'a4'])
def test_branch_sum_into_unaligned_output_planes(key, dev):
    """moe_net_forward writes the caller's tensor directly; when its planes do not start 16-byte aligned (a view one element into a buffer) the branch sums
    (tailadd / tailadd3, conv3x3_ps4.hip / conv3x3_ps9.hip) take their scalar-store form: the same values, bit for bit, as into an aligned tensor -- fp32 and fp16."""
    from moephoto_amd import _lib
    m = module_for(key)
    sc = m.scale
    x = gd.noise_image(61, (3, 24, 40))[:, None]
    for dt, code in ((torch.float32, _lib.F32), (torch.float16, _lib.F16)):
        xd = torch.from_numpy(x).to(dev).to(dt)
        md = module_for(key, dtype=dt) if dt == torch.float16 else m
        want = md(xd)[-1]
        n = want.numel()
        buf = torch.full((n + 16,), float('nan'), dtype=dt, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        sB, _, sH, sW = xd.stride()
        _lib.check(_lib.lib().moe_net_forward(md._h, xd.data_ptr(), code, 3, 24, 40, sB, sH, sW, None, buf.data_ptr() + buf.element_size(), code, None, stream))
        torch.cuda.synchronize()
        got = buf[1:1 + n].view(want.shape)
        assert torch.equal(got, want), (key, str(dt), float((got.float() - want.float()).abs().max()))
        assert torch.isnan(buf[0]) and torch.isnan(buf[1 + n:]).all()          # nothing written outside the planes


@pytest.mark.parametrize('key', ['lite4', 'lite8'])
def test_lite_last_two_upsampler_stages_in_one_launch(key, dev):
    """Option up_fuse2 (default on; conv1x1_f2.hip): the last two upsampler stages of MoeNet_lite2 and the folded 48 -> 1 tail in ONE launch -- every layer there is pointwise
    (1x1 convs, pixel shuffle, PReLU), the 4x-resolution tensor between the stages never exists -- against the stage-by-stage form (conv1x1.hip): per layer the same products
    in the same order and the same hi / lo roundings between the stages, so the outputs are EQUAL bit for bit; within 2e-5 of the oracle (split operands); on shapes ragged
    against the 32-pixel tiles, tiny ones, several planes; a launch repeated gives the same bits."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    try:
        for shape in ((3, 24, 40), (2, 16, 72), (1, 9, 35), (3, 8, 8), (5, 40, 33), (2, 64, 96)):
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(67, shape) if kind == 'natural' else gd.noise_image(67, shape))[:, None]
                xd = torch.from_numpy(x).to(dev)
                y0 = m.set_option('up_fuse2', 0)(xd)[-1].cpu().numpy()
                y1 = m.set_option('up_fuse2', 1)(xd)[-1].cpu().numpy()
                y2 = m(xd)[-1].cpu().numpy()
                assert np.isfinite(y1).all(), (key, shape, kind)
                assert np.array_equal(y1, y0), (key, shape, kind, float(np.abs(y1 - y0).max()))
                assert np.array_equal(y1, y2), (key, shape, kind)
                want = onets.forward(arch, sd, x).numpy()
                assert np.abs(y1 - want).max() <= 2e-5, (key, shape, kind, float(np.abs(y1 - want).max()))
    finally:
        m.set_option('up_fuse2', 1)


@pytest.mark.parametrize('key', ['lite2', 'lite4'])
def test_lite_frm_gate_from_conv2_input(key, dev):
    """Option frm_pre (default on; MoeNet_lite2.py:16-20, models.py:270-287): an LB's conv_2 has no bias and no activation, so the mean the FRM gate pools is linear in conv_2's
    INPUT -- conv_1's epilogue forms its totals, frm_pre_kernel the border sums, the product with conv_2's weights and the gate; conv_2 stores gate * conv + x and frm_apply's
    pass is gone.  Against the form that pools conv_2's output (frm_pre = 0): another summation order for the mean and g (conv + x / g) for g conv + x, i.e. fp32-rounding
    apart; both within 2e-5 of the oracle; ragged, tiny (one patch, one row) and multi-plane shapes; a repeated launch gives the same bits."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    try:
        for shape in ((3, 24, 40), (2, 16, 72), (1, 9, 35), (3, 8, 8), (5, 40, 33), (2, 64, 96), (1, 1, 7), (2, 3, 1)):
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(71, shape) if kind == 'natural' else gd.noise_image(71, shape))[:, None]
                xd = torch.from_numpy(x).to(dev)
                y0 = m.set_option('frm_pre', 0)(xd)[-1].cpu().numpy()
                y1 = m.set_option('frm_pre', 1)(xd)[-1].cpu().numpy()
                y2 = m(xd)[-1].cpu().numpy()
                assert np.isfinite(y1).all(), (key, shape, kind)
                assert np.array_equal(y1, y2), (key, shape, kind)
                want = onets.forward(arch, sd, x).numpy()
                assert np.abs(y1 - want).max() <= 2e-5 and np.abs(y0 - want).max() <= 2e-5, (key, shape, kind, float(np.abs(y1 - want).max()), float(np.abs(y0 - want).max()))
                assert np.abs(y1 - y0).max() <= 1e-5, (key, shape, kind, float(np.abs(y1 - y0).max()))
    finally:
        m.set_option('frm_pre', 1)


@pytest.mark.parametrize('key', ['lite2', 'lite8'])
def test_lite_conv_input2_in_closed_form(key, dev):
    """Option stem2 (default on; MoeNet_lite2.py:40-41): conv_input2(PReLU(conv_input(x))) has ONE input channel and 1x1 kernels, so it is x times a fixed 48-vector (one for
    x >= 0, one for x < 0) -- the stem writes that tensor beside its own output and the 48 -> 48 conv is not launched.  Against the launched form (stem2 = 0): fp32-rounding
    apart, both within 2e-5 of the oracle; inputs of both signs (the nets are only ever fed [0, 1], the identity holds for any x)."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    try:
        for shape in ((3, 24, 40), (1, 9, 35), (2, 64, 96), (1, 1, 7)):
            for kind in ('natural', 'noise', 'signed'):
                x = (gd.natural_image(73, shape) if kind == 'natural' else gd.noise_image(73, shape))[:, None]
                if kind == 'signed':
                    x = (x - np.float32(0.5)) * np.float32(1.5)
                xd = torch.from_numpy(x).to(dev)
                y0 = m.set_option('stem2', 0)(xd)[-1].cpu().numpy()
                y1 = m.set_option('stem2', 1)(xd)[-1].cpu().numpy()
                want = onets.forward(arch, sd, x).numpy()
                assert np.abs(y1 - want).max() <= 2e-5 and np.abs(y0 - want).max() <= 2e-5, (key, shape, kind, float(np.abs(y1 - want).max()), float(np.abs(y0 - want).max()))
                assert np.abs(y1 - y0).max() <= 1e-5, (key, shape, kind, float(np.abs(y1 - y0).max()))
        # plain fp16 operands (not lite's default: every layer of it is error-critical): the launched conv rounds its operands to fp16, the closed form does not -- the two
        # agree at that level
        mh = module_for(key, 'fp16')
        x = gd.natural_image(73, (2, 40, 56))[:, None]
        xd = torch.from_numpy(x).to(dev)
        try:
            h0 = mh.set_option('stem2', 0)(xd)[-1].cpu().numpy()
        finally:
            mh.set_option('stem2', 1)
        h1 = mh(xd)[-1].cpu().numpy()
        assert np.isfinite(h0).all() and np.isfinite(h1).all() and np.abs(h1 - h0).max() <= 2e-2, (key, float(np.abs(h1 - h0).max()))
    finally:
        m.set_option('stem2', 1)


@pytest.mark.parametrize('key', ['lite2', 'lite4', 'lite8'])
def test_lite_u_branch_as_a_table_for_fp16_inputs(key, dev):
    """Option lite_lut (default on; MoeNet_lite2.py:47,50): the U branch -- conv_input, PReLU, the uim stages, convt_I1 -- is pointwise on a ONE-channel input, so its value at an
    HR pixel depends on one input value and the pixel's phase.  For fp16 inputs the engine fills a table over the 65,536 bit patterns with the branch's own kernels (once per
    checkpoint, on the first fp16 forward) and the final sum looks the value up: BIT-IDENTICAL to computing the branch (lite_lut = 0), within 2e-5 (+ half an fp16 ulp of the
    output) of the oracle on the fp16-rounded input; fp32 inputs keep computing; a changed option or reloaded weights drop the table."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    try:
        for shape in ((3, 24, 40), (1, 9, 35), (2, 64, 96), (1, 1, 7), (4, 33, 17)):
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(79, shape) if kind == 'natural' else gd.noise_image(79, shape))[:, None]
                xh = torch.from_numpy(x).to(dev).half()
                y0 = m.set_option('lite_lut', 0)(xh)[-1]
                y1 = m.set_option('lite_lut', 1)(xh)[-1]
                y2 = m(xh)[-1]
                assert torch.equal(y1, y0), (key, shape, kind, float((y1.float() - y0.float()).abs().max()))
                assert torch.equal(y1, y2), (key, shape, kind)
                want = onets.forward(arch, sd, xh.float().cpu().numpy()).numpy()
                got = y1.float().cpu().numpy()
                assert np.abs(got - want).max() <= 2e-5 + HALF_OUT * (y1.dtype == torch.float16), (key, shape, kind, float(np.abs(got - want).max()))
        # a strided view (what doCrop's per-tile calls pass) and an fp32 input right behind an fp16 one
        big = torch.from_numpy(gd.natural_image(83, (3, 70, 90))[:, None]).to(dev).half()
        view = big[:, :, 5:53, 11:75]
        assert torch.equal(m(view)[-1], m(view.contiguous())[-1])
        x32 = view.float()
        want = onets.forward(arch, sd, x32.cpu().numpy()).numpy()
        assert np.abs(m(x32)[-1].float().cpu().numpy() - want).max() <= 2e-5 + HALF_OUT
    finally:
        m.set_option('lite_lut', 1)


def test_integration_md_stub_drives_every_family(dev):
    """INTEGRATION.md section 1 is the binding a MoePhoto maintainer would add (a ctypes stub over include/moephoto_amd.h).  This test EXECUTES that text --
    the first python block of the file, with the library path filled in -- and drives one SR key, one NetDN key, one SEDN key and one lite key through the
    reference's initModel sequence (python/imageProcess.py:319-334: ctor(); load_state_dict; requires_grad_; eval; .to(dtype, device)) and Option.__call__
    against the reference-generated goldens.  The stub passes MOE_PREC_AUTO: the per-family precision policy is the library's, not the caller's."""
    import re
    from moephoto_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'INTEGRATION.md')).read()
    code = re.search(r'```python\n(.*?)```', text, re.S).group(1)
    assert 'moe_net_finalize' in code and 'class SEDN' in code
    code = code.replace("'libmoephoto_amd.so'", repr(_lib.LIB_PATH))
    ns = {}
    exec(compile(code, 'INTEGRATION.md', 'exec'), ns)
    cases = [('a2', lambda: ns['Net2x']()), ('dn_lite5', lambda: ns['NetDN']()), ('l25', lambda: ns['SEDN']()), ('lite2', lambda: ns['Net'](2))]
    for key, ctor in cases:
        z = np.load(os.path.join(G, 'nets', key + '.npz'))
        h, w = [int(v) for v in z['hw']]
        seed = int(z['seed'])
        m = ctor()
        m.load_state_dict({n: torch.from_numpy(v) for n, v in gd.state_dict_for(key, load_state_dict_file).items()})
        for p in m.parameters():
            p.requires_grad_(False)
        m.eval()
        m = m.to(dtype=torch.float32, device=dev)
        for kind in ('natural', 'noise'):
            x = gd.natural_image(seed, (3, h, w))[:, None] if kind == 'natural' else gd.noise_image(seed, (3, 1, h, w))
            y = m(torch.from_numpy(x).to(dev))[-1].float().cpu().numpy()
            err = np.abs(y - z['y_' + kind]).max()
            assert err <= TOL, '{} {} through the INTEGRATION.md stub: {:.3e}'.format(key, kind, err)


def test_stitch_band_equals_rows_of_the_canvas(dev):
    """moe_stitch_band: the canvas in row bands along tile-row boundaries (dist.py's band-sharded stitch for jobs with fewer frames than ranks).  Every band,
    from whole tiles (strip = 0) and with the next tile row present only as the strips of its blend band (strip = 1: C planes of pad_sc rows, cut here the way
    dist.TileExchange.cut_strips does), must equal the same rows of moe_stitch's canvas bit for bit -- including the re-anchored last tile row."""
    import ctypes
    from moephoto_amd import _lib, imageProcess as ip
    for (H, W, crop, scale, model) in ((150, 200, 64, 4, 'a'), (293, 120, 96, 2, 'a'), (150, 101, 64, 2, 'a')):      # (the last: a canvas width of 202, no multiple of 8)
        opt = _opt_sr(model, scale, crop, fp16_io=True)
        xd = torch.from_numpy(gd.natural_image(3, (3, H, W))).to(dev).half()
        plan = ip._plan_for(opt, xd.shape)
        L = _lib.lib()
        stream = torch.cuda.current_stream().cuda_stream
        pool = torch.empty(plan.pool_elems(3), dtype=torch.float32, device=dev)
        canvas = torch.empty((3, plan.outH, plan.outW), dtype=torch.float16, device=dev)
        sC, sH, sW = xd.stride()
        _lib.check(L.moe_run_plan_ex(opt.modelCached._h, plan._h, xd.data_ptr(), _lib.F16, sC, sH, sW, canvas.data_ptr(), _lib.F16, 0, ctypes.c_void_p(pool.data_ptr()), 0, 1, 1, stream))
        off = plan.tile_offsets(3)
        nrow = plan.stepH
        assert nrow >= 3 and len(plan.rows) == nrow
        S = [r[1] for r in plan.rows] + [plan.outH]
        assert S[0] == 0
        for cuts in ([0, 1, nrow], [0, nrow // 2, nrow - 1, nrow], list(range(nrow + 1))):
            for i0, i1 in zip(cuts, cuts[1:]):
                for strip in (0, 1):
                    offs = list(off)
                    buf = pool
                    if strip and i1 < nrow:        # tile row i1 as strips, appended behind the pool
                        extra = []
                        base = pool.numel()
                        for j in range(plan.stepW):
                            k = i1 * plan.stepW + j
                            t = plan.tiles[k]
                            th, tw = (t[1] - t[0]) * scale, (t[3] - t[2]) * scale
                            r0 = plan.rows[i1][0] - plan.rows[i1][2]
                            extra.append(pool[off[k]:off[k] + 3 * th * tw].view(3, th, tw)[:, r0:r0 + plan.padSc].reshape(-1))
                            offs[k] = base
                            base += extra[-1].numel()
                        buf = torch.cat([pool] + extra)
                    tab = torch.tensor(offs, dtype=torch.int64, device=dev)
                    y = torch.full((3, S[i1] - S[i0], plan.outW), float('nan'), dtype=torch.float16, device=dev)
                    _lib.check(L.moe_stitch_band(plan._h, 0, buf.data_ptr(), ctypes.c_void_p(tab.data_ptr()), 3, y.data_ptr(), _lib.F16, i0, i1, strip, stream))
                    torch.cuda.synchronize()
                    assert torch.equal(y, canvas[:, S[i0]:S[i1]]), (H, W, i0, i1, strip)


def test_calibrate_exact_blocks_for_other_weights(dev):
    """moe_net_calibrate (behind the C ABI since round 5; EngineModule.calibrate is a thin call): the per-architecture number of split-operand blocks was chosen on
    the zoo's weights; a checkpoint whose trunk swings wider needs more (tools/margin_sweep.py).  `.to(device)` under precision 'auto' measures it by itself
    (moe_net_finalize(MOE_PREC_AUTO)): a2 as shipped keeps the default (4), a2 with its trunk weights x 1.15 -- where 4 blocks spend more than the target on uint8
    noise -- moves to more blocks with a smaller error; an explicit set_exact_blocks overrides, -1 returns to the measured count; option auto_calibrate = 0 keeps the
    architecture's default."""
    from moephoto_amd import models
    sd = gd.state_dict_for('a2', load_state_dict_file)

    def build(scale, pre=None):
        v = {k: (a * np.float32(scale) if (k.startswith('conv_input2') or (k.startswith('convt_F') and a.ndim == 4)) else a) for k, a in sd.items()}
        m = models.Net2x()
        if pre:
            pre(m)
        m.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(a, np.float32)) for n, a in v.items()})
        return m.eval().to(dtype=torch.float32, device=dev)
    m = build(1.0)
    assert m.exact_blocks() == 4 and m.resolved_precision() == 'mixed'
    n, err = m.calibrate()
    assert n == 4 and err <= 8.5e-4 * 1.05, (n, err)      # (err: the predicted worst tile of a full frame = measured x 1.10; the default count is kept up to 5 % above the target)
    m = build(1.15)
    na = m.exact_blocks()
    assert na > 4 or m.resolved_precision() == 'fp16x3', na
    x = torch.from_numpy(gd.noise_u8(0, (3, 192, 192)).astype(np.float32) / np.float32(255)).to(dev)[:, None]
    ya = m(x)[-1].clone()
    want = m.set_precision('fp16x3')(x)[-1].clone()
    m.set_precision('auto')
    ea = float((ya - want).abs().amax())
    if m.resolved_precision() == 'fp16x3':       # (round 6: the conservative calibration may find that not even six blocks keep the PREDICTED full-frame error inside its target)
        assert ea == 0.0, ea
    else:
        e4 = float((m.set_exact_blocks(4)(x)[-1] - want).abs().amax())
        assert ea < e4 and ea <= 9e-4, (na, ea, e4)
        m.set_exact_blocks(-1)
    assert m.exact_blocks() == na and torch.equal(m(x)[-1], ya)
    m0 = build(1.15, pre=lambda q: q.set_option('auto_calibrate', 0))
    assert m0.exact_blocks() == 4


def test_integration_md_stub_holds_the_contract_on_checkpoints_with_a_wider_trunk(dev):
    """the INTEGRATION.md stub, executed as written, loads checkpoints the defaults were NOT tuned on -- a2 and a4-synth with every trunk conv
    (conv_input2, the twelve ARSB convs) x 1.15, which the per-architecture block counts miss by 1.3e-3 / 1.8e-3 (profiles/r04/n_margin_sweep_and_fuzz_final_tree.txt)
    -- and must hold 1e-3 against the fp32 ORACLE on a full 256 x 256 uint8-noise tile: moe_net_finalize(MOE_PREC_AUTO) measures the checkpoint when it is loaded."""
    import re
    from moephoto_amd import _lib
    from oracle import nets as onets
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'INTEGRATION.md')).read()
    code = re.search(r'```python\n(.*?)```', text, re.S).group(1).replace("'libmoephoto_amd.so'", repr(_lib.LIB_PATH))
    ns = {}
    exec(compile(code, 'INTEGRATION.md', 'exec'), ns)
    x = gd.noise_u8(5, (3, 256, 256)).astype(np.float32)[:, None] / np.float32(255)
    for key, cls, oname in (('a2', 'Net2x', 'net2x'), ('a4', 'Net4x', 'net4x')):
        sd = gd.state_dict_for(key, load_state_dict_file)
        sd = {k: (np.ascontiguousarray(a * np.float32(1.15)) if (k.startswith('conv_input2') or (k.startswith('convt_F') and a.ndim == 4)) else a) for k, a in sd.items()}
        m = ns[cls]()
        m.load_state_dict({n: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for n, v in sd.items()})
        m.eval()
        m = m.to(dtype=torch.float32, device=dev)
        y = m(torch.from_numpy(x).to(dev))[-1].float().cpu().numpy()
        want = onets.forward(oname, sd, x).numpy()
        err = float(np.abs(y - want).max())
        assert err <= TOL, '{} x1.15 trunk through the INTEGRATION.md stub vs the oracle: {:.3e}'.format(key, err)


def test_one_launch_arsb_does_not_depend_on_how_its_ranges_are_cut(dev):
    """arsb32c.hip gives a workgroup a contiguous range of the column-major patch sequence; the first patch of a range recomputes the two m rows it would have
    inherited, from the same operands in the same order -- not a bit may depend on the number of workgroups, on ragged shapes, 48- and 64-channel nets, with and
    without the hi + lo stream.  (Round 4 held the streamed form arsb_s.hip against it here, bit for bit; that form measured 7 % slower and left the build in round 5
    -- profiles/r04/d_arsb_streamed_vs_patch.txt, history at 321d022.)"""
    touched = []
    try:
        for key, prec in (('a2', 'auto'), ('a2', 'fp16'), ('dn_lite5', 'auto'), ('dn_lite5', 'fp16'), ('a4', 'auto')):
            m = module_for(key, prec)
            touched.append(m)
            for shape in ((3, 8, 16), (3, 24, 40), (2, 40, 264), (3, 16, 35), (5, 88, 64), (2, 128, 61)):
                x = gd.noise_image(17, shape)[:, None]
                xd = torch.from_numpy(x).to(dev)
                y3 = m(xd)[-1]
                yg = m.set_option('max_groups', 5)(xd)[-1]
                m.set_option('max_groups', 0)
                assert torch.equal(y3, yg), (key, prec, shape, float((y3 - yg).abs().max()))
    finally:
        for m in touched:
            m.set_option('max_groups', 0)


def test_small_launch_sets_fork_the_u_branch_onto_a_second_stream(dev):
    """Option branch_streams (round 5, default on): a forward of a few planes (the reference's own per-tile loop: 3 planes of <= 256 x 256) runs its U branch on a second
    HIP stream beside the trunk + R branch, forked behind the stem and joined in front of the branch sum.  Same kernels: the result must be the single-stream result bit
    for bit -- on every SR family, fp16 and fp32 I/O, back to back with changing inputs (a missing fork / join edge shows up as one forward reading the other's buffers),
    on the caller's non-default stream, and through the reference-style loop."""
    side = torch.cuda.Stream()
    for key, prec in (('a2', 'auto'), ('a3', 'auto'), ('a4', 'auto'), ('a4', 'fp16')):
        m = module_for(key, prec)
        try:
            xs = [torch.from_numpy(gd.noise_image(40 + i, sh)[:, None]).to(dev) for i, sh in enumerate(((3, 64, 96), (3, 40, 72), (4, 88, 61), (3, 64, 96), (1, 8, 16), (3, 128, 128)))]
            m.set_option('branch_streams', 0)
            want = [m(x)[-1].clone() for x in xs]
            m.set_option('branch_streams', 1)
            for rep in range(3):
                got = [m(x)[-1] for x in xs]                  # enqueued back to back, nothing synchronises in between
                for i, (g, w) in enumerate(zip(got, want)):
                    assert torch.equal(g, w), (key, prec, rep, i, float((g - w).abs().max()))
            with torch.cuda.stream(side):
                side.wait_stream(torch.cuda.current_stream())
                got = [m(x.half())[-1] for x in xs]
            side.synchronize()
            m.set_option('branch_streams', 0)
            for i, (g, x) in enumerate(zip(got, xs)):
                assert torch.equal(g, m(x.half())[-1]), (key, prec, 'side stream', i)
        finally:
            m.set_option('branch_streams', 1)


def test_consecutive_forwards_on_slices_of_one_image_overlap_and_keep_their_bits(dev):
    """moe_net_forward_ex / MOE_FWD_INPUT_SINCE_PREV (round 6, option overlap_calls): the torch wrapper marks a forward whose input is a view of the same live storage, at
    the same version counter, as the previous call's -- the reference's tile loop (python/imageProcess.py:164-170) -- and the engine then runs consecutive forwards on two
    internal (stream, workspace) sets, forward k+1 beside forward k.  Everything the caller can observe must be as on one stream: (1) back-to-back forwards on slices of
    one image with their results consumed at once (the loop's blend reads r right behind the call) give the bits of single calls; (2) an input written IN PLACE between
    two calls (version bump: no flag) is seen; (3) a new image allocated where the old one lived (the weak reference is dead: no flag) is seen; (4) y memory that the
    caller's own kernels were still using when the call was made is not overwritten early; (5) the reference-style loop end to end, overlapped against not."""
    from moephoto_amd import _lib
    for key, prec, io in (('a4', 'auto', torch.float16), ('a2', 'auto', torch.float32), ('a3', 'auto', torch.float16)):
        m = module_for(key, prec)
        sc = m.scale
        img = torch.from_numpy(gd.noise_image(77, (3, 200, 328))).to(dev).to(io).unsqueeze(1)
        tiles = [(0, 64, 0, 96), (40, 104, 72, 168), (136, 200, 232, 328), (0, 64, 0, 96), (100, 164, 8, 104), (8, 72, 200, 296), (120, 128, 16, 32), (0, 128, 0, 128)]
        try:
            m.set_option('overlap_calls', 0)
            want = [m(img[..., t:b, l:r])[-1].clone() for (t, b, l, r) in tiles]
            torch.cuda.synchronize()
            m.set_option('overlap_calls', 1)
            for rep in range(3):
                acc = []
                flags = []
                for (t, b, l, r) in tiles:
                    y = m(img[..., t:b, l:r])[-1]
                    flags.append(m._last_flag)
                    acc.append(y * 1.0)                                   # consumed on the caller's stream at once; y itself is dropped and its memory reused by the next calls
                    del y
                for i, (g, w) in enumerate(zip(acc, want)):
                    assert torch.equal(g, w), (key, rep, i, float((g.float() - w.float()).abs().max()))
                assert flags[1:] == [_lib.FWD_INPUT_SINCE_PREV] * (len(tiles) - 1), flags      # (the first call of a burst after another input: plain order)
                img = img.clone()                                        # another storage for the next repetition: its first call must not be flagged
            # (2) in-place write between calls
            base = img.clone()
            y0 = m(base[..., 0:64, 0:96])[-1].clone()
            base.mul_(0.5)
            y1 = m(base[..., 0:64, 0:96])[-1].clone()
            assert m._last_flag == 0
            m.set_option('overlap_calls', 0)
            assert torch.equal(y1, m(base[..., 0:64, 0:96])[-1]) and not torch.equal(y0, y1)
            m.set_option('overlap_calls', 1)
            # (3) a new image at the old address
            a = torch.from_numpy(gd.noise_image(5, (3, 64, 96))).to(dev).to(io).unsqueeze(1)
            ya = m(a)[-1].clone()
            ptr = a.data_ptr()
            del a
            bimg = torch.from_numpy(gd.noise_image(6, (3, 64, 96))).to(dev).to(io).unsqueeze(1)
            yb = m(bimg)[-1].clone()
            assert m._last_flag == 0, (ptr, bimg.data_ptr())
            m.set_option('overlap_calls', 0)
            assert torch.equal(yb, m(bimg)[-1]) and not torch.equal(ya, yb)
            m.set_option('overlap_calls', 1)
            # (4) the caller's kernels still read the memory y will get: a long chain of torch ops on a buffer, freed right before the call (the caching allocator hands
            # the block to y at once -- legal on one stream); the chain's result must not see the forward's output
            x1 = img[..., 0:128, 0:128]
            m(x1)                                                       # (burst start)
            shape = (3, 1, 128 * sc, 128 * sc)
            for rep in range(4):
                buf = torch.full(shape, 1.0, dtype=io, device=dev)
                chk = buf
                for _ in range(30):
                    chk = chk * 1.0
                total = chk.float().sum()
                del buf, chk
                y = m(x1)[-1]
                assert m._last_flag == _lib.FWD_INPUT_SINCE_PREV
                assert float(total) == float(3 * 128 * sc * 128 * sc), (key, rep, float(total))
                del y
        finally:
            m.set_option('overlap_calls', 1)
    # (5) the reference-style loop around the class, overlapped against not
    import bench
    from moephoto_amd import imageProcess as ip
    opt = _opt_sr('a', 4, 64, fp16_io=True)
    x = torch.from_numpy(gd.natural_image(3, (3, 150, 212))).to(dev).half()
    plan = ip._plan_for(opt, x.shape)
    ramp = torch.from_numpy(plan.ramp.copy()).to(dev).half()
    model = opt.modelCached
    model.set_option('overlap_calls', 0)
    want = bench._reference_style_loop(opt, x, plan, ramp, torch)
    want_bt = bench._reference_style_loop(opt, x, plan, ramp, torch, blend_tile=ip.blendTile)      # (its own reference: bench's torch loop blends with torch.lerp, moe_blend_tile with the reference's expression)
    model.set_option('overlap_calls', 1)
    for rep in range(2):
        got = bench._reference_style_loop(opt, x, plan, ramp, torch)
        assert torch.equal(got, want)
        got = bench._reference_style_loop(opt, x, plan, ramp, torch, blend_tile=ip.blendTile)
        assert torch.equal(got, want_bt)


def test_overlapped_forwards_keep_their_bits_under_every_split_of_the_workgroups(dev):
    """The group arithmetic of a forward that runs ahead of the caller's stream: its persistent workgroups per launch are half of the chip or option overlap_groups (clamped
    to 16 .. all), and when it forks its U branch as well (overlap_fork) that share is split again between the side stream (branch_groups, or 5/16 of it) and the trunk +
    R branch.  Every kernel's result is independent of its workgroup count, so each tile of the loop must come out with the bits of a plain call on one stream -- under
    the default split, under both options at once and at the floor of the clamp -- and a forward must leave the net as it found it: the next plain call and the
    workspace a shape needs are what they were before the bursts."""
    from moephoto_amd import _lib
    defaults = (('overlap_calls', 1), ('overlap_fork', 0), ('overlap_groups', 0), ('branch_groups', 0), ('branch_streams', 1))
    m = module_for('a4', 'auto')
    img = torch.from_numpy(gd.noise_image(78, (3, 136, 200))).to(dev).half().unsqueeze(1)
    tiles = [(0, 64, 0, 96), (40, 104, 72, 168), (72, 136, 104, 200), (0, 8, 0, 16), (0, 64, 0, 96)]
    try:
        m.set_option('overlap_calls', 0).set_option('branch_streams', 0)
        want = [m(img[..., t:b, l:r])[-1].clone() for (t, b, l, r) in tiles]
        torch.cuda.synchronize()
        ws = _lib.check(_lib.lib().moe_net_workspace_bytes(m._h, 1, 64, 96))
        m.set_option('overlap_calls', 1).set_option('branch_streams', 1)
        for setting in ((('overlap_fork', 1),), (('overlap_fork', 1), ('overlap_groups', 64), ('branch_groups', 16)), (('overlap_fork', 0), ('overlap_groups', 16))):
            for k, v in setting:
                m.set_option(k, v)
            acc, flags = [], []
            for rep in range(3):                                          # one burst: nothing synchronises in between
                for (t, b, l, r) in tiles:
                    y = m(img[..., t:b, l:r])[-1]
                    flags.append(m._last_flag)
                    acc.append(y * 1.0)                                   # consumed on the caller's stream at once; y's memory is reused by the next calls
                    del y
            for i, g in enumerate(acc):
                w = want[i % len(tiles)]
                assert torch.equal(g, w), (setting, i, float((g.float() - w.float()).abs().max()))
            assert flags[1:] == [_lib.FWD_INPUT_SINCE_PREV] * (len(flags) - 1), (setting, flags)
            for k, v in defaults:
                m.set_option(k, v)
        t, b, l, r = tiles[0]
        assert torch.equal(m(img[..., t:b, l:r])[-1], want[0])
        assert _lib.check(_lib.lib().moe_net_workspace_bytes(m._h, 1, 64, 96)) == ws
    finally:
        for k, v in defaults:
            m.set_option(k, v)


def test_forward_takes_part_in_a_hip_graph_capture(dev):
    """A forward is plain stream work: captured into a hipGraph (torch.cuda.CUDAGraph) and replayed on new input data it gives the eager bits -- with the U branch's fork / join
    as event edges inside the capture (branch_streams) and without; the overlap path of moe_net_forward_ex stands aside while its stream captures.  (tools/graph_probe.py:
    replay is not faster than eager launches, 0.816 vs 0.815 ms per 3 x 256 x 256 forward of a4 -- the per-tile loop is bound by the GPU, not by launches.)"""
    for key in ('a4', 'a2'):
        m = module_for(key, 'auto', torch.float16)
        x = torch.from_numpy(gd.natural_image(3, (3, 128, 160))).to(dev).half()[:, None].contiguous()
        x2 = torch.from_numpy(gd.noise_image(4, (3, 128, 160))).to(dev).half()[:, None].contiguous()
        for fork in (1, 0):
            try:
                m.set_option('branch_streams', fork)
                want2 = m(x2)[-1].clone()
                xs = x.clone()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    m(xs)                                      # (workspace grown outside the capture)
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    y = m(xs)[-1]
                xs.copy_(x2)
                g.replay()
                torch.cuda.synchronize()
                assert torch.equal(y, want2), (key, fork, float((y.float() - want2.float()).abs().max()))
            finally:
                m.set_option('branch_streams', 1)


def test_wire_pack_unpack_kernels_vs_numpy_codec(dev):
    """moe_wire_pack / moe_wire_unpack (the 'f16s' wire format of dist.py: fp16 image + fp32 seam rows + fp32 seam columns per tile, strips as plain fp32)
    against tests/wire_codec.py, bit for bit, on the real seams of a plan plus synthetic records (odd sizes, empty ranges, one-range seams, a strip), and the
    canvas folded from unpacked tiles against the one folded from the fp32 tiles (fp16: same bits)."""
    import ctypes
    import wire_codec
    from moephoto_amd import _lib, dist as mdist, imageProcess as ip
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    opt = _opt_sr('a', 2, 64, fp16_io=True)
    xd = torch.from_numpy(gd.natural_image(9, (3, 150, 200))).to(dev).half()
    plan = ip._plan_for(opt, xd.shape)
    seams = plan.seams()
    dims = [(3, (t[1] - t[0]) * 2, (t[3] - t[2]) * 2) for t in plan.tiles]
    items = [(d, s) for d, s in zip(dims, seams)]
    items += [((1, 7, 13), (0, 2, 5, 7, 0, 0, 0, 0)), ((2, 5, 3), (0, 0, 0, 0, 1, 2, 2, 2)), ((3, 10, 24), (0, 10, 10, 10, 0, 0, 0, 0)), ((1, 1, 1), (0, 0, 0, 0, 0, 0, 0, 0)),
              ((2, 9, 31), (3, 4, 4, 4, 0, 5, 30, 31))]
    recs = np.zeros(len(items), mdist.WIRE_REC)
    off = wpos = 0
    for n, (d, s) in enumerate(items):
        recs[n] = (off, wpos) + tuple(d) + tuple(s) + (0,)
        assert mdist.wire_words(recs[n]) == L.moe_wire_words(recs[n:n + 1].ctypes.data)
        off += d[0] * d[1] * d[2]
        wpos += mdist.wire_words(recs[n])
    rng = np.random.default_rng(5)
    buf = (rng.standard_normal(off) * 0.8).astype(np.float32)
    buf[::97] *= 1e5                                                       # (beyond fp16: inf in the fp16 image, exact in the seams)
    want_wire = np.zeros(wpos, np.int32)
    wire_codec.codec(True, buf, want_wire, recs)
    want_back = np.full(off, np.nan, np.float32)
    wire_codec.codec(False, want_back, want_wire, recs)
    bd = torch.from_numpy(buf).to(dev)
    rd = torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
    wd = torch.zeros(wpos, dtype=torch.int32, device=dev)
    big = max(d[0] * d[1] * d[2] for d, _ in items)
    _lib.check(L.moe_wire_pack(bd.data_ptr(), wd.data_ptr(), rd.data_ptr(), len(items), big, stream))
    # compare only the words the format defines (the column area's entries inside seam rows are never written)
    back = torch.full((off,), float('nan'), dtype=torch.float32, device=dev)
    _lib.check(L.moe_wire_unpack(back.data_ptr(), wd.data_ptr(), rd.data_ptr(), len(items), big, stream))
    torch.cuda.synchronize()
    got_back = back.cpu().numpy()
    assert np.array_equal(got_back, want_back, equal_nan=True)
    got_wire = wd.cpu().numpy()
    chk = np.full(off, np.nan, np.float32)
    wire_codec.codec(False, chk, got_wire, recs)                           # the device's wire decodes, with the CPU codec, to the same tiles
    assert np.array_equal(chk, want_back, equal_nan=True)
    # the fold of a real frame: fp32 tiles -> pack -> unpack -> stitch == stitch of the fp32 tiles, as fp16
    pool = torch.empty(plan.pool_elems(3), dtype=torch.float32, device=dev)
    canvas = torch.empty((3, plan.outH, plan.outW), dtype=torch.float16, device=dev)
    sC, sH, sW = xd.stride()
    _lib.check(L.moe_run_plan_ex(opt.modelCached._h, plan._h, xd.data_ptr(), _lib.F16, sC, sH, sW, canvas.data_ptr(), _lib.F16, 0, ctypes.c_void_p(pool.data_ptr()), 0, 1, 1, stream))
    offs = plan.tile_offsets(3)
    recs2 = np.zeros(plan.n_tiles, mdist.WIRE_REC)
    wpos = 0
    for k in range(plan.n_tiles):
        recs2[k] = (offs[k], wpos) + dims[k] + tuple(seams[k]) + (0,)
        wpos += mdist.wire_words(recs2[k])
    assert wpos * 4 < 0.85 * pool.numel() * 4
    rd2 = torch.from_numpy(recs2.view(np.uint8).reshape(-1).copy()).to(dev)
    wd2 = torch.empty(wpos, dtype=torch.int32, device=dev)
    pool2 = torch.full_like(pool, float('nan'))
    big = max(d[0] * d[1] * d[2] for d in dims)
    _lib.check(L.moe_wire_pack(pool.data_ptr(), wd2.data_ptr(), rd2.data_ptr(), plan.n_tiles, big, stream))
    _lib.check(L.moe_wire_unpack(pool2.data_ptr(), wd2.data_ptr(), rd2.data_ptr(), plan.n_tiles, big, stream))
    tab = torch.tensor(offs, dtype=torch.int64, device=dev)
    canvas2 = torch.empty_like(canvas)
    _lib.check(L.moe_stitch_dev(plan._h, 0, pool2.data_ptr(), ctypes.c_void_p(tab.data_ptr()), 3, canvas2.data_ptr(), _lib.F16, stream))
    torch.cuda.synchronize()
    assert not torch.equal(pool2, pool) and torch.equal(canvas2, canvas)


def test_io_edges_vector_and_element_forms_agree(dev):
    """moe_to_float / moe_to_output (toTorch / toOutput, python/imageProcess.py:245-263): three-channel images whose pixel count is a multiple of 8 take the
    eight-pixels-per-thread kernels, everything else the per-element ones.  Both against the oracle's edges, bit for bit, for uint8 / uint16 against fp16 /
    fp32, with NaN, negative, > 1 and exactly-on-a-level values on the way out."""
    from moephoto_amd import _lib
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(11)
    for (H, W, C) in ((64, 40, 3), (7, 9, 3), (16, 24, 1), (33, 8, 3), (5, 8, 4)):
        for bits, np_t, lib_t in ((8, np.uint8, _lib.U8), (16, np.uint16, _lib.U16), (10, np.uint16, _lib.U16)):
            img = rng.integers(0, 1 << bits, (H, W, C)).astype(np_t)
            want = oio.to_float_image(img, bits)
            src = torch.from_numpy(img.view(np.int16) if np_t is np.uint16 else img).to(dev)
            for dt, ldt in ((torch.float32, _lib.F32), (torch.float16, _lib.F16)):
                dst = torch.full((C, H, W), float('nan'), dtype=dt, device=dev)
                _lib.check(L.moe_to_float(src.data_ptr(), lib_t, bits, H, W, C, dst.data_ptr(), ldt, 0, stream))
                w = torch.from_numpy(want).to(dt)
                assert torch.equal(dst.cpu(), w), (H, W, C, bits, dt)
            y = (rng.standard_normal((C, H, W)) * 0.6 + 0.5).astype(np.float32)
            y.reshape(-1)[::13] = np.nan
            y.reshape(-1)[1::17] = np.float32(37) / np.float32(1 << min(bits, 8))
            for dt, ldt in ((torch.float32, _lib.F32), (torch.float16, _lib.F16)):
                yd = torch.from_numpy(y).to(dev).to(dt)
                out = torch.zeros((H, W, C), dtype=torch.uint8 if bits <= 8 else torch.int16, device=dev)
                _lib.check(L.moe_to_output(yd.data_ptr(), ldt, H, W, C, bits, out.data_ptr(), lib_t, 0, stream))
                got = out.cpu().numpy()
                got = got.view(np.uint16) if bits > 8 else got
                yy = yd.float().cpu().numpy()
                q = np.float32(1 << bits)
                with np.errstate(invalid='ignore'):
                    ref = np.clip(yy * q, 0, q - 1)
                ref = np.where(np.isnan(ref), 0, ref).astype(np.int64).transpose(1, 2, 0)
                assert np.array_equal(got.astype(np.int64), ref), (H, W, C, bits, dt)


@pytest.mark.parametrize('key,blocks', [('a2', -1), ('a4', -1), ('a3', -1), ('a2', 6)])
def test_streamed_split_operand_layers_vs_patch_form(key, blocks, dev):
    """Option q8_impl = s (default; conv64_sq.hip): the chain layers of conv64_q8.hip -- same operands, products and scales -- streamed down 32-pixel columns
    by two-wave workgroups.  One accumulator set in both forms, a different order of the sums inside a row: the tensors between the layers agree to fp32
    rounding, and the fp8 low words they travel in turn that into a few 1e-5 .. 1e-4 at the output.  So: both forms inside the tolerance against the ORACLE,
    natural and noise, ragged shapes (odd widths, two-row tiles, heights the kernel does not take: odd ones fall back to the patch form); the streamed form
    repeats bit for bit, and its bits do not depend on the workgroup count (rows at range ends are recomputed, not approximated)."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    try:
        m.set_exact_blocks(blocks)
        for shape in ((3, 8, 8), (2, 24, 40), (2, 40, 264), (3, 16, 72), (1, 88, 64), (1, 6, 33), (2, 2, 40), (1, 9, 35)):
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(41, shape) if kind == 'natural' else gd.noise_image(41, shape))[:, None]
                want = onets.forward(arch, sd, x).numpy()
                xd = torch.from_numpy(x).to(dev)
                y_p = m.set_option('q8_impl', 'p')(xd)[-1].cpu().numpy()
                y_s = m.set_option('q8_impl', 's')(xd)[-1].cpu().numpy()
                assert np.isfinite(y_s).all(), (key, shape, kind)
                assert np.abs(y_s - want).max() <= TOL and np.abs(y_p - want).max() <= TOL, (key, shape, kind, float(np.abs(y_s - want).max()), float(np.abs(y_p - want).max()))
                assert np.abs(y_s - y_p).max() <= 7e-4, (key, shape, kind, float(np.abs(y_s - y_p).max()))
                assert np.array_equal(y_s, m(xd)[-1].cpu().numpy()), (key, shape, kind)
                y_g = m.set_option('max_groups', 5)(xd)[-1].cpu().numpy()
                m.set_option('max_groups', 0)
                assert np.array_equal(y_s, y_g), (key, shape, kind)
    finally:
        m.set_option('q8_impl', 's')
        m.set_exact_blocks(-1)


def test_a2_noise_full_tile_vs_oracle(dev):
    """A full 256 x 256 tile of uniform uint8 noise -- the input class with the least margin -- through a2 in the default arithmetic (nine split-operand layers
    on the streamed form, fp8 low words between them) against the ORACLE's fp32 forward, not only against the exact mode."""
    sd = gd.state_dict_for('a2', load_state_dict_file)
    m = module_for('a2')
    for seed in (0, 1):
        x = (gd.noise_u8(seed, (1, 256, 256)).astype(np.float32) / 255.0)[:, None]
        want = onets.forward('net2x', sd, x).numpy()
        got = m(torch.from_numpy(x).to(dev))[-1].cpu().numpy()
        err = float(np.abs(got - want).max())
        assert err <= TOL, (seed, err)


@pytest.mark.parametrize('key,blocks', [('a2', -1), ('a4', -1), ('a3', -1), ('a2', 6), ('a4', 3)])
def test_fused_exact_arsb_is_bit_identical_to_the_two_launch_form(key, blocks, dev):
    """Option exact_fuse (default on; arsb_sq.hip): an exact ARSB of the chain in ONE launch -- producer waves run conv_1 on the x rings and leave its rows (fp16,
    fp8 low word, fp8 image) in LDS, consumer waves run conv_2 on them and take the residual from the x rings.  Per conv the same MFMAs in the same order as
    conv64_sq.hip, the same epilogue arithmetic, and m crosses as the very (fp16, fp8 word) pair the two-launch form stores: the outputs must be the SAME BITS,
    on every shape (30-pixel columns against 32, ragged widths, two-row tiles), whatever the workgroup count -- and within the tolerance of the oracle."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    try:
        m.set_exact_blocks(blocks)
        for shape in ((3, 8, 8), (2, 24, 40), (2, 40, 264), (3, 16, 72), (1, 88, 64), (1, 6, 33), (2, 2, 40), (1, 64, 30), (1, 32, 61)):
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(43, shape) if kind == 'natural' else gd.noise_image(43, shape))[:, None]
                xd = torch.from_numpy(x).to(dev)
                y0 = m.set_option('exact_fuse', 0)(xd)[-1].cpu().numpy()
                y1 = m.set_option('exact_fuse', 1)(xd)[-1].cpu().numpy()
                assert np.array_equal(y1, y0), (key, shape, kind, float(np.abs(y1 - y0).max()))
                assert np.array_equal(y1, m(xd)[-1].cpu().numpy()), (key, shape, kind)
                y_g = m.set_option('max_groups', 3)(xd)[-1].cpu().numpy()
                m.set_option('max_groups', 0)
                assert np.array_equal(y1, y_g), (key, shape, kind)
                want = onets.forward(arch, sd, x).numpy()
                assert np.abs(y1 - want).max() <= TOL, (key, shape, kind, float(np.abs(y1 - want).max()))
    finally:
        m.set_option('exact_fuse', 1)
        m.set_exact_blocks(-1)


def test_sedn_block_tail_streamed_vs_patch_form(dev, key='l25'):
    """Option s64 (default on; conv64_s.hip): SEDN's fused block tail -- y = x + LeakyReLU(conv(W_eff[b], t)) with PER-PLANE weights -- streamed down 32-pixel columns with
    the plane's 36 A fragments in registers (reloaded where a range enters another plane), instead of conv3x3_sp<6>'s weights in LDS.  Same arithmetic (LeakyReLU in fp32, the
    residual added in fp32, one rounding), another order of the sums inside a row: both forms within the tolerance of the ORACLE on natural and noise inputs, ragged shapes,
    several planes per launch (each with its own weights); the streamed form repeats bit for bit."""
    arch = gd.MODELS[key][0]
    sd = gd.state_dict_for(key, load_state_dict_file)
    m = module_for(key)
    try:
        for shape in ((3, 8, 8), (2, 24, 40), (2, 40, 264), (3, 16, 72), (1, 88, 64), (1, 6, 33), (2, 2, 40), (5, 32, 30)):
            for kind in ('natural', 'noise'):
                x = (gd.natural_image(47, shape) if kind == 'natural' else gd.noise_image(47, shape))[:, None]
                xd = torch.from_numpy(x).to(dev)
                want = onets.forward(arch, sd, x).numpy()
                y0 = m.set_option('s64', 0)(xd)[-1].cpu().numpy()
                y1 = m.set_option('s64', 1)(xd)[-1].cpu().numpy()
                assert np.isfinite(y1).all(), (key, shape, kind)
                assert np.abs(y1 - want).max() <= TOL and np.abs(y0 - want).max() <= TOL, (key, shape, kind, float(np.abs(y1 - want).max()), float(np.abs(y0 - want).max()))
                assert np.abs(y1 - y0).max() <= 8e-4, (key, shape, kind, float(np.abs(y1 - y0).max()))
                assert np.array_equal(y1, m(xd)[-1].cpu().numpy()), (key, shape, kind)
    finally:
        m.set_option('s64', 1)
