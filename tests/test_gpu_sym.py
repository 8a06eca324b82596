"""The SR self-ensemble on the device (moephoto_amd/csrc/sym.hip, moe_run_plan_ens) against the torch expressions it replaces, BIT FOR BIT:

    moe_sym_pad        padImage(trans[s](x))                    (python/imageProcess.py:570 + getPad, :47-56)
    moe_sym_fold       v + transInv[s](t), then / d             (python/imageProcess.py:571, runSR.py:26)
    moe_run_plan_ens   runSR.sr(opt)(x) with config.ensembleOnDevice = False

Nothing here has a tolerance: both kernels move values or add two of them with one rounding, so equality of the bits is the only bound there is.
Needs a HIP device: `pytest -m gpu`."""
import ctypes
import types

import numpy as np
import pytest
import torch

import golden_defs as gd
from moephoto_amd import _lib

pytestmark = pytest.mark.gpu
DT = {torch.float16: _lib.F16, torch.float32: _lib.F32}
BITS = {torch.float16: torch.int16, torch.float32: torch.int32}
# (C, H, W) on the kernels' edges: one element; odd sizes; one past / one short of the 64 x 64 LDS tile in each direction; the vector width exactly
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 64, 65), (1, 63, 129), (1, 130, 8)]
GUARD = 64        # elements in front of and behind every destination (a multiple of 16 bytes: the destination keeps its alignment)


@pytest.fixture(scope='module')
def dev():
    _lib.require_device()
    return torch.device('cuda:0')


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))


def rand(shape, dtype, dev, seed, offset=0):
    """uniform values in [-1, 2) as a contiguous tensor; offset = 1: a view that starts one element into its buffer (no 16-byte alignment: the scalar path)"""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    buf = torch.empty(n + offset, dtype=dtype, device=dev)
    buf[offset:] = (torch.rand(n, generator=g) * 3 - 1).to(dtype).to(dev)
    return buf[offset:].view(shape)


def guarded(shape, dtype, dev, offset=0, fill=None):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + offset,), 777.0, dtype=dtype, device=dev)
    t = buf[GUARD + offset:GUARD + offset + n].view(shape)
    if fill is not None:
        t.copy_(fill)
    return buf, t


def guards_intact(buf, t):
    n = t.numel()
    off = t.storage_offset()
    return bool((buf[:off] == 777.0).all()) and bool((buf[off + n:] == 777.0).all())


def transformed(shape, s):
    C, H, W = shape
    return (W, H) if s in (0, 3, 4, 6) else (H, W)


def sym_pad(x, s, Hp, Wp, offset=0):
    C, H, W = x.shape
    buf, dst = guarded((C, Hp, Wp), x.dtype, x.device, offset)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _lib.check(_lib.lib().moe_sym_pad(x.data_ptr(), DT[x.dtype], C, H, W, x.stride(0), x.stride(1), x.stride(2), s, dst.data_ptr(), Hp, Wp, 0, stream))
    assert guards_intact(buf, dst), 'moe_sym_pad wrote outside its destination'
    return dst


def want_pad(x, s, Hp, Wp):
    from moephoto_amd import imageProcess as ip
    return ip.TilePlan.padImage(types.SimpleNamespace(padHTo=Hp, padWTo=Wp), ip.trans[s](x)).contiguous()


def sym_fold(acc, t, s, d, offset=0):
    C, H, W = acc.shape
    buf, a = guarded((C, H, W), acc.dtype, acc.device, offset, fill=acc)
    stream = torch.cuda.current_stream(acc.device).cuda_stream
    _lib.check(_lib.lib().moe_sym_fold(a.data_ptr(), t.data_ptr(), DT[acc.dtype], C, H, W, s, d, 0, stream))
    assert guards_intact(buf, a), 'moe_sym_fold wrote outside its canvas'
    return a


def want_fold(acc, t, s, d):
    from moephoto_amd import imageProcess as ip
    v = acc + ip.transInv[s](t)
    return v / d if d > 1 else v


# ---- the kernels alone ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['f16', 'f32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sym_pad_every_symmetry(shape, dtype, dev):
    """No padding (a pure transform), and a padding with rows AND columns of both kinds (reflection as far as the axis allows, zeros behind it), once to an
    unaligned width and once to a multiple of the vector width."""
    x = rand(shape, dtype, dev, 11)
    for s in range(7):
        Ht, Wt = transformed(shape, s)
        for Hp, Wp in ((Ht, Wt), (Ht + 7, Wt + 9), (Ht + 7, (Wt + 9 + 7) // 8 * 8)):
            assert same_bits(sym_pad(x, s, Hp, Wp), want_pad(x, s, Hp, Wp)), (s, Hp, Wp)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['f16', 'f32'])
def test_sym_pad_reflection_zeros_and_strided_sources(dtype, dev):
    for s in range(7):
        t = s in (0, 3, 4, 6)
        # pure reflection: the transformed image is 37 x 52, W = 52 -> Wp = 56, rows as they are
        x = rand((3, 52, 37) if t else (3, 37, 52), dtype, dev, 5)
        assert same_bits(sym_pad(x, s, 37, 56), want_pad(x, s, 37, 56)), s
        # reflection plus zeros on both axes: 2 x 3 -> 8 x 8 (one / two reflected samples, then zeros)
        x = rand((2, 3, 2) if t else (2, 2, 3), dtype, dev, 6)
        got = sym_pad(x, s, 8, 8)
        assert same_bits(got, want_pad(x, s, 8, 8)), s
        assert bool((got[:, 3:, :] == 0).all()) and bool((got[:, :, 5:] == 0).all())
        # a source that is not contiguous: a channel, row and column window of a larger tensor, and every second column of one
        big = rand((5, 70, 140), dtype, dev, 7)
        for src in (big[1:4, 2:66, 8:73], big[::2, 3:40, 1:130:2], big[1:3, :, :136]):
            C, H, W = src.shape
            Ht, Wt = (W, H) if t else (H, W)
            Hp, Wp = Ht + 3, (Wt + 7) // 8 * 8
            assert same_bits(sym_pad(src, s, Hp, Wp), want_pad(src, s, Hp, Wp)), (s, tuple(src.shape))


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['f16', 'f32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sym_fold_every_symmetry(shape, dtype, dev):
    acc = rand(shape, dtype, dev, 21)
    for s in range(7):
        Ht, Wt = transformed(shape, s)
        t = rand((shape[0], Ht, Wt), dtype, dev, 22 + s)
        for d in (0, 3):
            assert same_bits(sym_fold(acc, t, s, d), want_fold(acc, t, s, d)), (s, d)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['f16', 'f32'])
def test_sym_kernels_on_views_one_element_into_their_buffers(dtype, dev):
    """Nothing is 16-byte aligned: the scalar path of both kernels, same bits."""
    shape = (2, 64, 72)
    for s in range(7):
        Ht, Wt = transformed(shape, s)
        x = rand(shape, dtype, dev, 31, offset=1)
        assert same_bits(sym_pad(x, s, Ht + 8, Wt + 8, offset=1), want_pad(x, s, Ht + 8, Wt + 8)), s
        acc, t = rand(shape, dtype, dev, 32, offset=1), rand((2, Ht, Wt), dtype, dev, 33, offset=1)
        assert same_bits(sym_fold(acc, t, s, 5, offset=1), want_fold(acc, t, s, 5)), s


def _ties(dtype, dev):
    """(acc, addend) whose exact sums lie half way between two neighbours of the dtype: p = 11 bits (fp16) / 24 bits (fp32); in [2^p, 2^(p+1)) the spacing is 2, so
    even + odd is a tie; in [2^(p-1), 2^p) it is 1 and .5 makes one.  Both signs, both directions of the even neighbour."""
    p = 11 if dtype == torch.float16 else 24
    k = torch.arange(1, 1017, dtype=torch.float64)      # (1016 = 8 x 127 columns: 2^p - 1 and 2^(p+1) + 1 are no ties)
    hi, lo = 2.0 ** p + 2 * k, 2.0 ** (p - 1) + k
    rows = [(hi, 1.0), (hi, -1.0), (hi, 3.0), (-hi, 1.0), (lo, 0.5), (lo, -0.5), (-lo, 0.5), (lo, 1.5)]
    acc = torch.stack([a for a, _ in rows])[None]
    add = torch.stack([torch.full_like(a, b) for a, b in rows])[None]
    acc, add = acc.to(dtype).to(dev), add.to(dtype).to(dev)
    assert bool((acc.double() + add.double() != (acc + add).double()).all())      # every sum is inexact in the dtype: a rounding decides it
    return acc, add


def _all_values(dtype, dev):
    """fp16: every finite bit pattern, as (2 signs, 128, 248); fp32: the integers 1 .. 2 x 128 x 248 scaled by a non-power of two -- quotients by 3, 5, 6, 7 whose
    fp32 division and multiplication by the fp32 reciprocal differ in the last bit are a large share of them"""
    if dtype == torch.float16:
        mag = torch.arange(0x7C00, dtype=torch.int32)
        bits = torch.stack([mag, mag + 0x8000]).to(torch.int32)
        return (bits - (bits >= 0x8000).int() * 0x10000).to(torch.int16).view(torch.float16).view(2, 128, 248).to(dev)
    return (torch.arange(1, 2 * 128 * 248 + 1, dtype=torch.float32) * 0.37).view(2, 128, 248).to(dev)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['f16', 'f32'])
@pytest.mark.parametrize('d', range(2, 9))
def test_sym_fold_final_division_matches_torch(d, dtype, dev):
    """The closing / (n + 1) inside the last fold, for every divisor the ensemble can have: on random data, on sums that land on rounding ties (the sum is rounded
    once, to even, BEFORE it is divided) and on every fp16 value as the sum (a division and a multiplication by the fp32 reciprocal differ for 3, 5, 6, 7 on many of
    them: whichever torch's device kernel does is what the fold must do)."""
    from moephoto_amd import imageProcess as ip
    for s in (0, 1, 6):       # a transposing symmetry, a flip, both
        acc = rand((3, 40, 72), dtype, dev, 40 + d)
        t = rand((3,) + transformed((3, 40, 72), s), dtype, dev, 50 + d)
        assert same_bits(sym_fold(acc, t, s, d), want_fold(acc, t, s, d)), ('random', s)
        acc, add = _ties(dtype, dev)
        t = ip.trans[s](add).contiguous()                       # transInv[s](t) is the addend
        assert same_bits(sym_fold(acc, t, s, 0), want_fold(acc, t, s, 0)), ('ties, sum alone', s)
        assert same_bits(sym_fold(acc, t, s, d), want_fold(acc, t, s, d)), ('ties', s)
        acc = _all_values(dtype, dev)
        t = torch.zeros((2,) + transformed((2, 128, 248), s), dtype=dtype, device=dev)
        got, want = sym_fold(acc, t, s, d), want_fold(acc, t, s, d)
        bad = (got.view(BITS[dtype]) != want.view(BITS[dtype])).sum().item()
        assert bad == 0, ('all values', s, '{} of {} quotients differ from torch'.format(bad, got.numel()))


# ---- end to end: sr(opt)(x) with the switch on against the same call with it off ----------------------------------------------------------------------------
IMAGES = {'37x52': (3, 37, 52), '52x37': (3, 52, 37), '20x20': (3, 20, 20)}      # several tiles on one axis and one on the other (each plan pads one axis, the
                                                                                  # transposed plan the other one); a single tile with both axes padded


@pytest.fixture(scope='module')
def a2(dev):
    """runSR's Option for model a2 (real weights: tests/golden/zoo), cropsize 48; the configuration is put back afterwards"""
    from moephoto_amd import imageProcess as ip, runSR
    from moephoto_amd.config import config
    keep = (config.modelRoot, config.crop_sr, config.fp16, config.deviceId, config.ensembleOnDevice)
    config.modelRoot, config.crop_sr, config.fp16, config.deviceId = gd.ZOO, 48, False, 0
    ip.modelCache.pop('SRa2', None)
    opt = runSR.getOpt({'op': 'SR', 'model': 'a', 'scale': 2, 'ensemble': 1})
    yield opt
    ip.modelCache.pop('SRa2', None)
    config.modelRoot, config.crop_sr, config.fp16, config.deviceId, config.ensembleOnDevice = keep


def image(name, dtype, dev):
    return torch.from_numpy(gd.natural_image(101, IMAGES[name])).to(dtype).to(dev)


def run_sr(opt, x, n, on_device):
    from moephoto_amd import runSR
    from moephoto_amd.config import config
    opt.ensemble = n
    config.ensembleOnDevice = on_device
    try:
        y = runSR.sr(opt)(x)
        torch.cuda.synchronize()
        return y
    finally:
        config.ensembleOnDevice = True


_torch_path = {}


def torch_path(opt, name, n, dtype, dev):
    """the reference result of a case, computed once and shared"""
    key = (name, n, dtype)
    if key not in _torch_path:
        _torch_path[key] = run_sr(opt, image(name, dtype, dev), n, False)
    return _torch_path[key]


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['f16', 'f32'])
@pytest.mark.parametrize('n', [1, 3, 7])
@pytest.mark.parametrize('name', sorted(IMAGES))
def test_sr_ensemble_on_device_equals_the_torch_path(name, n, dtype, a2, dev):
    x = image(name, dtype, dev)
    got, want = run_sr(a2, x, n, True), torch_path(a2, name, n, dtype, dev)
    C, H, W = IMAGES[name]
    assert tuple(got.shape) == (C, 2 * H, 2 * W) and got.dtype == dtype
    assert same_bits(got, want)
    assert float(want.float().abs().max()) > 0.1          # (a picture, not zeros)


def test_ensemble_without_average_and_ensemble_zero(a2, dev):
    """imageProcess.ensemble(opt) alone is still the SUM whatever the switch says (the device path's last fold averages: it serves sr), sr is that sum / (n + 1), and
    ensemble = 0 is doCrop"""
    from moephoto_amd import imageProcess as ip
    from moephoto_amd.config import config
    x = image('37x52', torch.float16, dev)
    a2.ensemble = 3
    try:
        config.ensembleOnDevice = False
        want = ip.ensemble(a2)(x)
        config.ensembleOnDevice = True
        assert same_bits(ip.ensemble(a2)(x), want)
    finally:
        config.ensembleOnDevice = True
    assert same_bits(run_sr(a2, x, 3, True), want / 4)
    assert same_bits(run_sr(a2, x, 0, True), run_sr(a2, x, 0, False)) and same_bits(run_sr(a2, x, 0, True), ip.doCrop(a2, x))


def test_run_plan_ens_through_ctypes_equals_python(a2, dev):
    """A caller that never sees this package's Python: plans from moe_plan_create, one call."""
    from moephoto_amd import imageProcess as ip
    from moephoto_amd.config import config
    L = _lib.lib()
    name, n, dtype = '37x52', 3, torch.float16
    x = image(name, dtype, dev)
    want = run_sr(a2, x, n, True)
    C, H, W = IMAGES[name]
    ram = min(config.calcFreeMem(), a2.modelCached.max_tile_pixels() * C * C / a2.ramCoef)
    plans = []
    for shape in ((C, H, W), (C, W, H)):
        h = ctypes.c_void_p()
        _lib.check(L.moe_plan_create((ctypes.c_int64 * 3)(*shape), float(ram), float(a2.ramCoef), int(a2.padding), 2, int(a2.align), 48, ctypes.byref(h)))
        plans.append(h)
    try:
        info = (ctypes.c_int64 * 12)()
        _lib.check(L.moe_plan_info(plans[0], info))
        assert (int(info[3]), int(info[4])) == (2 * H, 2 * W)
        out = torch.empty((C, 2 * H, 2 * W), dtype=dtype, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.moe_run_plan_ens(a2.modelCached._h, plans[0], plans[1], n, x.data_ptr(), DT[dtype], x.stride(0), x.stride(1), x.stride(2),
                                      out.data_ptr(), DT[dtype], 0, stream))
        torch.cuda.synchronize()
        assert same_bits(out, want)
    finally:
        torch.cuda.synchronize()
        for h in plans:
            L.moe_plan_destroy(h)


def test_scratch_growth_keeps_the_bits(a2, dev):
    """The net's two scratch buffers only grow: a larger image after a small one reallocates them, and the small one afterwards runs in the larger buffers."""
    small, large = image('20x20', torch.float32, dev), torch.from_numpy(gd.natural_image(7, (3, 70, 90))).to(dev)
    first = run_sr(a2, small, 7, True)
    big = run_sr(a2, large, 7, True)
    again = run_sr(a2, small, 7, True)
    assert same_bits(first, again) and same_bits(first, torch_path(a2, '20x20', 7, torch.float32, dev))
    assert same_bits(big, run_sr(a2, large, 7, False))
