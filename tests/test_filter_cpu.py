"""The DN step's device edge without a device (include/moephoto_amd.h: moe_stitch_mix, moe_run_plan_filter; moephoto_amd/imageProcess.py: _RGBFilter, filterOut): the
symbols, what the entry points refuse before anything touches a device, when _RGBFilter keeps to the torch expressions, and the arithmetic of the blend written out
rounding by rounding in numpy against torch's own evaluation of `s * x + (1 - s) * inp`."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from moephoto_amd import _lib, imageProcess as ip
from moephoto_amd.config import config
from moephoto_amd.models import EngineModule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('moe_stitch_mix', 'moe_run_plan_filter')


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    dyn = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    L = _lib.lib()
    for name in NEW:
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr), name
        assert name in _lib.EXPORTS
        assert re.search(r'\sT\s+' + name + r'\s*$', dyn, re.M), name
        assert getattr(L, name).argtypes is not None
    assert L.moe_abi_version() == _lib.ABI_VERSION == 4          # additions only


def _mix(L, plan, p, **kw):
    """moe_stitch_mix on a 3-plane fp32 canvas form with every argument valid, then `kw` over them."""
    a = dict(plan=plan._h if plan is not None else None, tiles=p, C=3, inp=p, inp_dtype=_lib.F32, alpha=None, strength=0.6, bits=0, dst=p, dst_dtype=_lib.F32)
    a.update(kw)
    return L.moe_stitch_mix(a['plan'], 0, a['tiles'], None, a['C'], a['inp'], a['inp_dtype'], 140 * 100, 140, 1, a['alpha'], 140, 1,
                            a['strength'], a['bits'], a['dst'], a['dst_dtype'], None)


def _filter(L, net, plan, p, **kw):
    a = dict(net=net, plan=plan._h if plan is not None else None, img=p, img_dtype=_lib.F32, alpha=None, strength=0.6, bits=0, dst=p, dst_dtype=_lib.F32)
    a.update(kw)
    return L.moe_run_plan_filter(a['net'], a['plan'], a['img'], a['img_dtype'], 140 * 100, 140, 1, a['alpha'], 140, 1, a['strength'], a['bits'],
                                 a['dst'], a['dst_dtype'], 0, None)


REFUSALS = [(dict(inp=None), b'NULL'), (dict(dst=None), b'NULL'), (dict(bits=12, dst_dtype=_lib.U16), b'bits'), (dict(bits=4, dst_dtype=_lib.U8), b'bits'),
            (dict(bits=0, dst_dtype=_lib.F16), b'dst dtype'), (dict(bits=0, dst_dtype=_lib.U8), b'dst dtype'), (dict(bits=8, dst_dtype=_lib.F32), b'dst dtype'),
            (dict(bits=16, dst_dtype=_lib.U8), b'MOE_U8'), (dict(inp_dtype=_lib.U8, dst_dtype=_lib.U8), b'canvas dtype'),
            (dict(strength=float('nan')), b'strength'), (dict(strength=float('inf')), b'strength'), (dict(strength=float('-inf')), b'strength')]


def test_filter_entry_points_validate_their_arguments_without_a_device():
    L = _lib.lib()
    plan = ip.TilePlan((3, 100, 140), 1 << 40, 1e-3, 7, 1, 8, 48)
    plan2 = ip.TilePlan((3, 100, 140), 1 << 40, 1e-3, 5, 2, 8, 48)
    plan4 = ip.TilePlan((4, 100, 140), 1 << 40, 1e-3, 7, 1, 8, 48)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert _mix(L, None, p) == _lib.EINVAL and b'NULL' in L.moe_last_error()
    assert _mix(L, plan, p, tiles=None) == _lib.EINVAL and b'NULL' in L.moe_last_error()
    for kw, msg in REFUSALS:
        assert _mix(L, plan, p, **kw) == _lib.EINVAL, kw
        err = L.moe_last_error()
        assert msg in err and b'moe_stitch_mix' in err, (kw, err)
    assert _mix(L, plan2, p) == _lib.EINVAL and b'scale' in L.moe_last_error()
    for kw in (dict(C=0), dict(C=5), dict(C=4, alpha=p), dict(C=-1)):
        assert _mix(L, plan, p, **kw) == _lib.EINVAL and b'planes' in L.moe_last_error(), kw
    h = ctypes.c_void_p()
    _lib.check(L.moe_net_create(_lib.ARCH_NETDN, 1, ctypes.byref(h)))
    try:
        assert _filter(L, None, plan, p) == _lib.EINVAL and b'NULL' in L.moe_last_error()
        assert _filter(L, h, None, p) == _lib.EINVAL and b'NULL' in L.moe_last_error()
        assert _filter(L, h, plan, p, img=None) == _lib.EINVAL and b'NULL' in L.moe_last_error()
        for kw, msg in REFUSALS:
            if 'inp' in kw:
                continue
            kw = {dict(inp_dtype='img_dtype').get(k, k): v for k, v in kw.items()}
            assert _filter(L, h, plan, p, **kw) == _lib.EINVAL, kw
            err = L.moe_last_error()
            assert msg in err and b'moe_run_plan_filter' in err, (kw, err)
        assert _filter(L, h, plan2, p) == _lib.EINVAL and b'scale' in L.moe_last_error()
        assert _filter(L, h, plan4, p, alpha=p) == _lib.EINVAL and b'planes' in L.moe_last_error()      # four planes and alpha
        # every argument in order: the unfinalized net is what is left to refuse, canvas form and sample form alike
        assert _filter(L, h, plan, p) == _lib.ESTATE and b'moe_run_plan_filter: net is not finalized' in L.moe_last_error()
        assert _filter(L, h, plan, p, alpha=p, strength=1.0, bits=16, dst_dtype=_lib.U16) == _lib.ESTATE
        assert _filter(L, h, plan4, p, strength=0.0, bits=8, dst_dtype=_lib.U8) == _lib.ESTATE
    finally:
        L.moe_net_destroy(h)


# ---- _RGBFilter: when the torch expressions run ------------------------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """A CPU tensor that says it lives on a HIP device: what _RGBFilter's choice looks at, on a machine without one."""
    @property
    def device(self):
        return torch.device('cuda:0')


def _stub_opt(strength):
    opt = ip.Option()
    opt.modelCached = EngineModule.__new__(EngineModule)      # an engine model by type; it owns no net
    opt.strength = strength
    return opt


def test_rgbfilter_keeps_to_torch_when_there_is_nothing_to_fuse(monkeypatch):
    calls = []
    monkeypatch.setattr(ip, '_runPlan', lambda who, opt, x, *a, **kw: calls.append((who, kw.get('mix'))) or 'fused')
    monkeypatch.setattr(ip, 'doCrop', lambda opt, x, *a, **kw: torch.Tensor(x) * 0.5)
    lib_calls = []
    monkeypatch.setattr(_lib, 'lib', lambda: lib_calls.append(1) or None)
    base = torch.arange(4 * 6 * 8, dtype=torch.float32).reshape(4, 6, 8) / 64
    rgb, rgba = base[:3].as_subclass(_OnDevice), base.as_subclass(_OnDevice)
    want = lambda s, im: ip.mergeAlpha({'im': im[3]} if im.shape[0] == 4 else {})(ip.strengthOp(im[:3] * 0.5, im[:3], s))
    assert config.filterOnDevice is True
    try:
        # the positive control: with the flag on these reach the fused call
        assert ip._RGBFilter(_stub_opt(0.6), rgb) == 'fused' and calls[-1][0] == 'RGBFilter' and calls[-1][1][0] == 0.6 and calls[-1][1][1] is None
        assert ip._RGBFilter(_stub_opt(1.0), rgba) == 'fused' and calls[-1][1][0] == 1.0 and torch.equal(torch.Tensor(calls[-1][1][1]), base[3])
        assert ip._RGBFilter(_stub_opt(0), rgb) == 'fused'
        n = len(calls)
        # strength 1 without alpha, a strength that is not finite, another model type, a CPU image, a dtype the engine does not take, a view that is not dense
        for s, im in ((1.0, rgb), (1, rgb), (float('nan'), rgb), (float('inf'), rgba), (float('-inf'), rgb)):
            got = ip._RGBFilter(_stub_opt(s), im)
            assert torch.equal(torch.Tensor(got).view(torch.int32), want(s, base[:im.shape[0]]).view(torch.int32)), s      # (bits: the results hold NaNs)
        opt = _stub_opt(0.6)
        opt.modelCached = object()
        assert torch.equal(torch.Tensor(ip._RGBFilter(opt, rgba)), want(0.6, base))
        assert torch.equal(ip._RGBFilter(_stub_opt(0.6), base), want(0.6, base))
        assert torch.equal(torch.Tensor(ip._RGBFilter(_stub_opt(0.6), rgba.double())), want(0.6, base.double()))
        view = torch.zeros(3, 6, 16).as_subclass(_OnDevice)[:, :, ::2]              # a strided view: torch rounds its fp16 products otherwise than a dense image's
        assert torch.equal(torch.Tensor(ip._RGBFilter(_stub_opt(0.6), view)), torch.zeros(3, 6, 8))
        # the flag off: every case above is the torch path
        config.filterOnDevice = False
        for s, im in ((0.6, rgb), (1.0, rgba), (0.0, rgba)):
            assert torch.equal(torch.Tensor(ip._RGBFilter(_stub_opt(s), im)), want(s, base[:im.shape[0]])), s
        assert len(calls) == n and not lib_calls
    finally:
        config.filterOnDevice = True


def test_filterout_refuses_a_strength_that_is_not_finite():
    with pytest.raises(ValueError, match='finite'):
        ip.filterOut(_stub_opt(float('nan')), torch.zeros(3, 4, 4), 8)


# ---- the blend's arithmetic, rounding by rounding ----------------------------------------------------------------------------------------------
def blend_fp16(c, inp, s):
    """What the kernel must compute per element for an fp16 canvas.  c, inp: float16 arrays; s: the Python float of the step.
    The scalars reach the device as fp32; each product is formed in fp32 and rounded to fp32, then to fp16 (the tensor torch materialises); the sum of the two fp16
    tensors is formed in fp32 and rounded to fp16."""
    sf, tf = np.float32(s), np.float32(1.0 - s)                      # (the subtraction in double: what Python hands torch)
    p = (sf * c.astype(np.float32)).astype(np.float32).astype(np.float16)
    q = (tf * inp.astype(np.float32)).astype(np.float32).astype(np.float16)
    return (p.astype(np.float32) + q.astype(np.float32)).astype(np.float32).astype(np.float16)


def blend_fp32(c, inp, s):
    sf, tf = np.float32(s), np.float32(1.0 - s)
    return ((sf * c).astype(np.float32) + (tf * inp).astype(np.float32)).astype(np.float32)


STRENGTHS = (0.3, 0.6, 1 / 3)


@pytest.mark.parametrize('s', STRENGTHS)
def test_numpy_restatement_of_the_blend_equals_torch(s):
    rng = np.random.default_rng(4096)
    bits = rng.integers(0, 1 << 16, (2, 4096), dtype=np.uint16)
    bits = np.where((bits & 0x7C00) == 0x7C00, bits & 0x83FF, bits).astype(np.uint16)      # finite values only: exponent 31 becomes a subnormal
    c, inp = bits[0].view(np.float16), bits[1].view(np.float16)
    assert np.isfinite(c.astype(np.float32)).all() and np.isfinite(inp.astype(np.float32)).all()
    with np.errstate(over='ignore'):
        mine = blend_fp16(c, inp, s)
    x, i = torch.from_numpy(c.copy()), torch.from_numpy(inp.copy())
    want = (s * x + (1 - s) * i).numpy()
    assert want.dtype == np.float16
    assert np.array_equal(mine.view(np.uint16), want.view(np.uint16))
    # and with fp32 tensors of the same values
    x32, i32 = x.float(), i.float()
    want32 = (s * x32 + (1 - s) * i32).numpy()
    assert np.array_equal(blend_fp32(c.astype(np.float32), inp.astype(np.float32), s).view(np.uint32), want32.view(np.uint32))
