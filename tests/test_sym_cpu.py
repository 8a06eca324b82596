"""The self-ensemble's entry points (moe_sym_pad, moe_sym_fold, moe_run_plan_ens) on the host: declared, exported, and refusing bad arguments before anything touches
a device -- the reference's callers get an exception with a message (python/worker.py:52-74), not a launch on bad sizes.  The kernels themselves: tests/test_gpu_sym.py."""
import ctypes
import os
import re

import pytest

from moephoto_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('moe_sym_pad', 'moe_sym_fold', 'moe_run_plan_ens')


def test_header_library_and_exports_agree_on_the_ensemble_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'moephoto_amd.h')).read()
    declared = set(re.findall(r'\b(moe_[a-z0-9_]+)\s*\(', hdr))
    L = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name        # (bound with a signature, not called through ctypes' defaults)
        assert 'python/imageProcess.py:5' in hdr[hdr.index('int ' + name) - 2400:hdr.index('int ' + name)], name      # cites the reference lines it replaces
    assert sorted(_lib.EXPORTS) == sorted(declared)
    assert L.moe_abi_version() == 4                                 # additions only: the version stays


def _einval(rc, word):
    msg = _lib.lib().moe_last_error()
    assert rc == _lib.EINVAL and word in msg, (rc, msg)


def test_sym_pad_and_fold_refuse_bad_arguments_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    pad = lambda src, dt, C, H, W, sym, dst, Hp, Wp: L.moe_sym_pad(src, dt, C, H, W, H * W, W, 1, sym, dst, Hp, Wp, 0, None)
    _einval(pad(None, _lib.F32, 1, 2, 3, 0, p, 3, 2), b'NULL')
    _einval(pad(p, _lib.F32, 1, 2, 3, 0, None, 3, 2), b'NULL')
    for dt in (_lib.U8, _lib.U16, 7, -1):
        _einval(pad(p, dt, 1, 2, 3, 0, p, 3, 2), b'dtype')
    for sym in (-1, 7, 100):
        _einval(pad(p, _lib.F16, 1, 2, 3, sym, p, 3, 3), b'sym')
    for C, H, W in ((0, 2, 3), (1, 0, 3), (1, 2, 0), (-1, 2, 3)):
        _einval(pad(p, _lib.F32, C, H, W, 1, p, 8, 8), b'positive')
    # the padded size is that of the TRANSFORMED image: 2 x 3 transposed (symmetries 0, 3, 4, 6) is 3 x 2
    for sym, Hp, Wp in ((1, 1, 3), (1, 2, 2), (2, 2, 2), (5, 1, 8), (0, 2, 3), (3, 2, 8), (4, 8, 1), (6, 2, 2)):
        _einval(pad(p, _lib.F32, 1, 2, 3, sym, p, Hp, Wp), b'smaller')
    fold = lambda acc, t, dt, C, H, W, sym, d: L.moe_sym_fold(acc, t, dt, C, H, W, sym, d, 0, None)
    _einval(fold(None, p, _lib.F32, 1, 2, 3, 0, 0), b'NULL')
    _einval(fold(p, None, _lib.F32, 1, 2, 3, 0, 0), b'NULL')
    _einval(fold(p, p, _lib.U8, 1, 2, 3, 0, 0), b'dtype')
    for sym in (-1, 7):
        _einval(fold(p, p, _lib.F16, 1, 2, 3, sym, 0), b'sym')
    for C, H, W in ((0, 2, 3), (1, 0, 3), (1, 2, -3)):
        _einval(fold(p, p, _lib.F32, C, H, W, 2, 0), b'positive')
    _einval(fold(p, p, _lib.F32, 1, 2, 3, 2, -2), b'final_div')


def _plan(shape, scale=2, crop=48, pad=5):
    h = ctypes.c_void_p()
    _lib.check(_lib.lib().moe_plan_create((ctypes.c_int64 * 3)(*shape), float(1 << 40), 1e-3, pad, scale, 8, crop, ctypes.byref(h)))
    return h


def test_run_plan_ens_refuses_bad_arguments_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    net = ctypes.c_void_p()
    _lib.check(L.moe_net_create(_lib.ARCH_NET2X, 2, ctypes.byref(net)))
    pl, pl_t, pl_other, pl_x4 = _plan((3, 37, 52)), _plan((3, 52, 37)), _plan((3, 40, 52)), _plan((3, 52, 37), scale=4)
    ens = lambda net, pl, pl_t, n, img, dt_in, out, dt_out: L.moe_run_plan_ens(net, pl, pl_t, n, img, dt_in, 37 * 52, 52, 1, out, dt_out, 0, None)
    try:
        _einval(ens(None, pl, pl_t, 1, p, _lib.F32, p, _lib.F32), b'NULL')
        _einval(ens(net, None, pl_t, 1, p, _lib.F32, p, _lib.F32), b'NULL')
        _einval(ens(net, pl, pl_t, 1, None, _lib.F32, p, _lib.F32), b'NULL')
        _einval(ens(net, pl, pl_t, 1, p, _lib.F32, None, _lib.F32), b'NULL')
        for n in (-1, 8, 64):
            _einval(ens(net, pl, pl_t, n, p, _lib.F32, p, _lib.F32), b'n_sym')
        _einval(ens(net, pl, pl_t, 1, p, _lib.U8, p, _lib.F32), b'dtype')
        _einval(ens(net, pl, pl_t, 1, p, _lib.F16, p, _lib.U16), b'dtype')
        _einval(ens(net, pl, None, 1, p, _lib.F32, p, _lib.F32), b'plan_t')             # every n_sym > 0 includes the transpose
        _einval(ens(net, pl, pl_other, 3, p, _lib.F32, p, _lib.F32), b'transpose')      # not the plan of the transposed shape
        _einval(ens(net, pl, pl, 3, p, _lib.F32, p, _lib.F32), b'transpose')
        _einval(ens(net, pl, pl_x4, 3, p, _lib.F32, p, _lib.F32), b'transpose')         # ... nor one of another scale
        # past the argument checks (plan_t may be NULL for n_sym == 0): the net has no weights yet -- a state error, still before any device call
        assert ens(net, pl, None, 0, p, _lib.F32, p, _lib.F32) == _lib.ESTATE and b'finalized' in L.moe_last_error()
        assert ens(net, pl, pl_t, 7, p, _lib.F16, p, _lib.F16) == _lib.ESTATE and b'finalized' in L.moe_last_error()
    finally:
        for h in (pl, pl_t, pl_other, pl_x4):
            L.moe_plan_destroy(h)
        L.moe_net_destroy(net)


def test_sr_divides_once_on_either_path():
    """runSR.sr hands the average to the ensemble (on the device path it is the last fold's): nothing divides a second time, and ensemble = 0 divides nothing."""
    import torch
    from moephoto_amd import imageProcess as ip, runSR
    from moephoto_amd.config import config
    assert config.ensembleOnDevice is True
    calls = []
    real = ip.doCrop

    def fake(opt, x, *a, **k):          # (a stand-in net: the torch path on host tensors)
        calls.append(tuple(x.shape))
        return x * 2.0
    ip.doCrop = fake
    try:
        opt = ip.Option()
        x = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
        for n in (0, 1, 3, 7):
            opt.ensemble = n
            del calls[:]
            assert torch.equal(runSR.sr(opt)(x), x * 2.0 * (n + 1) / (n + 1)) and len(calls) == n + 1
            assert torch.equal(ip.ensemble(opt)(x), x * 2.0 * (n + 1))
    finally:
        ip.doCrop = real
