"""The AiLUT generator net's definition (moephoto_amd/ailut.py) against torch's functional ops in float64, its loader's refusals, and the builders' refusals for the
{'op': 'dehaze', 'model': 'AiLUT_*'} step -- no device."""
import ctypes

import numpy as np
import pytest
import torch

import ailut_util as au
from moephoto_amd import ailut, lut3d

SIZES = ((1, 1), (3, 2), (17, 5), (256, 256), (140, 100), (300, 260), (523, 259))          # (w, h)


@pytest.mark.parametrize('wh', SIZES)
def test_thumbnail_is_torchs_bilinear_interpolation(wh):
    """F.interpolate(.., (256, 256), 'bilinear', align_corners=False) in float64: torch's source coordinate is a float, the definition's an integer pair; the
    interpolant is continuous in it, so they differ by rounding alone."""
    w, h = wh
    for bits, order in ((16, 'bgr'), (8, 'rgb')):
        im = au.frame('noise', w, h, bits, seed=w + h)
        got = ailut.thumbnail(im, bits, order)
        want = au.torchForward(im, bits, order, au.stateDict(1, 2, 1), torch.float64)[0]
        assert got.shape == (3, 256, 256) and got.dtype == np.float64
        assert np.abs(got - want).max() <= 1e-9, (wh, bits, np.abs(got - want).max())
    if wh == (256, 256):          # the identity sampling
        assert (ailut.thumbnail(im, 8, 'rgb') == im.transpose(2, 0, 1) / 255.0).all()


def test_thumbnail_axis_and_refusals():
    i0, i1, f = ailut.axis(256)
    assert (i0 == np.arange(256)).all() and (f == 0).all()
    for n in (1, 2, 3, 255, 257, 1080, 7680):
        i0, i1, f = ailut.axis(n)
        assert i0.min() >= 0 and i1.max() <= n - 1 and (i1 - i0 <= 1).all() and (0 <= f).all() and (f < 1).all() and (np.diff(i0 + f) >= 0).all()
    for bad, match in (((np.zeros((4, 4)),), 'H, W, 3'), ((np.zeros((4, 4, 3)), 10), 'srcBits'), ((np.zeros((4, 4, 3)), 8, 'gbr'), "'order'")):
        with pytest.raises(ValueError, match=match):
            ailut.thumbnail(*bad)


@pytest.mark.parametrize('d,ranks', ((2, 1), (9, 3), (33, 3), (33, 5)))
def test_generate_is_the_functional_graph_in_float64(d, ranks):
    sd = au.stateDict(10 + d + ranks, d, ranks)
    params = ailut.loadParams(sd)
    assert params['d'] == d and params['ranks'] == ranks
    for kind in ('noise', 'flat', 'ramp'):
        thumb = ailut.thumbnail(au.frame(kind, 140, 100, 16, seed=3), 16, 'bgr')
        table, vertices = ailut.generate(thumb, params)
        want_t, want_v = au.torchGenerate(thumb, sd, torch.float64)
        assert table.shape == (3, d, d, d) and vertices.shape == (3, d)
        assert np.abs(table - want_t).max() <= 1e-9 and np.abs(vertices - want_v).max() <= 1e-9, (kind, np.abs(table - want_t).max(), np.abs(vertices - want_v).max())
        lut3d.check(table.astype(np.float32), vertices.astype(np.float32))          # (the layout and the order lut3d.check takes)
        # the vertices start at 0, end within 1e-6 of 1 and never decrease -- also with softmax and the cumulative sum redone in float32
        f = ailut.features(thumb, params)
        for v in (vertices, ailut.heads(f.astype(np.float32), params, np.float32)[1]):
            assert (v[:, 0] == 0).all() and np.abs(v[:, -1] - 1).max() <= 1e-6 and (np.diff(v, axis=1) >= 0).all()
    assert ailut.heads(f.astype(np.float32), params, np.float32)[1].dtype == np.float32


def test_features_are_ordered_c4_y2_x_with_a_one_hot_bank():
    """W_h0 = one row that picks feature k and a bank of ones: the table's every value is feature k.  Against the 8 x 8 map pooled by hand."""
    sd = dict(au.stateDict(5, 2, 1))
    params = ailut.loadParams(sd)
    thumb = ailut.thumbnail(au.frame('noise', 64, 48, 8, seed=1), 8, 'rgb')
    x = torch.from_numpy(thumb)[None]
    import torch.nn.functional as F
    for i in range(5):
        x = F.leaky_relu(F.conv2d(x, torch.from_numpy(sd['backbone.{}.0.weight'.format(i)]).double(), torch.from_numpy(sd['backbone.{}.0.bias'.format(i)]).double(), stride=2, padding=1), 0.2)
        if i < 4:
            x = F.instance_norm(x, weight=torch.from_numpy(sd['backbone.{}.2.weight'.format(i)]).double(), bias=torch.from_numpy(sd['backbone.{}.2.bias'.format(i)]).double(), eps=1e-5)
    last = x[0].numpy()
    assert last.shape == (128, 8, 8)
    for c, y, xx in ((0, 0, 0), (0, 0, 1), (0, 1, 0), (77, 1, 1), (127, 1, 0)):
        k = c * 4 + y * 2 + xx
        one = dict(params)
        one[ailut.KEY_H0 + '.weight'] = np.eye(512, dtype=np.float32)[k:k + 1]
        one[ailut.KEY_H0 + '.bias'] = np.zeros(1, np.float32)
        one[ailut.KEY_BANK + '.weight'] = np.ones((24, 1), np.float32)
        table = ailut.generate(thumb, one)[0]
        want = last[c, 4 * y:4 * y + 4, 4 * xx:4 * xx + 4].mean()
        assert np.abs(table - want).max() <= 1e-12, (c, y, xx)


def test_loadParams_refuses_by_key():
    sd = au.stateDict(7, 9, 3)
    good = ailut.loadParams(sd)
    assert set(good) == set(sd) | {'d', 'ranks'} and all(good[k].dtype == np.float32 for k in sd)
    for key in sd:
        with pytest.raises(ValueError, match="no '{}'".format(key)):
            ailut.loadParams({k: v for k, v in sd.items() if k != key})
    for key in ('backbone.0.0.weight', 'backbone.3.2.bias', 'backbone.4.0.bias', ailut.KEY_H0 + '.bias', ailut.KEY_G + '.bias'):
        with pytest.raises(ValueError, match="'{}' has shape".format(key)):
            ailut.loadParams(dict(sd, **{key: sd[key][1:]}))
        for bad in (np.nan, np.inf):
            a = sd[key].copy()
            a.reshape(-1)[-1] = bad
            with pytest.raises(ValueError, match="'{}' holds a value that is not finite".format(key)):
                ailut.loadParams(dict(sd, **{key: a}))
    with pytest.raises(ValueError, match="basis_luts_bank.weight' has 2186 rows, expected 3 d\\^3 = 2187"):
        ailut.loadParams(dict(sd, **{ailut.KEY_BANK + '.weight': sd[ailut.KEY_BANK + '.weight'][1:]}))
    with pytest.raises(ValueError, match='n_ranks 1 .. 8'):
        ailut.loadParams(dict(sd, **{ailut.KEY_H0 + '.weight': np.zeros((9, 512), np.float32)}))
    with pytest.raises(ValueError, match='d 2 .. 65'):
        ailut.loadParams(dict(sd, **{ailut.KEY_G + '.weight': np.zeros((3 * 65, 512), np.float32)}))
    with pytest.raises(ValueError, match='d 2 .. 65'):          # a Share-AdaInt checkpoint: d - 1 rows
        ailut.loadParams(dict(sd, **{ailut.KEY_G + '.weight': np.zeros((8, 512), np.float32)}))


def test_the_wrapper_refuses_before_it_needs_a_device():
    from moephoto_amd import imageProcess as ip
    params = ailut.loadParams(au.stateDict(7, 9, 3))
    for kw, match in ((dict(srcBits=10), 'srcBits'), (dict(bits=12), 'bits'), (dict(order='gbr'), "'order'"), (dict(strength=float('nan')), "'strength'"), (dict(dither='blue'), "'dither'"),
                      (dict(tableOut=3), "'tableOut'")):
        with pytest.raises(ValueError, match=match):
            ip.ailut(params, **kw)
    with pytest.raises(ValueError, match="loadParams' dict"):
        ip.ailut(au.stateDict(7, 9, 3))
    with pytest.raises(ValueError, match="no 'backbone.2.0.bias'"):
        ip.ailut({k: v for k, v in params.items() if k != 'backbone.2.0.bias'})
    assert callable(ip.ailut(params)) and callable(ip.ailut(params, 8, 8, 'rgb', 0.5, 'ordered', lambda t, v: None))


def test_entry_points_refuse_without_a_device():
    """The refusals tools/ailut_args_check.cpp runs under the sanitizers, a few of them through ctypes: every one returns before a device call."""
    from moephoto_amd import _lib
    L = _lib.lib()
    class Lut(ctypes.Structure):          # the table handle's host object (csrc/net.h), so that the checks that read its d can run without a device
        _fields_ = [('d', ctypes.c_int), ('device', ctypes.c_int), ('dev', ctypes.c_void_p), ('table_bytes', ctypes.c_size_t)]
    lut9, lut5 = Lut(9, 0, None, 0), Lut(5, 0, None, 0)
    g, fake, other = ctypes.c_void_p(), ctypes.cast(ctypes.pointer(lut9), ctypes.c_void_p), ctypes.cast(ctypes.pointer(lut5), ctypes.c_void_p)
    assert L.moe_ailut_create(1, 3, ctypes.byref(g)) == _lib.EINVAL and b'd = 1' in L.moe_last_error()
    assert L.moe_ailut_create(33, 9, ctypes.byref(g)) == _lib.EINVAL and b'ranks = 9' in L.moe_last_error()
    assert L.moe_ailut_create(33, 3, None) == _lib.EINVAL
    _lib.check(L.moe_ailut_create(9, 3, ctypes.byref(g)))
    try:
        shapes = ailut.paramShapes(9, 3)
        assert L.moe_ailut_num_params(g) == len(shapes) == 23
        name, shape, ndim = ctypes.c_char_p(), (ctypes.c_int64 * 4)(), ctypes.c_int()
        for i, (key, want) in enumerate(shapes.items()):
            _lib.check(L.moe_ailut_param_info(g, i, ctypes.byref(name), shape, ctypes.byref(ndim)))
            assert name.value.decode() == key and tuple(shape[:ndim.value]) == want
        assert L.moe_ailut_param_info(g, 23, ctypes.byref(name), shape, ctypes.byref(ndim)) == _lib.EINVAL
        a = np.zeros((16, 3, 3, 3), np.float32)
        sh = (ctypes.c_int64 * 4)(*a.shape)
        assert L.moe_ailut_set_param(g, b'backbone.0.1.weight', a.ctypes.data, sh, 4) == _lib.EINVAL and b'unknown parameter' in L.moe_last_error()
        assert L.moe_ailut_set_param(g, b'backbone.0.0.weight', a.ctypes.data, sh, 3) == _lib.EINVAL and b'another shape' in L.moe_last_error()
        a[-1, -1, -1, -1] = np.nan
        assert L.moe_ailut_set_param(g, b'backbone.0.0.weight', a.ctypes.data, sh, 4) == _lib.EINVAL and b'value 431' in L.moe_last_error()
        assert L.moe_ailut_finalize(g, 0) == _lib.ESTATE and b"'backbone.0.0.weight' is not set" in L.moe_last_error()
        buf = (ctypes.c_uint16 * 64)()
        assert L.moe_ailut_run(g, buf, 16, 2, 2, 0, fake, None) == _lib.ESTATE and b'not finalized' in L.moe_last_error()
        assert L.moe_ailut_run(None, buf, 16, 2, 2, 0, fake, None) == _lib.EINVAL
        assert L.moe_ailut_run(g, buf, 16, 2, 2, 0, other, None) == _lib.EINVAL and b'd = 5' in L.moe_last_error()
        assert L.moe_ailut_run(g, buf, 16, 2, 2, 2, fake, None) == _lib.EINVAL and b'order 2' in L.moe_last_error()
        assert L.moe_ailut_stage(g, 3, buf, 16, 0, 2, 0, fake, None) == _lib.EINVAL and b'must be positive' in L.moe_last_error()
        bad = ctypes.c_int64()
        assert L.moe_ailut_guards(g, ctypes.byref(bad), None) == _lib.ESTATE
    finally:
        L.moe_ailut_destroy(g)
    assert L.moe_lut3d_read(None, buf, buf, None) == _lib.EINVAL and b'moe_lut3d_read: NULL' in L.moe_last_error()
    assert L.moe_ailut_thumbnail(buf, 12, 2, 2, 0, buf, 0, None) == _lib.EINVAL and b'src_bits' in L.moe_last_error()


# ---- the builders --------------------------------------------------------------------------------------------------------------------------------
def test_builders_refuse_before_a_model_is_loaded(monkeypatch, tmp_path):
    from moephoto_amd import procedure, runDN, runSR
    from moephoto_amd.config import config

    def no_model(*_a, **_k):
        raise AssertionError('a model was asked for before the chain was checked')
    monkeypatch.setattr(runSR, 'getOpt', no_model)
    monkeypatch.setattr(runDN, 'getOpt', no_model)
    monkeypatch.setattr(config, 'modelRoot', str(tmp_path))
    au.writeCheckpoint(tmp_path, 'AiLUT_sRGB_3', au.stateDict(7, 9, 3))          # (AiLUT_XYZ_3's file is missing)
    sr = {'op': 'SR', 'model': 'a', 'scale': 2}
    ai = lambda model='AiLUT_sRGB_3', **kw: dict({'op': 'dehaze', 'model': model}, **kw)
    lut = {'op': 'lut', 'table': lut3d.identity(5)}
    out = lambda **kw: dict({'op': 'output'}, **kw)
    rgb, planar = {'op': 'buffer', 'bitDepth': 16}, {'op': 'buffer', 'pixFmt': 'yuv420p10le'}
    builders = (lambda steps: procedure.genFrameStream(steps, 140, 100), procedure.genProcess)
    for build in builders:
        for buf, tail in ((rgb, []), (planar, [out(pixFmt='bgr48le')])):
            with pytest.raises(NotImplementedError, match="'model': 'AiLUT_sRGB_5': the res18 backbone is not in this change"):
                build([buf, sr, ai('AiLUT_sRGB_5')] + tail)
            with pytest.raises(NotImplementedError, match="'AiLUT_sRGB_5'"):
                build([buf, ai('AiLUT_sRGB_5'), sr] + tail)
            with pytest.raises(ValueError, match="'model': 'AiLUT_sRGB_3' must be the last compute step"):
                build([buf, ai(), sr] + tail)
            with pytest.raises(ValueError, match="'model': 'AiLUT_XYZ_3' must be the last compute step"):
                build([buf, ai('AiLUT_XYZ_3'), sr] + tail)
            with pytest.raises(ValueError, match="'model': 'AiLUT_sRGB_3' writes the chain's one colour table: no 'lut' step"):
                build([buf, sr, ai(), lut] + tail)
            with pytest.raises(ValueError, match="'model': 'AiLUT_sRGB_3' writes the chain's one colour table: no 'lut' step"):
                build([buf, sr, lut, ai()] + tail)
            with pytest.raises(ValueError, match="'strength' .* is not finite"):
                build([buf, sr, ai(strength=float('nan'))] + tail)
            with pytest.raises(ValueError, match="'strength' 'much' is not a number"):
                build([buf, sr, ai(strength='much')] + tail)
            with pytest.raises(ValueError, match="'tableOut' is a callable"):
                build([buf, sr, ai(tableOut=[])] + tail)
            with pytest.raises(FileNotFoundError, match='AiLUT-FiveK-XYZ.pth'):          # the error the other families raise for a checkpoint that is not there
                build([buf, sr, ai('AiLUT_XYZ_3')] + tail)
            with pytest.raises(AssertionError, match='a model was asked for'):          # (a chain nothing is wrong with reaches the model)
                build([buf, sr, ai(strength=0.5)] + tail)
        with pytest.raises(ValueError, match="'model': 'AiLUT_sRGB_3': a planar Y'CbCr sink .'pixFmt': 'yuv420p10le'. behind the step is not in this change"):
            build([planar, sr, ai()])
        with pytest.raises(ValueError, match="a planar Y'CbCr sink .'pixFmt': 'yuv420p'. behind the step is not in this change"):
            build([planar, sr, ai(), out(pixFmt='yuv420p')])
        with pytest.raises(ValueError, match="a planar Y'CbCr sink .'pixFmt': 'yuv420p10le'. behind the step is not in this change"):
            build([rgb, sr, ai(), out(pixFmt='yuv420p10le')])
        with pytest.raises(ValueError, match="'order' does not apply to a chain on planar frames"):
            build([planar, sr, ai(order='rgb'), out(pixFmt='bgr48le')])
        # what is pinned stays refused, with its type and message: every other model, the default included
        for step in ({'op': 'dehaze'}, {'op': 'dehaze', 'model': 'dehaze'}, {'op': 'dehaze', 'model': 'sun'}, {'op': 'dehaze', 'model': 'AiLUT_sRGB_4'}):
            with pytest.raises(NotImplementedError, match='op "dehaze" is not part of the SR/DN hot path this engine implements'):
                build([rgb, step])
            with pytest.raises(NotImplementedError, match='op "dehaze" is not part of the SR/DN hot path this engine implements'):
                build([planar, step, out(pixFmt='bgr24')])
        with pytest.raises(NotImplementedError, match='op "slomo" is not part of the SR/DN hot path this engine implements'):
            build([rgb, {'op': 'slomo'}])
    with pytest.raises(ValueError, match="the chain's bitDepth is 10"):
        procedure.genProcess([sr, ai()], 10)
    # a checkpoint loadParams refuses is refused by key
    sd = dict(au.stateDict(7, 9, 3))
    del sd['backbone.1.2.bias']
    au.writeCheckpoint(tmp_path, 'AiLUT_XYZ_3', sd)
    with pytest.raises(ValueError, match="no 'backbone.1.2.bias'"):
        procedure.genProcess([rgb, sr, ai('AiLUT_XYZ_3')])
    got = procedure._lutStep([rgb, sr, ai(strength=0.25)], None, 16)
    assert got['order'] == 'bgr' and got['strength'] == 0.25 and got['params']['d'] == 9 and got['params']['ranks'] == 3 and got['edge'] == '+ailut'
    assert procedure._lutStep([planar, sr, ai(), out(pixFmt='rgb24')], ('yuv420p10le', 'rgb24'))['order'] == 'rgb'
    assert procedure._withoutLut([rgb, sr, ai()]) == [rgb, sr] and procedure._withoutLut([rgb, {'op': 'dehaze'}]) == [rgb, {'op': 'dehaze'}]
