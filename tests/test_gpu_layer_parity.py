"""Every tapped layer of the ARSB families in the default arithmetic ('mixed') against a float64 model of THAT layer fed the engine's own input tap
(tests/emu_layers.py) -- the plain high-precision reference of the same operation that an end-to-end comparison cannot be for this arithmetic: end to
end, two summation orders of the same roundings lie 3-4e-4 apart on noise, one layer from one input they lie 1e-5 apart.

    max|got - m64| <= 4 max|m32 - m64| + F          rms(got - m64) <= 4 rms(m32 - m64) + 2^-23 max|m64|

m64 / m32: the model with its products and sums in float64 / fp32; F: what one flipped fp16 rounding inside the layer can do (emu_layers.py).  The bound is
measured against the reference's two summation orders, never against the engine: both sides add the same exact fp16 x fp16 products in fp32, two draws of
that noise over 1e5 samples differ by well under 2x, and the other 2x is left for the MFMA's chunked accumulation, which nobody has measured -- so the 4 is
unmeasured, and a complete run writes every observed ratio to profiles/layer_parity/summary.md.  tests/test_layer_models_cpu.py shows, on the reference
alone, that these bounds catch a residual that drops the stream's low part, a lost border column of conv_1 and an R tail that reads fp16 activations.

The fp8 low-part chain (lo8, arsb_sq, drop_lo, the fork) that the default forward runs is held the same way by tests/test_gpu_chain8_layers.py, under set_debug's value 2.
Not bounded here: lite (held at 2e-5 end to end; SEDN has tests/test_gpu_sedn_layers.py), fp16 I/O edges."""
import os

import pytest
import torch

import emu_layers as el
import golden_defs as gd
from moephoto_amd.weights import load_state_dict_file

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ['a2', 'a3', 'a4', 'dn_lite5']
CASES = [('a2', -1), ('a2', 0), ('a2', 6), ('a3', -1), ('a3', 0), ('a4', -1), ('a4', 0), ('dn_lite5', -1), ('dn_lite5', 0)]      # (key, set_exact_blocks: -1 = the default count, 0 = every block on arsb32c)
SHAPES = [(3, 8, 16), (3, 9, 35), (2, 40, 264), (2, 131, 61)]      # one patch | odd and ragged | 33 patch columns | vertical continuation with a ragged end
KINDS = ('natural', 'noise')
PAIRS = ('stem', 'input2') + tuple('arsb%d' % i for i in range(1, 7))      # the taps that are hi + lo pairs in 'mixed'
shape_id = lambda s: 'x'.join(map(str, s))

ROWS = {}      # (test, key, blocks, shape, kind, layer) -> figures


@pytest.fixture(scope='module')
def dev():
    from moephoto_amd import _lib
    _lib.require_device()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def summary():
    yield
    want = len(CASES) * len(SHAPES) * len(KINDS) + 2 * len(KEYS) * len(SHAPES) * len(KINDS)      # (the production form: lo8 off and on)
    if len({k[:5] for k in ROWS}) != want:      # a partial run (-k ...) leaves the record of the last complete one alone
        return
    lines = ['# Layer parity: observed distance to the float64 model, in units of the reference\'s own spread', '',
             'Written by a complete run of `tests/test_gpu_layer_parity.py`. `max` = max|got - m64| / max|m32 - m64|, `rms` likewise; the test allows',
             '4 x the spread (+ the floor F on the max, + 2^-23 max|m64| on the rms). `beyond` = values further from m64 than 4 x the max spread, of `n`:',
             'where a max ratio above 4 sits on a handful of values it is isolated flipped roundings (what F is for), not an error everywhere.', '',
             '| test | net | blocks | shape | input | layer | max | rms | max / bound | rms / bound | beyond | n |', '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for (test, key, blocks, shape, kind, layer), f in ROWS.items():
        ratio = lambda a, b: 'inf' if b == 0 and a > 0 else '{:.2f}'.format(a / b if b else 0.0)
        lines.append('| {} | {} | {} | {} | {} | {} | {} | {} | {} | {} | {} | {} |'.format(
            test, key, blocks, shape_id(shape), kind, layer, ratio(f['dm'], f['sm']), ratio(f['dr'], f['sr']), ratio(f['dm'], f['bm']), ratio(f['dr'], f['br']), f['beyond'], f['n']))
    worst = max(ROWS.items(), key=lambda kv: kv[1]['dr'] / kv[1]['sr'] if kv[1]['sr'] else 0.0)
    lines[5:5] = ['Largest rms ratio: {:.2f} ({}).'.format(worst[1]['dr'] / worst[1]['sr'], ' '.join(map(str, worst[0]))), '']
    try:
        os.makedirs(os.path.join(ROOT, 'profiles', 'layer_parity'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'layer_parity', 'summary.md'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    except OSError:
        pass      # (a read-only tree: the assertions have been made)


_mods, _nets = {}, {}


def module_for(key):
    from moephoto_amd import models
    if key not in _mods:
        m = {'net2x': models.Net2x, 'net3x': models.Net3x, 'net4x': models.Net4x, 'netdn': models.NetDN}[gd.MODELS[key][0]]()
        sd = gd.state_dict_for(key, load_state_dict_file)
        m.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
        m.eval()
        m.precision = 'mixed'
        _mods[key] = m
        _nets[key] = el.Net(gd.MODELS[key][0], sd)
    return _mods[key].to(dtype=torch.float32, device='cuda:0'), _nets[key]


def image(kind, seed, shape):
    return (gd.natural_image(seed, shape) if kind == 'natural' else gd.noise_image(seed, shape))[:, None]


def tapped_forward(m, x, dev, names):
    """one forward under set_debug: the taps `names` (and the fp16 parts of those that are pairs), x and y"""
    m.set_debug(True)
    try:
        y = m(torch.from_numpy(x).to(dev))[-1]
        torch.cuda.synchronize()
        taps = {'x': torch.from_numpy(x), 'y': y.float().cpu()}
        for name in names:
            taps[name] = torch.from_numpy(m.debug_tap(name))
            if name in PAIRS:
                taps[name + '.hi'] = torch.from_numpy(m.debug_tap(name + '.hi'))
    finally:
        m.set_debug(False)
    return taps


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
@pytest.mark.parametrize('key,blocks', CASES)
def test_every_tapped_layer_against_its_float64_model(key, blocks, shape, kind, dev):
    m, net = module_for(key)
    names = el.layer_names(net.arch)
    bad = []
    try:
        m.set_exact_blocks(blocks)
        n = m.exact_blocks()
        taps = tapped_forward(m, image(kind, 43, shape), dev, names[:-1])
        with torch.no_grad():
            for name in names:
                ok, text, fig = el.check(taps[name], el.run_layer(net, name, taps, torch.float64, n), el.run_layer(net, name, taps, torch.float32, n))
                ROWS[('tapped', key, blocks, shape, kind, name)] = fig
                print('{} blocks {} {} {} {}: {}'.format(key, n, shape_id(shape), kind, name, text))
                if not ok:
                    bad.append('{}: {}'.format(name, text))
    finally:
        m.set_exact_blocks(-1)
    assert not bad, '{} with {} split-operand blocks, {} {}:\n  '.format(key, n, shape_id(shape), kind) + '\n  '.join(bad)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
@pytest.mark.parametrize('key', KEYS)
def test_production_form_against_the_float64_composite(key, shape, kind, dev):
    """set_debug's value 1 turns off the fused tail, the fp8 low-part chain, drop_lo and the branch fork, so the fused tail has no taps.  With debug off and lo8 off
    the trunk's kernels are the tapped run's: y of THAT run is held to the float64 composite "R branch from tap arsb6 + U branch from tap stem"
    (emu_layers.tail_fused) under the same two bounds, computed for the composite.  Where this fails while the tapped layers pass, the message says whether
    the run with fuse_tail off holds ITS composite (then the fused tail is at fault) or not (then the untapped trunk: drop_lo, the fork)."""
    m, net = module_for(key)
    bad = ''
    try:
        m.set_option('lo8', 'off')
        x = image(kind, 47, shape)
        taps = tapped_forward(m, x, dev, ('stem', 'arsb6'))
        xd = torch.from_numpy(x).to(dev)
        y = m(xd)[-1].float().cpu()
        fused = el.tail_is_fused(net.arch, shape[2])
        with torch.no_grad():
            ok, text, fig = el.check(y, el.tail_fused(net, taps, torch.float64, fused), el.tail_fused(net, taps, torch.float32, fused))
            ROWS[('production', key, -1, shape, kind, 'y (fused tail)' if fused else 'y')] = fig
            print('{} {} {} y ({}): {}'.format(key, shape_id(shape), kind, 'fused tail' if fused else 'stored branches', text))
            if not ok:
                y0 = m.set_option('fuse_tail', 0)(xd)[-1].float().cpu()
                ok0, text0, _ = el.check(y0, el.tail_fused(net, taps, torch.float64, False), el.tail_fused(net, taps, torch.float32, False))
                bad = '{}\n  with fuse_tail off {} -> the difference is in the {}'.format(
                    text, 'the run holds its composite (' + text0 + ')' if ok0 else 'it fails too (' + text0 + ')', 'fused tail' if ok0 else 'untapped trunk')
    finally:
        m.set_option('lo8', 'on').set_option('fuse_tail', 1)
    assert not bad, '{} {} {}: {}'.format(key, shape_id(shape), kind, bad)
    # The same with lo8 ON, the form that ships: set_debug(2) taps the production forward and changes nothing else (tests/test_gpu_chain8_layers.py holds its layers), so y
    # of THAT run is held to the composite fed that run's own `stem` and `arsb6` -- arsb6 without a low part (drop_lo), the stem as (fp16, word); NetDN: its tail on arsb6
    # and the stem's pair as stored (emu_layers.tail_dn8).  The same two bounds.
    from moephoto_amd import _lib
    m.set_debug(2)
    try:
        y2 = m(xd)[-1].float().cpu()
        torch.cuda.synchronize()
        taps2 = {}
        for name in ('stem', 'arsb6'):
            for part in ('', '.hi', '.w8'):
                try:
                    taps2[name + part] = torch.from_numpy(m.debug_tap(name + part))
                except _lib.EngineError:
                    pass      # (a part this form does not store)
    finally:
        m.set_debug(False)
    assert 'stem.w8' in taps2 and ('arsb6.hi' in taps2) == (net.arch == 'netdn'), sorted(taps2)
    with torch.no_grad():
        ok, text, fig = el.check(y2, el.run_layer(net, 'y', taps2, torch.float64, chain8=True, fused=fused), el.run_layer(net, 'y', taps2, torch.float32, chain8=True, fused=fused))
    ROWS[('production, lo8 on', key, -1, shape, kind, 'y (fused tail)' if fused else 'y')] = fig
    print('{} {} {} y with lo8 on ({}): {}'.format(key, shape_id(shape), kind, 'fused tail' if fused else 'stored branches', text))
    assert ok, '{} {} {} with lo8 on: {}'.format(key, shape_id(shape), kind, text)
