"""The production form of the ARSB families -- the fp8 low-part chain (option lo8, arsb_sq, drop_lo, the forked U branch, NetDN's tail3<2>) that the benchmark times --
layer by layer against a float64 model of THAT layer fed the engine's own input tap (tests/emu_layers.py, the chain form).  The taps are those of moe_net_set_debug's
value 2: taps and nothing else, so y of the tapped forward is bit-equal to y with debugging off, asserted in every case.

Every layer is held by emu_layers.check's two bounds (max <= 4 spread + F, rms <= 4 rms spread + 2^-23 max), the spread being the largest of the fp32 orders that
emu_layers.orders_for gives a tensor of its size (up to 12 at the small shapes: emu_sedn's rule).  A layer that stores (fp16, word) is discrete at the word's step, where
those two leave room for an error of one step everywhere; it is also held in the code domain (emu_layers.code_check): the share of positions whose stored pair differs from
m64's, overall and on the bands where a kernel's edge handling acts (two rows / columns at the image edges, two columns each side of every kernel-column seam: multiples of
30 under arsb_sq, of 32 under conv64_sq / conv64_q8 -- derived from the shape by the engine's rules and checked against the profile's launch counts), against 4 x the share
by which fp32 evaluations of the model (the `cv` order and emu_sedn's chunked one) differ from m64; and every differing position must hold a neighbouring code.
tests/test_layer_models_cpu.py shows on the reference alone that this resolves a dropped residual word, a word added at 2^-11 and lost words of conv_1's last column / row.
A complete run writes every observed ratio to profiles/layer_parity/chain8.md.

Not bounded here: lite, fp16 I/O edges, SEDN in fp16x3; and 'direct8' (a word made from the unrounded remainder), a distinction these tests cannot draw (emu_layers.pair8)."""
import os

import pytest
import torch

import emu_layers as el
from moephoto_amd import _lib
from test_gpu_layer_parity import image, module_for, shape_id

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('a2', -1), ('a2', 6), ('a3', -1), ('a4', -1), ('a4', 3), ('dn_lite5', -1), ('a2', 0)]      # (key, set_exact_blocks)
SHAPES = [(3, 8, 16), (2, 2, 40), (1, 6, 33), (1, 64, 30), (1, 32, 61), (2, 40, 264), (3, 9, 35)]
# one column | two rows, 30 + 10 | 32 + 1 / 30 + 3 | one arsb_sq column, many ring steps | 30 + 30 + 1 | nine columns, a plane boundary in a launch | odd height: conv64_q8
KINDS = ('natural', 'noise')
LEGS = [('exact_fuse', 0), ('max_groups', 3)]      # a2, default blocks, 2 x 24 x 40: m through HBM as (fp16, word) | range ends that recompute rows

ROWS = {}      # (key, blocks, leg, shape, kind, layer) -> figures


@pytest.fixture(scope='module')
def dev():
    _lib.require_device()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def summary():
    yield
    want = (len(CASES) * len(SHAPES) + len(LEGS)) * len(KINDS)
    if len({k[:5] for k in ROWS}) != want:      # a partial run leaves the record of the last complete one alone
        return
    ratio = lambda a, b: 'inf' if b == 0 and a > 0 else '{:.2f}'.format(a / b if b else 0.0)
    lines = ['# The production form (fp8 low-part chain) layer by layer: observed distance to the float64 model', '',
             'Written by a complete run of `tests/test_gpu_chain8_layers.py`. `max`, `rms`: distance to m64 in units of the spread of the two fp32 models, and of the bound',
             '(4 x spread + floor). Layers that store (fp16, word): `share` = share of positions whose stored pair differs from m64\'s, `ref` = the largest such share of an fp32',
             'evaluation of the model, `share / ref` is held to 4; `band` = the band with the largest share against its own limit (4 x ref + 5 sigma of a binomial share over the',
             'band); `far` = positions beyond one code (must be 0).', '',
             '| net | blocks | leg | shape | input | layer | kernel | max / spread | rms / spread | max / bound | rms / bound | share | ref | share / ref | worst band | band share / limit | far |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|']
    top = ('', 0.0)
    for (key, blocks, leg, shape, kind, layer), (f, c, kern) in ROWS.items():
        row = [key, blocks, leg, shape_id(shape), kind, layer, kern, ratio(f['dm'], f['sm']), ratio(f['dr'], f['sr']), ratio(f['dm'], f['bm']), ratio(f['dr'], f['br'])]
        if c:
            b = max(c['bands'].items(), key=lambda kv: kv[1][0] / kv[1][1] if kv[1][1] else 0.0)
            row += ['{:.4f}'.format(c['share']), '{:.4f}'.format(c['p']), ratio(c['share'], c['p']), b[0], ratio(b[1][0], b[1][1]), c['far']]
            if c['p'] and c['share'] / c['p'] > top[1]:
                top = (' '.join(map(str, (key, blocks, leg, shape_id(shape), kind, layer))), c['share'] / c['p'])
        else:
            row += [''] * 6
        lines.append('| ' + ' | '.join(map(str, row)) + ' |')
    lines[7:7] = ['Largest share / ref: {:.2f} ({}).'.format(top[1], top[0]), '']
    try:
        os.makedirs(os.path.join(ROOT, 'profiles', 'layer_parity'), exist_ok=True)
        with open(os.path.join(ROOT, 'profiles', 'layer_parity', 'chain8.md'), 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    except OSError:
        pass      # (a read-only tree: the assertions have been made)


def tap_or_none(m, name):
    try:
        return torch.from_numpy(m.debug_tap(name))
    except _lib.EngineError:
        return None


def production_taps(m, xd, names):
    """one forward under value 2: y, and of every layer in `names` that left a tap: NAME, NAME.hi, NAME.w8 as far as they exist"""
    m.set_debug(2)
    try:
        y = m(xd)[-1]
        torch.cuda.synchronize()
        taps = {}
        for name in names:
            for k in ('', '.hi', '.w8'):
                t = tap_or_none(m, name + k)
                if t is not None:
                    taps[name + k] = t
    finally:
        m.set_debug(0)
    return y, taps


def launches(m, xd, keys):
    """launch counts of the profile's layer keys over one untapped forward"""
    m.set_profile(','.join(keys))
    try:
        m.get_profile()
        y = m(xd)[-1]
        torch.cuda.synchronize()
        return y, {k: p['launches'] for k, p in zip(keys, m.get_profile(all_keys=True))}
    finally:
        m.set_profile(None)


def run_case(key, blocks, shape, kind, leg=None):
    m, net = module_for(key)
    x = image(kind, 53, shape)
    xd = torch.from_numpy(x).to('cuda:0')
    names = el.layer_names(net.arch)
    bad = []
    try:
        m.set_exact_blocks(blocks)
        if leg:
            m.set_option(*leg)
        n = m.exact_blocks()
        fuse = not (leg and leg[0] == 'exact_fuse')
        y0 = m(xd)[-1].clone()
        y, taps = production_taps(m, xd, names[:-1])
        assert torch.equal(y, y0), 'y under set_debug(2) differs from the untapped forward: max {:.3e}'.format(float((y.float() - y0.float()).abs().max()))
        # which kernel took the exact blocks: the rule (emu_layers.chain_kernel) against the profile's own record
        yp, cnt = launches(m, xd, ['xpair', 'c1_'])
        assert torch.equal(yp, y0)
        on_sq = n >= 1 and el.chain_kernel('arsb1', n, shape[1], fuse)[0] == 'arsb_sq'
        assert cnt['xpair'] == (n if on_sq else 0), (cnt, 'arsb_sq expected for {} blocks'.format(n) if on_sq else 'two launches per exact block expected')
        assert on_sq or cnt['c1_'] >= n, (cnt, 'a conv_1 launch per exact block expected')
        # what the form must have left: words where the chain stores them, fp16 pairs behind it, block 6 of an SR net alone
        for name in names[:8]:
            assert name in taps, 'no tap ' + name
            words, pair = name + '.w8' in taps, name + '.hi' in taps
            assert words == el.stores_words(net.arch, name, n), (name, 'words' if words else 'no words')
            assert pair == (not (name == 'arsb6' and net.arch != 'netdn' and n < 6)), (name, 'a pair' if pair else 'no pair')
        taps['x'], taps['y'] = torch.from_numpy(x), y.float().cpu()
        fused = not any(k.startswith('r.up%d' % (net.stages - 1)) for k in taps) and net.arch != 'netdn'
        if net.arch != 'netdn':
            assert fused == el.tail_is_fused(net.arch, shape[2]), 'fused tail: {} against the rule'.format(fused)
        with torch.no_grad():
            for name in [k for k in names if k in taps]:
                m64 = el.run_layer(net, name, taps, torch.float64, n, chain8=True, fused=fused)
                words = el.stores_words(net.arch, name, n)
                m32 = [el.run_layer(net, name, taps, torch.float32, n, chain8=True, fused=fused, order=o) for o in el.orders_for(m64.value.numel(), 2 if words else 1)]
                ok, text, fig = el.check_orders(taps[name], m64, m32)
                kern, seam = el.chain_kernel(name, n, shape[1], fuse) if words or (name.startswith('arsb') and int(name[4:]) <= n) else ('', 0)
                cfig = None
                if words:
                    ok2, text2, cfig = el.code_check(taps[name + '.hi'], taps[name + '.w8'], m64, m32, seam)
                    ok, text = ok and ok2, text + '\n      ' + text2
                ROWS[(key, blocks, '{}={}'.format(*leg) if leg else '', shape, kind, name)] = (fig, cfig, kern)
                print('{} blocks {} {} {} {} [{}]: {}'.format(key, n, shape_id(shape), kind, name, kern, text))
                if not ok:
                    bad.append('{}: {}'.format(name, text))
    finally:
        m.set_exact_blocks(-1)
        if leg:
            m.set_option(leg[0], {'exact_fuse': 1, 'max_groups': 0}[leg[0]])
    assert not bad, '{} with {} split-operand blocks, {} {}:\n  '.format(key, n, shape_id(shape), kind) + '\n  '.join(bad)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
@pytest.mark.parametrize('key,blocks', CASES)
def test_every_layer_of_the_production_form_against_its_float64_model(key, blocks, shape, kind, dev):
    run_case(key, blocks, shape, kind)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('leg', LEGS, ids=lambda l: '{}={}'.format(*l))
def test_the_two_launch_form_and_recomputed_range_ends(leg, kind, dev):
    """a2, default blocks, 2 x 24 x 40.  exact_fuse = 0: conv_1 and conv_2 of an exact block are two launches of conv64_sq, m through HBM as (fp16, word).
    max_groups = 3: three persistent workgroups, so ranges end inside columns and their ends recompute rows."""
    run_case('a2', -1, (2, 24, 40), kind, leg)
