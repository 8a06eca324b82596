"""tests/emu_layers.py on the CPU: the per-layer float64 models behind tests/test_gpu_layer_parity.py are the nets they claim to be, they agree with the
whole-forward emulation that pins the precision budget (tests/emu_precision.py), and the bounds they yield resolve the bugs they are there to find."""
import hashlib
import math
import os

import numpy as np
import pytest
import torch

import emu_layers as el
import emu_precision as emu
import golden_defs as gd
from moephoto_amd.weights import load_state_dict_file

KEYS = ['a2', 'a3', 'a4', 'dn_lite5']
SHAPES = [(3, 8, 16), (3, 9, 35), (2, 40, 264), (2, 131, 61)]      # tests/test_gpu_layer_parity.py runs these
KINDS = ('natural', 'noise')

_nets, _trunks = {}, {}


def net_for(key):
    if key not in _nets:
        _nets[key] = el.Net(gd.MODELS[key][0], gd.state_dict_for(key, load_state_dict_file))
    return _nets[key]


def image(kind, seed, shape):
    return (gd.natural_image(seed, shape) if kind == 'natural' else gd.noise_image(seed, shape))[:, None]


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))


@pytest.mark.parametrize('key', KEYS)
def test_chain_with_nothing_rounded_is_the_oracle(key):
    from oracle import nets as onets
    net = net_for(key)
    x = image('natural', 3, (2, 24, 40))
    with torch.no_grad():
        _, y = el.chain(net, x, torch.float32, exact=True)
    want = onets.forward(net.arch, net.sd, x)
    assert float((y - want).abs().max()) <= 2e-6


def test_a_pair_tap_does_not_determine_its_fp16_part():
    """why the engine leaves NAME.hi beside the tap of a pair: v just below the midpoint of two fp16 values has lo = +half an ulp exactly, and the tap's
    sum hi + lo 2^-11 IS the midpoint -- rounding it to fp16 (ties to even) takes the other neighbour when hi is odd."""
    u = 2.0 ** -10                                                                   # fp16's ulp in [1, 2)
    v = torch.tensor([1.0 + 2.5 * u - 2.0 ** -23], dtype=torch.float32)              # one fp32 step below the midpoint of 1 + 2u and 1 + 3u
    h, l = emu.hilo(v)
    tap = h + l / 2048.0
    assert float(h) == 1.0 + 2 * u and float(l) == 1.0 and float(tap) == 1.0 + 2.5 * u
    assert float(emu.r16(tap)) == float(h)                                           # hi is even here: the tie goes back to it
    h, l = emu.hilo(v + u)                                                           # the next interval: hi = 1 + 3u is odd
    tap = h + l / 2048.0
    assert float(h) == 1.0 + 3 * u and float(tap) == 1.0 + 3.5 * u and float(emu.r16(tap)) == 1.0 + 4 * u


@pytest.mark.parametrize('key', KEYS)
def test_layer_models_against_the_forward_emulation(key):
    """emu_precision.forward in 'mixed' as it ships (fp8 corrections, default block count) plays the engine: every layer's model, fed the emulation's own
    taps, holds the emulation's next tap to the bounds of the GPU test.  Most layers are the same fp32 operations and agree to the bit; the bound is the
    distance allowed where they are not (the order of the three products, the fused tail's low-order sums)."""
    net = net_for(key)
    n = emu.DEFAULT_EXACT[net.arch]
    ex = ['input2'] + ['c%d_%d' % (j, i) for i in range(1, n + 1) for j in (1, 2)]
    x = image('noise', 5, (3, 40, 48))
    taps = {}
    with torch.no_grad():
        y = emu.forward(net.arch, net.sd, x, *emu.mode_sets(net.arch, 'mixed', n), corr8=ex, taps=taps)
        taps['x'] = torch.from_numpy(x)
        last_r = 'r.up%d' % (net.stages - 1)
        for name in el.layer_names(net.arch):
            if name == last_r:
                continue                      # a pair inside the fused tail there, an fp16 tensor in the tapped run: part of y below
            if name == 'y':
                m64, m32, got = el.tail_fused(net, taps, torch.float64), el.tail_fused(net, taps, torch.float32), y
            else:
                m64, m32, got = el.run_layer(net, name, taps, torch.float64, n), el.run_layer(net, name, taps, torch.float32, n), taps[name]
            ok, text, _ = el.check(got, m64, m32)
            assert ok, (key, name, text)


def exceeds(bug, m64, m32):
    bm, br = el.bounds(m64, m32)
    dm, dr = el.distance(bug.value, m64)
    return dm > bm or dr > br, 'max {:.2e} / {:.2e}  rms {:.2e} / {:.2e}'.format(dm, bm, dr, br)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('key', KEYS)
def test_bounds_resolve_the_modelled_bugs(key, shape):
    """A condition on the reference alone: for every family, shape and input class of tests/test_gpu_layer_parity.py, the float64 model with a bug in it
    lies outside the bounds the two correct models give.
      'res16'  the residual adds only the stream's fp16 part           -- every single-pass block, both classes: the rms bound (a bias on every value)
      'col'    the last column of conv_1's output is treated as zero   -- every single-pass block, both classes: the max bound, by orders of magnitude
      'tail16' the R tail reads fp16 activations only                  -- the fused tail (the widths it takes), NOISE only: the rms bound, 3.6 to 8 times.
               Natural input is dropped for this bug: its rms reaches 4.9 to 5.7 times the bound on a3, 0.9 to 1.9 on a2 and 0.7 to 0.9 on a4, whose U
               branch's flipped fp16 roundings (each worth 1e-4 of y) set the composite's own spread.  The figures are printed.
    The inputs of each layer are the models' own chain (all six blocks single-pass, as under set_exact_blocks(0))."""
    net = net_for(key)
    trunk = hashlib.sha1(b''.join(np.ascontiguousarray(v).tobytes() for k, v in sorted(net.sd.items()) if k.startswith(('conv_input', 'relu', 'convt_F')))).hexdigest()
    for kind in KINDS:
        x = image(kind, 41, shape)
        with torch.no_grad():
            if (trunk, shape, kind) not in _trunks:      # (a3 and a4 are built on a2's trunk, bit for bit: the same taps, the same verdicts)
                _trunks[(trunk, shape, kind)] = el.chain(net, x, torch.float32, n_exact=0, trunk_only=True)[0]
                checked = False
            else:
                checked = True
            taps = _trunks[(trunk, shape, kind)]
            for i in (() if checked else range(1, 7)):
                m64, res16, col = el.arsb_single(net, i, taps, torch.float64, (None, 'res16', 'col'))
                m32 = el.arsb_single(net, i, taps, torch.float32)
                for name, bug in (('res16', res16), ('col', col)):
                    hit, text = exceeds(bug, m64, m32)
                    assert hit, (key, shape, kind, 'arsb%d' % i, name, text)
            if el.tail_is_fused(net.arch, shape[2]):
                (m64, bug), m32 = el.tail_fused(net, taps, torch.float64, bug=(None, 'tail16')), el.tail_fused(net, taps, torch.float32)
                hit, text = exceeds(bug, m64, m32)
                print(key, shape, kind, 'tail16', text)
                assert hit or kind == 'natural', (key, shape, kind, 'y', 'tail16', text)


# ---- the production form: the fp8 low-part chain (tests/test_gpu_chain8_layers.py) ------------------------------------------------------------------------------

import test_gpu_chain8_layers as g8      # (its cases and shapes, so that the two files cannot drift apart; importing it needs no device)

SHAPES8 = list(g8.SHAPES) + [(2, 24, 40)]
_trunks8 = {}


@pytest.mark.parametrize('key', KEYS)
def test_chain8_models_with_nothing_rounded_are_the_oracle(key):
    from oracle import nets as onets
    net = net_for(key)
    x = image('natural', 3, (2, 24, 40))
    with torch.no_grad():
        _, y = el.chain(net, x, torch.float32, n_exact=emu.DEFAULT_EXACT[net.arch], exact=True, chain8=True)
    assert float((y - onets.forward(net.arch, net.sd, x)).abs().max()) <= 2e-6


def test_pair8_round_trips_every_e4m3_code_and_saturates():
    """word8 is the identity on the 254 finite e4m3 codes (fed as the fp16 low part 4 w) and pair8 puts such a pair together again where the low part fits under its fp16
    part; beyond +-448 the word saturates and is never a NaN (the two NaN codes, 0x7f and 0xff, are never produced)."""
    codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
    fin = codes[~codes.isnan()]
    assert fin.numel() == 254 and float(fin.abs().max()) == 448.0
    assert torch.equal(el.word8(fin * 4.0), fin)
    for h in (1.5, -1.5, 0.375, 1536.0):      # (mid-binade) |lo| < 2^floor(log2 |h|) is what a split can leave beside h: lo = (v - h) 2^11 with |v - h| < ulp16(h) / 2
        w = fin[(fin * 4.0).abs() < 2.0 ** math.floor(math.log2(abs(h)))]
        val, hi, word = el.pair8(h + w * el.W8)
        assert torch.equal(hi, torch.full_like(w, h)) and torch.equal(word, w) and torch.equal(val, h + w * el.W8), h
    big = torch.tensor([4096.0 + 1.9, -4096.0 - 1.9, 32768.0 + 15.9, 65504.0], dtype=torch.float64)      # low parts of 3891, -3891, 32563, 0: words of 973 and 8141 do not exist
    val, hi, word = el.pair8(big)
    assert not word.isnan().any() and not val.isnan().any()
    assert word.tolist() == [448.0, -448.0, 448.0, 0.0] and hi.tolist() == [4096.0, -4096.0, 32768.0, 65504.0]
    assert el.ulp8(448.0) == 32.0 and el.ulp8(0.25) == 2.0 ** -5 and el.ulp8(2.0 ** -9) == 2.0 ** -9 and el.ulp8(0.0) == 2.0 ** -9


@pytest.mark.parametrize('key', KEYS)
def test_chain_layer_models_against_the_forward_emulation_with_lo8(key):
    """emu_precision.forward(.., lo8=True) plays the engine's chain: it stores the stream as fp16 + e4m3((t - fp16(t)) 2^9) behind every block and hands the correction
    product the same word, and its taps are the pairs BEFORE that store -- so a tap's word is word8 of its low part.  conv_input2 and the exact blocks in the chain form,
    fed the emulation's taps as (hi, word), hold the emulation's next tap -- as stored, (hi, word) again, for the blocks before the last exact one; the fp16 pair for the
    last -- to the value bounds, and the stored pairs to the code-domain shares.  Not to adjacency: the emulation's sums are F.conv2d's, the library's own blocked order, and
    its absolute error on a cancelling sum of O(1) terms reaches 4e-6 -- 34 fp16 steps of a result of 1e-4, whose word is zero: one position of 368 640 lay 3 % past one
    code.  (The models' own orders and the engine's kernels stay inside it at every case of the bug test below and of the GPU test.)"""
    net = net_for(key)
    n = max(2, emu.DEFAULT_EXACT[net.arch])      # (at least one block that stores words)
    ex = ['input2'] + ['c%d_%d' % (j, i) for i in range(1, n + 1) for j in (1, 2)]
    x = image('noise', 5, (3, 40, 48))
    taps = {}
    with torch.no_grad():
        emu.forward(net.arch, net.sd, x, *emu.mode_sets(net.arch, 'mixed', n), corr8=ex, lo8=True, taps=taps)
        names = ['stem', 'input2'] + ['arsb%d' % i for i in range(1, n + 1)]
        for name in names:
            hi = taps[name + '.hi']
            taps[name + '.w8'] = el.word8((taps[name] - hi) * 2048.0)
        for name in names[1:]:
            words = el.stores_words(net.arch, name, n)
            m64 = el.run_layer(net, name, taps, torch.float64, n, chain8=True)
            m32 = [el.run_layer(net, name, taps, torch.float32, n, chain8=True, order=o) for o in el.orders_for(m64.value.numel())]
            got = taps[name + '.hi'] + taps[name + '.w8'] * el.W8 if words else taps[name]
            ok, text, _ = el.check_orders(got, m64, m32)
            assert ok, (key, name, text)
            if words:
                ok, text, _ = el.code_check(taps[name + '.hi'], taps[name + '.w8'], m64, m32, 0, adjacent=False)
                assert ok, (key, name, text)


@pytest.mark.parametrize('shape', SHAPES8, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('key', sorted({k for k, _ in g8.CASES}))
def test_chain_bounds_resolve_the_modelled_bugs(key, shape):
    """A condition on the reference alone, at every net and shape of tests/test_gpu_chain8_layers.py: an exact block of the chain with a bug in it lies outside what the
    correct models allow -- for a block that stores (fp16, word) (blocks 1 and 3 in the OUT8 form) the value bounds OR the code-domain conditions, for the last exact block
    (block 1 storing an fp16 pair) the value bounds alone.
      'res16'  the residual's word is dropped          'res11'  it is added at 2^-11 instead of 2^-9
      'mcol'   the words of m's last column are lost    'mrow'   those of its last row
    Required on NOISE; on natural input res16 and res11 do not always clear 4 x (the figures are printed).  The fp32 evaluations themselves must stay inside the conditions:
    every position they differ in holds a neighbouring code.  The inputs are the models' own chain with every block exact.  NOT resolved, by anything here: 'direct8'
    (emu_layers.pair8)."""
    net = net_for(key)
    trunk = hashlib.sha1(b''.join(np.ascontiguousarray(v).tobytes() for k, v in sorted(net.sd.items()) if k.startswith(('conv_input', 'relu', 'convt_F')))).hexdigest()
    if (trunk, shape) in _trunks8:      # (a3 and a4 are built on a2's trunk, bit for bit)
        return
    _trunks8[(trunk, shape)] = True
    missed = []
    for kind in ('noise', 'natural'):
        x = image(kind, 41, shape)
        with torch.no_grad():
            taps = el.chain(net, x, torch.float32, n_exact=6, trunk_only=True, chain8=True)[0]
            for i, out8 in ((1, True), (3, True), (1, False)):
                outs = el.arsb_chain(net, i, taps, torch.float64, out8, 0, (None,) + el.BUGS8)
                m64 = outs[0]
                m32 = [el.arsb_chain(net, i, taps, torch.float32, out8, o) for o in el.orders_for(m64.value.numel())]
                seam = el.chain_kernel('arsb%d' % i, 6, shape[1])[1]
                if out8:
                    for m in m32:
                        ok, text, _ = el.code_check(m.hi, m.w8, m64, m32, seam)
                        assert ok, (key, shape, kind, i, 'the reference itself', text)
                for name, bug in zip(el.BUGS8, outs[1:]):
                    ok, text, _ = el.check_orders(bug.value, m64, m32)
                    if out8 and ok:
                        ok, text, _ = el.code_check(bug.hi, bug.w8, m64, m32, seam)
                    print(key, shape, kind, 'arsb%d' % i, 'words' if out8 else 'fp16 pair', name, 'resolved' if not ok else 'NOT resolved', text[:160])
                    if ok and kind == 'noise':
                        missed.append((kind, i, out8, name, text))
    assert not missed, (key, shape, missed)
