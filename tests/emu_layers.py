"""Per-layer models of the ARSB families (Net2x / Net3x / Net4x, NetDN) in the default arithmetic, 'mixed' -- test infrastructure, CPU only.

tests/emu_precision.py emulates a whole forward; end to end that arithmetic is chaotic at the level of its own error (two fp32 summation orders of the
same roundings end 3-4e-4 apart on noise), so no end-to-end comparison can see a kernel that is wrong by 1e-4.  One layer at a time, from the SAME
input, it is not: here every tapped layer of forward_arsb.cpp is a pure function of the tap(s) before it, the state dict and the layer's form,

    model(net, taps, dtype) -> Out(value, hi, floor)

evaluated with dtype = torch.float64 (the reference) and torch.float32 (a second summation order of the same arithmetic: the yardstick of the bound).
Operands are rounded where the kernel rounds them -- read from the kernels, file:line in each docstring (paths under moephoto_amd/csrc) -- products and
sums are taken in `dtype`, the value is returned as fp32.

WHAT A TAP IS (net.h Fwd::tap, misc_kernels.hip:1163-1164): the activation as fp32; of a hi + lo pair the sum fp32(hi) + fp32(lo) * 2^-11.  That sum
does not determine `hi` (a low part of exactly half an ulp -- one value in ~4000 -- puts it midway between two fp16 values), and a single-pass layer
reads `hi` alone, so a pair also leaves the tap NAME.hi.  `pair_of` puts the two together again: lo = (tap - hi) * 2^11.

`taps` is a dict name -> fp32 tensor (NCHW) holding the engine's taps, emu_precision.forward's, or the models' own outputs (`chain`).

THE BOUNDS (`bounds`, `check`): a layer's output `got` is held to the float64 model m64 by
    max|got - m64| <= 4 max|m32 - m64| + F        rms(got - m64) <= 4 rms(m32 - m64) + 2^-23 max|m64|
F (`Out.floor`) is the largest change ONE flipped fp16 rounding inside the layer can cause, computed from the model: late blocks on natural input see
0 to 3 flips, so max|m32 - m64| does not sample them.  Single-pass ARSB: max|w2| ulp16(max|m|).  Up-conv that stores fp16: ulp16(max|out|) (its own
rounding and the PReLU product's are the flips).  0 where the layer rounds to pairs only (a flipped low part moves the value by 2^-22 of it).

THE PRODUCTION FORM (`run_layer(.., chain8=True)`; moe_net_set_debug's value 2 taps it, tests/test_gpu_chain8_layers.py): with the option lo8 on, the default, the
stem, conv_input2 and the exact blocks before the last one store their low part as an e4m3 word, hi + word 2^-9; such a pair's tap comes with NAME.hi and
NAME.w8 (`pair8_of`).  Their output is discrete at the word's step, so beside the two bounds (floor: one step of the largest word) the stored pair is compared
code by code (`code_check`).  Not resolved by any of it: 'direct8', a word made from the unrounded remainder (`pair8`).
"""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

from emu_precision import hilo, prelu, prelu16, q8, r16, shuffle

Out = collections.namedtuple('Out', 'value hi floor w8', defaults=(None,))      # value: fp32 tensor, what the tap returns; hi: fp32 tensor, the pair's fp16 part, or None; w8: the pair's e4m3 word (chain form), or None

INV = 1.0 / 2048.0
BUGS = ('res16', 'col', 'tail16')      # the modelled bugs of tests/test_layer_models_cpu.py (see arsb_single, tail_fused)
W8 = 2.0 ** -9                        # what one unit of a chain pair's e4m3 word is worth: the word holds lo / 4, lo in units of 2^-11
BUGS8 = ('res16', 'res11', 'mcol', 'mrow')      # ... and those of the chain form (see arsb_chain)


def ulp16(v):
    """spacing of fp16 at magnitude v"""
    v = abs(float(v))
    return 2.0 ** -24 if v < 2.0 ** -14 else 2.0 ** (math.floor(math.log2(v)) - 10)


class Net:
    """a checkpoint's weights as the engine packs them, per dtype"""

    def __init__(self, arch, sd):
        self.arch, self.sd = arch, sd
        self.r = 3 if arch == 'net3x' else 2
        self.stages = {'net2x': 1, 'net3x': 1, 'net4x': 2, 'netdn': 0}[arch]
        self._cache = {}

    def T(self, k):
        return torch.from_numpy(np.asarray(self.sd[k], dtype=np.float32))

    def scalar(self, k):
        return float(self.T(k).reshape(-1)[0])

    def w(self, key, dtype, fold=None):
        """(w32, w_hi, w_lo, fp8(w_hi), fp8(w_lo)) of a conv's weights in `dtype`.  weights.cpp:128: the ScaleLayer factor is multiplied in as an fp32
        product BEFORE the split; :130-132: w_hi = fp16(w), w_lo = fp16((w - w_hi) 2^11); :235-236 (pack_q8): e4m3(w_hi 2^8) and e4m3(w_lo 2^8) -- `fp8(.)`
        here carries the 2^-8 the MFMA's scale takes out again (conv64_q8.hip:207-209)."""
        ck = (key, dtype, fold)
        if ck not in self._cache:
            w = self.T(key)
            if fold is not None:
                w = w * float(self.scalar(fold))          # fp32 tensor times a Python float: an fp32 product
            wh, wl = hilo(w)
            self._cache[ck] = tuple(t.to(dtype) for t in (w, wh, wl, q8(wh, 8), q8(wl, 8)))
        return self._cache[ck]

    def up_keys(self, tag):
        pre = 'convt_R1.' if tag == 'r' else 'u.'
        return ['{}{}.'.format(pre, k) for k in range(self.stages)], '{}{}.weight'.format(pre, self.stages) if self.stages else pre[:-1] + '.weight'


def conv(v, w, order=0):
    """the 3x3 convolution in summation order `order`: 0 = `cv`; >= 1: emu_sedn.conv's chunked orders, the MFMA kernels' structure (one 16-channel slice of one tap at a time into
    one accumulator).  In float64 the order is immaterial at the level of these tests; in fp32 each is one more correct evaluation of the same arithmetic."""
    if order == 0:
        return cv(v, w)
    from emu_sedn import conv as chunked      # (emu_sedn imports this module)
    return chunked(v, w, order)


def cv(v, w, b=None):
    """3x3 convolution, zero padding 1, as one matrix product over the unfolded input: three to four times F.conv2d's speed in float64, and in fp32 one more
    summation order that is not the kernels' (the bias is added last; the kernels start their accumulators from it)"""
    B, _, H, W = v.shape
    o = torch.matmul(w.reshape(w.shape[0], -1), F.unfold(v, 3, padding=1)).view(B, w.shape[0], H, W)
    return o if b is None else o + b.view(1, -1, 1, 1)


def pair_of(taps, name, dtype):
    """(value, hi, lo in units of 2^-11) of tap `name` in `dtype`; an fp16 activation (no NAME.hi) is its own fp16 part."""
    v = taps[name].to(dtype)
    h = taps[name + '.hi'].to(dtype) if name + '.hi' in taps else r16(v)
    return v, h, (v - h) * 2048.0


def store_pair(v):
    h, l = hilo(v)
    return h + l * INV, h


def out_pair(v, floor=0.0):
    val, h = store_pair(v)
    return Out(val.float(), h.float(), floor)


# ---- the layers -----------------------------------------------------------------------------------------------------------------------------------------

def stem(net, x, dtype, exact=False):
    """`stem` from x.  fp32 in every mode: misc_kernels.hip:73 (nine fp32 multiply-adds, taps ascending), :78 PReLU in fp32 as v >= 0 ? v : v * slope,
    :78-83 stored as hi = fp16(v), lo = fp16((v - hi) 2^11).  exact: nothing rounded (the fp32 chain against the oracle)."""
    v = prelu(cv(x.to(dtype), net.T('conv_input.weight').to(dtype)), net.scalar('relu.weight'))
    return Out(v.float(), None, 0.0) if exact else out_pair(v)


def conv_q8(a_hi, a_lo, W):
    """conv64_q8.hip:4 (conv64_sq.hip streams the same MFMAs down a column): conv(w_hi, a_hi) + 2^-11 (conv(fp8 w_lo, fp8 a_hi) + conv(fp8 w_hi, fp8 a_lo)),
    all three in one fp32 accumulator.  The activations' fp8 words are e4m3(a / 4), saturating (mfma_stream.h:99-107 cvt4, conv64_q8.hip:151 FP16_OVFL), for
    the fp16 part and for the fp16 remainder alike; scales conv64_q8.hip:207-209.  The w_lo * a_lo product does not exist."""
    _, wh, wl, wh8, wl8 = W
    return cv(a_hi, wh) + (cv(q8(a_hi, -2), wl8) + cv(q8(a_lo, -2), wh8)) * INV


def input2(net, taps, dtype, exact=False):
    """`input2` from `stem`: split operands with the two fp8 correction products (forward_arsb.cpp:160, e.exact = mixed), the output stored as a pair
    (conv64_q8.hip:453 split2)."""
    v, h, l = pair_of(taps, 'stem', dtype)
    W = net.w('conv_input2.weight', dtype)
    return Out(cv(v, W[0]).float(), None, 0.0) if exact else out_pair(conv_q8(h, l, W))


def arsb_keys(i):
    p = 'convt_F{}.0.'.format(i)
    return p + 'conv_1.weight', p + 'conv_2.weight', p + 'relu.weight', p + 'scale.scale'


def arsb_fp32(net, i, taps, dtype):
    """the block with nothing rounded: t + conv_2(PReLU(conv_1(t))) with the ScaleLayer folded into conv_2's weights"""
    k1, k2, ks, kf = arsb_keys(i)
    t = taps['input2' if i == 1 else 'arsb%d' % (i - 1)].to(dtype)
    m = prelu(cv(t, net.w(k1, dtype)[0]), net.scalar(ks))
    return Out((t + cv(m, net.w(k2, dtype, kf)[0])).float(), None, 0.0)


def arsb_exact(net, i, taps, dtype):
    """`arsb{i}` from `arsb{i-1}`, split-operand form as the tapped run launches it (forward_arsb.cpp:225-234: two launches of the conv64_q8 arithmetic;
    the one-launch arsb_sq.hip needs the fp8 chain, which set_debug's value 1 and lo8 = off both turn off, forward_arsb.cpp:204,296; `arsb_chain` is that form).
    conv_1: PReLU in fp32 as max(v, v * slope) (conv64_q8.hip:448), m stored as a pair (:453).  conv_2: weights w * scale split AFTER the fp32 product
    (weights.cpp:128,350), the residual pair added into the accumulator as hi + lo 2^-11 (conv64_q8.hip:436-437), the sum stored as a pair."""
    k1, k2, ks, kf = arsb_keys(i)
    x, xh, xl = pair_of(taps, 'input2' if i == 1 else 'arsb%d' % (i - 1), dtype)
    a = conv_q8(xh, xl, net.w(k1, dtype))
    mh, ml = hilo(torch.maximum(a, a * net.scalar(ks)))
    return out_pair(x + conv_q8(mh, ml, net.w(k2, dtype, kf)))


# ---- the fp8 low-part chain (forward_arsb.cpp:296 chain8; option lo8 on, the default): what the untapped forward runs and moe_net_set_debug's value 2 taps --------------

def ulp8(v):
    """spacing of e4m3 at magnitude v (three mantissa bits; subnormals below 2^-6 in steps of 2^-9)"""
    v = abs(float(v))
    return 2.0 ** -9 if v < 2.0 ** -6 else 2.0 ** (math.floor(math.log2(min(v, 448.0))) - 3)


def step8(w):
    """ulp8, elementwise on a tensor of words"""
    a = w.abs().double().clamp(2.0 ** -6, 448.0)
    return torch.exp2(torch.floor(torch.log2(a)) - 3.0)


def word8(l16):
    """the e4m3 word of an fp16 low part: e4m3(l16 / 4), round to nearest even, saturating at +-448 (never a NaN: MODE.FP16_OVFL, conv64_q8.hip:151, misc_kernels.hip:34).
    mfma_stream.h:99-107 cvt4 (v_cvt_scalef32_pk_fp8_f16 divides by its scale operand, 4.0); the stem's own copy of that block, misc_kernels.hip:93-98."""
    return q8(l16, -2) * 0.25


def pair8(v):
    """(value, hi, word) of v stored as a pair of the chain: hi = fp16(v), lo16 = fp16((v - hi) 2^11) (split2: conv64_sq.hip:385, misc_kernels.hip:79,84), word =
    e4m3(lo16 / 4) (`word8`; conv64_sq.hip:397 cvt4 of the split's low halves, arsb_sq.hip:386-, conv64_q8.hip:460-) -- the word is made from the ROUNDED fp16 low part, two
    roundings.  value = hi + word 2^-9, what a reader adds (conv64_sq.hip:371-373 op_add).
    NOT RESOLVED by anything in these tests ('direct8'): a word made from the unrounded remainder e4m3((v - hi) 2^9) differs from this one only where the fp16 rounding
    of the low part crosses an e4m3 tie -- 0 to 582 of up to 1.35 M positions on the reference, far inside the share two correct summation orders differ by."""
    h, l = hilo(v)
    w = word8(l)
    return h + w * W8, h, w


def out_pair8(v):
    """an OUT8 layer's output.  floor: one step of the e4m3 word at the largest low part, times 2^-9 -- what ONE flipped word rounding moves the value by; the output is
    discrete at that step, so the two correct models' spread is made of such flips and need not hold the largest"""
    val, h, w = pair8(v)
    return Out(val.float(), h.float(), ulp8(w.abs().max()) * W8, w.float())


def pair8_of(taps, name, dtype):
    """(value, hi, word) of tap `name` stored as (fp16, word), from NAME.hi and NAME.w8: the stored pair exactly (the tap's own sum is rounded to fp32)"""
    h, w = taps[name + '.hi'].to(dtype), taps[name + '.w8'].to(dtype)
    return h + w * W8, h, w


def stem8(net, x, dtype, order=0):
    """`stem` of the chain: `stem`'s fp32 sums and PReLU, stored as (fp16, word) (StemArgs::out_lo8, misc_kernels.hip:84-99: the fp16 low part is formed, then converted)"""
    return out_pair8(prelu(conv(x.to(dtype), net.T('conv_input.weight').to(dtype), order), net.scalar('relu.weight')))


def conv_q8_in8(a_hi, a_w8, W, order=0):
    """`conv_q8` with IN8 (conv64_q8.hip:142-143, :355-; conv64_sq.hip:120): the a_lo operand of the w_hi8 product IS the stored word -- fetched by DMA into the fp8 image, not
    converted again; its 2^2 rides in the MFMA's scale (conv64_q8.hip:207-209) as it does for a converted low part"""
    _, wh, wl, wh8, wl8 = W
    return conv(a_hi, wh, order) + (conv(q8(a_hi, -2), wl8, order) + conv(a_w8 * 4.0, wh8, order)) * INV


def input2_chain(net, taps, dtype, order=0):
    """`input2` of the chain from the stem's (fp16, word): IN8, OUT8 (forward_arsb.cpp:302 A.lo8 = Bb.lo8 = chain8; conv64_sq<0, true> or conv64_q8<0, true, true>)"""
    _, h, w = pair8_of(taps, 'stem', dtype)
    return out_pair8(conv_q8_in8(h, w, net.w('conv_input2.weight', dtype), order))


def arsb_chain(net, i, taps, dtype, out8, order=0, bug=None):
    """`arsb{i}` from `arsb{i-1}`, an exact block of the chain: one launch of arsb_sq.hip (forward_arsb.cpp:204-223) or conv64_sq / conv64_q8 twice with IN8 (:225-234) -- the same
    arithmetic (the bit-identity test of tests/test_gpu_parity.py).  conv_1 on (x_hi, x word), PReLU in fp32 as max(v, v * slope) (conv64_sq.hip:380), m crosses as (fp16, word)
    (in LDS: arsb_sq.hip:15-16 m_hi, m_lo8; through HBM: forward_arsb.cpp:227 m.lo8); conv_2 on it with w * scale split after the fp32 product; the residual added into the
    accumulator as x_hi + x word 2^-9 (conv64_sq.hip:371-373, arsb_sq.hip:371-378).  out8 (i < n_exact, forward_arsb.cpp:213,220): stored as (fp16, word); else the last exact
    block: fp16 low part again (forward_arsb.cpp:232, into the stem's low buffer or lo16x), floor 0 as for every pair.
    bugs, a tuple gives a tuple of outputs (None: the correct layer): 'res16' the residual's word is dropped; 'res11' it is added at 2^-11; 'mcol' / 'mrow' the words of m's last
    column / row are lost (read as zero)."""
    k1, k2, ks, kf = arsb_keys(i)
    x, xh, xw = pair8_of(taps, 'input2' if i == 1 else 'arsb%d' % (i - 1), dtype)
    a = conv_q8_in8(xh, xw, net.w(k1, dtype), order)
    _, mh, mw = pair8(torch.maximum(a, a * net.scalar(ks)))
    W2 = net.w(k2, dtype, kf)
    store = out_pair8 if out8 else out_pair
    c2, outs = None, []
    for b in (bug if isinstance(bug, tuple) else (bug,)):
        if b in ('mcol', 'mrow'):
            mb = mw.clone()
            if b == 'mcol':
                mb[..., -1] = 0.0
            else:
                mb[..., -1, :] = 0.0
            outs.append(store(x + conv_q8_in8(mh, mb, W2, order)))
            continue
        if c2 is None:
            c2 = conv_q8_in8(mh, mw, W2, order)
        outs.append(store((xh if b == 'res16' else xh + xw * INV if b == 'res11' else x) + c2))
    return tuple(outs) if isinstance(bug, tuple) else outs[0]


def tail_dn8(net, taps, dtype, order=0):
    """NetDN's y on the chain: tail3_kernel<2> (misc_kernels.hip:221,1254) -- `tail_tapped`'s NetDN arithmetic with the stem read as hi + word 2^-9 (:285-290) against the
    22-bit weights w_hi + w_lo 2^-11; `arsb6` is an fp16 pair (the last exact block's lo16x, or a single-pass block's)."""
    Wr, Wu = net.w(net.up_keys('r')[1], dtype), net.w(net.up_keys('u')[1], dtype)
    r = pair_of(taps, 'arsb6', dtype)[0]
    u = pair8_of(taps, 'stem', dtype)[0] if 'stem.w8' in taps else pair_of(taps, 'stem', dtype)[0]
    return Out((conv(r, Wr[1] + Wr[2] * INV, order) + conv(u, Wu[1] + Wu[2] * INV, order)).float(), None, 0.0)


def arsb_single(net, i, taps, dtype, bug=None, drop_lo=False, order=0):
    """drop_lo (block 6 of an SR net in the production form, forward_arsb.cpp:174 drop6, arsb32c.hip's drop_lo): the sum is stored as its fp16 part alone -- one more rounding
    whose flip is worth ulp16(max|out|), added to the floor.
    `arsb{i}` from `arsb{i-1}`, single-pass form (arsb32c.hip; forward_arsb.cpp:175-203): hi + lo(t) + conv_2(m), m = PReLU16(fp16(conv_1(hi(t)))).
    conv_1 reads the stream's fp16 part only (the x patch DMA is of x_hi, arsb32c.hip:386) against fp16(w1); its output is rounded to fp16 FIRST and
    PReLU'd on packed halves, max(h, fp16(h * fp16(slope))) (arsb32c.hip:398-400) -- not PReLU in fp32 and then the rounding; m is zero outside the
    image (:360-368).  conv_2: fp16(w2 * scale), the product formed in fp32 (weights.cpp:128,350; forward_arsb.cpp:179).  The residual is added in fp32
    as x_hi + x_lo 2^-11 (arsb32c.hip:447-448) and the sum stored as a pair (:465).
    floor: max|w2| ulp16(max|m|), one flipped rounding of m.
    bug 'res16': the residual adds only the stream's fp16 part.  bug 'col': the last column of conv_1's output is treated as zero.  A tuple of bugs
    (None among them: the correct layer) gives a tuple of outputs from one evaluation of conv_1."""
    k1, k2, ks, kf = arsb_keys(i)
    x, xh, _ = pair_of(taps, 'input2' if i == 1 else 'arsb%d' % (i - 1), dtype)
    w2 = net.w(k2, dtype, kf)[1]
    m = prelu16(r16(conv(xh, net.w(k1, dtype)[1], order)), net.scalar(ks))
    floor = float(w2.abs().max()) * ulp16(m.abs().max())
    c2 = conv(m, w2, order)
    outs = []
    if drop_lo:
        o = r16(x + c2)
        return Out(o.float(), None, floor + ulp16(o.abs().max()))
    for b in (bug if isinstance(bug, tuple) else (bug,)):
        if b == 'col':
            mb = m.clone()
            mb[..., -1] = 0.0
            outs.append(out_pair(x + conv(mb, w2, order), floor))
        else:
            outs.append(out_pair((xh if b == 'res16' else x) + c2, floor))
    return tuple(outs) if isinstance(bug, tuple) else outs[0]


def up_conv(net, p, a_hi, dtype, form, order=0):
    """one upsampler stage from the fp16 activation `a_hi` (forward_arsb.cpp:117: in 'mixed' the upsampler convs take the fp16 parts): fp16(w), the bias as
    the accumulators' initial value (fp32; conv3x3_sp.hip:67), pixel shuffle.
    form 'fp16' (every stage that stores its tensor; the fused tail without the split): rounded to fp16 FIRST, then PReLU on packed halves with an fp16
        slope (conv3x3_rw.hip:388-394 act8, conv3x3_sp.hip:331-342, conv3x3_ps4.hip:323-325, conv3x3_ps9.hip:306).  floor: ulp16(max|out|).
    form 'split' (the R branch's fused tail): PReLU in fp32 as max(v, v * slope), then hi / lo (conv3x3_rw.hip:397-402 act8s, conv3x3_sp.hip:327-329,
        conv3x3_ps4.hip:320-321, conv3x3_ps9.hip:302-303).
    form 'fp32': nothing rounded."""
    W = net.w(p + '0.weight', dtype)
    slope = net.scalar(p + '2.weight')
    v = shuffle(conv(a_hi, W[0] if form == 'fp32' else W[1], order) + net.T(p + '0.bias').to(dtype).view(1, -1, 1, 1), net.r)
    if form == 'fp32':
        return Out(prelu(v, slope).float(), None, 0.0)
    if form == 'split':
        return out_pair(torch.maximum(v, v * slope))
    o = prelu16(r16(v), slope)
    return Out(o.float(), None, ulp16(o.abs().max()))


def up(net, tag, k, taps, dtype, exact=False, order=0):
    """`r.up{k}` / `u.up{k}` from the stage before (`arsb6` / `stem` for k = 0), as the tapped run stores it: fp16"""
    src = '%s.up%d' % (tag, k - 1) if k else ('arsb6' if tag == 'r' else 'stem')
    v, h, _ = pair_of(taps, src, dtype)
    return up_conv(net, net.up_keys(tag)[0][k], v if exact else h, dtype, 'fp32' if exact else 'fp16', order)


def tail_tapped(net, taps, dtype, exact=False):
    """The final y of the tapped run.
    SR nets, from the last `r.up*` and `u.up*` taps: set_debug turns the fused tail off (forward_arsb.cpp:20), the branches end in fp16 tensors without a
    low part and Fwd::tail then passes no low parts at all (forward.cpp:304-309): tail3_kernel<0> (misc_kernels.hip:1191, :313-337) -- fp16(w) times fp16
    activations, both branches, fp32 sums.  Neither the 22-bit weights nor the split R activations of the fused tail exist in this run (`tail_fused`).
    NetDN, from `arsb6` and `stem` (forward_arsb.cpp:355): both are pairs, so tail3_kernel<1>: x = hi + lo 2^-11 and w = w_hi + w_lo 2^-11 put together in
    fp32 (exact there), fp32 FMAs (misc_kernels.hip:260,293,302) -- the lo * lo term included."""
    ra, ua = ('arsb6', 'stem') if net.arch == 'netdn' else ('r.up%d' % (net.stages - 1), 'u.up%d' % (net.stages - 1))
    Wr, Wu = net.w(net.up_keys('r')[1], dtype), net.w(net.up_keys('u')[1], dtype)
    r, u = taps[ra].to(dtype), taps[ua].to(dtype)
    if exact:
        return Out((cv(r, Wr[0]) + cv(u, Wu[0])).float(), None, 0.0)
    if net.arch == 'netdn':
        return Out((cv(r, Wr[1] + Wr[2] * INV) + cv(u, Wu[1] + Wu[2] * INV)).float(), None, 0.0)
    return Out((cv(r, Wr[1]) + cv(u, Wu[1])).float(), None, 0.0)


def tail_is_fused(arch, w):
    """Does the production run of a small tile of width w end in the fused tail?  can_fuse_tail (forward_arsb.cpp:17-33) asks conv3x3_sp_applicable with
    c.tail, which wants the last stage's input width to be a multiple of 4 (conv3x3_sp.hip:721); the other conditions hold for the zoo's nets at small
    shapes.  Otherwise the branches store fp16 tensors and end in tail3_kernel<0>, exactly as the tapped run does."""
    if arch == 'netdn':
        return False
    return (2 * w if arch == 'net4x' else w) % 4 == 0


def tail_fused(net, taps, dtype, fused=True, bug=None, order=0):
    """y of the production run as the composite "R branch from tap `arsb6` + U branch from tap `stem`" (the fused tail has no taps).
    Both branches read fp16 parts (forward_arsb.cpp:356); every stage but the last stores fp16 (`up_conv` form 'fp16').  The last stage and the 64 -> 1 tail
    conv are one kernel: the tail's weights as fp16 part + fp16 remainder (weights.cpp:316-337; the low-order rows are folded in with 2^-11,
    conv3x3_sp.hip:355, conv3x3_ps4.hip:350), so ~22 bits.  R (tail_split = r, net.h Fwd::tail_split_for): the activation is split too, and the tail sum
    is (w_hi + w_lo 2^-11) hi + w_hi lo 2^-11 -- fragments 4..7 carry w_hi only (weights.cpp:334), there is no w_lo * lo product.  U: fp16 activation.
    The two sums are added in fp32 (tailadd / tapsum).  fused = False: `tail_tapped`'s arithmetic on the same two taps.  NetDN: `tail_tapped`.
    floor: one flipped fp16 rounding of a stored stage, carried to y through |weights| (a flip of stage 0 of Net4x through stage 1 and the tail; PReLU
    slopes are below 1 in magnitude), or of U's last activation through the tail.
    bug 'tail16': the R tail reads fp16 activations only (the low parts dropped).  A tuple of bugs (None: the correct composite) gives a tuple of outputs."""
    if net.arch == 'netdn':
        return tail_tapped(net, taps, dtype)
    cv = lambda v, w: conv(v, w, order)
    ys, floor = [], 0.0
    for tag, src in (('r', 'arsb6'), ('u', 'stem')):
        ups, tk = net.up_keys(tag)
        _, a, _ = pair_of(taps, src, dtype)
        W = net.w(tk, dtype)
        for k, p in enumerate(ups):
            last = k == len(ups) - 1
            o = up_conv(net, p, a, dtype, 'split' if (last and fused and tag == 'r') else 'fp16', order)
            if o.hi is None:      # a stored fp16 tensor: its flips reach y through what follows
                floor = max(floor, o.floor * _gain(net, ups[k + 1:], tk))
            a = o.value.to(dtype)
            if o.hi is not None:
                hi = o.hi.to(dtype)
                lo = (a - hi) * 2048.0
        if not fused:
            ys.append(cv(a, W[1]))
        elif tag == 'r':
            ys.append(cv(hi, W[1] + W[2] * INV))
            low = cv(lo, W[1]) * INV
        else:
            ys.append(cv(a, W[1] + W[2] * INV))
    outs = tuple(Out((ys[0] + (0.0 if (b == 'tail16' or not fused) else low) + ys[1]).float(), None, floor) for b in (bug if isinstance(bug, tuple) else (bug,)))
    return outs if isinstance(bug, tuple) else outs[0]


def _gain(net, later, tail_key):
    """largest |dy| a unit change of ONE element of a stored stage can cause: through the absolute weights of the stages behind it and of the tail conv"""
    ck = ('gain', tuple(later), tail_key)
    if ck not in net._cache:
        d = torch.zeros(64, 64, 7, 7, dtype=torch.float64)
        d[torch.arange(64), torch.arange(64), 3, 3] = 1.0      # plane c: a unit at channel c
        for p in later:
            d = shuffle(cv(d, net.w(p + '0.weight', torch.float64)[1].abs()), net.r)
        net._cache[ck] = float(cv(d, net.w(tail_key, torch.float64)[1].abs()).max())
    return net._cache[ck]


# ---- a net's tapped layers in order, and the chain --------------------------------------------------------------------------------------------------------

def layer_names(arch):
    st = {'net2x': 1, 'net3x': 1, 'net4x': 2, 'netdn': 0}[arch]
    return ['stem', 'input2'] + ['arsb%d' % i for i in range(1, 7)] + ['%s.up%d' % (t, k) for t in ('u', 'r') for k in range(st)] + ['y']


def run_layer(net, name, taps, dtype, n_exact=0, exact=False, bug=None, chain8=False, order=0, fused=True):
    """layer `name` from `taps` ('stem' from taps['x']); n_exact: the leading blocks in the split-operand form; exact: nothing rounded.
    chain8 = False: the run tapped under set_debug's value 1.  chain8 = True: the production form, what value 2 taps -- selected by (n_exact, i): with n_exact >= 1 the stem,
    conv_input2 and blocks 1 .. n_exact - 1 store (fp16, word), block n_exact reads words and stores an fp16 pair, the blocks behind it are single-pass on fp16 pairs
    (`arsb_single`, unchanged: what they show is that the low-part buffer handed over, A.lo / lo16x, is the one read); with n_exact = 0 there is no chain and the pairs are
    fp16 (forward_arsb.cpp:296 nx >= 1).  Either way block 6 of an SR net stores its fp16 part alone (drop_lo), and y is the fused composite (`fused`: `tail_is_fused`) or
    NetDN's tail on the stem's pair as stored.  order: the summation order of the layer's convolutions (`conv`; the layers of the run tapped under value 1 keep `cv`)."""
    c8 = chain8 and n_exact >= 1 and not exact
    if name == 'stem':
        return stem8(net, taps['x'], dtype, order) if c8 else stem(net, taps['x'], dtype, exact)
    if name == 'input2':
        return input2_chain(net, taps, dtype, order) if c8 else input2(net, taps, dtype, exact)
    if name.startswith('arsb'):
        i = int(name[4:])
        if exact:
            return arsb_fp32(net, i, taps, dtype)
        if i <= n_exact:
            return arsb_chain(net, i, taps, dtype, i < n_exact, order, bug) if c8 else arsb_exact(net, i, taps, dtype)
        return arsb_single(net, i, taps, dtype, bug, drop_lo=chain8 and i == 6 and net.arch != 'netdn', order=order)
    if name == 'y':
        if chain8 and not exact:
            return tail_dn8(net, taps, dtype, order) if net.arch == 'netdn' else tail_fused(net, taps, dtype, fused, order=order)
        return tail_tapped(net, taps, dtype, exact)
    tag, k = name.split('.up')
    return up(net, tag, int(k), taps, dtype, exact, order)


def put(taps, name, o):
    """a layer's output as the taps it leaves: NAME, NAME.hi of a pair, NAME.w8 of a chain pair"""
    taps[name] = o.value
    for k, v in (('.hi', o.hi), ('.w8', o.w8)):
        if v is not None:
            taps[name + k] = v
        else:
            taps.pop(name + k, None)


def chain(net, x, dtype, n_exact=0, exact=False, trunk_only=False, chain8=False):
    """every layer (trunk_only: stem .. arsb6) from the models' own taps: (taps, y).  chain8: the production form (`run_layer`); its stored upsampler stages are not
    listed (the composite y runs them)."""
    taps = {'x': torch.from_numpy(np.asarray(x, dtype=np.float32))}
    names = layer_names(net.arch)
    for name in (names[:8] + ([] if trunk_only else ['y'])) if (chain8 and not exact) else names[:8 if trunk_only else None]:
        put(taps, name, run_layer(net, name, taps, dtype, n_exact, exact, chain8=chain8))
    return taps, taps.get('y')


def stores_words(arch, name, n_exact):
    """does layer `name` of the production form store (fp16, word)?  (forward_arsb.cpp:302, :220)"""
    return n_exact >= 1 and (name in ('stem', 'input2') or (name.startswith('arsb') and int(name[4:]) < n_exact))


def chain_kernel(name, n_exact, H, exact_fuse=True):
    """(kernel, seam) of a chain layer at height H, by the engine's rules: an exact block runs on arsb_sq (30-pixel columns, arsb_sq.hip:34) where exact_fuse is on and
    arsb_sq_applicable (arsb_sq.hip:492-: H even, at least 2; the zoo's slopes are below 1 and these shapes far inside the addressing range); otherwise, and for conv_input2,
    one conv at a time on conv64_sq where conv64_sq_applicable (conv64_sq.hip:505-: the same condition on H) or on conv64_q8, the patch form -- 32-pixel columns both
    (conv64_sq.hip:51, conv64_q8.hip:42).  The stem is pointwise in its output: no seam."""
    if name == 'stem':
        return 'stem', 0
    even = H % 2 == 0 and H >= 2
    if name != 'input2' and exact_fuse and even:
        return 'arsb_sq', 30
    return ('conv64_sq' if even else 'conv64_q8'), 32


# ---- the bounds -------------------------------------------------------------------------------------------------------------------------------------------

def _rms(d):
    return float(d.double().pow(2).mean().sqrt())


def bounds(m64, m32):
    """(max bound, rms bound) of a layer from its two correct models"""
    d = m32.value.double() - m64.value.double()
    return 4.0 * float(d.abs().max()) + m64.floor, 4.0 * _rms(d) + 2.0 ** -23 * float(m64.value.abs().max())


def distance(got, m64):
    d = torch.as_tensor(got).double() - m64.value.double()
    return float(d.abs().max()), _rms(d)


def check(got, m64, m32):
    """(ok, text, figures): `got` against the float64 model under the two bounds.  figures: the distances dm, dr, the reference's own spread sm, sr
    (max and rms of m32 - m64), the floor, and `beyond`: how many values lie further from m64 than 4 sm (isolated flips, or everywhere?)."""
    bm, br = bounds(m64, m32)
    d = torch.as_tensor(got).double() - m64.value.double()
    dm, dr = float(d.abs().max()), _rms(d)
    s = m32.value.double() - m64.value.double()
    sm, sr = float(s.abs().max()), _rms(s)
    fig = dict(dm=dm, dr=dr, sm=sm, sr=sr, floor=m64.floor, bm=bm, br=br, beyond=int((d.abs() > 4.0 * sm).sum()), n=d.numel())
    text = 'max {dm:.3e} (bound {bm:.3e} = 4 x {sm:.3e} + floor {floor:.1e}; {beyond} of {n} values beyond 4 x spread)  rms {dr:.3e} (bound {br:.3e}, spread {sr:.3e})'.format(**fig)
    return dm <= bm and dr <= br, text, fig


def orders_for(n, least=2):
    """the fp32 orders whose largest spread is the yardstick of a layer with n output values: emu_sedn.orders_of's rule.  Two correct evaluations of a layer with an fp16
    rounding inside differ in the values whose fp32 sum lies within an fp32 step of an fp16 tie, about one in 2^13 per order; a spread taken over fewer than 2^18 values and
    orders together expects fewer than 32 of them and is no estimate (at 2 x 2 x 40 x 64 values ONE flipped rounding of m is the whole rms, and one order has one or has
    none), so small shapes get more orders -- permuted chunk sequences -- until n x orders reaches 2^18, at most 12; from 131 072 values on the two named ones.  The count
    comes from n alone.  least: 2 for a layer that stores words (its code-domain share wants `cv` and the chunked order at every size), 1 elsewhere (from 2^18 values on
    `cv` alone, as tests/test_gpu_layer_parity.py has it)."""
    return tuple(range(max(least, min(12, -(-2 ** 18 // n)))))


def check_orders(got, m64, m32s):
    """`check` with the spreads sm, sr being the largest of the fp32 orders `m32s` (emu_sedn.check2): the bounds are the same two"""
    figs = [check(got, m64, m)[2] for m in m32s]
    f = figs[0]
    f['sm'], f['sr'] = max(g['sm'] for g in figs), max(g['sr'] for g in figs)
    f['bm'] = 4.0 * f['sm'] + m64.floor
    f['br'] = 4.0 * f['sr'] + 2.0 ** -23 * float(m64.value.abs().max())
    f['beyond'] = min(g['beyond'] for g in figs)
    text = 'max {dm:.3e} (bound {bm:.3e} = 4 x {sm:.3e} + floor {floor:.1e}; {beyond} of {n} values beyond 4 x spread)  rms {dr:.3e} (bound {br:.3e}, spread {sr:.3e}; {k} orders)'.format(k=len(m32s), **f)
    return f['dm'] <= f['bm'] and f['dr'] <= f['br'], text, f


# ---- the code domain: layers that store (fp16, word) ------------------------------------------------------------------------------------------------------
# Such a layer's output is discrete at the word's step (2^-18 at the smallest), so the spread of two correct models is made of flipped words and the value bounds
# alone leave room for a bug worth one step everywhere.  What two correct evaluations share is HOW OFTEN they differ: the stored pair (hi, word) is compared code by code.

Z_BAND = 5.0


def ulp16_t(v):
    a = v.abs().double().clamp(2.0 ** -14, 65504.0)
    return torch.exp2(torch.floor(torch.log2(a)) - 10.0)


def code_bands(H, W, seam):
    """name -> (H, W) mask: the two outermost rows / columns at the four image edges, and the two columns on each side of every interior kernel-column seam (multiples of `seam`)"""
    z = lambda: torch.zeros(H, W, dtype=torch.bool)
    out = {}
    for nm, sl in (('top', (slice(0, 2), slice(None))), ('bottom', (slice(max(H - 2, 0), H), slice(None))), ('left', (slice(None), slice(0, 2))), ('right', (slice(None), slice(max(W - 2, 0), W)))):
        m = z()
        m[sl] = True
        out[nm] = m
    if seam:
        m = z()
        for c in range(seam, W, seam):
            m[:, max(c - 2, 0):min(c + 2, W)] = True
        if m.any():
            out['seams/%d' % seam] = m
    return out


def code_check(ghi, gw8, m64, m32s, seam, adjacent=True):
    """(ok, text, figures): the stored pair (ghi, gw8) against the float64 model's, in the code domain.
      share   the share of positions whose pair differs from m64's is at most 4 x the largest share by which an fp32 evaluation in `m32s` differs from it (the project's 4:
              2 for two draws of the same noise, 2 for the kernels' own orders, unmeasured -- tests/test_gpu_layer_parity.py).
      bands   the same share on each band of `code_bands`, held to 4 x the reference's OVERALL share p plus Z_BAND standard deviations of a binomial share at that rate over the
              band's n positions, 5 sqrt(4p (1 - 4p) / n): positions flip nearly independently (each is its own sum), a correct kernel's band is then a draw at a rate of
              at most 4p, and 5 sigma leaves 3e-7 per band -- under one false alarm in a thousand runs of the ~2 000 bands of the GPU suite.  Derived, not measured.
      adjacent  every differing position holds a NEIGHBOURING code: |value - m64's| <= one step of the word there x 2^-9, plus one fp16 step where hi differs.  (False: counted
              and reported only -- for a comparison whose fp32 order is a library's, tests/test_layer_models_cpu.py.)"""
    ghi, gw8 = torch.as_tensor(ghi).double(), torch.as_tensor(gw8).double()
    mhi, mw8 = m64.hi.double(), m64.w8.double()
    diff = (ghi != mhi) | (gw8 != mw8)
    p = max(float(((m.hi.double() != mhi) | (m.w8.double() != mw8)).double().mean()) for m in m32s)
    cap = 4.0 * p
    share = float(diff.double().mean())
    H, W = diff.shape[2:]
    fig = dict(p=p, share=share, n=diff.numel(), bands={})
    bad = [] if share <= cap else ['share %.4f > 4 x %.4f' % (share, p)]
    for nm, mask in code_bands(H, W, seam).items():
        d = diff[:, :, mask]
        n = d.numel()
        lim = cap + Z_BAND * math.sqrt(max(cap * (1.0 - cap), 0.0) / n)
        sb = float(d.double().mean())
        fig['bands'][nm] = (sb, lim, n)
        if sb > lim:
            bad.append('band %s share %.4f > %.4f (n %d)' % (nm, sb, lim, n))
    dv = ((ghi + gw8 * W8) - (mhi + mw8 * W8)).abs()
    allow = step8(torch.maximum(gw8.abs(), mw8.abs())) * W8 + (ghi != mhi).double() * ulp16_t(torch.maximum(ghi.abs(), mhi.abs()))
    far = int((dv > allow).sum())
    fig['far'] = far
    if far and adjacent:
        bad.append('%d positions differ by more than one code (worst %.3e against %.3e allowed there)' % (far, float(dv[dv > allow].max()), float(allow[dv > allow].min())))
    worst = max(fig['bands'].items(), key=lambda kv: kv[1][0] / kv[1][1] if kv[1][1] else (float('inf') if kv[1][0] else 0.0))
    text = 'codes: share {:.4f} (reference {:.4f}, cap {:.4f}); worst band {} {:.4f} / {:.4f}; {} beyond one code'.format(share, p, cap, worst[0], worst[1][0], worst[1][1], far)
    return not bad, text + ('  <<< ' + '; '.join(bad) if bad else ''), fig
