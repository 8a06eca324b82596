"""Per-layer models of SEDN in plain fp16, the arithmetic it ships in -- test infrastructure, CPU only; the companion of tests/emu_layers.py, same helpers, same bounds.

End to end SEDN sits 4-6e-4 from the oracle by its own fp16 rounding and every comparison with the oracle allows 1e-3, so a kernel that is wrong by 1e-4 passes all of
them.  One layer from one input is not chaotic: every tap of forward_sedn.cpp is a pure function of the taps before it and the state dict,

    model(net, k, taps, dtype) -> Out(value, None, floor)

evaluated with dtype = torch.float64 (m64, the reference) and torch.float32 (m32, a second summation order of the same arithmetic: the yardstick of the bound, see
emu_layers.bounds).  Operands are rounded where the kernel rounds them -- read from the kernels, file:line in each docstring (paths under moephoto_amd/csrc).

THE TAPS (forward_sedn.cpp, moe_net_set_debug value 2: taps and nothing else -- the production forward).  Fused block tail, per block K: bK.rb0, bK.rb2, bK.mean, bK.weff,
blockK; `stem` in front, `y` behind.  bK.weff is the fp16 A-fragment buffer as it lies in memory and bK.wtrans (unfused form: bK.rb0, bK.rb2, bK.rb4, bK.wtrans, blockK)
likewise: `unpack_weff` / `unpack_wtrans` undo the fragment order, and `taps` holds the UNPACKED tensors under those names.

ACCUMULATORS ARE fp32.  A kernel's sum is an fp32 number before it is rounded to fp16, and the LeakyReLU product and the residual sum of a block's epilogue are fp32
operations: the float64 model rounds to fp32 there too (`r32`), because fp16(fp32(v)) is not fp16(v) for one value in 2^13 -- as many flipped values as the order of
the sums itself produces at these sizes.  What stays between m64 and the engine is the ORDER of the sums inside the accumulator.

TWO fp32 ORDERS (`order`).  The yardstick of a bound is the spread of an fp32 evaluation around m64; `check2` takes the largest spread of its orders: order 0 (emu_layers.cv: one
matrix product over the unfolded input) and order 1 (the accumulator fed one tap and 16-channel slice at a time, as the MFMA kernels feed theirs; at small sizes further permutations of that sequence, `orders_of`; W_eff in four chunks of 64 terms; `mean` with the pixels summed FIRST and the 576-term product last; the gate as the kernels step through it, and with its v_exp_f32 one fp32 step off either way: `gate`).  One
order samples a layer's handful of flipped fp16 roundings poorly at 2e4 values, and for `mean` order 0 is no yardstick of the kernels at all: a mean over H W of per-pixel
sums averages H W independent rounding errors away (it agrees with m64 to one fp32 step), while every kernel form adds up 1e4 pixels per channel first and multiplies
last, as order 1 does.  The factor 4 and the form of the bounds are emu_layers.bounds', unchanged; both spreads are the reference's own, never the engine's.

FLOORS.  Every layer that stores fp16 gets F = ulp16(max|out|): a sum that differs in its last fp32 bit flips the fp16 rounding of a value that lies at a tie, and the
flipped value is wrong by one fp16 step of ITS magnitude, at most that of the largest.  `mean` and `y` store fp32: F = 0.
"""
import numpy as np
import torch
import torch.nn.functional as F

import emu_layers as el
from emu_layers import Out, cv, prelu16, r16, ulp16

S32 = float(np.float32(0.2))      # LeakyReLU's slope where a kernel multiplies in fp32 (weights.cpp:371,374-377: 0.2f)
BUGS = ('corner', 'ragged', 'gateperm')      # the modelled bugs of tests/test_sedn_models_cpu.py (see mean_shifted, weff)
# input kind 'planes': plane k of the natural image times PLANE_FACTORS[k].  Twelve factors inside [0, 1] lie too close for twelve planes (two planes 0.07 apart differ by
# 2e-4 in their gates): beyond the first five the factors leave the image range, which a layer test may do
PLANE_FACTORS = (1.0, 0.5, 0.1, 0.75, 0.25, 1.5, 2.0, 2.75, 3.5, -0.5, -1.0, -2.0)
SEED = 43      # of the images of tests/test_gpu_sedn_layers.py; tests/test_sedn_models_cpu.py checks its conditions on the same images


class Net:
    """an SEDN checkpoint's weights per dtype"""

    def __init__(self, sd):
        self.arch, self.sd = 'sedn', sd
        self._cache = {}

    def T(self, k, dtype=torch.float32):
        ck = (k, dtype)
        if ck not in self._cache:
            self._cache[ck] = torch.from_numpy(np.asarray(self.sd[k], dtype=np.float32)).to(dtype)
        return self._cache[ck]

    def w16(self, k, dtype):
        """fp16(w): what pack_conv stores for a single-pass layer (weights.cpp:128-131)"""
        ck = (k, dtype, 16)
        if ck not in self._cache:
            self._cache[ck] = r16(self.T(k)).to(dtype)
        return self._cache[ck]

    def blk(self, k, name, dtype, half=False):
        key = 'convt_F1.{}.{}.weight'.format(k, name)
        return self.w16(key, dtype) if half else self.T(key, dtype)


def lrelu(v, slope=S32):
    """LeakyReLU in the accumulator's precision: max(v, v * slope) = v >= 0 ? v : v * slope for a slope below 1"""
    return torch.maximum(v, v * slope)


def planes_image(natural):
    """input kind 'planes': the natural image (B, H, W) with plane k multiplied by PLANE_FACTORS[k], so that the planes' squeeze-excite gates differ by many fp16 steps of
    W_eff -- on the natural image two planes' gates differ by 7e-4 to 4e-2, about one step, and a kernel that took another plane's weights would pass"""
    f = np.asarray(PLANE_FACTORS[:natural.shape[0]], dtype=np.float32)
    return (natural * f[:, None, None]).astype(np.float32)


# ---- the fragment orders ------------------------------------------------------------------------------------------------------------------------------------

def _weff_index():
    """flat index into a plane's 72 * 512 fp16 values of W_eff[co][ci][tap].  misc_kernels.hip:893-894,899-902 (sedn_weff's stores), the order of weights.cpp:103-104,120-129
    (pack_conv): fragment f = tap * 8 + ks * 2 + nblk, lane l, element e hold co = 32 nblk + l % 32, ci = 16 ks + 8 (l / 32) + e"""
    co, ci, tap = np.meshgrid(np.arange(64), np.arange(64), np.arange(9), indexing='ij')
    f = tap * 8 + (ci // 16) * 2 + co // 32
    lane = 32 * ((ci % 16) // 8) + co % 32
    return torch.from_numpy(((f * 64 + lane) * 8 + ci % 8).reshape(-1))


def _wtrans_index():
    """flat index into a plane's 32 * 512 values of the 1x1 trans weights W[co][ci], 256 input channels in four segments.  misc_kernels.hip:662-667 (sedn_se), weights.cpp:103-104:
    fragment f = (seg * 4 + ks) * 2 + nblk, lane l, element e hold co = 32 nblk + l % 32, ci = 64 seg + 16 ks + 8 (l / 32) + e"""
    co, ci = np.meshgrid(np.arange(64), np.arange(256), indexing='ij')
    f = ((ci // 64) * 4 + (ci % 64) // 16) * 2 + co // 32
    lane = 32 * ((ci % 16) // 8) + co % 32
    return torch.from_numpy(((f * 64 + lane) * 8 + ci % 8).reshape(-1))


_WEFF_IDX, _WTRANS_IDX = _weff_index(), _wtrans_index()


def unpack_weff(raw):
    """tap bK.weff, (B, 72 * 512, 1, 1) -> W_eff (B, 64 co, 64 ci, 3, 3)"""
    r = torch.as_tensor(raw).reshape(-1, 72 * 512)
    return r[:, _WEFF_IDX].reshape(-1, 64, 64, 3, 3)


def unpack_wtrans(raw):
    """tap bK.wtrans, (B, 32 * 512, 1, 1) -> W' (B, 64 co, 256 ci)"""
    r = torch.as_tensor(raw).reshape(-1, 32 * 512)
    return r[:, _WTRANS_IDX].reshape(-1, 64, 256)


# ---- the layers -----------------------------------------------------------------------------------------------------------------------------------------------

def r32(v):
    """v rounded to fp32, in v's own dtype: where a kernel holds the value in an fp32 register"""
    return v.float().to(v.dtype)


def conv(v, w, order=0):
    """3x3 convolution, zero padding 1.  order 0: emu_layers.cv, one matrix product over the unfolded input.  order 1: the MFMA kernels' structure -- the accumulator takes
    one 16-channel slice of one tap at a time, 9 x C / 16 additions in a row (conv3x3_sp.hip, conv3x3_rw.hip, conv64_s.hip: one v_mfma_f32_32x32x16_f16 per tap and slice),
    so that in fp32 every partial sum is rounded at the magnitude the running sum has there, not at that of the result"""
    if order == 0:
        return cv(v, w)
    H, W = v.shape[2:]
    p = F.pad(v, (1, 1, 1, 1))
    acc = torch.zeros(v.shape[0], w.shape[0], H, W, dtype=v.dtype)
    slices = (v.shape[1] + 15) // 16
    for j in chunk_order(9 * slices, order):
        (dy, dx), c = divmod(j // slices, 3), 16 * (j % slices)
        acc = acc + torch.einsum('oc,bchw->bohw', w[:, c:c + 16, dy, dx], p[:, c:c + 16, dy:dy + H, dx:dx + W])
    return acc


def chunk_order(n, order):
    """the sequence in which an accumulator takes its n chunks: order 1 ascending, order >= 2 a fixed permutation of its own (the kernels differ among themselves in it)"""
    return range(n) if order == 1 else np.random.default_rng(order).permutation(n).tolist()


def lrelu32(v, dtype):
    """LeakyReLU of an fp32 accumulator: the product v * 0.2f is an fp32 number"""
    return torch.maximum(v, r32(v * S32))


def prev_name(k):
    return 'stem' if k == 0 else 'block%d' % (k - 1)


def stem(net, x, dtype, exact=False, order=0):
    """`stem` from x.  misc_kernels.hip:73 nine fp32 multiply-adds, :78 LeakyReLU in fp32 as v >= 0 ? v : v * 0.2f and the one rounding to fp16; no low part in 'fp16'
    (net.h Fwd::act: a low part only under fp16x3).  exact: nothing rounded, slope 0.2."""
    v = conv(x.to(dtype), net.T('conv_input.weight', dtype), order)
    if exact:
        return Out(lrelu(v, 0.2), None, 0.0)
    o = r16(lrelu32(r32(v), dtype))
    return Out(o.float(), None, ulp16(o.abs().max()))


def rb(net, k, j, taps, dtype, exact=False, order=0):
    """`bK.rb0` (j = 0) from the block's input, `bK.rb2` (j = 2) from `bK.rb0`: conv3x3_rw<1> / <4> (forward.cpp:102; the pooled epilogue stores what EPI 1 stores,
    conv3x3_rw.hip:404), or conv3x3_sp where rw does not apply.  fp16(w) (weights.cpp:130), fp16 activations, fp32 accumulators that start from the zero bias image, the sum
    rounded to fp16 FIRST and LeakyReLU'd on packed halves with an fp16 slope: max(h, fp16(h * fp16(0.2))) (conv3x3_rw.hip:289,388-394 act8; conv3x3_sp.hip:331-341)."""
    src = taps[prev_name(k) if j == 0 else 'b%d.rb0' % k].to(dtype)
    if exact:
        return Out(lrelu(conv(src, net.blk(k, 'rblock.%d' % j, dtype), order), 0.2), None, 0.0)
    o = prelu16(r16(r32(conv(src, net.blk(k, 'rblock.%d' % j, dtype, True), order))), 0.2)
    return Out(o.float(), None, ulp16(o.abs().max()))


def mean(net, k, taps, dtype, exact=False, order=0):
    """`bK.mean` from `bK.rb2`: the mean over H x W of the 256-channel 3x3 convolution (rblock.4, fp32 weights: weights.cpp:381-390) of the STORED fp16 values, zero padding --
    the plain operation.  How the kernels get there (conv3x3_rw.hip:404-427 totals, misc_kernels.hip:684-733 sedn_xsum, :736-838 sedn_fmean: totals minus border rows and
    columns plus corners, then 576 terms per channel) is not restated here; `mean_shifted` restates it for the modelled bugs only.  fp32 out: no floor.
    order 1 (fp32 yardstick only): the same operation with the pixels summed first -- the mean over the pixels of each of the 576 unfolded rows, then the product with W_256."""
    t, w = taps['b%d.rb2' % k].to(dtype), net.blk(k, 'rblock.4', dtype)
    if order == 0:
        v = cv(t, w).mean(dim=(2, 3), keepdim=True)
    else:
        v = torch.matmul(F.unfold(t, 3, padding=1).sum(dim=2), w.reshape(256, 576).t()).reshape(-1, 256, 1, 1) / float(t.shape[2] * t.shape[3])
    return Out(v if exact else v.float(), None, 0.0)


def mean_shifted(net, k, taps, dtype, bug=None):
    """sedn_fmean's algebra (misc_kernels.hip:812-837), for the modelled bugs: per tap (dy, dx) the window sum of x = channel total, minus the last / first row for dy = 0 / 2,
    minus the last / first column for dx = 0 / 2, plus the corner both took away; the 256 means are W_256 applied to the 576 window sums, over H W.
    bug 'corner': no corner is added back.  bug 'ragged': the totals include one pixel column beyond W, replicated from column W - 1 (predicated-off lanes of a ragged patch
    reaching the pooled sum).  bug None: the correct algebra -- another summation order of `mean`."""
    t = taps['b%d.rb2' % k].to(dtype)
    H, W = t.shape[2:]
    tot = t.sum(dim=(2, 3))
    r0, rl, c0, cl = t[:, :, 0].sum(-1), t[:, :, -1].sum(-1), t[:, :, :, 0].sum(-1), t[:, :, :, -1].sum(-1)
    if bug == 'ragged':
        tot = tot + cl
    sh = []
    for dy in range(3):
        for dx in range(3):
            v = tot
            if dy == 0: v = v - rl
            if dy == 2: v = v - r0
            if dx == 0: v = v - cl
            if dx == 2: v = v - c0
            if bug != 'corner' and dy != 1 and dx != 1:
                v = v + t[:, :, -1 if dy == 0 else 0, -1 if dx == 0 else 0]
            sh.append(v)
    sh = torch.stack(sh, dim=2)                                             # (B, ci, tap)
    w = net.blk(k, 'rblock.4', dtype).reshape(256, 64, 9)
    return Out((torch.einsum('mct,bct->bm', w, sh) / float(H * W)).reshape(-1, 256, 1, 1).float(), None, 0.0)


def gate(net, k, m, dtype, slope=S32, order=0):
    """the squeeze-excite gate of per-plane channel means m (B, 256): sigmoid(W_up lrelu(W_down m)), fp32 weights and arithmetic, LeakyReLU as v >= 0 ? v : v * 0.2f
    (misc_kernels.hip:850-870 in sedn_weff, :630-652 in sedn_se).  order 0: one product per layer and torch.sigmoid, in fp32 the correctly rounded gate almost everywhere.
    order 1: the kernels' own steps -- the squeeze as 16 partial sums of 16 channels added up in a row (:853-863), and 1 / (1 + __expf(-u)) as it compiles for gfx950
    (read from the assembly of both kernels): v_mul_f32 by -log2(e) = 0xbfb8aa3b, v_exp_f32, + 1, an IEEE division -- exp2 of the ROUNDED product.
    orders 2, 3: order 1 with the exponential one fp32 step larger / smaller.  v_exp_f32 is the one operation of the gate that is not correctly rounded (the ISA gives it
    1 ulp), so its error belongs to the spread, and torch's exp2 does not have it: without these two the fp32 yardstick of a layer that only MULTIPLIES by the gate
    (`wtrans`) agrees with m64 to the bit in half of the blocks, and 4 x nothing allows nothing"""
    wd, wu = net.blk(k, 'conv_down', dtype).reshape(16, 256), net.blk(k, 'conv_up', dtype).reshape(256, 16)
    m = m.to(dtype)
    if order == 0:
        return torch.sigmoid(lrelu(m @ wd.t(), slope) @ wu.t())
    h = torch.zeros(m.shape[0], 16, dtype=dtype)
    for q in range(16):
        h = h + m[:, 16 * q:16 * q + 16] @ wd[:, 16 * q:16 * q + 16].t()
    u = lrelu(h, slope) @ wu.t()
    e = torch.exp2(r32(-u * float(np.float32(1.4426950408889634))))
    if order in (2, 3):
        e = r32(e * (1.0 + (2.0 ** -23 if order == 2 else -2.0 ** -23)))
    return 1.0 / (1.0 + e)


def weff(net, k, taps, dtype, bug=None, exact=False, order=0):
    """`bK.weff` from the engine's own `bK.mean`: W_eff[b] = W_t diag(g_b) W_256, the gate an fp32 number, the product W_t[co][m] * g[m] formed in fp32 and the 256 terms
    summed on fp32 MFMAs (misc_kernels.hip:870,884-892), the fp32 sum rounded to fp16 once (:896).  Floor: ulp16(max|W_eff|).  order 1: the 256 terms in four chunks of 64.
    The gate's 1 / (1 + __expf(-u)) (misc_kernels.hip:870) is the fast exponential: v_exp_f32 of u * log2(e), good to about 2 fp32 ulps plus |u| 2^-24 from the
    rounded product -- for this checkpoint's |u| <= 1 a relative error of the gate below 2e-7.  Carried through the 256 terms that moves W_eff by at most 2e-7 sum|terms|,
    measured on l25 (tests/test_sedn_models_cpu.py prints it): 1.4e-3 of one fp16 step of the largest W_eff, the size of the spread between m32 and m64.  It is part of
    what the bound's 4 x spread allows and shows only as a flipped rounding, which the floor covers.
    bug 'gateperm': the gate applied with channels 8q .. 8q + 3 and 8q + 4 .. 8q + 7 swapped -- the k-pair map of sedn_weff's MFMAs (misc_kernels.hip:874-875,885-891)."""
    g = gate(net, k, taps['b%d.mean' % k].reshape(-1, 256), dtype, 0.2 if exact else S32, order)
    if bug == 'gateperm':
        g = g[:, torch.arange(256) ^ 4]
    wt = net.blk(k, 'trans.0', dtype).reshape(64, 256)
    w256 = net.blk(k, 'rblock.4', dtype).reshape(256, 576)
    a = wt[None] * g[:, None, :] if exact else r32(wt[None] * r32(g)[:, None, :])
    if order == 0:
        v = torch.matmul(a, w256)
    else:
        v = sum(torch.matmul(a[:, :, c:c + 64], w256[c:c + 64]) for c in range(0, 256, 64))
    v = v.reshape(-1, 64, 64, 3, 3)
    if exact:
        return Out(v, None, 0.0)
    o = r16(r32(v))
    return Out(o.float(), None, ulp16(o.abs().max()))


def conv_planes(t, w, order=0):
    """3x3 convolution with per-plane weights w (B, co, ci, 3, 3)"""
    return torch.cat([conv(t[b:b + 1], w[b], order) for b in range(t.shape[0])])


def block(net, k, taps, dtype, exact=False, order=0):
    """`blockK` from the block's input x, `bK.rb2` and the engine's own `bK.weff`: fp16(x + lrelu(conv(W_eff16[b], t))) -- the accumulator, the product v * 0.2f of the
    LeakyReLU max(v, v * 0.2f) and the sum with the fp16 residual are fp32 numbers, then ONE rounding to fp16 (conv3x3_sp.hip:403-409,410-426 EPI 6; conv64_s.hip:232-234).
    Floor: ulp16(max|out|)."""
    x, t, w = taps[prev_name(k)].to(dtype), taps['b%d.rb2' % k].to(dtype), taps['b%d.weff' % k].to(dtype)
    if exact:
        return Out(x + lrelu(conv_planes(t, w, order), 0.2), None, 0.0)
    o = r16(r32(x + lrelu32(r32(conv_planes(t, w, order)), dtype)))
    return Out(o.float(), None, ulp16(o.abs().max()))


def tail(net, taps, dtype, exact=False, order=0):
    """`y` from `block15` and x: tail3_kernel<0> (misc_kernels.hip:313-337,348-355; forward.cpp:299-312 with no low parts) -- fp16(w) times the fp16 activations, fp32 sums,
    the image added in fp32, stored as fp32."""
    w = net.T('convt_R1.weight', dtype) if exact else net.w16('convt_R1.weight', dtype)
    v = conv(taps['block15'].to(dtype), w, order)
    v = v + taps['x'].to(dtype) if exact else r32(v) + taps['x'].to(dtype)
    return Out(v if exact else v.float(), None, 0.0)


# ---- the unfused form (more planes than workgroups; set_debug(1)) ---------------------------------------------------------------------------------------------

def rb4(net, k, taps, dtype, order=0):
    """`bK.rb4` from `bK.rb2`: the 64 -> 256 convolution on the fast 3x3 kernel, fp16(w), no activation (slope 1: conv3x3_sp.hip:331-336), the fp32 sum stored as fp16"""
    o = r16(r32(conv(taps['b%d.rb2' % k].to(dtype), net.blk(k, 'rblock.4', dtype, True), order)))
    return Out(o.float(), None, ulp16(o.abs().max()))


def wtrans(net, k, taps, dtype, order=0):
    """`bK.wtrans` from `bK.rb4`: pool_partial sums the STORED fp16 values in fp32 (misc_kernels.hip:591-595), sedn_se divides by H W (:630-631), forms the gate (an fp32
    number) and stores fp16(W_t[o][c] * g[c]), the product in fp32 (:668-670).  Floor: ulp16(max|W'|).  order 1: the rows summed first, then the columns."""
    t = taps['b%d.rb4' % k].to(dtype)
    m = t.mean(dim=(2, 3)) if order == 0 else t.sum(dim=3).sum(dim=2) / float(t.shape[2] * t.shape[3])
    g = r32(gate(net, k, r32(m), dtype, order=order))
    o = r16(r32(net.blk(k, 'trans.0', dtype).reshape(1, 64, 256) * g[:, None, :]))
    return Out(o.float(), None, ulp16(o.abs().max()))


def block_unfused(net, k, taps, dtype, order=0):
    """`blockK` from the block's input x, `bK.rb4` and the engine's own `bK.wtrans`: the 1x1 conv with per-plane weights on the generic kernel -- LeakyReLU of the fp32
    accumulator as v >= 0 ? v : v * 0.2f, + the fp16 residual in fp32, one rounding (conv_mfma.hip:268-288).  order >= 1: the 256 terms in sixteen chunks of 16, added up in a row."""
    x, t, w = taps[prev_name(k)].to(dtype), taps['b%d.rb4' % k].to(dtype), taps['b%d.wtrans' % k].to(dtype)
    if order == 0:
        c = torch.einsum('boc,bchw->bohw', w, t)
    else:
        c = torch.zeros_like(x)
        for j in chunk_order(16, order):
            c = c + torch.einsum('boc,bchw->bohw', w[:, :, 16 * j:16 * j + 16], t[:, 16 * j:16 * j + 16])
    o = r16(r32(x + lrelu32(r32(c), dtype)))
    return Out(o.float(), None, ulp16(o.abs().max()))


# ---- the layers in order, and the chain -------------------------------------------------------------------------------------------------------------------------

def layer_names(fused=True):
    per = ('b%d.rb0', 'b%d.rb2', 'b%d.mean', 'b%d.weff', 'block%d') if fused else ('b%d.rb0', 'b%d.rb2', 'b%d.rb4', 'b%d.wtrans', 'block%d')
    return ['stem'] + [p % k for k in range(16) for p in per] + ['y']


def run_layer(net, name, taps, dtype, fused=True, exact=False, bug=None, order=0):
    """layer `name` from `taps` ('stem' from taps['x']); exact: nothing rounded (fused form only); bug: see mean_shifted, weff; order: the summation order (0 or 1)"""
    if name == 'stem':
        return stem(net, taps['x'], dtype, exact, order)
    if name == 'y':
        return tail(net, taps, dtype, exact, order)
    if name.startswith('block'):
        k = int(name[5:])
        return block(net, k, taps, dtype, exact, order) if fused else block_unfused(net, k, taps, dtype, order)
    k, what = int(name[1:name.index('.')]), name[name.index('.') + 1:]
    if what in ('rb0', 'rb2'):
        return rb(net, k, int(what[2]), taps, dtype, exact, order)
    if what == 'mean':
        return mean_shifted(net, k, taps, dtype, bug) if bug in ('corner', 'ragged') else mean(net, k, taps, dtype, exact, order)
    if what == 'weff':
        return weff(net, k, taps, dtype, bug, exact, order)
    return rb4(net, k, taps, dtype, order) if what == 'rb4' else wtrans(net, k, taps, dtype, order)


def chain(net, x, dtype, fused=True, exact=False, bug=None):
    """every layer from the models' own taps (bug: in every block): (taps, y).  exact keeps `dtype` throughout (the float64 chain against the oracle)."""
    x = torch.as_tensor(x)
    taps = {'x': x.to(dtype) if exact else x.float()}
    for name in layer_names(fused):
        taps[name] = run_layer(net, name, taps, dtype, fused, exact, bug).value
    return taps, taps['y']


# ---- the bounds: emu_layers', with the larger spread of the two fp32 orders as the yardstick ------------------------------------------------------------------------

GATE_ORDERS = (0, 1, 2, 3)      # the fp32 orders of a layer that carries the gate (`weff`, `wtrans`); every other layer has (0, 1)


def orders_of(name, n):
    """the fp32 orders whose largest spread is the yardstick of layer `name` with n output values.  A layer that stores fp16 differs between two correct evaluations only
    in the values whose fp32 sum lies within an fp32 step of an fp16 tie: about one in 2^13 per order (measured on the reference alone: at 24 576 values an order turns
    0 to 5 roundings against m64, and which of them -- a value of 1e-5 or one of 0.1 -- decides its rms).  A spread taken over fewer than 2^18 values and orders together
    expects fewer than 32 such values and is no estimate of them, so the convolutions get more orders (permuted chunk sequences, `chunk_order`) until n x orders reaches
    2^18: 11 at 3 x 8 x 16 x 64, 5 at 3 x 9 x 35 x 64, the two named ones from 131 072 values on.  The count comes from n alone."""
    if name.endswith(('.weff', '.wtrans')):
        return GATE_ORDERS
    if name.endswith('.mean'):
        return (0, 1)
    return tuple(range(max(2, min(12, -(-2 ** 18 // n)))))


def check2(got, m64, *m32s):
    """(ok, text, figures) as emu_layers.check, the spreads sm, sr being the largest of the fp32 orders' (see the head of the file)"""
    figs = [el.check(got, m64, m)[2] for m in m32s]
    f = figs[0]
    f['sm'], f['sr'] = max(g['sm'] for g in figs), max(g['sr'] for g in figs)
    f['bm'] = 4.0 * f['sm'] + m64.floor
    f['br'] = 4.0 * f['sr'] + 2.0 ** -23 * float(m64.value.abs().max())
    f['beyond'] = min(g['beyond'] for g in figs)
    text = 'max {dm:.3e} (bound {bm:.3e} = 4 x {sm:.3e} + floor {floor:.1e}; {beyond} of {n} values beyond 4 x spread)  rms {dr:.3e} (bound {br:.3e}, spread {sr:.3e})'.format(**f)
    return f['dm'] <= f['bm'] and f['dr'] <= f['br'], text, f


# ---- which path a forward takes: a RESTATEMENT of the host code, for the tests to assert that a case reaches what it is there for -------------------------------------

def pooled_groups(P, items, max_groups):
    """common.h:302-308"""
    G = 1
    if P <= max_groups:
        G = P * (max_groups // P)
    else:
        G = next(d for d in range(max_groups, 0, -1) if P % d == 0)
    return min(G, items)


def pooled_groups_ok(P, items, max_groups):
    """common.h:309-313"""
    return 2 * pooled_groups(P, items, max_groups) >= min(items, max_groups)


def path(B, H, W, groups=256, pool_fuse=1, s64=1, debug=2):
    """What forward_sedn.cpp does with B planes of H x W in 'fp16' on `groups` workgroups.  form: 'fused' unless debug is 1 or B > groups (forward_sedn.cpp:26); sums: 'epilogue'
    when rblock.2's conv pools (option pool_fuse, forward.cpp:69-71: patch ROWS are the work items, P = py) else 'xsum'; py, G, pooled_count (forward_sedn.cpp:45-47); tail:
    'conv64_s' for an even H under option s64 (conv64_s.hip:318) else 'conv3x3_sp<6>'.  The other conditions of these routes (address ranges, conv3x3_rw_applicable's G | py
    or py | G, which pooled_groups guarantees) hold for every shape of the tests."""
    py = (H + 7) // 8
    if debug == 1 or B > groups:
        return dict(form='unfused', py=py)
    pooled = bool(pool_fuse) and pooled_groups_ok(py, B * py, groups)
    G = pooled_groups(py, B * py, groups)
    return dict(form='fused', sums='epilogue' if pooled else 'xsum', py=py, G=G if pooled else None, pooled_count=2 * min(G, py) if pooled else None,
                tail='conv64_s' if (s64 and H % 2 == 0 and H >= 2) else 'conv3x3_sp<6>')
