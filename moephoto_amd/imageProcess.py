"""Host-side mirror of the tiling runtime of python/imageProcess.py, on top of the HIP engine.

Same names and argument meaning as the reference so callers (runSR/runDN adapters, the pipeline
builder) read unchanged; the work itself is done on the device by libmoephoto_amd.so:

  Option, initModel, getStateDict      python/imageProcess.py:304-334, 379-395
  prepare / getAnchors / TilePlan      :19-35, 73-118   -> C planner (moe_plan_create)
  prepareOpt, doCrop                   :133-172         -> moe_run_plan (tile gather, net, stitch on device)
  ensemble, trans/transInv             :563-572         -> moe_run_plan_ens (symmetry + pad, doCrop, fold + average on device)
  RGBFilter, strengthOp, alpha helpers :350-377, 562   -> moe_run_plan_filter (blend with the input and alpha inside the final fold)
  toTorch / toFloat / toOutput         :238-263         -> moe_to_float / moe_to_output kernels
  doCropYuv, toYuv                     (python/video.py:24,219,230 fix the pipe to bgr24 / bgr48le) -> moe_run_plan_yuv / moe_to_yuv: the encoder's 4:2:0 planes
  fromPlanes, doCropPlanes, toPlanes   (python/video.py:24,219 ask the decoder for bgr24 / bgr48le) -> moe_planes_to_float / moe_run_plan_planes / moe_to_output: chains on
                                       the decoder's own 4:2:0 planes, Y' as a (1, H, W) image and Cb / Cr as a (2, H / 2, W / 2) image (pixfmt.toPlanes / fromPlanes)
  resampleChroma                       (no counterpart: the reference's pipe is RGB) -> moe_chroma_resample: the chroma planes of a luma-only chain, by the integer
                                       polyphase filter of pixfmt.resampleChroma
  guidedChroma                         (no counterpart) -> moe_chroma_guided: the same planes by a joint bilateral filter steered by the finished luma (pixfmt.guidedChroma)
  planesToRGB                          (python/video.py:230 asks for bgr48le on the encoder's pipe) -> moe_planes_to_rgb: the interleaved RGB frame of a chain on 4:2:0
                                       planes -- chroma x2 by the same integer filter, then the standard's inverse matrix in fixed point (pixfmt.toRGB)
  lut3d                                (python/AiLUT.py's transform: site-packages/ailut/csrc/ailut_transform_cuda.cu) -> moe_lut3d_create / moe_lut3d_run: a 3D LUT with
                                       non-uniform vertices on interleaved samples, with the strength blend and the quantiser in the same launch (lut3d.apply)
  ailut                                (python/AiLUT.py's generator: AiLUT.forward up to ailut_transform) -> moe_ailut_run + moe_lut3d_run: the net that writes a frame's own
                                       table and vertices from its 256 x 256 thumbnail, in front of lut3d's launch (ailut.generate, lut3d.apply)
  fitPlanes                            (no counterpart: the reference resizes floats, python/imageProcess.py:174-214) -> moe_fit_create / moe_fit_run: planes of codes
                                       brought to a fitted size by the rational integer polyphase filter of pixfmt.fitPlanes, antialiased where it shrinks
  fitPixels                            (no counterpart) -> moe_fit_create_px / moe_fit_run: the same filter on an interleaved image (pixfmt.fitPixels)
  lumaSplit, lumaMerge, doCropLuma     (no counterpart: the reference sends every plane of an RGB image through the net, python/runSR.py:37-40) -> moe_luma_split /
                                       moe_luma_merge / moe_run_plan_luma: a luma-only step -- the net on Y' alone, Cb / Cr resized, merged inside the last fold
                                       (the definition: moephoto_amd/luma.py)
  readFile / writeFile                 :265-302         (PIL, host)

There is no CPU path: models must be moephoto_amd.models.EngineModule instances on a HIP device.
"""
import ctypes
import logging
import math
import time
from functools import reduce

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, pixfmt, quant
from .config import config
from .models import EngineModule
from .weights import load_state_dict_file

log = logging.getLogger('Moe')
modelCache = {}
weightCache = {}
minSize = 28
PLAN_CACHE = 4           # tile plans (with their device pools) kept per Option: an image shape and its transposed twin for the ensemble, x2
identity = lambda x, *_, **__: x
apply = lambda v, f: f(v)
_DT = {torch.float32: _lib.F32, torch.float16: _lib.F16}


def ceilBy(d):
    return lambda x: ((int(x) + d - 1) // d) * d


alignF = {1: identity}
alignF.update((1 << k, ceilBy(1 << k)) for k in (3, 4, 5, 6, 7, 9))


# ---------------------------------------------------------------------------------------------------
# planner
# ---------------------------------------------------------------------------------------------------
class TilePlan(object):
    """A tile plan for one image shape: the C planner's result plus its device tables."""

    def __init__(self, shape, ram, ramCoef, pad, sc, align=8, cropsize=0):
        L = _lib.lib()
        self.shape = tuple(int(v) for v in shape[-3:])
        self._h = ctypes.c_void_p()
        _lib.check(L.moe_plan_create((ctypes.c_int64 * 3)(*self.shape), float(ram), float(ramCoef), int(pad), int(sc),
                                     int(align), int(cropsize), ctypes.byref(self._h)))
        info = (ctypes.c_int64 * 12)()
        _lib.check(L.moe_plan_info(self._h, info))
        (self.n_tiles, self.stepH, self.stepW, self.outH, self.outW, self.padHTo, self.padWTo, self.padSc,
         self.tileH, self.tileW, self.clipH, self.clipW) = [int(v) for v in info]
        t = (ctypes.c_int32 * (8 * self.n_tiles))()
        _lib.check(L.moe_plan_tiles(self._h, t))
        self.tiles = [tuple(t[k * 8:(k + 1) * 8]) for k in range(self.n_tiles)]
        r = (ctypes.c_float * max(1, self.padSc))()
        _lib.check(L.moe_plan_ramp(self._h, r))
        self.ramp = np.array(r[:self.padSc], np.float32)
        rt = (ctypes.c_int32 * (4 * self.stepH))()
        _lib.check(L.moe_plan_rows(self._h, rt))
        self.rows = [tuple(rt[i * 4:(i + 1) * 4]) for i in range(self.stepH)]      # (first written row, first un-blended row, row of the tiles' row 0, tiles' height) per tile row
        self.sc, self.pad, self.align = int(sc), int(pad), int(align)

    def __del__(self):
        try:
            if self._h.value:
                _lib.lib().moe_plan_destroy(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass

    def pool_elems(self, C):
        return int(_lib.check(_lib.lib().moe_plan_pool_elems(self._h, int(C))))

    def tile_offsets(self, C):
        off = (ctypes.c_int64 * self.n_tiles)()
        _lib.check(_lib.lib().moe_plan_tile_offsets(self._h, int(C), off))
        return list(off)

    def seams(self):
        """per tile (ra0, ra1, rb0, rb1, ca0, ca1, cb0, cb1): the rows / columns of the tile a blend reads (moe_plan_seams; the wire format of dist.py)"""
        t = (ctypes.c_int32 * (8 * self.n_tiles))()
        _lib.check(_lib.lib().moe_plan_seams(self._h, t))
        return [tuple(t[k * 8:(k + 1) * 8]) for k in range(self.n_tiles)]

    def padImage(self, x):
        """getPad (python/imageProcess.py:47-56) restricted to the region a single-tile axis reads:
        reflect (edge not repeated) up to len-1, then zeros."""
        def pad_axis(t, from_end, to):      # from_end: 1 = width, 2 = height
            n = t.shape[-from_end]
            if not to or to <= n:
                return t
            refl = min(n - 1, to - n)
            if refl > 0:
                p = (0, refl, 0, 0) if from_end == 1 else (0, 0, 0, refl)
                t = F.pad(t.unsqueeze(0), p, mode='reflect').squeeze(0)
            rest = to - n - refl
            if rest > 0:
                t = F.pad(t, (0, rest, 0, 0) if from_end == 1 else (0, 0, 0, rest))
            return t
        x = pad_axis(x, 1, self.padWTo)
        x = pad_axis(x, 2, self.padHTo)
        return x

    def unpad(self, im):
        return im[..., :self.outH, :self.outW]


def getAnchors(s, ns, l, pad, af, sc):
    """python/imageProcess.py:19-35 (host arithmetic; the C planner computes the same per axis)."""
    n = l - 2 * pad
    step = 1 if l >= af(s) else max(2, -(-int(ns) // n))
    start = [k * n + pad for k in range(step)]
    start[0] = 0
    end = [a + l for a in start]
    endSc = [e * sc for e in end]
    if step > 1:
        start[-1] = s - af(s - end[-2] + pad)
        end[-1] = s
        clip = int((end[-2] - s) * sc)
    else:
        end[-1] = af(s)
        clip = 0
    endSc[-1] = s * sc
    return start, end, clip, step, [int(e) for e in endSc]


def prepare(shape, ram, opt, pad, sc, align=8, cropsize=0):
    """python/imageProcess.py:73-118.  Returns (iterClip, padImage, unpad, outShape, blend) like the
    reference; the TilePlan itself is attached to the returned iterClip as `.plan`."""
    plan = TilePlan(shape, ram, opt.ramCoef, pad, sc, align, cropsize)

    def iterClip():
        for t in plan.tiles:
            yield t
    iterClip.plan = plan
    b = torch.from_numpy(plan.ramp.copy()).view(1, -1)
    return iterClip, plan.padImage, plan.unpad, (*shape[:-2], plan.outH, plan.outW), b


class Option(object):
    """The per-op settings bag of python/imageProcess.py:379-395: the adapters (runSR / runDN .getOpt) fill in the fields, doCrop and
    the pipeline builder read them, and calling it runs the net on one tile batch (a list result means "take the last entry")."""
    _DEFAULTS = dict(ramCoef=1e-3, count=0, padding=1, cropsize=0, align=8, fixChannel=1, scale=1, ensemble=0, strength=1.0,
                     outShape=None, oShape=None, iterClip=None, modelCached=None)

    def __init__(self, path=''):
        for name, value in self._DEFAULTS.items():
            setattr(self, name, value)
        self.model = path
        self.prepare = identity
        # planes-as-batch adapters; the SR / DN tables replace them with dim-1 versions
        self.squeeze = lambda t: t.squeeze(0)
        self.unsqueeze = lambda t: t.unsqueeze(0)
        self._plans = {}          # image shape -> [TilePlan, uses]  (LRU, see _plan_for)

    def __call__(self, x, *args, **kwargs):
        result = self.modelCached(x, *args, **kwargs)
        return result[-1] if isinstance(result, list) else result


def getStateDict(path):
    """python/imageProcess.py:304-307, with our own closed parser of the legacy zoo format."""
    if path not in weightCache:
        sd = load_state_dict_file(path)
        weightCache[path] = type(sd)((k, torch.from_numpy(v)) for k, v in sd.items())
    return weightCache[path]


def castModel(model):
    """python/imageProcess.py:309-317.  Every engine model computes with fp16 MFMA operands and fp32
    accumulation whatever castDtype says; the dtype only selects the I/O element type."""
    return model.to(dtype=config.dtype(), device=config.device())


def initModel(opt, weights=None, key=None, f=lambda opt: opt.modelDef(), args=[]):
    """python/imageProcess.py:319-334: one instance per cache key for the life of the process; construction = constructor slot of
    the plugin table, strict load_state_dict (a path is read through the zoo parser), frozen, eval; every call re-casts to the
    configured dtype / device (castModel)."""
    model = modelCache.get(key) if key else None
    if model is None:
        log.info('loading model {}'.format(opt.model))
        model = f(opt, *args)
        if weights:
            log.info('reloading weights')
            model.load_state_dict(getStateDict(weights) if isinstance(weights, str) else weights)
        for p in model.parameters():
            p.requires_grad_(False)
        model.eval()
        if key:
            modelCache[key] = model
    return castModel(model)


def _plan_for(opt, shape):
    """prepareOpt (python/imageProcess.py:133-155): plans are cached per image shape; the reference
    re-plans every 29 calls to follow free memory -- here the plan only depends on free memory when
    cropsize is 'auto', and is then re-derived with the same cadence."""
    key = tuple(int(v) for v in shape[-3:])
    ent = opt._plans.pop(key, None)
    if ent is None or (opt.cropsize <= 0 and ent[1] > 28):
        model = opt.modelCached

        def plan_with(emptyCache):
            try:
                freeMem = config.calcFreeMem(emptyCache=emptyCache)
            except Exception:
                raise MemoryError('Can not calculate free memory.')
            if isinstance(model, EngineModule):
                # the planner's pixel budget is ram * ramCoef / C^2 (solveRam with fixChannel = 0): keep it within the largest
                # tile the convolution kernels address, however much memory is free (288 GB would otherwise plan whole 8K images)
                freeMem = min(freeMem, model.max_tile_pixels() * key[0] * key[0] / opt.ramCoef)
            return prepare(key, freeMem, opt, opt.padding, opt.scale, opt.align, opt.cropsize)
        try:
            it, padImage, unpad, outShape, bl = plan_with(False)
            # 'auto' tile size: memory torch has reserved but not handed out is invisible to hipMemGetInfo and unusable by the engine (hipMalloc).  The
            # reference counts it as free (python/config.py:61-71); here it is RELEASED when it is a large share of what is free -- otherwise the planner
            # would silently settle for smaller tiles while gigabytes sit in torch's cache (once per re-plan, i.e. every 29 calls at most)
            if opt.cropsize <= 0:
                slack = torch.cuda.memory_reserved(config.deviceId) - torch.cuda.memory_allocated(config.deviceId)
                if slack > (1 << 30) and slack > 0.1 * max(1, config.getFreeMem()):
                    it, padImage, unpad, outShape, bl = plan_with(True)
        except MemoryError:          # the smallest tile did not fit: hand torch's cached blocks back to the driver and ask again, once
            it, padImage, unpad, outShape, bl = plan_with(True)
        ent = [it.plan, 0]
        while len(opt._plans) >= PLAN_CACHE:       # each plan owns a device tile pool of ~1.1x its output image: keep a few, drop the
            opt._plans.pop(next(iter(opt._plans)))   # least recently used (the reference keeps exactly one, re-planning on a shape change)
        opt._plans[key] = ent
        opt.iterClip, opt.padImage, opt.unpad, opt.blend = it, padImage, unpad, bl
        opt.outShape = list(outShape)
    else:
        ent[1] += 1
        opt._plans[key] = ent                      # re-inserted last = most recently used
    return ent[0]


def prepareOpt(opt, shape):
    _plan_for(opt, shape)
    return opt.scale, int(opt.padding * opt.scale)


def _outStorage(bitDepth):
    """(torch dtype, numpy dtype, library dtype) of the quantised image: uint8, or uint16 samples in int16 storage (toOutput's convention)."""
    if bitDepth not in (8, 16):
        raise ValueError('bitDepth must be 8 or 16, got {}'.format(bitDepth))
    return (torch.uint8, np.uint8, _lib.U8) if bitDepth == 8 else (torch.int16, np.uint16, _lib.U16)


def _yuvOut(who, fmt, w, h, out, device):
    """The flat uint8 device tensor a Y'CbCr frame of w x h is written into: `out` checked, or a new one."""
    n = pixfmt.frameBytes(fmt, w, h)
    if out is None:
        return torch.empty((n,), dtype=torch.uint8, device=device)
    if tuple(out.shape) != (n,) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
        raise ValueError('{}: out must be a flat contiguous uint8 tensor of {} bytes ({} at {} x {}) on {}'.format(who, n, fmt, w, h, device))
    return out


def _planesOut(who, depth, C, h, w, out, device):
    """The flat uint8 device tensor C planes of h x w samples at `depth` bits are written into (a frame, or a view into one: the Y plane, the two chroma planes)."""
    if depth not in pixfmt.FORMATS.values():
        raise ValueError('{}: depth must be one of {}, got {!r}'.format(who, sorted(pixfmt.FORMATS.values()), depth))
    n = C * h * w * (1 if depth == 8 else 2)
    if out is None:
        return torch.empty((n,), dtype=torch.uint8, device=device)
    if tuple(out.shape) != (n,) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device or out.data_ptr() % (1 if depth == 8 else 2):
        raise ValueError('{}: out must be a flat contiguous uint8 tensor of {} bytes ({} planes of {} x {} at {} bits) on {}'.format(who, n, C, w, h, depth, device))
    return out


def ditherFlags(who, dither, bits, kind):
    """The MOE_Q_* flags of a `dither` keyword (None | 'none' | 'round' | 'ordered') for an edge of `kind` ('rgb', 'planes', 'yuv': quant.flags) -- RGB samples at 8 bits
    take the unit scale (their reader is / 255), at 16 bits and planar samples do not.  ValueError naming the keyword for an unknown value."""
    if dither is not None and dither not in quant.MODES:
        raise ValueError("{}: 'dither' \"{}\" is not supported ({})".format(who, dither, ', '.join(quant.MODES)))
    return quant.flags(dither, bits, kind)


def _runPlan(who, opt, x, bitDepth=None, out=None, mix=None, yuv=None, planes=None, reuse=None, luma=None, dither=None):
    """doCrop, doCropOut and the DN step's fused forms: the checks, the plan, the pad, the call (moe_run_plan, with bitDepth moe_run_plan_out, with mix = (strength,
    alpha plane or None) moe_run_plan_filter: the blend with x and the alpha plane inside the final fold, with yuv = (pixFmt, matrix, order) moe_run_plan_yuv: the
    encoder's planar frame from the final fold, with planes = depth moe_run_plan_planes: the image's own planes as samples of that depth) and its one retry after
    a MemoryError.  With luma = (C', matrix, order) x is the Y image of a luma-only step (luma.lumaSplit: 1 plane, or 2 with alpha) and the call is moe_run_plan_luma:
    the final fold merges Y' with the fp32 chroma planes C' (2, outH, outW) into the colour planes -- the canvas (x's planes + 2, outH, outW), or with bitDepth its samples.
    reuse (the frame stream's): a callable (plan, planes) -> (mask, pool) -- the plan's tiles that have to run for this image as n_tiles uint8 on
    the host, and the fp32 device tensor of plan.pool_elems(planes) that holds every other tile's result from the previous frame.  The call is then moe_run_plan_subset
    into that pool followed by the same edge's stitch-only entry point on it (moe_stitch, moe_stitch_out, moe_stitch_mix, moe_stitch_yuv, moe_stitch_planes).
    dither ('round' | 'ordered'; moephoto_amd/quant.py): the edge's quantiser rounds or dithers -- its MOE_Q_* flags ride in the bits / depth argument of whichever call is
    made, the reuse path's stitch included; a canvas form quantises nothing and refuses the keyword."""
    qf = ditherFlags(who, dither, bitDepth, 'yuv' if yuv is not None else 'planes' if planes is not None else 'rgb')
    if qf and bitDepth is None and yuv is None and planes is None:
        raise ValueError("{}: 'dither' applies to a quantising edge; the canvas form quantises nothing".format(who))
    model = opt.modelCached
    if not isinstance(model, EngineModule):
        raise TypeError('{} needs an engine-backed model (moephoto_amd.models.*), got {}'.format(who, type(model).__name__))
    if x.device.type != 'cuda':
        raise _lib.EngineError('{}: input must live on a HIP device (moephoto_amd has no CPU path)'.format(who))
    if x.dim() != 3:
        raise ValueError('{} expects a (C,H,W) image'.format(who))
    if bitDepth is not None:
        out_dt, _, lib_dt = _outStorage(bitDepth)
    plan = _plan_for(opt, x.shape)
    xp = plan.padImage(x)
    if xp.dtype not in _DT:
        xp = xp.to(config.dtype())
    model.to(device=x.device)
    C = xp.shape[0]
    if mix is not None:
        strength, alpha = float(mix[0]), mix[1]
        if alpha is not None:
            if alpha.dim() != 2 or alpha.shape[0] < plan.outH or alpha.shape[1] < plan.outW or alpha.device != x.device:
                raise ValueError('{}: the alpha plane must be (H, W) on {}'.format(who, x.device))
            alpha = alpha.to(xp.dtype)
            C += 1
        aH, aW = alpha.stride() if alpha is not None else (0, 0)
    if luma is not None:
        chroma, matrix, order = luma[0], pixfmt.MATRICES[luma[1]], pixfmt.ORDERS[luma[2]]
        if C not in (1, 2):
            raise ValueError('{}: a Y image of 1 plane (2 with alpha) expected, got {} planes'.format(who, C))
        if (tuple(chroma.shape) != (2, plan.outH, plan.outW) or chroma.dtype != torch.float32 or not chroma.is_contiguous() or chroma.device != x.device):
            raise ValueError('{}: the chroma planes must be a contiguous fp32 tensor of shape {} on {}'.format(who, (2, plan.outH, plan.outW), x.device))
        C += 2
    if yuv is not None:
        depth, matrix, order = pixfmt.check(*yuv)
        if C != 3:
            raise ValueError('{}: a three-plane image expected, got {} planes'.format(who, C))
        out = _yuvOut(who, yuv[0], plan.outW, plan.outH, out, x.device)
    elif planes is not None:
        if not 1 <= C <= 4:
            raise ValueError('{}: an image of 1 to 4 planes expected, got {}'.format(who, C))
        out = _planesOut(who, planes, C, plan.outH, plan.outW, out, x.device)
    elif bitDepth is None:
        out = xp.new_empty((C, plan.outH, plan.outW))
    elif out is None:
        out = torch.empty((plan.outH, plan.outW, C), dtype=out_dt, device=x.device)
    elif tuple(out.shape) != (plan.outH, plan.outW, C) or out.dtype != out_dt or not out.is_contiguous() or out.device != x.device:
        raise ValueError('{}: out must be a contiguous {} tensor of shape {} on {}'.format(who, out_dt, (plan.outH, plan.outW, C), x.device))
    sC, sH, sW = xp.stride()
    stream = torch.cuda.current_stream(x.device).cuda_stream
    L = _lib.lib()
    if reuse is not None:
        mask, pool = reuse(plan, xp.shape[0])
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        if mask.shape != (plan.n_tiles,) or pool.dtype != torch.float32 or pool.numel() < plan.pool_elems(xp.shape[0]) or pool.device != x.device or not pool.is_contiguous():
            raise ValueError('{}: reuse must give {} uint8 flags and a contiguous fp32 pool of {} elements on {}'.format(who, plan.n_tiles, plan.pool_elems(xp.shape[0]), x.device))
        dev, P, dt = x.device.index or 0, xp.shape[0], _DT[xp.dtype]

    def fold():        # the edge alone, on the stream's pool in the plan's own layout
        if luma is not None:
            _lib.check(L.moe_stitch_luma(plan._h, dev, pool.data_ptr(), None, P, dt, chroma.data_ptr(), matrix, order, int(bitDepth or 0) | qf, out.data_ptr(),
                                         _DT[out.dtype] if bitDepth is None else lib_dt, stream))
        elif yuv is not None:
            _lib.check(L.moe_stitch_yuv(plan._h, dev, pool.data_ptr(), None, dt, depth | qf, matrix, order, out.data_ptr(), stream))
        elif planes is not None:
            _lib.check(L.moe_stitch_planes(plan._h, dev, pool.data_ptr(), None, P, dt, int(planes) | qf, out.data_ptr(), stream))
        elif mix is not None:
            _lib.check(L.moe_stitch_mix(plan._h, dev, pool.data_ptr(), None, P, xp.data_ptr(), dt, sC, sH, sW, alpha.data_ptr() if alpha is not None else None, aH, aW,
                                        strength, int(bitDepth or 0) | qf, out.data_ptr(), _DT[out.dtype] if bitDepth is None else lib_dt, stream))
        elif bitDepth is None:
            _lib.check(L.moe_stitch(plan._h, dev, pool.data_ptr(), None, P, out.data_ptr(), _DT[out.dtype], stream))
        else:
            _lib.check(L.moe_stitch_out(plan._h, dev, pool.data_ptr(), None, P, dt, int(bitDepth) | qf, out.data_ptr(), lib_dt, stream))

    def run():
        if reuse is not None:
            _lib.check(L.moe_run_plan_subset(model._h, plan._h, xp.data_ptr(), dt, sC, sH, sW, mask.ctypes.data, pool.data_ptr(), int(config.tilesPerBatch), stream))
            fold()
        elif luma is not None:       # the canvas doCrop would have returned for Y has xp's dtype: its rounding comes first, then the merge in that dtype
            _lib.check(L.moe_run_plan_luma(model._h, plan._h, xp.data_ptr(), _DT[xp.dtype], sC, sH, sW, chroma.data_ptr(), matrix, order, int(bitDepth or 0) | qf,
                                           out.data_ptr(), _DT[out.dtype] if bitDepth is None else lib_dt, int(config.tilesPerBatch), stream))
        elif yuv is not None:        # (as doCropOut: the rounding of the canvas doCrop would have returned comes first)
            _lib.check(L.moe_run_plan_yuv(model._h, plan._h, xp.data_ptr(), _DT[xp.dtype], sC, sH, sW, _DT[xp.dtype], depth | qf, matrix, order,
                                          out.data_ptr(), int(config.tilesPerBatch), stream))
        elif planes is not None:
            _lib.check(L.moe_run_plan_planes(model._h, plan._h, xp.data_ptr(), _DT[xp.dtype], sC, sH, sW, _DT[xp.dtype], int(planes) | qf,
                                             out.data_ptr(), int(config.tilesPerBatch), stream))
        elif mix is not None:     # the canvas RGBFilter would have returned has xp's dtype; bits = 0 asks for that canvas, else for its samples
            _lib.check(L.moe_run_plan_filter(model._h, plan._h, xp.data_ptr(), _DT[xp.dtype], sC, sH, sW, alpha.data_ptr() if alpha is not None else None, aH, aW,
                                             strength, int(bitDepth or 0) | qf, out.data_ptr(), _DT[out.dtype] if bitDepth is None else lib_dt, int(config.tilesPerBatch), stream))
        elif bitDepth is None:
            _lib.check(L.moe_run_plan(model._h, plan._h, xp.data_ptr(), _DT[xp.dtype], sC, sH, sW, out.data_ptr(), _DT[out.dtype], int(config.tilesPerBatch), stream))
        else:          # the canvas doCrop would have returned has xp's dtype: its rounding is applied before the quantiser
            _lib.check(L.moe_run_plan_out(model._h, plan._h, xp.data_ptr(), _DT[xp.dtype], sC, sH, sW, _DT[xp.dtype], int(bitDepth) | qf,
                                          out.data_ptr(), lib_dt, int(config.tilesPerBatch), stream))
    try:
        run()
    except MemoryError:              # the engine's workspace / tile pool is hipMalloc'ed beside torch's caching allocator: release the
        torch.cuda.empty_cache()     # cache and try once more before reporting "does not fit" (python/imageProcess.py:58-59)
        run()
    # the engine reads xp asynchronously: keep it alive until the stream has consumed it
    xp.record_stream(torch.cuda.current_stream(x.device))
    if mix is not None and alpha is not None:
        alpha.record_stream(torch.cuda.current_stream(x.device))
    if luma is not None:
        chroma.record_stream(torch.cuda.current_stream(x.device))
    return out


def doCrop(opt, x, *args, reuse=None, **_):
    """python/imageProcess.py:157-172, entirely on the device: the planes of x (C,H,W) become the batch
    (runSR.py:37-40), tiles are gathered straight from x by the stem kernel, same-shaped tiles are batched
    through the net, and the gather-stitch kernel folds them with the reference's sequential blend."""
    return _runPlan('doCrop', opt, x, reuse=reuse)


def doCropOut(opt, x, bitDepth, out=None, reuse=None, dither=None):
    """toOutput(bitDepth)(toFloat(doCrop(opt, x))) without the download, as ONE call (moe_run_plan_out): doCrop up to the final fold, which rounds each pixel as the
    canvas of x's dtype would have and writes the quantised (H, W, C) image (uint8, or uint16 samples in int16 storage) -- the canvas and its fp32 copy never exist
    (python/imageProcess.py:157-172,238-257).  out: a contiguous device tensor of that shape and dtype to write into (the frame stream's slot buffers), else a new one.
    dither: None | 'round' | 'ordered' -- the fold's quantiser rounds to nearest or adds the 8 x 8 ordered dither (moephoto_amd/quant.py; 8 bits at unit scale)."""
    return _runPlan('doCropOut', opt, x, bitDepth, out, reuse=reuse, dither=dither)


def doCropYuv(opt, x, fmt, out=None, matrix='bt709', order='bgr', reuse=None, dither=None):
    """doCropOut(opt, x, 16) followed by pixfmt.fromSamples16, as ONE call (moe_run_plan_yuv): the final fold writes the encoder's planar Y'CbCr 4:2:0 frame -- fmt one of
    pixfmt.FORMATS (yuv420p, yuv420p10le, yuv420p12le, yuv420p16le), limited range, matrix bt709 / bt601 / bt2020nc; order says whether plane 0 of x is blue ('bgr', the
    video path's frames) or red.  Half the bytes of the interleaved image.  Returns a flat uint8 device tensor of pixfmt.frameBytes(fmt, outW, outH); out: one to write into."""
    pixfmt.check(fmt, matrix, order)          # (dither: quant.yuvFromSamples16 -- 'ordered' dithers the integer conversion's rounding, 'round' is the plain frame)
    return _runPlan('doCropYuv', opt, x, out=out, yuv=(fmt, matrix, order), reuse=reuse, dither=dither)


def doCropPlanes(opt, x, depth, out=None, reuse=None, dither=None):
    """doCrop(opt, x) quantised plane by plane at `depth` bits (8, 10, 12, 16), as ONE call (moe_run_plan_planes): the final fold rounds each pixel as the canvas of x's
    dtype would have and writes C = 1 .. 4 planes of outH x outW samples (uint8 for depth 8, else little-endian uint16) -- the Y plane or the two chroma planes of a
    planar 4:2:0 frame (pixfmt.fromPlanes).  Returns a flat uint8 device tensor of those bytes; out: one to write into, e.g. a view into a frame at a plane's offset."""
    return _runPlan('doCropPlanes', opt, x, out=out, planes=int(depth), reuse=reuse, dither=dither)          # (dither: each sample at its coordinates in its own plane)


# ---- luma-only steps (no counterpart: the reference sends every plane through the net; the definition: moephoto_amd/luma.py) -------------------
def _lumaIds(who, matrix, order):
    if matrix not in pixfmt.MATRICES:
        raise ValueError('{}: chromaMatrix "{}" is not supported ({})'.format(who, matrix, ', '.join(pixfmt.MATRICES)))
    if order not in pixfmt.ORDERS:
        raise ValueError('{}: order "{}" is not supported ({})'.format(who, order, ', '.join(pixfmt.ORDERS)))
    return pixfmt.MATRICES[matrix], pixfmt.ORDERS[order]


LUMA_KEYS = ('chroma', 'chromaMatrix', 'order')


def lumaKeys(step, defaultOrder='rgb'):
    """(chroma, chromaMatrix, order) of an SR / DN step dict, checked: 'chroma' is 'net' (the default: every plane goes through the net, today's path), 'nearest',
    'bilinear' or 'bicubic' (the step is luma-only and Cb / Cr are resized by that method); 'chromaMatrix' defaults to 'bt709'; 'order' says whether plane 0 is red
    ('rgb', behind a file source) or blue ('bgr', behind a buffer source).  ValueError naming the key for an unknown value and for 'chromaMatrix' / 'order' beside 'net'."""
    op = step.get('op', 'step')
    chroma = step.get('chroma', 'net')
    if chroma != 'net' and chroma not in _lib.RESIZE_MODES:
        raise ValueError("{}: 'chroma' \"{}\" is not supported (net, {})".format(op, chroma, ', '.join(_lib.RESIZE_MODES)))
    if chroma == 'net':
        for k in LUMA_KEYS[1:]:
            if k in step:
                raise ValueError("{}: '{}' does not apply to 'chroma': 'net' (every plane goes through the net, nothing is converted)".format(op, k))
        return 'net', 'bt709', defaultOrder
    matrix, order = step.get('chromaMatrix', 'bt709'), step.get('order', defaultOrder)
    if matrix not in pixfmt.MATRICES:
        raise ValueError("{}: 'chromaMatrix' \"{}\" is not supported ({})".format(op, matrix, ', '.join(pixfmt.MATRICES)))
    if order not in pixfmt.ORDERS:
        raise ValueError("{}: 'order' \"{}\" is not supported ({})".format(op, order, ', '.join(pixfmt.ORDERS)))
    return chroma, matrix, order


def lumaSplit(matrix='bt709', order='rgb'):
    """luma.lumaSplit on the device (moe_luma_split, one launch): f(x) takes a (3 | 4, H, W) fp16 / fp32 device image, strided or dense, and returns Y (1 | 2, H, W) of
    x's dtype -- Y', and alpha behind it -- and C (2, H, W) fp32 -- Cb, Cr."""
    mat, ordr = _lumaIds('lumaSplit', matrix, order)

    def f(x):
        if x.device.type != 'cuda':
            raise _lib.EngineError('lumaSplit: input must live on a HIP device (moephoto_amd has no CPU path)')
        if x.dim() != 3 or x.shape[0] not in (3, 4):
            raise ValueError('lumaSplit expects a (3 | 4, H, W) image, got {}'.format(tuple(x.shape)))
        if x.dtype not in _DT:
            x = x.to(config.dtype())
        C, H, W = x.shape
        Y = torch.empty((C - 2, H, W), dtype=x.dtype, device=x.device)
        Cc = torch.empty((2, H, W), dtype=torch.float32, device=x.device)
        cur = torch.cuda.current_stream(x.device)
        _lib.check(_lib.lib().moe_luma_split(x.data_ptr(), _DT[x.dtype], C, x.stride(0), x.stride(1), x.stride(2), H, W, mat, ordr, Y.data_ptr(), Cc.data_ptr(),
                                             x.device.index or 0, cur.cuda_stream))
        x.record_stream(cur)
        return Y, Cc
    return f


def lumaMerge(matrix='bt709', order='rgb'):
    """luma.lumaMerge on the device (moe_luma_merge): f(Y, C, bitDepth=None, out=None) takes Y' (1 | 2, H, W) fp16 / fp32 and C' (2, H, W) fp32 and returns the canvas
    (3 | 4, H, W) of Y's dtype, or with bitDepth 8 | 16 the quantised (H, W, 3 | 4) image as doCropOut gives it; out: a tensor of that shape and dtype to write into."""
    mat, ordr = _lumaIds('lumaMerge', matrix, order)

    def f(Y, Cc, bitDepth=None, out=None, dither=None):          # (dither: the sample form only -- quant.py)
        qf = ditherFlags('lumaMerge', dither, bitDepth, 'rgb')
        if qf and bitDepth is None:
            raise ValueError("lumaMerge: 'dither' applies to the sample form (bitDepth 8 | 16); the canvas form quantises nothing")
        if Y.device.type != 'cuda' or Cc.device != Y.device:
            raise _lib.EngineError('lumaMerge: both inputs must live on one HIP device (moephoto_amd has no CPU path)')
        if Y.dim() != 3 or Y.shape[0] not in (1, 2):
            raise ValueError('lumaMerge expects a (1 | 2, H, W) Y image, got {}'.format(tuple(Y.shape)))
        if Y.dtype not in _DT:
            Y = Y.to(config.dtype())
        P, H, W = Y.shape
        if tuple(Cc.shape) != (2, H, W) or Cc.dtype != torch.float32:
            raise ValueError('lumaMerge: the chroma planes must be fp32 of shape {}, got {} {}'.format((2, H, W), Cc.dtype, tuple(Cc.shape)))
        Y, Cc = Y.contiguous(), Cc.contiguous()
        if bitDepth is None:
            shape, o_dt, lib_dt = (P + 2, H, W), Y.dtype, _DT[Y.dtype]
        else:
            o_dt, _, lib_dt = _outStorage(bitDepth)
            shape = (H, W, P + 2)
        if out is None:
            out = torch.empty(shape, dtype=o_dt, device=Y.device)
        elif tuple(out.shape) != shape or out.dtype != o_dt or not out.is_contiguous() or out.device != Y.device:
            raise ValueError('lumaMerge: out must be a contiguous {} tensor of shape {} on {}'.format(o_dt, shape, Y.device))
        cur = torch.cuda.current_stream(Y.device)
        _lib.check(_lib.lib().moe_luma_merge(Y.data_ptr(), _DT[Y.dtype], Cc.data_ptr(), P + 2, H, W, mat, ordr, int(bitDepth or 0) | qf, out.data_ptr(), lib_dt,
                                             Y.device.index or 0, cur.cuda_stream))
        Y.record_stream(cur)
        Cc.record_stream(cur)
        return out
    return f


def lumaChroma(Cc, height, width, method):
    """The chroma planes of a luma-only step at the size of its Y': the existing resize on fp32 with the method the step's 'chroma' key names; the planes themselves
    when the size does not change (a DN step)."""
    if tuple(Cc.shape[-2:]) == (int(height), int(width)):
        return Cc
    return resizeByTorch(Cc, width, height, method)


def doCropLuma(opt, x, method, matrix='bt709', order='rgb', bitDepth=None, out=None, reuse=None, dither=None):
    """A luma-only step with the merge inside the last fold (moe_run_plan_luma; with reuse moe_run_plan_subset + moe_stitch_luma): lumaSplit(x), the chroma planes
    resized to the step's output size, doCrop on Y with the final fold writing the colour planes -- the Y' canvas never exists.  The bytes of
    lumaMerge(doCrop(opt, Y), lumaChroma(C, ..)).  With bitDepth the fold writes the encoder's samples into `out`, as doCropOut does.  An image of fewer than three
    planes has no chroma to set aside: it runs as doCrop / doCropOut."""
    if method not in _lib.RESIZE_MODES:
        raise ValueError('doCropLuma: chroma "{}" is not supported ({})'.format(method, ', '.join(_lib.RESIZE_MODES)))
    _lumaIds('doCropLuma', matrix, order)
    if x.dim() == 3 and x.shape[0] < 3:
        return _runPlan('doCropLuma', opt, x, bitDepth, out, reuse=reuse, dither=dither)
    Y, Cc = lumaSplit(matrix, order)(x)
    plan = _plan_for(opt, Y.shape)
    return _runPlan('doCropLuma', opt, Y, bitDepth, out, reuse=reuse, luma=(lumaChroma(Cc, plan.outH, plan.outW, method), matrix, order), dither=dither)


# ---- resize step (python/imageProcess.py:174-214, 555-556) --------------------------------------------------
def blendTile(r, canvas, tile, sc, padSc, ramp):
    """The two `blend` calls and the slice-assign of the reference's tile loop (python/imageProcess.py:120-131,167-170) for ONE tile, as one kernel
    (moe_blend_tile) -- for a caller that keeps MoePhoto's own doCrop loop around the drop-in model class:

        for tile in opt.iterClip():                          # tile = (top, bottom, left, right, topT, leftT, bsc, rsc)
            r = opt.squeeze(opt(x[..., tile[0]:tile[1], tile[2]:tile[3]]))
            blendTile(r, tmp_image, tile, sc, padSc, opt.blend)      # instead of: t = ...; q, _ = blend(*blend(...)); tmp_image[...] = q

    r: (C, h, w) tile result (rows / columns beyond the window are ignored: opt.unpad); canvas: (C, H, W); ramp: opt.blend (padSc values); all three of one
    dtype (fp16 / fp32), on the device, unit stride along the last axis.  The canvas receives the bits the reference's torch expression produces."""
    top, bottom, left, right, topT, leftT, bsc, rsc = [int(v) for v in tile]
    canvas_in = canvas
    # moe_blend_tile takes raw pointers and (plane, row) strides: this wrapper is the only guard against a canvas / tile of another rank (the reference's
    # tmp_image is (1, C, H, W) when opt.oShape is set; a (C, 1, H, W) result is the net's own output shape).  Singleton leading / second axes are dropped, anything
    # else is refused -- stride(1) of a 4-D tensor is NOT the row stride
    if r.dim() == 4 and r.shape[1] == 1:
        r = r.squeeze(1)
    while r.dim() > 3 and r.shape[0] == 1:
        r = r[0]
    while canvas.dim() > 3 and canvas.shape[0] == 1:
        canvas = canvas[0]
    if canvas.dim() == 4 and canvas.shape[1] == 1:
        canvas = canvas[:, 0]
    if r.dim() != 3 or canvas.dim() != 3:
        raise ValueError('blendTile: a (C, h, w) tile result and a (C, H, W) canvas expected, got {} and {}'.format(tuple(r.shape), tuple(canvas.shape)))
    if not (r.dtype == canvas.dtype and (ramp is None or ramp.dtype == canvas.dtype)) or r.dtype not in _DT:
        raise TypeError('blendTile: tile, canvas and ramp must share one dtype (fp16 or fp32)')
    if r.stride(-1) != 1 or canvas.stride(-1) != 1 or r.device != canvas.device or r.shape[0] != canvas.shape[0]:
        raise ValueError('blendTile: unit stride along the last axis, one device and one plane count expected')
    if r.shape[-2] < bsc - top * sc or r.shape[-1] < rsc - left * sc or bsc > canvas.shape[-2] or rsc > canvas.shape[-1]:
        raise ValueError('blendTile: the window {}..{} x {}..{} does not fit the tile result {} / the canvas {}'.format(top * sc, bsc, left * sc, rsc, tuple(r.shape), tuple(canvas.shape)))
    rp = ramp.reshape(-1) if ramp is not None else None
    if rp is not None and (rp.numel() < padSc or rp.stride(0) != 1):
        raise ValueError('blendTile: ramp must hold padSc contiguous values')
    stream = torch.cuda.current_stream(canvas.device).cuda_stream
    _lib.check(_lib.lib().moe_blend_tile(r.data_ptr(), r.stride(-3), r.stride(-2), canvas.data_ptr(), canvas.stride(-3), canvas.stride(-2), _DT[canvas.dtype], int(canvas.shape[0]),
                                         int(top * sc), int(left * sc), bsc, rsc, topT, leftT, int(padSc), rp.data_ptr() if rp is not None else None, stream))
    return canvas_in


def resizeByTorch(x, width, height, mode='bilinear'):
    """The reference's `resizeByTorch` = F.interpolate(x[None], size=(height, width), mode=mode, align_corners=False)[0]; the name
    is kept for the callers, the work is moe_resize on the device (nearest / bilinear / bicubic)."""
    if mode not in _lib.RESIZE_MODES:
        raise ValueError('resize: interpolation method "{}" is not supported (nearest, bilinear, bicubic)'.format(mode))
    if x.device.type != 'cuda':
        raise _lib.EngineError('resize: input must live on a HIP device (moephoto_amd has no CPU path)')
    if x.dtype not in _DT:
        x = x.to(config.dtype())
    x = x.contiguous()
    C, H, W = x.shape
    out = torch.empty((C, int(height), int(width)), dtype=x.dtype, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _lib.check(_lib.lib().moe_resize(x.data_ptr(), out.data_ptr(), _DT[x.dtype], C, H, W, int(height), int(width),
                                     _lib.RESIZE_MODES[mode], x.device.index or 0, stream))
    x.record_stream(torch.cuda.current_stream(x.device))
    return out


def resize(opt, out=None, pos=0, nodes=(), h=1, w=1):
    """The `resize` step: target size from scaleH / scaleW (rounded like the reference) or height / width; once the size is known
    for a stream source it is kept (opt['update'])."""
    opt['update'] = True
    opt.setdefault('method', 'bilinear')

    def f(im):
        nonlocal h, w
        if opt['update']:
            _, ih, iw = im.shape
            h = round(ih * opt['scaleH']) if 'scaleH' in opt else opt['height']
            w = round(iw * opt['scaleW']) if 'scaleW' in opt else opt['width']
            if out and out.get('source'):
                opt['update'] = False
        return resizeByTorch(im, w, h, opt['method'])
    return f


def restrictSize(width, height=0, method='bilinear'):
    """Shrink to fit width x height keeping the aspect ratio; images that already fit pass through (python/imageProcess.py:197-214)."""
    height = height or width
    st = {}

    def f(im):
        if not st:
            _, ih, iw = im.shape
            st['fit'] = ih <= height and iw <= width
            sh, sw = height / ih, width / iw
            st['hw'] = (height, round(iw * sh)) if sh < sw else (round(ih * sw), width)
        return im if st['fit'] else resizeByTorch(im, st['hw'][1], st['hw'][0], method)
    return f


# ---- self-ensemble (python/imageProcess.py:563-572) -------------------------------------------------
def _dihedral(t, fh, fv):
    """One element of the square's symmetry group as (transpose first?, flip width?, flip height?), and its inverse."""
    def fwd(x):
        if t:
            x = x.transpose(-1, -2)
        dims = ([-1] if fh else []) + ([-2] if fv else [])
        return x.flip(*dims) if dims else x

    def inv(x):
        dims = ([-1] if fh else []) + ([-2] if fv else [])
        if dims:
            x = x.flip(*dims)
        return x.transpose(-1, -2) if t else x
    return fwd, inv


# the seven non-identity symmetries in the reference's order (python/imageProcess.py:563-569: transpose, flip, flip2, flip.transpose,
# transpose.flip, transpose.flip.transpose, flip2.transpose -- "a.b" applies a first); transpose.flip.transpose is a height flip
_SYMMETRIES = [_dihedral(True, False, False), _dihedral(False, True, False), _dihedral(False, True, True), _dihedral(True, False, True),
               _dihedral(True, True, False), _dihedral(False, False, True), _dihedral(True, True, True)]
trans = [f for f, _ in _SYMMETRIES]
transInv = [g for _, g in _SYMMETRIES]


def _ensembleOnDevice(opt, x):
    """The whole averaged ensemble as one call (moe_run_plan_ens): per symmetry one pass that transforms and pads x, doCrop on the device into a canvas the net owns,
    and one pass that folds it into the result in place -- the last one dividing by opt.ensemble + 1.  Bit for bit what the torch expressions of `ensemble` give."""
    if x.dim() != 3:
        raise ValueError('doCrop expects a (C,H,W) image')
    model = opt.modelCached
    if x.dtype not in _DT:
        x = x.to(config.dtype())
    C, H, W = x.shape
    plan = _plan_for(opt, (C, H, W))
    planT = _plan_for(opt, (C, W, H))          # (symmetry 0 is the transpose: every ensemble needs it)
    model.to(device=x.device)
    out = x.new_empty((C, plan.outH, plan.outW))
    sC, sH, sW = x.stride()
    stream = torch.cuda.current_stream(x.device).cuda_stream

    def run():
        _lib.check(_lib.lib().moe_run_plan_ens(model._h, plan._h, planT._h, int(opt.ensemble), x.data_ptr(), _DT[x.dtype], sC, sH, sW,
                                               out.data_ptr(), _DT[out.dtype], int(config.tilesPerBatch), stream))
    try:
        run()
    except MemoryError:              # (as doCrop: the engine's buffers are hipMalloc'ed beside torch's caching allocator)
        torch.cuda.empty_cache()
        run()
    x.record_stream(torch.cuda.current_stream(x.device))      # the engine reads x asynchronously
    return out


def ensemble(opt, average=False):
    """x -> doCrop(x) + sum_i transInv_i(doCrop(trans_i(x))) for the first opt.ensemble transforms.
    (The reference keeps a second Option for transposed shapes; here plans are keyed by shape.)
    average: the result is also divided by opt.ensemble + 1 (runSR.sr; nothing is divided when opt.ensemble is 0).  With config.ensembleOnDevice the transforms,
    the sums and that division run as the engine's own passes (_ensembleOnDevice: the average is its last fold's, so the plain sum stays with torch); the torch
    expressions below are the other form of the same bits."""
    def f(x):
        v = doCrop(opt, x)
        for i in range(opt.ensemble):
            v = v + transInv[i](doCrop(opt, trans[i](x)))
        return v

    def g(x):
        if average and opt.ensemble > 0 and config.ensembleOnDevice and isinstance(opt.modelCached, EngineModule) and x.device.type == 'cuda':
            return _ensembleOnDevice(opt, x)
        v = f(x)
        return v / (opt.ensemble + 1) if average and opt.ensemble else v
    return g


# ---- DN wrapper (python/imageProcess.py:336-377, 562) -----------------------------------------------
def strengthOp(x, inp, s=1):
    """Blend the denoised image with its input: s * x + (1 - s) * inp (python/imageProcess.py:562)."""
    return x if s == 1 else s * x + (1 - s) * inp


def extractAlpha(t):
    """Splits a 4-plane image into RGB (returned) and alpha (kept in `t`); other plane counts pass through."""
    def f(im):
        if im.shape[0] != 4:
            return im
        t['im'] = im[3]
        return im[:3]
    return f


def mergeAlpha(t):
    """Re-attaches the alpha plane extractAlpha put aside (none: the image passes through)."""
    def f(im):
        if 'im' not in t:
            return im
        return torch.cat([im, t['im'].unsqueeze(0).to(im.dtype)], 0)
    return f


def _finite(s):
    return isinstance(s, (int, float)) and math.isfinite(s)


def _RGBFilter(opt, img, reuse=None):
    """The DN wrapper (python/imageProcess.py:350-377): the denoiser sees the colour planes only, `strength` blends its result
    with the input, alpha rides around it.  With config.filterOnDevice the blend and the alpha plane are the final fold's own work (moe_run_plan_filter: one call, no
    temporaries, no concatenation) whenever there is something to blend or to carry; the torch expressions below are the other form of the same bits.  The image
    must be dense and 16-byte aligned, as every image of the pipeline is: torch rounds the fp16 products of a strided view differently (stitch_mix_kernel's comment)."""
    alpha = {}
    rgb = opt.prepare(extractAlpha(alpha)(img))
    if (config.filterOnDevice and isinstance(opt.modelCached, EngineModule) and rgb.device.type == 'cuda' and rgb.dtype in _DT and rgb.dim() == 3
            and rgb.is_contiguous() and rgb.data_ptr() % 16 == 0 and _finite(opt.strength) and (opt.strength != 1 or 'im' in alpha)):
        return _runPlan('RGBFilter', opt, rgb, mix=(opt.strength, alpha.get('im')), reuse=reuse)
    return mergeAlpha(alpha)(strengthOp(doCrop(opt, rgb, reuse=reuse), rgb, opt.strength))


def filterOut(opt, img, bitDepth, out=None, reuse=None, dither=None):
    """toOutput(bitDepth)(toFloat(_RGBFilter(opt, img))) without the download, as ONE call (moe_run_plan_filter), as doCropOut is to doCrop: the final fold blends each
    pixel with the input, rounds as the canvas of img's dtype would have and writes the quantised (H, W, C) image, alpha included; neither the canvas nor its fp32
    copy exists.  strength must be finite.  out: as doCropOut's."""
    if not _finite(opt.strength):
        raise ValueError('filterOut: strength must be finite, got {!r}'.format(opt.strength))
    alpha = {}
    rgb = opt.prepare(extractAlpha(alpha)(img))
    return _runPlan('filterOut', opt, rgb, bitDepth, out, mix=(opt.strength, alpha.get('im')), reuse=reuse, dither=dither)          # (dither: the fold's quantiser, quant.py)


RGBFilter = lambda opt: lambda img: _RGBFilter(opt, img)


# ---- image edges (python/imageProcess.py:238-302) ----------------------------------------------------
def toTorch(bitDepth, dtype=None, device=None):
    """HWC uint8 / uint16 numpy image -> (C,H,W) tensor on the device, v/255 (8 bit) or v/2^bits."""
    def f(image):
        dt = dtype if dtype is not None else config.dtype()
        dev = torch.device(device if device is not None else config.device())
        a = np.ascontiguousarray(image)
        if a.ndim == 2:
            a = a[:, :, None]
        if bitDepth <= 8:
            a = a.astype(np.uint8, copy=False)
            src_dt = _lib.U8
        else:
            a = a.astype(np.uint16)
            src_dt = _lib.U16
        H, W, C = a.shape
        src = torch.from_numpy(a).to(dev)
        dst = torch.empty((C, H, W), dtype=dt, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib().moe_to_float(src.data_ptr(), src_dt, int(bitDepth), H, W, C, dst.data_ptr(), _DT[dt], dev.index or 0, stream))
        src.record_stream(torch.cuda.current_stream(dev))
        return dst
    return f


def toFloat(image):
    """python/imageProcess.py:238-243: (C,H,W) -> (H,W,C) fp32 (a permuted view when already fp32)."""
    if len(image.shape) == 3:
        image = image.permute(1, 2, 0)
    else:
        image = image.squeeze(0)
    return image.to(dtype=torch.float)


def toOutput(bitDepth, dither=None):
    """python/imageProcess.py:245-257: x * 2^bits, clamp [0, 2^bits - 1], truncate, to host numpy (H,W,C).  dither: None | 'round' | 'ordered' -- the rounding or
    ordered-dither quantiser instead (moephoto_amd/quant.py; 8 bits at unit scale, the inverse of toTorch's / 255)."""
    qf = ditherFlags('toOutput', dither, 8 if bitDepth <= 8 else bitDepth, 'rgb')

    def f(image):
        if image.dim() == 2:
            image = image.unsqueeze(2)
        H, W, C = image.shape
        planar = image.permute(2, 0, 1)
        if not planar.is_contiguous():
            planar = planar.contiguous()
        if planar.dtype not in _DT:
            planar = planar.float()
        dev = planar.device
        out_dt, np_dt, lib_dt = (torch.uint8, np.uint8, _lib.U8) if bitDepth <= 8 else (torch.int16, np.uint16, _lib.U16)
        dst = torch.empty((H, W, C), dtype=out_dt, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib().moe_to_output(planar.data_ptr(), _DT[planar.dtype], H, W, C, int(bitDepth) | qf, dst.data_ptr(), lib_dt, dev.index or 0, stream))
        planar.record_stream(torch.cuda.current_stream(dev))
        res = dst.cpu().numpy()
        return res.view(np_dt) if bitDepth > 8 else res
    return f


toOutput8 = toOutput(8)


def toYuv(fmt, matrix='bt709', order='bgr', dither=None):
    """The unfused form of doCropYuv (moe_to_yuv): a (3, H, W) fp16 / fp32 device image -> the flat uint8 device tensor of its Y'CbCr 4:2:0 frame, from the samples
    toOutput(16)(toFloat(y)) would give.  f(y, out=None); out as doCropYuv's."""
    depth, mat, ordr = pixfmt.check(fmt, matrix, order)
    depth |= ditherFlags('toYuv', dither, depth, 'yuv')          # (quant.yuvFromSamples16)

    def f(y, out=None):
        if y.device.type != 'cuda':
            raise _lib.EngineError('toYuv: input must live on a HIP device (moephoto_amd has no CPU path)')
        if y.dim() != 3 or y.shape[0] != 3:
            raise ValueError('toYuv expects a (3,H,W) image, got {}'.format(tuple(y.shape)))
        if y.dtype not in _DT:
            y = y.float()
        y = y.contiguous()
        _, H, W = y.shape
        out = _yuvOut('toYuv', fmt, W, H, out, y.device)
        cur = torch.cuda.current_stream(y.device)
        _lib.check(_lib.lib().moe_to_yuv(y.data_ptr(), _DT[y.dtype], H, W, depth, mat, ordr, out.data_ptr(), y.device.index or 0, cur.cuda_stream))
        y.record_stream(cur)
        return out
    return f


def fromPlanes(fmt, w, h, dtype=None):
    """The source edge of a chain on the decoder's planes (moe_planes_to_float; the definition: pixfmt.toPlanes): f(raw_dev, outY=None, outC=None) takes the planar
    4:2:0 frame as a flat uint8 device tensor of pixfmt.frameBytes(fmt, w, h) and returns Y (1, h, w) and C (2, h / 2, w / 2) of dtype (default: config.dtype()),
    code * 2^-depth; outY / outC: tensors of those shapes to write into."""
    (yh, yw), (ch, cw) = pixfmt.planeShapes(fmt, w, h)
    depth, n = pixfmt.FORMATS[fmt], pixfmt.frameBytes(fmt, w, h)

    def f(raw_dev, outY=None, outC=None):
        if raw_dev.device.type != 'cuda':
            raise _lib.EngineError('fromPlanes: input must live on a HIP device (moephoto_amd has no CPU path)')
        if tuple(raw_dev.shape) != (n,) or raw_dev.dtype != torch.uint8 or not raw_dev.is_contiguous():
            raise ValueError('fromPlanes: a flat contiguous uint8 tensor of {} bytes ({} at {} x {}) expected, got {} {}'.format(n, fmt, w, h, raw_dev.dtype, tuple(raw_dev.shape)))
        dt = dtype if dtype is not None else config.dtype()
        if dt not in _DT:
            raise ValueError('fromPlanes: dtype must be torch.float16 or torch.float32, got {}'.format(dt))
        outs = []
        for o, shape in ((outY, (1, yh, yw)), (outC, (2, ch, cw))):
            if o is None:
                o = torch.empty(shape, dtype=dt, device=raw_dev.device)
            elif tuple(o.shape) != shape or o.dtype != dt or not o.is_contiguous() or o.device != raw_dev.device:
                raise ValueError('fromPlanes: a contiguous {} tensor of shape {} on {} expected'.format(dt, shape, raw_dev.device))
            outs.append(o)
        cur = torch.cuda.current_stream(raw_dev.device)
        _lib.check(_lib.lib().moe_planes_to_float(raw_dev.data_ptr(), depth, yh, yw, outs[0].data_ptr(), outs[1].data_ptr(), _DT[dt], raw_dev.device.index or 0, cur.cuda_stream))
        raw_dev.record_stream(cur)
        return outs[0], outs[1]
    return f


def toPlanes(depth, dither=None):
    """The unfused form of doCropPlanes (moe_to_output on the dense planes: H = C * h, W = w, C = 1, bits = depth): f(y, out=None) quantises a (C, h, w) fp16 / fp32 device
    image plane by plane into a flat uint8 device tensor of C * h * w samples (uint8 for depth 8, else uint16); out as doCropPlanes'."""
    if depth not in pixfmt.FORMATS.values():
        raise ValueError('toPlanes: depth must be one of {}, got {!r}'.format(sorted(pixfmt.FORMATS.values()), depth))
    qf = ditherFlags('toPlanes', dither, depth, 'planes')          # (with a mode: one call per plane, so that a sample's coordinates are its own plane's -- the fused edge's bytes)

    def f(y, out=None):
        if y.device.type != 'cuda':
            raise _lib.EngineError('toPlanes: input must live on a HIP device (moephoto_amd has no CPU path)')
        if y.dim() != 3:
            raise ValueError('toPlanes expects a (C,H,W) image, got {}'.format(tuple(y.shape)))
        if y.dtype not in _DT:
            y = y.float()
        y = y.contiguous()
        C, H, W = y.shape
        out = _planesOut('toPlanes', depth, C, H, W, out, y.device)
        cur = torch.cuda.current_stream(y.device)
        o_dt, es = (_lib.U8, 1) if depth == 8 else (_lib.U16, 2)
        for c in range(C) if qf else (0,):
            _lib.check(_lib.lib().moe_to_output(y.data_ptr() + c * H * W * y.element_size(), _DT[y.dtype], H if qf else C * H, W, 1, int(depth) | qf,
                                                out.data_ptr() + c * H * W * es, o_dt, y.device.index or 0, cur.cuda_stream))
        y.record_stream(cur)
        return out
    return f


def _flatPair(who, what, src, n_in, out, n_out):
    """What resampleChroma's and fitPlanes' f check of their two buffers: one HIP device, flat contiguous uint8 tensors of exactly n_in and n_out bytes."""
    if src.device.type != 'cuda' or out.device != src.device:
        raise _lib.EngineError('{}: both {} must live on one HIP device (moephoto_amd has no CPU path)'.format(who, what))
    for t, n in ((src, n_in), (out, n_out)):
        if tuple(t.shape) != (n,) or t.dtype != torch.uint8 or not t.is_contiguous():
            raise ValueError('{}: a flat contiguous uint8 tensor of {} bytes expected, got {} {}'.format(who, n, t.dtype, tuple(t.shape)))


def resampleChroma(srcFmt, dstFmt, w, h, scale, method, loc='center'):
    """The chroma planes of a luma-only chain (moe_chroma_resample; the definition: pixfmt.resampleChroma): f(raw_dev, out) reads the Cb and Cr planes of the planar
    4:2:0 frame of w x h in raw_dev (a flat uint8 device tensor of pixfmt.frameBytes(srcFmt, w, h)) and writes them, `scale` times as large and at dstFmt's depth,
    into the chroma planes of the frame of w * scale x h * scale in out (flat uint8, pixfmt.frameBytes(dstFmt, w * scale, h * scale)); out's Y plane is not touched.
    The tables are pixfmt.chromaTable's: `loc` sites the horizontal axis, the vertical one is always 'center'."""
    (_, _), (ch, cw) = pixfmt.planeShapes(srcFmt, w, h)
    if dstFmt not in pixfmt.FORMATS:
        raise ValueError('pixFmt "{}" is not supported ({})'.format(dstFmt, ', '.join(pixfmt.FORMATS)))
    (ox, cx), (oy, cy) = pixfmt.chromaTable(method, scale, loc), pixfmt.chromaTable(method, scale, 'center')
    taps = pixfmt.CHROMA_METHODS[method]
    tabs = ((ctypes.c_int16 * (scale * taps))(*sum(cx, [])), (ctypes.c_int8 * scale)(*ox), (ctypes.c_int16 * (scale * taps))(*sum(cy, [])), (ctypes.c_int8 * scale)(*oy))
    n_in, n_out = pixfmt.frameBytes(srcFmt, w, h), pixfmt.frameBytes(dstFmt, w * scale, h * scale)
    at_in, at_out = pixfmt.planeOffsets(srcFmt, w, h)[1], pixfmt.planeOffsets(dstFmt, w * scale, h * scale)[1]
    Ds, Dd = pixfmt.FORMATS[srcFmt], pixfmt.FORMATS[dstFmt]

    def f(raw_dev, out):
        _flatPair('resampleChroma', 'frames', raw_dev, n_in, out, n_out)
        cur = torch.cuda.current_stream(raw_dev.device)
        _lib.check(_lib.lib().moe_chroma_resample(raw_dev.data_ptr() + at_in, Ds, ch, cw, out.data_ptr() + at_out, Dd, scale, taps, *tabs,
                                                  raw_dev.device.index or 0, cur.cuda_stream))
        raw_dev.record_stream(cur)
        return out
    return f


def guidedChroma(srcFmt, dstFmt, w, h, scale, loc='center'):
    """The chroma planes of a luma-only chain steered by the finished luma (moe_chroma_guided; the definition: pixfmt.guidedChroma): f(raw_dev, out) reads the Cb, Cr
    and Y' planes of the planar 4:2:0 frame of w x h in raw_dev (a flat uint8 device tensor of pixfmt.frameBytes(srcFmt, w, h)) and the Y' plane of the frame of
    w * scale x h * scale in out (flat uint8, pixfmt.frameBytes(dstFmt, w * scale, h * scale)) as the chain wrote it, and writes out's chroma planes; out's Y plane is
    not touched.  The tables are pixfmt.guidedTable's and guidedRange's: `loc` sites the horizontal axis, the vertical one is always 'center'."""
    (_, _), (ch, cw) = pixfmt.planeShapes(srcFmt, w, h)
    if dstFmt not in pixfmt.FORMATS:
        raise ValueError('pixFmt "{}" is not supported ({})'.format(dstFmt, ', '.join(pixfmt.FORMATS)))
    (ox, cx), (oy, cy) = pixfmt.guidedTable(scale, loc), pixfmt.guidedTable(scale, 'center')
    tabs = ((ctypes.c_uint8 * (scale * 4))(*sum(cx, [])), (ctypes.c_int8 * scale)(*ox), (ctypes.c_uint8 * (scale * 4))(*sum(cy, [])), (ctypes.c_int8 * scale)(*oy),
            (ctypes.c_uint8 * 64)(*pixfmt.guidedRange()))
    n_in, n_out = pixfmt.frameBytes(srcFmt, w, h), pixfmt.frameBytes(dstFmt, w * scale, h * scale)
    at_in, at_out = pixfmt.planeOffsets(srcFmt, w, h)[1], pixfmt.planeOffsets(dstFmt, w * scale, h * scale)[1]
    Ds, Dd = pixfmt.FORMATS[srcFmt], pixfmt.FORMATS[dstFmt]

    def f(raw_dev, out):
        _flatPair('guidedChroma', 'frames', raw_dev, n_in, out, n_out)
        cur = torch.cuda.current_stream(raw_dev.device)
        _lib.check(_lib.lib().moe_chroma_guided(raw_dev.data_ptr() + at_in, raw_dev.data_ptr(), Ds, ch, cw, out.data_ptr() + at_out, out.data_ptr(), Dd, scale,
                                                _lib.CHROMA_LOCS[loc], *tabs, raw_dev.device.index or 0, cur.cuda_stream))
        raw_dev.record_stream(cur)
        return out
    return f


def planesToRGB(srcFmt, w, h, rgbFmt, matrix='bt709', method='bicubic', loc='center', dither=None):
    """RGB frames from a chain on 4:2:0 planes (moe_planes_to_rgb; the definition: pixfmt.toRGB): f(planar_dev, out) reads the planar 4:2:0 frame of w x h in
    planar_dev (a flat uint8 device tensor of pixfmt.frameBytes(srcFmt, w, h)) and writes the interleaved h x w x 3 frame at rgbFmt ('bgr24', 'rgb24', 'bgr48le',
    'rgb48le') into out (flat uint8, 3 w h bytes or twice that), in one launch; the chroma planes at luma size never exist.  The tables are pixfmt.chromaTable's at
    scale 2 (`loc` sites the horizontal axis, the vertical one is always 'center'), the constants pixfmt.rgbCoefficients'; dither: None / 'round' (the same bytes) or
    'ordered'."""
    pixfmt.planeShapes(srcFmt, w, h)
    if rgbFmt not in pixfmt.RGB_FORMATS:
        raise ValueError('pixFmt "{}" is not an RGB format ({})'.format(rgbFmt, ', '.join(pixfmt.RGB_FORMATS)))
    D, (bits, order) = pixfmt.FORMATS[srcFmt], pixfmt.RGB_FORMATS[rgbFmt]
    ids = pixfmt.check(srcFmt, matrix, order)
    (ox, cx), (oy, cy) = pixfmt.chromaTable(method, 2, loc), pixfmt.chromaTable(method, 2, 'center')
    taps = pixfmt.CHROMA_METHODS[method]
    tabs = ((ctypes.c_int16 * (2 * taps))(*sum(cx, [])), (ctypes.c_int8 * 2)(*ox), (ctypes.c_int16 * (2 * taps))(*sum(cy, [])), (ctypes.c_int8 * 2)(*oy),
            (ctypes.c_int32 * 5)(*pixfmt.rgbCoefficients(matrix, D, bits)))
    qf = ditherFlags('planesToRGB', dither, bits, 'yuv')          # (an integer edge: no unit flag, as the Y'CbCr edge)
    n_in, n_out = pixfmt.frameBytes(srcFmt, w, h), 3 * int(w) * int(h) * (bits // 8)

    def f(planar_dev, out):
        _flatPair('planesToRGB', 'frames', planar_dev, n_in, out, n_out)
        cur = torch.cuda.current_stream(planar_dev.device)
        _lib.check(_lib.lib().moe_planes_to_rgb(planar_dev.data_ptr(), D, int(h), int(w), out.data_ptr(), bits | qf, ids[1], ids[2], taps, *tabs,
                                                planar_dev.device.index or 0, cur.cuda_stream))
        planar_dev.record_stream(cur)
        return out
    return f


_fitTabs = {}          # (method, n, m, loc) -> (taps, coefficients as c_int16[m * taps], offsets as c_int32[m]): built once per size (exact fractions: seconds at 8K)


def fitTables(method, n, m, loc='center'):
    """pixfmt.fitTable(method, n, m, loc) as moe_fit_create takes one axis: (taps, c_int16[m * taps], c_int32[m]), cached per size.  One normalisation: an offset
    beyond the plane's last sample -- 'nearest' with 'left' when the axis grows: floor(c + 1/2) = n for its last outputs -- is passed as n - 1, the sample the
    definition's own clamp reads; moe_fit_create refuses a row that does not reach the plane."""
    key = (method, n, m, loc)
    if key not in _fitTabs:
        off, coef = pixfmt.fitTable(method, n, m, loc)
        taps = len(coef[0])
        off = [min(o, n - 1) for o in off]
        if len(_fitTabs) >= 32:
            _fitTabs.clear()
        _fitTabs[key] = (taps, (ctypes.c_int16 * (m * taps))(*[c for row in coef for c in row]), (ctypes.c_int32 * m)(*off))
    return _fitTabs[key]


class _FitHandle(object):
    """A moe_fit handle: the geometry and the tables on the device, freed with the object."""

    def __init__(self, planes, srcDepth, h, w, dstDepth, oh, ow, tx, ty, device, create='moe_fit_create'):
        self._h = ctypes.c_void_p()          # (create = 'moe_fit_create_px': `planes` are the channels of one interleaved image)
        _lib.check(getattr(_lib.lib(), create)(planes, srcDepth, h, w, dstDepth, oh, ow, tx[0], tx[1], tx[2], ty[0], ty[1], ty[2], device, ctypes.byref(self._h)))

    def info(self):
        """dict(tile=(width, height), lds=bytes per workgroup, planes=..) of the kernel's launch."""
        v = (ctypes.c_int64 * 4)()
        _lib.check(_lib.lib().moe_fit_info(self._h, v))
        return dict(tile=(int(v[0]), int(v[1])), lds=int(v[2]), planes=int(v[3]))

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h and _lib._lib is not None:
            _lib._lib.moe_fit_destroy(h)


def fitPlanes(srcDepth, dstDepth, planes, h, w, oh, ow, method, loc='center'):
    """Planes of codes brought to a fitted size (moe_fit_create / moe_fit_run; the definition: pixfmt.fitPlanes): f(src_dev, out) reads `planes` planes of h x w codes
    at srcDepth from src_dev (a flat contiguous uint8 device tensor of exactly those bytes: a frame's Y plane, its two chroma planes, or a view of them) and writes as
    many planes of oh x ow at dstDepth into out, likewise.  The tables are pixfmt.fitTable's, cached per size: `loc` sites the horizontal axis, the vertical one is
    always 'center'.  The handle (tables on the device) is made at the first call, for that call's device, and lives as long as f; f.info() describes its launch."""
    for d in (srcDepth, dstDepth):
        if d not in pixfmt.FORMATS.values():
            raise ValueError('fitPlanes: depth must be one of {}, got {!r}'.format(sorted(pixfmt.FORMATS.values()), d))
    if not isinstance(planes, int) or isinstance(planes, bool) or not 1 <= planes <= 4:
        raise ValueError('fitPlanes: planes must be 1..4, got {!r}'.format(planes))
    h, w, oh, ow = int(h), int(w), int(oh), int(ow)
    tx, ty = fitTables(method, w, ow, loc), fitTables(method, h, oh, 'center')          # (ValueError for what fitTable refuses)
    n_in, n_out = planes * h * w * (1 if srcDepth == 8 else 2), planes * oh * ow * (1 if dstDepth == 8 else 2)
    handles = {}

    def handle(device):
        if device not in handles:
            handles[device] = _FitHandle(planes, srcDepth, h, w, dstDepth, oh, ow, tx, ty, device.index or 0)
        return handles[device]

    def f(src_dev, out):
        _flatPair('fitPlanes', 'buffers', src_dev, n_in, out, n_out)
        cur = torch.cuda.current_stream(src_dev.device)
        _lib.check(_lib.lib().moe_fit_run(handle(src_dev.device)._h, src_dev.data_ptr(), out.data_ptr(), cur.cuda_stream))
        src_dev.record_stream(cur)
        return out
    f.info = lambda device=None: handle(device if device is not None else torch.device(config.device())).info()
    return f


def fitPixels(srcDepth, dstDepth, channels, h, w, oh, ow, method):
    """An interleaved image of codes brought to a fitted size (moe_fit_create_px / moe_fit_run; the definition: pixfmt.fitPixels): f(src_dev, out) reads h x w pixels
    of `channels` codes each at srcDepth from src_dev (a flat contiguous uint8 device tensor of exactly those bytes: a bgr24 / bgr48le frame, or a view of one) and
    writes oh x ow pixels at dstDepth into out, likewise.  fitPlanes' tables ('center' on both axes), cache, per-device handle and f.info() (planes = the channels)."""
    for d in (srcDepth, dstDepth):
        if d not in pixfmt.FORMATS.values():
            raise ValueError('fitPixels: depth must be one of {}, got {!r}'.format(sorted(pixfmt.FORMATS.values()), d))
    if not isinstance(channels, int) or isinstance(channels, bool) or not 1 <= channels <= 4:
        raise ValueError('fitPixels: channels must be 1..4, got {!r}'.format(channels))
    h, w, oh, ow = int(h), int(w), int(oh), int(ow)
    tx, ty = fitTables(method, w, ow), fitTables(method, h, oh)          # (ValueError for what fitTable refuses)
    n_in, n_out = channels * h * w * (1 if srcDepth == 8 else 2), channels * oh * ow * (1 if dstDepth == 8 else 2)
    handles = {}

    def handle(device):
        if device not in handles:
            handles[device] = _FitHandle(channels, srcDepth, h, w, dstDepth, oh, ow, tx, ty, device.index or 0, 'moe_fit_create_px')
        return handles[device]

    def f(src_dev, out):
        _flatPair('fitPixels', 'buffers', src_dev, n_in, out, n_out)
        cur = torch.cuda.current_stream(src_dev.device)
        _lib.check(_lib.lib().moe_fit_run(handle(src_dev.device)._h, src_dev.data_ptr(), out.data_ptr(), cur.cuda_stream))
        src_dev.record_stream(cur)
        return out
    f.info = lambda device=None: handle(device if device is not None else torch.device(config.device())).info()
    return f


class _LutHandle(object):
    """A moe_lut3d handle: the re-laid table and the vertices on the device, freed with the object."""

    def __init__(self, table, vertices, device):
        self._h = ctypes.c_void_p()
        _lib.check(_lib.lib().moe_lut3d_create(int(table.shape[1]), table.ctypes.data, vertices.ctypes.data, device, ctypes.byref(self._h)))

    def info(self):
        """dict(d=.., tableBytes=the device's table, lds=bytes per workgroup, pixels=per thread) of the kernel's launch."""
        v = (ctypes.c_int64 * 4)()
        _lib.check(_lib.lib().moe_lut3d_info(self._h, v))
        return dict(d=int(v[0]), tableBytes=int(v[1]), lds=int(v[2]), pixels=int(v[3]))

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h and _lib._lib is not None:
            _lib._lib.moe_lut3d_destroy(h)


def lut3d(table, vertices=None, srcBits=16, bits=16, order='bgr', strength=1.0, dither=None):
    """The 3D LUT colour step (moe_lut3d_create / moe_lut3d_run; the definition: lut3d.apply): f(src_dev, out, h, w) reads the h x w x 3 interleaved samples at srcBits
    (8 | 16) in src_dev (a flat contiguous uint8 device tensor of exactly those bytes) and writes as many at `bits` (8 | 16) into out, likewise, in one launch: the
    reader, the trilinear lookup in `table` (float32 (3, d, d, d), [c, b, g, r]) over `vertices` (float32 (3, d); lut3d.uniform(d) by default), the blend with
    `strength`, the quantiser with `dither` (None | 'round' | 'ordered').  order: 'bgr' | 'rgb', of both sides.  Everything lut3d.check refuses is refused here, before
    a device is needed.  The handle (the table on the device) is made at the first call, for that call's device, and lives as long as f; f.info() describes it."""
    from . import lut3d as _def
    table = np.asarray(table)
    table, vertices = _def.check(table, _def.uniform(table.shape[1]) if vertices is None and table.ndim == 4 else vertices)
    for name, b in (('srcBits', srcBits), ('bits', bits)):
        if b not in (8, 16):
            raise ValueError('lut3d: {} must be 8 or 16, got {!r}'.format(name, b))
    if order not in _def.ORDERS:
        raise ValueError("lut3d: 'order' {!r} is not supported ({})".format(order, ', '.join(_def.ORDERS)))
    strength = float(strength)
    if not math.isfinite(strength):
        raise ValueError("lut3d: 'strength' {!r} is not finite".format(strength))
    qf = ditherFlags('lut3d', dither, bits, 'rgb')
    oid = 1 if order == 'rgb' else 0          # MOE_ORDER_RGB / MOE_ORDER_BGR
    handles = {}

    def handle(device):
        if device not in handles:
            handles[device] = _LutHandle(table, vertices, device.index or 0)
        return handles[device]

    def f(src_dev, out, h, w):
        n = 3 * int(h) * int(w)
        _flatPair('lut3d', 'buffers', src_dev, n * (srcBits // 8), out, n * (bits // 8))
        cur = torch.cuda.current_stream(src_dev.device)
        _lib.check(_lib.lib().moe_lut3d_run(handle(src_dev.device)._h, src_dev.data_ptr(), srcBits, int(h), int(w), out.data_ptr(), bits | qf, oid, strength, cur.cuda_stream))
        src_dev.record_stream(cur)
        return out
    f.info = lambda device=None: handle(device if device is not None else torch.device(config.device())).info()
    return f


class _AilutHandle(object):
    """A moe_ailut handle: the generator's parameters and workspace on the device, freed with the object."""

    def __init__(self, params, device):
        L = _lib.lib()
        self._h = ctypes.c_void_p()
        _lib.check(L.moe_ailut_create(int(params['d']), int(params['ranks']), ctypes.byref(self._h)))
        name, shape, ndim = ctypes.c_char_p(), (ctypes.c_int64 * 4)(), ctypes.c_int()
        for i in range(_lib.check(L.moe_ailut_num_params(self._h))):
            _lib.check(L.moe_ailut_param_info(self._h, i, ctypes.byref(name), shape, ctypes.byref(ndim)))
            a = np.ascontiguousarray(params[name.value.decode()], np.float32)
            _lib.check(L.moe_ailut_set_param(self._h, name.value, a.ctypes.data, (ctypes.c_int64 * 4)(*a.shape), a.ndim))
        _lib.check(L.moe_ailut_finalize(self._h, device))

    def guards(self, stream=None):
        """How many guard bytes between the handle's device buffers, and parameters, no longer hold what finalize wrote (moe_ailut_guards)."""
        bad = ctypes.c_int64()
        _lib.check(_lib.lib().moe_ailut_guards(self._h, ctypes.byref(bad), stream))
        return int(bad.value)

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h and _lib._lib is not None:
            _lib._lib.moe_ailut_destroy(h)


def readLut3d(handle, stream=None):
    """(table float32 (3, d, d, d), vertices float32 (3, d)) of a _LutHandle as they stand on the device behind `stream`'s work (moe_lut3d_read; synchronises it)."""
    d = handle.info()['d']
    table, vertices = np.empty((3, d, d, d), np.float32), np.empty((3, d), np.float32)
    _lib.check(_lib.lib().moe_lut3d_read(handle._h, table.ctypes.data, vertices.ctypes.data, stream))
    return table, vertices


def ailut(params, srcBits=16, bits=16, order='bgr', strength=1.0, dither=None, tableOut=None):
    """The image-adaptive 3D LUT (moe_ailut_run + moe_lut3d_run; the definition: lut3d.apply with ailut.generate(ailut.thumbnail(frame))'s table): f(src_dev, out, h,
    w) as lut3d's f, but the table is the one the generator net writes for THIS frame -- eight launches from the frame's thumbnail to the table in the handle's own
    device layout, then the LUT's launch, all on the current stream, no host round trip.  params: ailut.loadParams' dict.  tableOut: a callable handed every frame's
    (table, vertices) behind its launches -- it synchronises the stream, so it is for a caller who wants the tables (lut3d.formatCube), not for speed.  f.read(device)
    returns the (table, vertices) of the last frame queued on that device (it synchronises too); f.generator(device) / f.table(device) are the two handles."""
    from . import ailut as _net, lut3d as _def
    if not isinstance(params, dict) or 'd' not in params or 'ranks' not in params:
        raise ValueError("ailut: 'params' is ailut.loadParams' dict")
    for name, b in (('srcBits', srcBits), ('bits', bits)):
        if b not in (8, 16):
            raise ValueError('ailut: {} must be 8 or 16, got {!r}'.format(name, b))
    if order not in _def.ORDERS:
        raise ValueError("ailut: 'order' {!r} is not supported ({})".format(order, ', '.join(_def.ORDERS)))
    strength = float(strength)
    if not math.isfinite(strength):
        raise ValueError("ailut: 'strength' {!r} is not finite".format(strength))
    for key in _net.paramShapes(params['d'], params['ranks']):
        if key not in params:
            raise ValueError("ailut: 'params' has no '{}'".format(key))
    if tableOut is not None and not callable(tableOut):
        raise ValueError("ailut: 'tableOut' is a callable taking (table, vertices)")
    qf = ditherFlags('ailut', dither, bits, 'rgb')
    oid = 1 if order == 'rgb' else 0          # MOE_ORDER_RGB / MOE_ORDER_BGR
    d, handles = int(params['d']), {}

    def handle(device):
        if device not in handles:          # the table handle starts as the identity; every run overwrites it
            handles[device] = (_AilutHandle(params, device.index or 0), _LutHandle(_def.identity(d), _def.uniform(d), device.index or 0))
        return handles[device]

    def f(src_dev, out, h, w):
        n = 3 * int(h) * int(w)
        _flatPair('ailut', 'buffers', src_dev, n * (srcBits // 8), out, n * (bits // 8))
        cur = torch.cuda.current_stream(src_dev.device)
        gen, lut = handle(src_dev.device)
        _lib.check(_lib.lib().moe_ailut_run(gen._h, src_dev.data_ptr(), srcBits, int(h), int(w), oid, lut._h, cur.cuda_stream))
        _lib.check(_lib.lib().moe_lut3d_run(lut._h, src_dev.data_ptr(), srcBits, int(h), int(w), out.data_ptr(), bits | qf, oid, strength, cur.cuda_stream))
        src_dev.record_stream(cur)
        if tableOut is not None:
            tableOut(*readLut3d(lut, cur.cuda_stream))
        return out

    def dev(device):
        return torch.device(device) if device is not None else torch.device(config.device())
    f.generator = lambda device=None: handle(dev(device))[0]
    f.table = lambda device=None: handle(dev(device))[1]
    f.read = lambda device=None: readLut3d(handle(dev(device))[1], torch.cuda.current_stream(dev(device)).cuda_stream)
    return f


def toNumPy(bitDepth):
    """python/imageProcess.py:216-229: (raw frame bytes, height, width) -> (H,W,3) array (the video path's `buffer` source;
    ffmpeg delivers bgr24 / bgr48le).  The reference widens to fp32 here and divides in toTorch; the integer view is kept
    instead and `toTorch` does the division on the device -- same values, one host copy less."""
    dtype = np.uint8 if bitDepth <= 8 else np.uint16

    def f(args):
        buffer, height, width = args
        if not buffer:
            return None
        return np.frombuffer(buffer, dtype=dtype).reshape((height, width, 3))
    return f


def toBuffer(bitDepth):
    """python/imageProcess.py:231-236: quantised (H,W,C) array -> raw bytes for the encoder pipe."""
    dtype = np.uint8 if bitDepth <= 8 else np.uint16
    return lambda im: np.ascontiguousarray(im, dtype=dtype).tobytes() if im is not None else None


def readFile(nodes=[], context=None):
    from PIL import Image

    def f(file):
        image = Image.open(file)
        if context is not None:
            context.imageMode = image.mode
        if image.mode == 'P':
            if context is not None:
                context.palette = image
            image = image.convert('RGB')
        image = np.array(image)
        if len(image.shape) == 2:
            return image.reshape(*image.shape, 1)
        if image.shape[2] in (3, 4):
            return image
        raise RuntimeError('Unknown image format')
    return f


def writeFile(image, name, context=None, *args):
    from PIL import Image
    if not name:
        name = 'output_{}.png'.format(int(time.time()))
    elif hasattr(name, 'seek'):
        name.seek(0)
    if image.shape[2] == 1:
        image = image.squeeze(2)
    Image.fromarray(image).save(name, *args)
    return name
