"""Pipeline builder for the SR / DN steps -- the callers of the hot path (python/procedure.py:46-73,109-136,156-201).

`genProcess(steps)` turns a MoePhoto step list such as

    [{'op': 'file'}, {'op': 'DN', 'model': 'lite5', 'strength': 1.0}, {'op': 'SR', 'model': 'a', 'scale': 2}]

into one callable: image in (HWC uint8/uint16 numpy array, a file when the first step is 'file', or a raw video frame
`(bytes, height, width)` when it is {'op': 'buffer', 'bitDepth': 16} -- python/video.py:23, procedure.py:141-142) -> image out, with
everything between the upload (toTorch) and the download (toOutput) resident on the device: DN through RGBFilter
(python/procedure.py:52-55), SR through runSR.sr (:63-73), resize through moe_resize (:104-107), output = toFloat -> toOutput (:128-136).  The progress/ETA
nodes of the reference are observability only and are not reproduced; `nodes` lists the resolved
steps.  Ops other than file / buffer / DN / SR / resize / output belong to other model families and raise.

`genFrameStream(steps, width, height, depth)` builds the same chain for a video source as a ring of `depth` frames in flight -- upload, compute and download on
three queues, the last fold writing the encoder's samples itself (imageProcess.doCropOut) -- and `runFramesStreamed` is `runFrames` over it.

With {'op': 'buffer', 'pixFmt': 'yuv420p' | 'yuv420p10le' | 'yuv420p12le' | 'yuv420p16le'} as the source step both builders take the decoder's planar Y'CbCr 4:2:0
frames as they are and run the chain on Y' and on Cb / Cr as two images.

`genFrameStream(.., reuse=True)` keeps each step's tile pool from the previous frame and runs only the tiles whose input changed, bit for bit.

With 'chroma': 'nearest' | 'bilinear' | 'bicubic' on such a source step the chain is luma-only: the net runs on Y' alone and Cb / Cr are brought to the output's size
by a fixed integer resampling filter (pixfmt.resampleChroma, moe_chroma_resample); `genFrameStream(.., views=True)` hands the finished frames out as read-only views of
the ring's pinned buffers instead of copies.

With 'chroma': 'guided' there the chain is luma-only as well, and Cb / Cr are written by a joint bilateral filter steered by the Y' the chain has just written into the
frame (pixfmt.guidedChroma, moe_chroma_guided).

With {'op': 'output', 'width': W, 'height': H, 'fit': 'bicubic'} on such a chain both builders deliver W x H frames: the planes the chain gives are brought to the size
asked for by a rational integer polyphase filter that antialiases where it shrinks (pixfmt.fitPlanes, moe_fit_create / moe_fit_run).

With 'chroma': 'nearest' | 'bilinear' | 'bicubic' on an SR or DN step of a chain on an RGB source (a file, an array, a bgr24 / bgr48le buffer) that step is luma-only:
the net runs on Y' alone and Cb / Cr go to its output size through the existing resize; a last step whose fold writes the samples merges the planes inside that fold
(moephoto_amd/luma.py, imageProcess.doCropLuma, moe_run_plan_luma).

With {'op': 'output', 'dither': 'round' | 'ordered'} the chain's last operation -- a float becomes an 8-, 10-, 12- or 16-bit sample -- rounds to nearest or adds an 8 x 8
ordered dither instead of truncating, in whichever edge writes the samples: the last fold, the unfused quantiser, the Y'CbCr conversion (moephoto_amd/quant.py is the
definition; the MOE_Q_* flags of include/moephoto_amd.h).  'none', the default, changes nothing.

With {'op': 'resize', 'width': W, 'height': H, 'fit': 'bicubic'} as the last compute step of a chain on an RGB source both builders deliver W x H frames through the
integer filter instead of moe_resize on a float canvas: the chain in front of the step writes its 16-bit samples as it would without the step, and one
moe_fit_run on the interleaved frame (pixfmt.fitPixels, moe_fit_create_px) brings them to the size and the depth asked for.

With {'op': 'output', 'pixFmt': 'bgr24' | 'rgb24' | 'bgr48le' | 'rgb48le'} behind a planar source both builders deliver interleaved RGB frames: the chain writes its
frame as yuv420p16le through the edge it always used, into one intermediate on the compute queue, and one moe_planes_to_rgb -- the chroma planes x2 by the integer
filter, the standard's inverse matrix in fixed point -- writes the frame handed out (pixfmt.toRGB is the definition).  Beside such a pixFmt the
step takes 'matrix', 'chromaUp' (the filter of the final x2), 'chromaLoc' (how the frame's chroma is sited: H.264 / HEVC material is 'left') and 'dither'.

With {'op': 'lut', 'file': path} or {'op': 'lut', 'table': array, 'vertices': array} ('strength': s is optional) as the last compute step of a chain whose frames are
interleaved RGB samples both builders end the chain in a 3D LUT: whatever edge wrote the frame writes it at 16 bits into one intermediate, and one moe_lut3d_run --
the reference's AiLUT transform, a trilinear lookup over non-uniform vertices, with the strength blend and the quantiser -- writes the frame at the depth asked for
(lut3d.apply is the definition).

With {'op': 'dehaze', 'model': 'AiLUT_sRGB_3' | 'AiLUT_XYZ_3', 'strength': s} -- the reference's own step (python/dehaze.py:27-28) -- in that place the table is made
per frame: moe_ailut_run, the AiLUT generator net, reads the 16-bit intermediate and writes the table the moe_lut3d_run behind it applies (ailut.generate is the
definition).  Every other 'dehaze' model stays NotImplementedError.
"""
import math
import time
from functools import reduce

from . import _lib, ailut as _ailut, lut3d as _lut3d, pixfmt, quant, reuse as _reuse, runDN, runSR
from .config import config
from .imageProcess import (LUMA_KEYS, ailut as ailutSamples, RGBFilter, _RGBFilter, apply, doCrop, doCropLuma, doCropOut, doCropPlanes, doCropYuv, extractAlpha, filterOut, fitPixels, fitPlanes, fromPlanes, identity, guidedChroma, lumaChroma, lumaKeys,
                           lumaMerge, lumaSplit, lut3d as lutSamples, mergeAlpha, planesToRGB, readFile, resampleChroma, resize, toBuffer, toFloat, toNumPy, toOutput, toPlanes, toTorch, toYuv, writeFile, _DT, _outStorage)

stepOpts = dict(SR={'toInt': ['scale', 'ensemble'], 'getOpt': runSR}, DN={'toFloat': ['strength'], 'getOpt': runDN},
                resize={'toInt': ['width', 'height'], 'toFloat': ['scaleW', 'scaleH']})


def convertValues(T, o, keys):
    for key in keys:
        if key in o:
            o[key] = T(o[key])


def _outputFormat(steps):
    """(pixFmt, matrix, order) of the first `output` step that asks for a pixel format, checked (ValueError), or None: the step list is where MoePhoto keeps such
    requests -- {'op': 'output', 'pixFmt': 'yuv420p10le', 'matrix': 'bt709'}; order defaults to 'bgr', the video path's frames."""
    for s in steps:
        if s.get('op') == 'output' and s.get('pixFmt') is not None:
            req = (s['pixFmt'], s.get('matrix', 'bt709'), s.get('order', 'bgr'))
            pixfmt.check(*req)
            return req
    return None


def _outputDither(steps):
    """The `dither` key of the output step -- {'op': 'output', 'dither': 'round' | 'ordered'}; 'none' is the default -- checked before any model is loaded: 'round' / 'ordered'
    or None.  The chain's quantising edge then rounds to nearest or adds the 8 x 8 ordered dither (moephoto_amd/quant.py): RGB samples at 8 bits at unit scale (the
    inverse of the reader's / 255), 16-bit and planar samples at 2^bits, a Y'CbCr output in the integer conversion's rounding constants.  It needs no pixFmt and is valid
    behind file, array, buffer and planar sources.  On a luma-only planar chain the key governs Y' alone: Cb / Cr come from the integer resampling filter
    (resize_kernel_codes), which already rounds to nearest.  ValueError naming the key for an unknown value and for 'dither' beside 'width' / 'height' / 'fit': the
    integer fit filter writes those samples, not a quantiser."""
    mode = None
    for s in steps:
        if s.get('op') != 'output' or 'dither' not in s:
            continue
        v = s['dither']
        if not isinstance(v, str) or v not in quant.MODES:
            raise ValueError("output: 'dither' {!r} is not supported ({})".format(v, ', '.join(quant.MODES)))
        mode = None if v == 'none' else v
        for k in FIT_KEYS:
            if k in s and mode is not None:
                raise ValueError("output: 'dither' does not apply beside '{}': the integer fit filter writes those samples (it rounds to nearest)".format(k))
    if mode is not None and any(k in s for s in steps if s.get('op') == 'output' for k in FIT_KEYS):
        raise ValueError("output: 'dither' does not apply to a chain with 'width' / 'height' / 'fit': the integer fit filter writes those samples (it rounds to nearest)")
    return mode


# ---- luma-only steps on an RGB source --------------------------------------------------------------------------------------
# {'op': 'SR', .., 'chroma': 'bicubic'}: the step runs on Y' alone and Cb / Cr go to its output size through the existing resize (moephoto_amd/luma.py is the definition).
def _lumaCheck(steps, planar=False):
    """Every SR / DN step's 'chroma' / 'chromaMatrix' / 'order' keys, checked before any model is loaded (ValueError naming the key: imageProcess.lumaKeys; and any of
    the three on a step of a planar chain, which has its own 'chroma' key on the source step).  A luma-only step's defaults are written into its dict: 'order' is 'bgr'
    behind a buffer source (the video path's frames), 'rgb' behind a file."""
    default = 'bgr' if steps and steps[0].get('op') == 'buffer' else 'rgb'
    for s in steps:
        if s.get('op') not in ('SR', 'DN'):
            continue
        if planar:
            for k in LUMA_KEYS:
                if k in s:
                    raise ValueError("{}: '{}' does not apply to a step of a chain on planar Y'CbCr 4:2:0 frames: its source step has its own 'chroma' key".format(s['op'], k))
            continue
        chroma, matrix, order = lumaKeys(s, default)
        if chroma != 'net':
            s['chromaMatrix'], s['order'] = matrix, order


def _isLuma(o):
    return getattr(o, 'chroma', 'net') != 'net'


def _lumaStep(op, o):
    """A luma-only SR / DN step in its unfused form -> (f, its reuse form): lumaSplit, the step on Y (runSR.sr: doCrop or the ensemble; RGBFilter's blend), the chroma
    planes resized to Y' 's size, lumaMerge.  The DN step keeps RGBFilter's alpha handling: alpha is split off first and re-attached behind the merge; the SR step sends
    alpha through the net as Y's second plane.  An image of fewer than three planes runs as without the key.  The reuse form is g(x, reuse, changed) -> (y, the
    region of y): the tiles' rule on Y, joined with the resize rule on the same input region for the chroma planes."""
    split, merge = lumaSplit(o.chromaMatrix, o.order), lumaMerge(o.chromaMatrix, o.order)
    plain = runSR.sr(o) if op == 'SR' else RGBFilter(o)

    def run(x, net):
        if x.shape[0] < 3:
            return net(x)
        alpha = {}
        if op == 'DN':
            x = o.prepare(extractAlpha(alpha)(x))
        Y, C = split(x)
        Y = net(Y)
        y = merge(Y, lumaChroma(C, Y.shape[-2], Y.shape[-1], o.chroma))
        return mergeAlpha(alpha)(y) if op == 'DN' else y
    f = lambda x: run(x, plain)
    if op == 'SR' and o.ensemble != 0:
        return f, ('opaque', f)

    def g(x, reuse, changed):
        y = run(x, (lambda Y: doCrop(o, Y, reuse=reuse)) if op == 'SR' else (lambda Y: _RGBFilter(o, Y, reuse)))
        region = reuse.out
        if region is not None and changed is not None:
            inHW, outHW = tuple(x.shape[-2:]), tuple(y.shape[-2:])
            region = region | (changed if inHW == outHW else _reuse.resizeRegion(changed, inHW, outHW, o.chroma))
        else:
            region = None
        return y, region
    return f, ('luma', g)


def _lumaLast(op, o, unfused, bitDepth, dither=None):
    """genProcess' last step when it is a luma-only SR without ensemble or DN of strength 1: doCropLuma with the merge and the quantiser inside the last fold, downloaded
    as toOutput returns its image.  A four-plane image through a DN step (alpha rides around the net) takes the unfused form: the same bytes."""
    import numpy as np
    quantise = toOutput(bitDepth, dither)

    def f(x):
        if op == 'DN' and x.shape[0] == 4:
            return quantise(toFloat(unfused(x)))
        a = doCropLuma(o, o.prepare(x) if op == 'DN' else x, o.chroma, o.chromaMatrix, o.order, bitDepth, dither=dither).cpu().numpy()
        return a.view(np.uint16) if bitDepth > 8 else a
    return f


def _lumaLastOnDevice(op, o, unfused):
    """_lumaLast at 16 bits without the download, for a 'fit' resize step behind it (_pixelFitLast): the (H, W, C) samples stay on the device."""
    quantise = _samplesOnDevice(16)

    def f(x):
        if op == 'DN' and x.shape[0] == 4:
            return quantise(unfused(x))
        return doCropLuma(o, o.prepare(x) if op == 'DN' else x, o.chroma, o.chromaMatrix, o.order, 16)
    return f


def _samplesOnDevice(bitDepth):
    """toOutput(bitDepth)(toFloat(y)) without the download: y (C, H, W) -> the (H, W, C) samples on y's device (_quantiseInto)."""
    into = _quantiseInto(bitDepth)

    def f(y):
        import torch
        C, H, W = y.shape
        out = torch.empty((H, W, C), dtype=_outStorage(bitDepth)[0], device=y.device)
        into(y, out)
        return out
    return f


def _pixelFitLast(fit, fused, bitDepth, download=True):
    """genProcess' tail behind a 'fit' resize step: the chain's 16-bit samples on the device (the fused luma fold's, or the unfused quantiser's), one fitPixels to the
    step's size and the chain's bitDepth, downloaded as toOutput returns its image (download=False: left on the device, for a 'lut' step behind it).  The handle is
    kept per image shape."""
    import numpy as np
    import torch
    samples, fitters = fused or _samplesOnDevice(16), {}

    def f(y):
        mid = samples(y).contiguous()
        H, W, C = mid.shape
        if (H, W, C) not in fitters:
            oh, ow = _pixelFitSize(fit, H, W)          # (the ratios, now that the chain's size is known)
            if len(fitters) >= 8:
                fitters.clear()
            fitters[(H, W, C)] = (oh, ow, fitPixels(16, bitDepth, C, H, W, oh, ow, fit['fit']))
        oh, ow, run = fitters[(H, W, C)]
        out = torch.empty((oh, ow, C), dtype=_outStorage(bitDepth)[0], device=mid.device)
        run(_flatBytes(mid), _flatBytes(out))
        if not download:
            return out
        a = out.cpu().numpy()
        return a.view(np.uint16) if bitDepth > 8 else a
    return f


# ---- chains on the decoder's own planes -----------------------------------------------------------------------------------------------------
# {'op': 'buffer', 'pixFmt': 'yuv420p10le'} as the source step: a frame is the decoder's planar Y'CbCr 4:2:0 frame (pixfmt.frameBytes bytes), the chain runs on Y' as a
# (1, h, w) image and then on Cb / Cr as a (2, h / 2, w / 2) image -- every step treats each as it treats any (C, H, W) image, plans cached per shape on the step's
# Option -- and the frame returned is planar 4:2:0 again, at the source's format or at the one an {'op': 'output', 'pixFmt': ..} step names.  No colour conversion
# takes place anywhere.
def _planeFormats(steps, width=None, height=None):
    """(source pixFmt, output pixFmt) of a step list whose source is planar, or None for every other list.  Everything such a chain refuses is refused here, as a
    ValueError before any model is loaded: an unknown format, a resize step, matrix / order on the output step (there is no conversion they could steer), an odd size,
    what _planeChroma refuses of the source step's 'chroma' / 'chromaLoc' keys and what _planeFit refuses of the output step's 'width' / 'height' / 'fit'.
    The output pixFmt may be one of pixfmt.RGB_FORMATS: 'matrix' then steers that conversion, 'order' stays refused (the format's name carries
    it), and 'chromaUp' / 'chromaLoc' on the output step are refused without such a pixFmt, as is an unknown value of either (_planeRGB)."""
    if not steps or steps[0].get('op') != 'buffer' or steps[0].get('pixFmt') is None:
        return None
    src = dst = steps[0]['pixFmt']
    if src not in pixfmt.FORMATS:
        raise ValueError('buffer: pixFmt "{}" is not supported ({})'.format(src, ', '.join(pixfmt.FORMATS)))
    for s in steps[1:]:
        if s.get('op') == 'resize':
            raise ValueError('a chain on {} planes cannot hold a resize step (chroma would need its own size)'.format(src))
        if s.get('op') == 'output':
            rgb = s.get('pixFmt') in pixfmt.RGB_FORMATS
            if 'order' in s or ('matrix' in s and not rgb):          # (an RGB pixFmt carries its order in its name)
                raise ValueError("output: 'matrix' / 'order' do not apply to a chain on {} planes: no colour conversion takes place".format(src))
            for k in RGB_KEYS:
                if k in s and not rgb:
                    raise ValueError("output: '{}' applies beside an RGB 'pixFmt' only ({}): it steers the conversion of the chain's planes to RGB".format(k, ', '.join(pixfmt.RGB_FORMATS)))
            if rgb:
                _planeRGB(s)
            if s.get('pixFmt') is not None:
                dst = s['pixFmt']
                if dst not in pixfmt.FORMATS and not rgb:
                    raise ValueError('output: pixFmt "{}" is not supported ({})'.format(dst, ', '.join(pixfmt.FORMATS)))
    if width is not None:
        pixfmt.planeShapes(src, width, height)
    _planeChroma(steps)
    _planeFit(steps, width, height)
    return src, dst


# ---- RGB frames from a planar chain: {'op': 'output', 'pixFmt': 'bgr48le'} ----------------------------------------------------------
RGB_KEYS = ('chromaUp', 'chromaLoc')          # the output step's keys that exist beside an RGB pixFmt only ('matrix' is shared with the RGB -> Y'CbCr edge)
PLANAR16 = 'yuv420p16le'                      # the chain's own frame in front of the conversion


def _planeRGB(s):
    """(rgbFmt, matrix, method, loc) of an output step whose 'pixFmt' is one of pixfmt.RGB_FORMATS ('bgr24', 'rgb24', 'bgr48le', 'rgb48le') behind a planar source:
    the chain writes its frame as yuv420p16le exactly as it would for that pixFmt, without 'dither', and one moe_planes_to_rgb turns it into interleaved RGB samples
    (pixfmt.toRGB is the definition).  'matrix': 'bt709' (the default) | 'bt601' | 'bt2020nc'; 'chromaUp': 'nearest' | 'bilinear' | 'bicubic' (the default), the
    filter of the final x2 of the chroma planes; 'chromaLoc': 'center' (the default) | 'left', how the frame's chroma is sited horizontally -- H.264 / HEVC material
    is 'left' (MPEG-2's and their default co-sited columns), JPEG / MPEG-1 'center'.  The step's 'dither' ('round' | 'ordered') then governs the conversion's one
    rounding.  ValueError naming the key for an unknown value."""
    matrix, method, loc = s.get('matrix', 'bt709'), s.get('chromaUp', 'bicubic'), s.get('chromaLoc', 'center')
    if matrix not in pixfmt.MATRICES:
        raise ValueError("output: 'matrix' \"{}\" is not supported ({})".format(matrix, ', '.join(pixfmt.MATRICES)))
    if method not in pixfmt.CHROMA_METHODS:
        raise ValueError("output: 'chromaUp' \"{}\" is not supported ({})".format(method, ', '.join(pixfmt.CHROMA_METHODS)))
    if loc not in pixfmt.CHROMA_LOCS:
        raise ValueError("output: 'chromaLoc' \"{}\" is not supported ({})".format(loc, ', '.join(pixfmt.CHROMA_LOCS)))
    return s['pixFmt'], matrix, method, loc


def _planeRGBStep(steps, dst):
    """_planeRGB of the output step that names `dst`, the format _planeFormats returned, or None where that is a planar format."""
    if dst not in pixfmt.RGB_FORMATS:
        return None
    return _planeRGB([s for s in steps[1:] if s.get('op') == 'output' and s.get('pixFmt') is not None][-1])


FIT_KEYS = ('width', 'height', 'fit')


def _planeFit(steps, width=None, height=None):
    """(W, H, method) of a planar chain whose output step names a size -- {'op': 'output', 'width': W, 'height': H, 'fit': 'nearest' | 'bilinear' | 'bicubic'}, 'fit'
    defaults to 'bicubic': every plane is brought from the size the chain gives to W x H (chroma to W / 2 x H / 2) by pixfmt.fitPlanes -- or None.  ValueError naming
    the key for a width or height that is not a positive even int, one without the other, an unknown 'fit', 'fit' without a size and, where the source's size is
    known (width, height), a ratio beyond pixfmt.FIT_MAX_DOWN down or pixfmt.FIT_MAX_UP up on either axis against the chain's own output size (and, for a luma-only
    chain, of its one pass from the source's chroma planes)."""
    req = None
    for s in steps[1:]:
        if s.get('op') != 'output' or not any(k in s for k in FIT_KEYS):
            continue
        fit = s.get('fit', 'bicubic')
        if fit not in pixfmt.CHROMA_METHODS:
            raise ValueError('output: fit "{}" is not supported ({})'.format(fit, ', '.join(pixfmt.CHROMA_METHODS)))
        if 'width' not in s and 'height' not in s:
            raise ValueError("output: 'fit' needs a size ('width' and 'height')")
        for k, other in (('width', 'height'), ('height', 'width')):
            if k not in s:
                raise ValueError("output: '{}' is missing beside '{}'".format(k, other))
            v = s[k]
            if not isinstance(v, int) or isinstance(v, bool) or v < 2 or v % 2:
                raise ValueError("output: '{}' must be a positive even int (a 4:2:0 frame), got {!r}".format(k, v))
        req = (s['width'], s['height'], fit)
    if req is None or width is None:
        return req
    scale = 1
    for s in steps[1:]:
        if s.get('op') == 'SR':
            scale *= int(s.get('scale', 1))
    lumaOnly = steps[0].get('chroma', 'net') != 'net'
    for k, have, want in (('width', int(width), req[0]), ('height', int(height), req[1])):
        for n, what in ((have * scale, "the chain's"),) + (((have, "the source's chroma (one pass)"),) if lumaOnly else ()):
            if n > pixfmt.FIT_MAX_DOWN * want:
                raise ValueError("output: '{}' {} shrinks {} {} by more than {}".format(k, want, what, n, pixfmt.FIT_MAX_DOWN))
            if want > pixfmt.FIT_MAX_UP * n:
                raise ValueError("output: '{}' {} enlarges {} {} by more than {}".format(k, want, what, n, pixfmt.FIT_MAX_UP))
    return req


def _refuseFit(steps):
    """A chain whose source is not planar has a resize step for this: the output step's size keys are refused, by name."""
    for s in steps:
        if s.get('op') == 'output':
            for k in FIT_KEYS:
                if k in s:
                    raise ValueError("output: '{}' applies to a chain on planar Y'CbCr 4:2:0 frames only ({{'op': 'buffer', 'pixFmt': ..}}); an RGB chain takes a resize step".format(k))


# ---- a fitted size on an RGB chain: {'op': 'resize', .., 'fit': ..} ----------------------------------------------------------------
def _pixelFit(steps, bitDepth):
    """The resize step that carries a 'fit' key -- {'op': 'resize', 'width': W, 'height': H (or 'scaleW' / 'scaleH'), 'fit': 'nearest' | 'bilinear' | 'bicubic'} -- of a
    chain whose source is not planar, its size keys converted, or None: the frame's samples are pixfmt.fitPixels of the 16-bit samples the chain in front of the step
    writes, at the chain's bitDepth.  ValueError naming the key, before any model is loaded: such a step that is not the last compute step, 'method' beside 'fit', an
    unknown 'fit', an axis without a size, a size below 1, 'dither' or 'pixFmt' on the output step (the filter rounds to nearest and writes RGB samples)."""
    work = [s for s in steps if s.get('op') not in ('file', 'buffer', 'output')]
    fits = [s for s in work if s.get('op') == 'resize' and 'fit' in s]
    if not fits:
        return None
    s = fits[0]
    if s is not work[-1]:
        raise ValueError("resize: a step with 'fit' must be the last compute step of the chain: the integer filter writes the frame's samples")
    if 'method' in s:
        raise ValueError("resize: 'method' does not apply beside 'fit' (one of them names the filter: 'method' moe_resize's on floats, 'fit' the integer one)")
    if not isinstance(s['fit'], str) or s['fit'] not in pixfmt.CHROMA_METHODS:
        raise ValueError("resize: 'fit' {!r} is not supported ({})".format(s['fit'], ', '.join(pixfmt.CHROMA_METHODS)))
    for size, scale in (('width', 'scaleW'), ('height', 'scaleH')):
        if size not in s and scale not in s:
            raise ValueError("resize: 'fit' needs a size: '{}' or '{}' is missing".format(size, scale))
    for o in steps:
        if o.get('op') == 'output':
            if o.get('dither', 'none') != 'none':
                raise ValueError("output: 'dither' does not apply to a chain whose resize step has 'fit': the integer fit filter writes those samples (it rounds to nearest)")
            if o.get('pixFmt') is not None:
                raise ValueError("output: 'pixFmt' does not apply to a chain whose resize step has 'fit': the filter writes the interleaved RGB samples")
    if bitDepth not in (8, 16):
        raise ValueError("resize: 'fit' writes 8- or 16-bit samples, the chain's bitDepth is {!r}".format(bitDepth))
    convertValues(int, s, stepOpts['resize']['toInt'])
    convertValues(float, s, stepOpts['resize']['toFloat'])
    for k in ('width', 'height', 'scaleW', 'scaleH'):
        if k in s and not s[k] > 0:
            raise ValueError("resize: '{}' must be positive, got {!r}".format(k, s[k]))
    return s


def _pixelFitSize(s, h, w):
    """(oh, ow) of a 'fit' resize step behind a chain that gives h x w, rounded as imageProcess.resize rounds; ValueError naming the key for a ratio beyond
    pixfmt.FIT_MAX_DOWN down or pixfmt.FIT_MAX_UP up."""
    oh = round(h * s['scaleH']) if 'scaleH' in s else s['height']
    ow = round(w * s['scaleW']) if 'scaleW' in s else s['width']
    for have, want, size, scale in ((w, ow, 'width', 'scaleW'), (h, oh, 'height', 'scaleH')):
        k = scale if scale in s else size
        if want < 1 or have > pixfmt.FIT_MAX_DOWN * want:
            raise ValueError("resize: '{}' ({} samples) shrinks the chain's {} by more than {}".format(k, want, have, pixfmt.FIT_MAX_DOWN))
        if want > pixfmt.FIT_MAX_UP * have:
            raise ValueError("resize: '{}' ({} samples) enlarges the chain's {} by more than {}".format(k, want, have, pixfmt.FIT_MAX_UP))
    return oh, ow


def _chainSize(work, h, w):
    """(h, w) a chain of compute steps gives from h x w frames, from the step dicts alone -- an SR step's 'scale', a resize step's size keys as the builders convert
    and round them -- so that a 'fit' step's ratio can be refused before the first model is loaded; None where a step's keys do not say (the builder's own walk then
    raises what it always raised)."""
    try:
        for s in work:
            if s['op'] == 'SR':
                h, w = h * int(s['scale']), w * int(s['scale'])
            elif s['op'] == 'resize':
                h = round(h * float(s['scaleH'])) if 'scaleH' in s else int(s['height'])
                w = round(w * float(s['scaleW'])) if 'scaleW' in s else int(s['width'])
    except (KeyError, TypeError, ValueError):
        return None
    return h, w


def _flatBytes(t):
    """A contiguous device tensor of samples as fitPixels takes it: flat uint8."""
    import torch
    return t.view(torch.uint8).reshape(-1)


# ---- the 3D LUT colour step: {'op': 'lut', 'file': path} | {'op': 'lut', 'table': array, 'vertices': array} --------------------------------
LUT_FMT16 = {'bgr24': 'bgr48le', 'rgb24': 'rgb48le', 'bgr48le': 'bgr48le', 'rgb48le': 'rgb48le'}          # the frame in front of the step, for the pixFmt asked for


def _lutStep(steps, planar, bitDepth=None):
    """dict(table, vertices, strength, order) of the step list's 'lut' step, or None where it has none.  The step is the last compute step of a chain whose frames
    are interleaved RGB samples: an RGB source (files, arrays, bgr24 / bgr48le frames) or a planar source whose output step names an RGB 'pixFmt'.  'file': a .cube
    file (lut3d.parseCube); or 'table': float32 (3, d, d, d) with 'vertices': float32 (3, d), lut3d.uniform(d) by default; 'strength': the blend with the frame in
    front of the step, 1 by default.  The samples' order is the pixFmt's on a planar chain, 'bgr' behind another buffer source and 'rgb' behind a file or an array;
    'order' on the step overrides the latter two.  ValueError naming the key, before any model is loaded: a 'lut' step that is not the last compute step, two of them,
    both or neither of 'file' / 'table', 'vertices' without 'table', a planar Y'CbCr sink, a strength that is not finite, and what lut3d.parseCube / lut3d.check
    refuse of the table."""
    import numpy as np
    for t in steps:          # (before anything else: the key that is not in this change is named as such wherever it stands)
        if t.get('op') == 'dehaze' and t.get('model') in _ailut.NOT_HERE:
            raise NotImplementedError("dehaze: 'model': '{}': {}".format(t['model'], _ailut.NOT_HERE[t['model']]))
    luts = [s for s in steps if s.get('op') == 'lut' or _isAilut(s)]
    if not luts:
        return None
    if len(luts) > 1:
        if any(_isAilut(t) for t in luts):
            raise ValueError("dehaze: 'model': '{}' writes the chain's one colour table: no 'lut' step and no second 'AiLUT_*' step beside it (the chain has {})".format(
                [t for t in luts if _isAilut(t)][0]['model'], len(luts)))
        raise ValueError("lut: a chain holds one 'lut' step at most, this one has {}".format(len(luts)))
    s = luts[0]
    if _isAilut(s):
        return _ailutStep(steps, s, planar, bitDepth)
    work = [t for t in steps if t.get('op') not in ('file', 'buffer', 'output')]
    if s is not work[-1]:
        raise ValueError("lut: the 'lut' step must be the last compute step of the chain: it writes the frame's samples")
    if 'vertices' in s and 'table' not in s:
        raise ValueError("lut: 'vertices' needs 'table' beside it (a 'file' brings its own uniform vertices)")
    if ('file' in s) == ('table' in s):
        raise ValueError("lut: exactly one of 'file' and 'table' names the table, the step has {}".format('both' if 'file' in s else 'neither'))
    try:
        strength = float(s.get('strength', 1.0))
    except (TypeError, ValueError):
        raise ValueError("lut: 'strength' {!r} is not a number".format(s.get('strength')))
    if not math.isfinite(strength):
        raise ValueError("lut: 'strength' {!r} is not finite".format(s['strength']))
    if planar:
        if planar[1] not in pixfmt.RGB_FORMATS:
            raise ValueError("lut: a planar Y'CbCr sink ('pixFmt': '{}') behind a 'lut' step is not in this change: the step writes interleaved RGB samples "
                             "(output 'pixFmt': {})".format(planar[1], ', '.join(pixfmt.RGB_FORMATS)))
        if 'order' in s:
            raise ValueError("lut: 'order' does not apply to a chain on planar frames: the output step's 'pixFmt' carries it")
        order = pixfmt.RGB_FORMATS[planar[1]][1]
    else:
        for o in steps:
            if o.get('op') == 'output' and o.get('pixFmt') is not None:
                raise ValueError("lut: a planar Y'CbCr sink ('pixFmt': '{}') behind a 'lut' step is not in this change: the step writes interleaved RGB samples".format(o['pixFmt']))
        order = s.get('order', 'bgr' if steps[0].get('op') == 'buffer' else 'rgb')
        if order not in _lut3d.ORDERS:
            raise ValueError("lut: 'order' {!r} is not supported ({})".format(order, ', '.join(_lut3d.ORDERS)))
        if bitDepth not in (8, 16):
            raise ValueError("lut: the step writes 8- or 16-bit samples, the chain's bitDepth is {!r}".format(bitDepth))
    if 'file' in s:
        with open(s['file'], 'r') as f:
            table, vertices = _lut3d.parseCube(f.read())
    else:
        table = np.asarray(s['table'], np.float32)
        vertices = np.asarray(s['vertices'], np.float32) if s.get('vertices') is not None else (_lut3d.uniform(table.shape[1]) if table.ndim == 4 else None)
        table, vertices = _lut3d.check(table, vertices)
    return dict(table=table, vertices=vertices, strength=strength, order=order, op='lut', edge='+lut')


def _isAilut(s):
    return s.get('op') == 'dehaze' and s.get('model') in _ailut.MODELS


def _ailutStep(steps, s, planar, bitDepth):
    """_lutStep's dict for {'op': 'dehaze', 'model': 'AiLUT_sRGB_3' | 'AiLUT_XYZ_3', 'strength': s} (the reference's own spelling: python/dehaze.py:27-28,33-41): the
    step goes where a 'lut' step goes and the chain is built as one, but the table is written per frame by the generator net (ailut.generate is the definition;
    DESIGN.md section 23).  The checkpoint is read from config.modelRoot at the reference's path (ailut.MODELS) -- a file that is not there is the error every family
    raises -- and checked by ailut.loadParams.  'tableOut': a callable handed every frame's (table, vertices).  ValueError naming the key, before any model is
    loaded: the step anywhere but last, a planar Y'CbCr sink behind it, a strength that is not finite."""
    import os
    from .weights import load_state_dict_file
    key = "dehaze: 'model': '{}'".format(s['model'])
    work = [t for t in steps if t.get('op') not in ('file', 'buffer', 'output')]
    if s is not work[-1]:
        raise ValueError("{} must be the last compute step of the chain: it writes the frame's samples".format(key))
    try:
        strength = float(s.get('strength', 1.0))
    except (TypeError, ValueError):
        raise ValueError("{}: 'strength' {!r} is not a number".format(key, s.get('strength')))
    if not math.isfinite(strength):
        raise ValueError("{}: 'strength' {!r} is not finite".format(key, s['strength']))
    if planar:
        if planar[1] not in pixfmt.RGB_FORMATS:
            raise ValueError("{}: a planar Y'CbCr sink ('pixFmt': '{}') behind the step is not in this change: the step writes interleaved RGB samples "
                             "(output 'pixFmt': {})".format(key, planar[1], ', '.join(pixfmt.RGB_FORMATS)))
        if 'order' in s:
            raise ValueError("{}: 'order' does not apply to a chain on planar frames: the output step's 'pixFmt' carries it".format(key))
        order = pixfmt.RGB_FORMATS[planar[1]][1]
    else:
        for o in steps:
            if o.get('op') == 'output' and o.get('pixFmt') is not None:
                raise ValueError("{}: a planar Y'CbCr sink ('pixFmt': '{}') behind the step is not in this change: the step writes interleaved RGB samples".format(key, o['pixFmt']))
        order = s.get('order', 'bgr' if steps[0].get('op') == 'buffer' else 'rgb')
        if order not in _lut3d.ORDERS:
            raise ValueError("{}: 'order' {!r} is not supported ({})".format(key, order, ', '.join(_lut3d.ORDERS)))
        if bitDepth not in (8, 16):
            raise ValueError("{}: the step writes 8- or 16-bit samples, the chain's bitDepth is {!r}".format(key, bitDepth))
    if s.get('tableOut') is not None and not callable(s['tableOut']):
        raise ValueError("{}: 'tableOut' is a callable taking (table, vertices)".format(key))
    params = _ailut.loadParams(load_state_dict_file(os.path.join(config.modelRoot, _ailut.MODELS[s['model']])))
    return dict(params=params, strength=strength, order=order, tableOut=s.get('tableOut'), op='dehaze', edge='+ailut')


def _withoutLut(steps):
    return [s for s in steps if s.get('op') != 'lut' and not _isAilut(s)]


def _lutRunner(lut, srcBits, bits, dither):
    """f(src_dev, out, h, w) of _lutStep's dict: a fixed table (imageProcess.lut3d), or the generator net in front of it (imageProcess.ailut)."""
    if 'params' in lut:
        return ailutSamples(lut['params'], srcBits, bits, lut['order'], lut['strength'], dither, lut['tableOut'])
    return lutSamples(lut['table'], lut['vertices'], srcBits, bits, lut['order'], lut['strength'], dither)


def _lutLast(lut, bitDepth, dither):
    """genProcess' tail behind a 'lut' step: the chain's 16-bit samples on the device (H, W, C), one moe_lut3d_run on the three colour samples at the chain's bitDepth,
    downloaded as toOutput returns its image.  With four planes alpha passes around the step, as RGBFilter passes it around its net: its 16-bit code, or at 8 bits that
    code's high byte (the truncating quantiser's sample)."""
    import numpy as np
    import torch
    run = _lutRunner(lut, 16, bitDepth, dither)

    def f(mid):
        H, W, C = mid.shape
        if C not in (3, 4):
            raise ValueError("lut: the step takes an image of 3 or 4 planes (colour, or colour and alpha), this one has {}".format(C))
        rgb = (mid if C == 3 else mid[:, :, :3]).contiguous()
        out = torch.empty((H, W, 3), dtype=_outStorage(bitDepth)[0], device=mid.device)
        run(_flatBytes(rgb), _flatBytes(out), H, W)
        if C == 4:
            alpha = mid[:, :, 3:]
            if bitDepth == 8:
                alpha = ((alpha.to(torch.int32) & 0xffff) >> 8).to(torch.uint8)
            out = torch.cat([out, alpha], 2)
        a = out.cpu().numpy()
        return a.view(np.uint16) if bitDepth > 8 else a
    return f


GUIDED = 'guided'          # the source step's 'chroma' value that names the luma-guided filter


def _planeChroma(steps):
    """(method, loc) of a luma-only chain -- the source step's 'chroma' is 'nearest', 'bilinear' or 'bicubic': the net runs on Y' alone and Cb / Cr are resampled by
    pixfmt.resampleChroma; or 'guided': by pixfmt.guidedChroma, steered by the Y' the chain has written -- or None for 'chroma': 'net' (the default: Cb / Cr go
    through the net as a second image).  ValueError for an unknown value of either key, 'chromaLoc' beside 'net' (the net path has no siting to choose), a chain
    whose total scale exceeds the filter's 16 and, for 'guided', a chain of total scale 1 and a size on the output step."""
    method, loc = steps[0].get('chroma', 'net'), steps[0].get('chromaLoc')
    if method not in ('net', GUIDED) and method not in pixfmt.CHROMA_METHODS:
        raise ValueError('buffer: chroma "{}" is not supported (net, {}, {})'.format(method, ', '.join(pixfmt.CHROMA_METHODS), GUIDED))
    if loc is not None and loc not in pixfmt.CHROMA_LOCS:
        raise ValueError('buffer: chromaLoc "{}" is not supported ({})'.format(loc, ', '.join(pixfmt.CHROMA_LOCS)))
    if method == 'net':
        if loc is not None:
            raise ValueError("buffer: 'chromaLoc' does not apply to 'chroma': 'net' (the planes go through the net, no filter is sited)")
        return None
    scale = 1
    for s in steps[1:]:
        if s.get('op') == 'SR':
            scale *= int(s.get('scale', 1))
    if scale > 16:
        raise ValueError('buffer: chroma "{}" resamples by 16 at most, the chain scales by {}'.format(method, scale))
    if method == GUIDED:
        if scale == 1:
            raise ValueError('buffer: chroma "guided" needs a chain that enlarges the frame (an SR step): at scale 1 the filter would blur planes that need no resampling')
        for s in steps[1:]:
            if s.get('op') == 'output' and any(k in s for k in FIT_KEYS):
                raise ValueError("buffer: chroma \"guided\" does not go with '{}' on the output step: the fitted Y' does not exist when the chroma planes are "
                                 'written'.format(next(k for k in FIT_KEYS if k in s)))
    return method, loc or 'center'


def _chromaPass(chroma, src, dst, width, height, scale):
    """f(raw, out) that writes the chroma planes of a luma-only chain's frame: moe_chroma_resample, or for 'guided' moe_chroma_guided, which also reads the Y' plane
    the chain has written into `out` -- it runs behind the chain's last edge, on the same stream."""
    method, loc = chroma
    return guidedChroma(src, dst, width, height, scale, loc) if method == GUIDED else resampleChroma(src, dst, width, height, scale, method, loc)


def _planeChain(steps, fuse, rsteps=None):
    """The compute steps of a planar chain -> (funcs, nodes, scale, last): funcs map a (C, H, W) image to the next; with fuse, a last step whose final fold can write
    the samples itself (an SR without ensemble, a DN of strength 1) is left out of funcs and returned as last = (Option, its prepare).  rsteps: a list that receives
    the reuse form of every entry of funcs (_ReuseState)."""
    rsteps = [] if rsteps is None else rsteps
    work = [s for s in steps if s['op'] not in ('file', 'buffer', 'output')]
    for opt in work:
        if opt['op'] not in stepOpts:
            raise NotImplementedError('op "{}" is not part of the SR/DN hot path this engine implements'.format(opt['op']))
    funcs, nodes, scale, last = [], [], 1, None
    for k, opt in enumerate(work):
        op, so = opt['op'], stepOpts[opt['op']]
        convertValues(int, opt, so.get('toInt', []))
        convertValues(float, opt, so.get('toFloat', []))
        o = so['getOpt'].getOpt(opt)
        if o is None:
            raise ValueError('unknown model for step {}'.format(opt))
        opt['opt'] = o
        final = fuse and k == len(work) - 1
        if op == 'SR':
            if not opt['scale'] > 1:
                raise TypeError('Invalid scale setting for SR.')
            if final and o.ensemble == 0:
                last = (o, identity)
            else:
                funcs.append(runSR.sr(o))
                rsteps.append(_reuseSR(o, funcs[-1]))
            scale *= opt['scale']
        elif final and o.strength == 1:
            last = (o, o.prepare)
        else:
            funcs.append(RGBFilter(o))
            rsteps.append(_reuseDN(o))
        nodes.append(dict(op=op, model=opt.get('model'), scale=opt.get('scale', 1)))
    return funcs, nodes, scale, last


def _genProcessPlanes(steps, fmts, dither=None, lut=None):
    import numpy as np
    import torch
    src, dst = fmts
    rgb, converters = _planeRGBStep(steps, dst), {}
    if rgb:          # the chain's frame as yuv420p16le without 'dither', then one moe_planes_to_rgb: the key governs that conversion's rounding
        dst, dither, rgbDither = PLANAR16, None, dither
    if lut:          # a 'lut' step: the RGB frame at 16 bits without 'dither', then one moe_lut3d_run at the pixFmt's depth: the key governs the step's quantiser
        lutBits = pixfmt.RGB_FORMATS[rgb[0]][0]
        lutRun = _lutRunner(lut, 16, lutBits, rgbDither)
        rgb, rgbDither = (LUT_FMT16[rgb[0]],) + tuple(rgb[1:]), None
    funcs, nodes, scale, _ = _planeChain(steps, False)
    if lut:
        nodes.append(dict(op=lut['op']))
    quantise = toPlanes(pixfmt.FORMATS[dst], dither)
    chroma, resamplers = _planeChroma(steps), {}
    fit, quantise16, fitters = _planeFit(steps), toPlanes(16), {}

    def finish(out, W, H):
        """The bytes of the frame of W x H in `out`: the planar frame itself, or its RGB form."""
        if rgb:
            if (W, H) not in converters:
                converters[(W, H)] = planesToRGB(dst, W, H, *rgb, dither=rgbDither)
            out = converters[(W, H)](out, torch.empty((3 * W * H * (pixfmt.RGB_FORMATS[rgb[0]][0] // 8),), dtype=torch.uint8, device=out.device))
        if lut:
            out = lutRun(out, torch.empty((3 * W * H * (lutBits // 8),), dtype=torch.uint8, device=out.device), H, W)
        return out.cpu().numpy().tobytes()

    def runFit(rawDev, y, c, width, height, dev):
        """The frame at the size the output step names: the chain's planes at 16 bits (the existing edge), then pixfmt.fitPlanes' kernel per image."""
        W, H, method = fit
        _planeFit(steps, width, height)          # (the ratios, now that the source's size is known)
        w, h = width * scale, height * scale
        Ds, Dd = pixfmt.FORMATS[src], pixfmt.FORMATS[dst]
        if (width, height) not in fitters:
            fitters[(width, height)] = (fitPlanes(16, Dd, 1, h, w, H, W, method),
                                        fitPlanes(Ds, Dd, 2, height // 2, width // 2, H // 2, W // 2, *chroma) if chroma
                                        else fitPlanes(16, Dd, 2, h // 2, w // 2, H // 2, W // 2, method))
        fitY, fitC = fitters[(width, height)]
        cb = pixfmt.planeOffsets(dst, W, H)[1]
        out = torch.empty((pixfmt.frameBytes(dst, W, H),), dtype=torch.uint8, device=dev)
        fitY(quantise16(reduce(apply, funcs, y)), out[:cb])
        if chroma:
            fitC(rawDev[pixfmt.planeOffsets(src, width, height)[1]:], out[cb:])
        else:
            fitC(quantise16(reduce(apply, funcs, c)), out[cb:])
        return finish(out, W, H)

    def run(frame):
        raw, height, width = frame
        pixfmt.planeShapes(src, width, height)
        if len(raw) != pixfmt.frameBytes(src, width, height):
            raise ValueError('short frame: {} of {} bytes'.format(len(raw), pixfmt.frameBytes(src, width, height)))
        dev = torch.device(config.device())
        rawDev = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(dev)
        y, c = fromPlanes(src, width, height, config.dtype())(rawDev)
        if fit:
            return runFit(rawDev, y, c, width, height, dev)
        w, h = width * scale, height * scale
        cb = pixfmt.planeOffsets(dst, w, h)[1]
        out = torch.empty((pixfmt.frameBytes(dst, w, h),), dtype=torch.uint8, device=dev)
        quantise(reduce(apply, funcs, y), out[:cb])
        if chroma:          # luma-only: Cb / Cr from the raw frame's codes, by the integer filter ('guided': and from the Y' plane just written)
            if (width, height) not in resamplers:
                resamplers[(width, height)] = _chromaPass(chroma, src, dst, width, height, scale)
            resamplers[(width, height)](rawDev, out)
        else:
            quantise(reduce(apply, funcs, c), out[cb:])
        return finish(out, w, h)
    return (lambda frame: [] if not frame[0] else [run(frame)]), nodes


class Context(object):
    imageMode = 'RGB'
    palette = None


def genProcess(steps, bitDepth=8, outFile=None):
    steps = [dict(s) for s in steps]
    planar = _planeFormats(steps)
    _lumaCheck(steps, bool(planar))
    dither = _outputDither(steps)          # (before any model is loaded)
    if planar:          # the decoder's own Y'CbCr 4:2:0 planes in, planar frames out
        return _genProcessPlanes(_withoutLut(steps), planar, dither, _lutStep(steps, planar))
    _refuseFit(steps)
    lut = _lutStep(steps, None, int(steps[0].get('bitDepth', 16)) if steps and steps[0].get('op') == 'buffer' else bitDepth)          # (likewise)
    steps = _withoutLut(steps)
    ctx = Context()
    funcs, nodes = [], []
    has_file = bool(steps) and steps[0]['op'] == 'file'
    has_buffer = bool(steps) and steps[0]['op'] == 'buffer'
    yuv = _outputFormat(steps)
    if yuv and not has_buffer:
        raise ValueError("output pixFmt '{}' needs a 'buffer' source (raw video frames); image files are written as RGB".format(yuv[0]))
    if has_file:
        funcs.append(readFile(context=ctx))
    if has_buffer:     # video frames: raw bgr24 / bgr48le in, the same out (channel order is irrelevant: planes are independent)
        bitDepth = int(steps[0].get('bitDepth', 16))
    fit = _pixelFit(steps, bitDepth)          # (before any model is loaded)
    if has_buffer:
        funcs.append(toNumPy(bitDepth))
    funcs.append(toTorch(bitDepth, config.dtype(), config.device()))
    work, fused = [s for s in steps if s['op'] not in ('file', 'buffer', 'output') and s is not fit], None
    for opt in steps:
        op = opt['op']
        if op in ('file', 'buffer', 'output') or opt is fit:
            continue
        if op not in stepOpts:
            raise NotImplementedError('op "{}" is not part of the SR/DN hot path this engine implements'.format(op))
        so = stepOpts[op]
        convertValues(int, opt, so.get('toInt', []))
        convertValues(float, opt, so.get('toFloat', []))
        if op == 'resize':      # procResize (python/procedure.py:104-107)
            funcs.append(resize(opt, dict(source=has_buffer)))
            nodes.append(dict(op='resize', mode=opt['method']))
            continue
        o = so['getOpt'].getOpt(opt)
        if o is None:
            raise ValueError('unknown model for step {}'.format(opt))
        opt['opt'] = o
        if op == 'SR' and not opt['scale'] > 1:
            raise TypeError('Invalid scale setting for SR.')
        if _isLuma(o):          # a luma-only step; the last one's fold writes the samples itself where it can (an SR without ensemble, a DN of strength 1)
            f = _lumaStep(op, o)[0]
            if opt is work[-1] and not yuv and bitDepth in (8, 16) and (o.ensemble == 0 if op == 'SR' else o.strength == 1):
                fused = _lumaLastOnDevice(op, o, f) if fit or lut else _lumaLast(op, o, f, bitDepth, dither)
            else:
                funcs.append(f)
        elif op == 'SR':
            funcs.append(runSR.sr(o))
        else:
            funcs.append(RGBFilter(o))
        nodes.append(dict(op=op, model=opt.get('model'), scale=opt.get('scale', 1)))
    if yuv:          # the encoder's planes from the canvas, then bytes
        funcs += [toYuv(*yuv, dither=dither), lambda t: t.cpu().numpy().tobytes()]
        run = lambda im: reduce(apply, funcs, im)
        return (lambda frame: [] if not frame[0] else [run(frame)]), nodes
    if fit:
        funcs.append(_pixelFitLast(fit, fused, 16, False) if lut else _pixelFitLast(fit, fused, bitDepth))
        nodes.append(dict(op='resize', mode=fit['fit']))
    elif lut:
        funcs.append(fused or _samplesOnDevice(16))
    else:
        funcs += [fused] if fused else [toFloat, toOutput(bitDepth, dither)]
    if lut:          # the frame above at 16 bits, on the device; one moe_lut3d_run writes the samples handed out
        funcs.append(_lutLast(lut, bitDepth, dither))
        nodes.append(dict(op=lut['op']))
    if has_file and outFile is not None:
        funcs.append(lambda im: writeFile(im, outFile, ctx))
    if has_buffer:
        funcs.append(toBuffer(bitDepth))
        run = lambda im: reduce(apply, funcs, im)
        return (lambda frame: [] if not frame[0] else [run(frame)]), nodes     # a list of buffers per frame (procedure.py:122-125)
    return (lambda im: reduce(apply, funcs, im)), nodes


def runFrames(process, read, write, width, height, bitDepth=16, start=0, stop=-1, frameBytes=None):
    """The per-frame loop of SR_vid (python/video.py:349-360) without the ffmpeg plumbing: `read(nbytes)` yields raw frames of
    width*height*3 samples (or of frameBytes bytes: a planar source, pixfmt.frameBytes), every frame from `start` on goes through `process` (a genProcess 'buffer'
    pipeline) and each returned buffer is handed to `write`.  Returns the number of frames written."""
    if frameBytes is None:
        frameBytes = width * height * 3 * (1 if bitDepth <= 8 else 2)
    i = n = 0
    while stop < 0 or i <= stop:
        raw = read(frameBytes)
        if len(raw) == 0:
            break
        if len(raw) != frameBytes:
            raise ValueError('short frame: {} of {} bytes'.format(len(raw), frameBytes))
        if i >= start:
            for buf in process((raw, height, width)):
                if buf:
                    write(buf)
                    n += 1
        i += 1
    return n


# ---- streamed frames: a ring of `depth` frames in flight ---------------------------------------------------------------------------------
# runFrames above is serial per frame: a blocking pageable upload, the chain, stitch -> fp32 copy -> quantise, a blocking pageable download.  The stream keeps `depth`
# slots (pinned input, device raw frame, device output, pinned output, three events -- all allocated once) and three queues: frame k's upload, compute and download are
# enqueued in push(k), each waiting on the DEVICE for the events of what it depends on; the host then waits for the download of frame k - depth + 1 only.
#
# FrameStream is the ordering logic alone (which slot, which event is waited on before which stage, what push / flush return); it drives a backend object
#     event() -> e          upload(slot, raw, wait, record)          compute(slot, wait, record)          download(slot, wait, record)
#     wait(slot, e) -> bytes of the slot's finished frame            abort()   close()
# where a stage first makes its queue wait for every event of `wait`, enqueues its work, then records `record` behind it.  _DeviceBackend is the one on the GPU.
def _checkRing(depth, bitDepth):
    if not isinstance(depth, int) or isinstance(depth, bool) or not 1 <= depth <= 4:
        raise ValueError('frame stream: depth must be 1..4, got {!r}'.format(depth))
    if bitDepth not in (8, 16):
        raise ValueError('frame stream: bitDepth must be 8 or 16, got {!r}'.format(bitDepth))


# ---- reuse between frames ------------------------------------------------------------------------------------------------
# With reuse the backend keeps the previous raw frame on the device; the upload stage compares the new one against it (moe_changed_blocks, which also retains it) and
# sends the cell map(s) to pinned memory in front of the `uploaded` event; the compute stage waits for that event on the host, then walks the chain with the rules of
# moephoto_amd/reuse.py: every tiled step runs the tiles whose support touches a changed cell into the pool it kept from the previous frame (moe_run_plan_subset) and
# folds the whole pool as always.  A step is described to the walk as (kind, f, ..): 'tiles' -- f(x, reuse) takes _runPlan's reuse callback; 'resize' -- f(x) with the
# step's dict behind it; 'opaque' -- f(x), no rule: it runs as it is and its output counts as wholly changed.
def _reuseSR(o, f):
    return ('tiles', lambda x, reuse, o=o: doCrop(o, x, reuse=reuse)) if o.ensemble == 0 else ('opaque', f)


def _reuseDN(o):
    return ('tiles', lambda x, reuse, o=o: _RGBFilter(o, x, reuse))


def _checkReuse(reuse):
    if not isinstance(reuse, bool):
        raise ValueError('frame stream: reuse must be True or False, got {!r}'.format(reuse))


def _checkViews(views):
    if not isinstance(views, bool):
        raise ValueError('frame stream: views must be True or False, got {!r}'.format(views))


class _ReuseState(object):
    """What a reuse stream owns besides its slots: the tracker (which plan each step ran with), one pool per step and image, the counters (`stream.reuse`):
    tiles[(step, image)] = [planned, run] over the stream, frames = the same per frame for the last 256 frames, pixels_planned / pixels_run = input pixels of the
    planes of those tiles."""

    def __init__(self, steps, tiledEdge):
        from collections import deque
        self.steps, self.tiledEdge = list(steps), tiledEdge
        self.tracker, self.pools = _reuse.Tracker(), {}
        self.stats = dict(frames=deque(maxlen=256), tiles={}, pixels_planned=0, pixels_run=0)
        self.n = 0

    def begin(self):
        self.frame = {}
        self.stats['frames'].append(self.frame)
        self.n += 1
        return self.n == 1          # the first frame: there is no frame before it, whatever the map says

    def callback(self, key, changed):
        """_runPlan's reuse callback for one step of one image; its .out is the region of the step's output once it has been called."""
        import torch

        def cb(plan, C):
            mask, cb.out = self.tracker.step(key, plan, changed)
            n, ent = plan.pool_elems(C), self.pools.get(key)
            if ent is None or ent[0] is not plan or ent[1].numel() != n:          # no results of the previous frame under this plan: everything runs
                ent = self.pools[key] = (plan, torch.empty((n,), dtype=torch.float32, device=torch.device(config.device())))
                mask[:] = 1
                cb.out = None
            px = self.tracker.regions(plan).pixels
            planned, run = len(mask), int(mask.sum())
            self.frame[key] = (planned, run)
            tot = self.stats['tiles'].setdefault(key, [0, 0])
            tot[0] += planned
            tot[1] += run
            self.stats['pixels_planned'] += C * sum(px)
            self.stats['pixels_run'] += C * sum(p for p, m in zip(px, mask) if m)
            return mask, ent[1]
        cb.out = None
        return cb

    def walk(self, image, x, changed):
        """The chain's steps in front of the edge on one image: -> (the edge's input, its region; None = all of it)."""
        for i, step in enumerate(self.steps):
            kind, f = step[0], step[1]
            if kind == 'tiles':
                cb = self.callback((i, image), changed)
                x, changed = f(x, cb), cb.out
            elif kind == 'luma':          # a luma-only step (_lumaStep): the tiles' rule on Y and the resize rule on the chroma planes, joined by the step itself
                x, changed = f(x, self.callback((i, image), changed), changed)
            elif kind == 'resize':
                y = f(x)
                changed = _reuse.resizeRegion(changed, tuple(x.shape[-2:]), tuple(y.shape[-2:]), step[2]['method']) if changed is not None else None
                x = y
            else:
                x, changed = f(x), None
        return x, changed

    def edgeCallback(self, image, changed):
        return self.callback((len(self.steps), image), changed) if self.tiledEdge else None

    def close(self):
        self.pools.clear()


class FrameStream(object):
    def __init__(self, backend, width, height, bitDepth, depth=2, nodes=(), frameBytes=None):
        _checkRing(depth, bitDepth)
        self.backend, self.depth, self.nodes = backend, depth, list(nodes)
        self.width, self.height, self.bitDepth = int(width), int(height), bitDepth
        if frameBytes is not None and (not isinstance(frameBytes, int) or isinstance(frameBytes, bool) or frameBytes < 1):
            raise ValueError('frame stream: frameBytes must be a positive int, got {!r}'.format(frameBytes))
        # (frameBytes: a source that is not width x height x 3 interleaved samples -- a planar 4:2:0 frame)
        self.frameBytes = frameBytes if frameBytes is not None else self.width * self.height * 3 * (1 if bitDepth <= 8 else 2)
        self.events = [dict(uploaded=backend.event(), computed=backend.event(), downloaded=backend.event()) for _ in range(depth)]
        self.pushed = self.returned = 0       # frames enqueued / handed back; frame k lives in slot k % depth
        self.closed = self._released = False

    def _guard(self, f):
        if self.closed:
            raise RuntimeError('frame stream is closed')
        try:
            return f()
        except BaseException:          # nothing is retried: one device synchronise, the stream is dead, the caller sees the error
            self.closed = True
            self.backend.abort()
            raise

    def _collect(self):
        """The oldest frame in flight.  Its download event was recorded by an earlier push on this thread, so the host wait cannot hang; once it has passed, every stage
        of that frame and of the frames before it is over -- the next push may overwrite the slot's pinned input and the caller owns a copy of its pinned output."""
        slot = self.returned % self.depth
        buf = self.backend.wait(slot, self.events[slot]['downloaded'])
        self.returned += 1
        return buf

    def push(self, raw):
        """Enqueue one raw frame; returns the frames that are finished, in input order: none while fewer than `depth` are in flight, then one per push."""
        if self.closed:
            raise RuntimeError('frame stream is closed')
        if not raw:
            return []
        if len(raw) != self.frameBytes:
            raise ValueError('short frame: {} of {} bytes'.format(len(raw), self.frameBytes))

        def f():
            slot = self.pushed % self.depth
            ev, again = self.events[slot], self.pushed >= self.depth
            b = self.backend
            # upload: the slot's raw frame was read by the compute of frame k - depth
            b.upload(slot, raw, [ev['computed']] if again else [], ev['uploaded'])
            # compute: needs this frame's upload, and overwrites the output buffer the download of frame k - depth read
            b.compute(slot, [ev['uploaded']] + ([ev['downloaded']] if again else []), ev['computed'])
            b.download(slot, [ev['computed']], ev['downloaded'])
            self.pushed += 1
            return [self._collect()] if self.pushed - self.returned >= self.depth else []
        return self._guard(f)

    def flush(self):
        """Every frame still in flight, in input order."""
        return self._guard(lambda: [self._collect() for _ in range(self.pushed - self.returned)])

    def close(self):
        """Frames still in flight are dropped.  Also after a failed stage: the backend lets go of its slots exactly once."""
        self.closed = True
        if not self._released:
            self._released = True
            self.backend.close()


class _DeviceBackend(object):
    """The stages on the GPU: upload = host memcpy into the slot's pinned buffer + async H2D on its own stream; compute = moe_to_float, the chain's steps and the output
    edge on torch's current stream; download = async D2H into the slot's pinned buffer on a third stream.  timing: the events take timestamps and `stats` sums the
    milliseconds per stage over the collected frames (tools/frame_stream_bench.py)."""

    def __init__(self, funcs, edge, bitDepth, width, height, outHW, depth, timing=False, outBytes=None, reuse=None, views=False, fit=None):
        import torch
        self.torch, self.funcs, self.edge, self.bitDepth, self.timing, self.reuse, self.views = torch, funcs, edge, bitDepth, timing, reuse, views
        self.fit = fit          # ((h, w), imageProcess.fitPixels' f) behind a 'fit' resize step: the edge writes a slot's `mid` (16-bit samples of h x w), f the slot's `out`
        self.dev = torch.device(config.device())
        if self.dev.type != 'cuda':
            raise _lib.EngineError('frame stream: needs a HIP device (moephoto_amd has no CPU path)')
        self.H, self.W = int(height), int(width)
        out_dt, _, _ = _outStorage(bitDepth)
        self.src_dt = _lib.U8 if bitDepth <= 8 else _lib.U16
        self.up, self.down = torch.cuda.Stream(self.dev), torch.cuda.Stream(self.dev)
        self.slots = []
        oshape, o_dt = ((outHW[0], outHW[1], 3), out_dt) if outBytes is None else ((int(outBytes),), torch.uint8)      # (outBytes: a planar frame, flat)
        for _ in range(depth):
            s = self._slot(out_dt)
            s.update(out=torch.empty(oshape, dtype=o_dt, device=self.dev), pin_out=torch.empty(oshape, dtype=o_dt, pin_memory=True))
            if fit is not None:
                s['mid'] = torch.empty((fit[0][0], fit[0][1], 3), dtype=_outStorage(16)[0], device=self.dev)
            s['in_bytes'] = s['pin_in'].numpy().view('uint8').reshape(-1)
            s['out_np'] = s['pin_out'].numpy()
            if views:          # the slot's pinned output as the caller sees it: flat bytes, read-only (the ring writes it through the tensor)
                s['out_view'] = memoryview(s['out_np'].view('uint8').reshape(-1)).toreadonly()
            if timing:
                s.update(t_up=self.event(), t_comp=self.event(), t_down=self.event())
            self.slots.append(s)
        self.stats = dict(frames=0, memcpy_ms=0.0, h2d_ms=0.0, compute_ms=0.0, d2h_ms=0.0, tobytes_ms=0.0)
        if reuse is not None:          # the retained raw frame, the change map(s) on the device and one pinned copy per slot
            self.prev = torch.empty_like(self.slots[0]['raw'])
            self.maps = self._maps()
            self.map_dev = torch.empty((sum(a * b for a, b in self.maps),), dtype=torch.uint8, device=self.dev)
            for s in self.slots:
                s['pin_map'] = torch.empty((self.map_dev.numel(),), dtype=torch.uint8, pin_memory=True)
                s['map_np'] = s['pin_map'].numpy()

    def _maps(self):
        """The cell grids of the images the chain starts from, in the order of the map buffer."""
        return [_reuse.cells(self.H, self.W)]

    def _detect(self, s, stream):
        """moe_changed_blocks on the slot's raw frame against the retained one: an interleaved frame is one matrix, a cell 16 pixels of 3 samples wide."""
        es = 1 if self.bitDepth <= 8 else 2
        _lib.check(_lib.lib().moe_changed_blocks(s['raw'].data_ptr(), self.prev.data_ptr(), 1, self.H, self.W * 3 * es, _reuse.CELL, _reuse.CELL * 3 * es,
                                                 self.map_dev.data_ptr(), self.dev.index or 0, stream.cuda_stream))

    def _changed(self, s, first):
        """The regions of the chain's input images for the slot's frame, from its pinned map (None: the first frame)."""
        out, at = [], 0
        for a, b in self.maps:
            out.append(None if first else s['map_np'][at:at + a * b].reshape(a, b) != 0)
            at += a * b
        return out

    def _slot(self, in_dt):
        """A slot's input side: the pinned and the device copy of the raw frame, and the image(s) the chain starts from."""
        torch = self.torch
        return dict(pin_in=torch.empty((self.H, self.W, 3), dtype=in_dt, pin_memory=True), raw=torch.empty((self.H, self.W, 3), dtype=in_dt, device=self.dev),
                    x=torch.empty((3, self.H, self.W), dtype=config.dtype(), device=self.dev))

    def event(self):
        return self.torch.cuda.Event(enable_timing=self.timing)

    def _stage(self, stream, s, name, wait, record, work):
        for e in wait:
            stream.wait_event(e)
        if self.timing:
            s['t_' + name].record(stream)
            s['e_' + name] = record
        work(stream)
        record.record(stream)

    def upload(self, slot, raw, wait, record):
        import numpy as np
        s = self.slots[slot]
        t0 = time.perf_counter()
        s['in_bytes'][:] = np.frombuffer(raw, np.uint8)
        self.stats['memcpy_ms'] += (time.perf_counter() - t0) * 1e3

        def work(stream):
            with self.torch.cuda.stream(stream):
                s['raw'].copy_(s['pin_in'], non_blocking=True)
                if self.reuse is not None:          # right behind the copy, in front of the `uploaded` event: the map is on the host once that event has passed
                    self._detect(s, stream)
                    s['pin_map'].copy_(self.map_dev, non_blocking=True)
        if self.reuse is not None:
            s['uploaded'] = record
        self._stage(self.up, s, 'up', wait, record, work)

    def _regions(self, s):
        """The compute stage's first act with reuse: wait on the host for the frame's own `uploaded` event -- recorded by an earlier statement of this thread, so the
        wait cannot hang -- and read the regions the chain starts from."""
        s['uploaded'].synchronize()
        return self._changed(s, self.reuse.begin())

    def compute(self, slot, wait, record):
        s = self.slots[slot]
        R = self.reuse
        changed = self._regions(s)[0] if R is not None else None

        def work(stream):
            _lib.check(_lib.lib().moe_to_float(s['raw'].data_ptr(), self.src_dt, self.bitDepth, self.H, self.W, 3, s['x'].data_ptr(), _DT[s['x'].dtype],
                                               self.dev.index or 0, stream.cuda_stream))
            into = s['out'] if self.fit is None else s['mid']
            if R is None:
                self.edge(reduce(apply, self.funcs, s['x']), into)
            else:
                x, region = R.walk('rgb', s['x'], changed)
                if R.tiledEdge:
                    self.edge(x, into, R.edgeCallback('rgb', region))
                else:
                    self.edge(x, into)
            if self.fit is not None:
                self.fit[1](_flatBytes(into), _flatBytes(s['out']))
        self._stage(self.torch.cuda.current_stream(self.dev), s, 'comp', wait, record, work)

    def download(self, slot, wait, record):
        s = self.slots[slot]

        def work(stream):
            with self.torch.cuda.stream(stream):
                s['pin_out'].copy_(s['out'], non_blocking=True)
        self._stage(self.down, s, 'down', wait, record, work)

    def wait(self, slot, event):
        s = self.slots[slot]
        event.synchronize()
        if self.timing:
            for name, key in (('up', 'h2d_ms'), ('comp', 'compute_ms'), ('down', 'd2h_ms')):      # (the download is over, so is everything before it)
                self.stats[key] += s['t_' + name].elapsed_time(s['e_' + name])
        t0 = time.perf_counter()
        buf = s['out_view'] if self.views else s['out_np'].tobytes()          # (a view: valid until the next push / flush / close, see genFrameStream)
        self.stats['tobytes_ms'] += (time.perf_counter() - t0) * 1e3
        self.stats['frames'] += 1
        return buf

    def abort(self):
        self.torch.cuda.synchronize(self.dev)

    def close(self):
        self.torch.cuda.synchronize(self.dev)
        self.slots = []
        if self.reuse is not None:
            self.reuse.close()
            self.prev = self.map_dev = None


class _PlanesBackend(_DeviceBackend):
    """The same three queues for a chain on the decoder's planes: a slot's input is the flat planar frame (pinned and on the device), its images are Y (1, H, W) and
    C (2, H / 2, W / 2), its output the flat planar frame of outBytes.  compute = moe_planes_to_float, the chain on Y and then on C, and edge(y, c, out).
    lumaOnly: the chain runs on Y alone -- no C image is walked and the change map covers Y only; edge(y, raw, out) writes the chroma planes from the raw frame (every
    frame, reuse or not: the output frame is the slot's).  moe_planes_to_float still fills one C image, shared by the slots and read by nobody (it refuses a NULL)."""

    def __init__(self, funcs, edge, fmt, width, height, depth, timing, outBytes, reuse=None, views=False, lumaOnly=False):
        self.convert, self.inBytes, self.lumaOnly = fromPlanes(fmt, width, height, config.dtype()), pixfmt.frameBytes(fmt, width, height), lumaOnly
        self.unusedC = None
        super().__init__(funcs, edge, 8 if pixfmt.FORMATS[fmt] == 8 else 16, width, height, None, depth, timing, outBytes, reuse, views)

    def _maps(self):
        return [_reuse.cells(self.H, self.W)] + ([] if self.lumaOnly else [_reuse.cells(self.H // 2, self.W // 2)])

    def _detect(self, s, stream):
        """The Y plane is one matrix, Cb and Cr are two matrices folded into one map: a cell is 16 x 16 pixels of the image the chain sees."""
        es = 1 if self.bitDepth <= 8 else 2
        L, raw, prev, m, ny = _lib.lib(), s['raw'].data_ptr(), self.prev.data_ptr(), self.map_dev.data_ptr(), self.H * self.W * es
        _lib.check(L.moe_changed_blocks(raw, prev, 1, self.H, self.W * es, _reuse.CELL, _reuse.CELL * es, m, self.dev.index or 0, stream.cuda_stream))
        if self.lumaOnly:
            return
        _lib.check(L.moe_changed_blocks(raw + ny, prev + ny, 2, self.H // 2, self.W // 2 * es, _reuse.CELL, _reuse.CELL * es, m + self.maps[0][0] * self.maps[0][1],
                                        self.dev.index or 0, stream.cuda_stream))

    def _slot(self, in_dt):
        torch = self.torch
        if self.lumaOnly and self.unusedC is None:
            self.unusedC = torch.empty((2, self.H // 2, self.W // 2), dtype=config.dtype(), device=self.dev)
        return dict(pin_in=torch.empty((self.inBytes,), dtype=torch.uint8, pin_memory=True), raw=torch.empty((self.inBytes,), dtype=torch.uint8, device=self.dev),
                    y=torch.empty((1, self.H, self.W), dtype=config.dtype(), device=self.dev),
                    c=self.unusedC if self.lumaOnly else torch.empty((2, self.H // 2, self.W // 2), dtype=config.dtype(), device=self.dev))

    def compute(self, slot, wait, record):
        s = self.slots[slot]

        R = self.reuse
        changed = self._regions(s) if R is not None else None

        def work(stream):
            y, c = self.convert(s['raw'], s['y'], s['c'])
            if self.lumaOnly:
                if R is None:
                    self.edge(reduce(apply, self.funcs, y), s['raw'], s['out'])
                    return
                y, ry = R.walk('y', y, changed[0])
                self.edge(y, s['raw'], s['out'], R.edgeCallback('y', ry))
                return
            if R is None:
                self.edge(reduce(apply, self.funcs, y), reduce(apply, self.funcs, c), s['out'])
                return
            (y, ry), (c, rc) = R.walk('y', y, changed[0]), R.walk('c', c, changed[1])
            if R.tiledEdge:
                self.edge(y, c, s['out'], R.edgeCallback('y', ry), R.edgeCallback('c', rc))
            else:
                self.edge(y, c, s['out'])
        self._stage(self.torch.cuda.current_stream(self.dev), s, 'comp', wait, record, work)


def _genFrameStreamPlanes(steps, fmts, width, height, depth, timing, reuse=False, views=False, dither=None, lut=None):
    src, dst = fmts
    rgb = _planeRGBStep(steps, dst)
    if rgb:          # the chain's frame as yuv420p16le without 'dither', then one moe_planes_to_rgb: the key governs that conversion's rounding
        dst, dither, rgbDither = PLANAR16, None, dither
    if lut:          # a 'lut' step: the RGB frame at 16 bits without 'dither', then one moe_lut3d_run at the pixFmt's depth: the key governs the step's quantiser
        lutBits = pixfmt.RGB_FORMATS[rgb[0]][0]
        lutRun = _lutRunner(lut, 16, lutBits, rgbDither)
        rgb, rgbDither = (LUT_FMT16[rgb[0]],) + tuple(rgb[1:]), None
    bitDepth = 8 if pixfmt.FORMATS[src] == 8 else 16
    _checkRing(depth, bitDepth)          # (before any model is loaded)
    _checkReuse(reuse)
    _checkViews(views)
    chroma = _planeChroma(steps)
    rsteps = []
    funcs, nodes, scale, last = _planeChain(steps, True, rsteps)
    w, h = int(width) * scale, int(height) * scale
    D, cb = pixfmt.FORMATS[dst], pixfmt.planeOffsets(dst, w, h)[1]
    if last:          # the last step's two folds write straight into the slot's frame, at the Y and at the Cb offset: no canvas exists
        o, prepare = last
        into, edgeName = (lambda x, out, reuse=None: doCropPlanes(o, prepare(x), D, out, reuse=reuse, dither=dither)), 'crop'
    else:
        quantise = toPlanes(D, dither)
        into, edgeName = (lambda x, out, reuse=None: quantise(x, out)), 'quantise'

    def edge(y, c, out, reuseY=None, reuseC=None):
        into(y, out[:cb], reuseY)
        into(c, out[cb:], reuseC)
    if chroma:          # luma-only: the Y edge as above, then one moe_chroma_resample (moe_chroma_guided) from the raw frame's chroma codes into the frame's Cb / Cr planes, on the compute stream
        resample = _chromaPass(chroma, src, dst, int(width), int(height), scale)

        def edge(y, raw, out, reuseY=None):
            into(y, out[:cb], reuseY)
            resample(raw, out)
    outBytes = pixfmt.frameBytes(dst, w, h)
    fit = _planeFit(steps, width, height)
    if fit:          # a size on the output step: the edge above runs at 16 bits into one intermediate (compute queue only), then one fitPlanes per image into the slot's frame
        import torch
        W, H, method = fit
        Dd, cb16, cbOut, cbIn = pixfmt.FORMATS[dst], w * h * 2, pixfmt.planeOffsets(dst, W, H)[1], pixfmt.planeOffsets(src, int(width), int(height))[1]
        if last:
            o, prepare = last
            into = lambda x, out, reuse=None: doCropPlanes(o, prepare(x), 16, out, reuse=reuse)
        else:
            quantise16 = toPlanes(16)
            into = lambda x, out, reuse=None: quantise16(x, out)
        edgeName += '+fit'
        outBytes = pixfmt.frameBytes(dst, W, H)
        inter = {}          # the 16-bit planes of the chain's own size: allocated once, at the first frame

        def intermediate(dev):
            if 'buf' not in inter:
                inter['buf'] = torch.empty((cb16 if chroma else pixfmt.frameBytes('yuv420p16le', w, h),), dtype=torch.uint8, device=dev)
            return inter['buf']
        fitY = fitPlanes(16, Dd, 1, h, w, H, W, method)
        if chroma:          # luma-only: one pass from the source's chroma codes to the fitted size; no intermediate, no moe_chroma_resample
            fitC = fitPlanes(pixfmt.FORMATS[src], Dd, 2, int(height) // 2, int(width) // 2, H // 2, W // 2, *chroma)

            def edge(y, raw, out, reuseY=None):
                mid = intermediate(out.device)
                into(y, mid, reuseY)
                fitY(mid, out[:cbOut])
                fitC(raw[cbIn:], out[cbOut:])
        else:
            fitC = fitPlanes(16, Dd, 2, h // 2, w // 2, H // 2, W // 2, method)

            def edge(y, c, out, reuseY=None, reuseC=None):
                mid = intermediate(out.device)
                into(y, mid[:cb16], reuseY)
                into(c, mid[cb16:], reuseC)
                fitY(mid[:cb16], out[:cbOut])
                fitC(mid[cb16:], out[cbOut:])
    if rgb:          # an RGB pixFmt: the edge above writes one intermediate planar frame (compute queue only), then one moe_planes_to_rgb into the slot's frame, every frame
        import torch
        fw, fh = fit[:2] if fit else (w, h)
        toRGB, planarBytes, planarEdge, planar = planesToRGB(dst, fw, fh, *rgb, dither=rgbDither), outBytes, edge, {}
        edgeName += '+rgb'
        outBytes = 3 * fw * fh * (pixfmt.RGB_FORMATS[rgb[0]][0] // 8)

        def edge(y, c, out, *reuses):          # (c: the raw frame on a luma-only chain)
            if 'buf' not in planar:          # allocated once, at the first frame
                planar['buf'] = torch.empty((planarBytes,), dtype=torch.uint8, device=out.device)
            planarEdge(y, c, planar['buf'], *reuses)
            toRGB(planar['buf'], out)
    if lut:          # the RGB edge above writes one intermediate frame at 16 bits (compute queue only), then one moe_lut3d_run into the slot's frame, every frame
        rgbBytes, rgbEdge, mid16 = outBytes, edge, {}
        edgeName += lut['edge']
        outBytes = 3 * fw * fh * (lutBits // 8)
        nodes.append(dict(op=lut['op']))

        def edge(y, c, out, *reuses):
            if 'buf' not in mid16:          # allocated once, at the first frame
                mid16['buf'] = torch.empty((rgbBytes,), dtype=torch.uint8, device=out.device)
            rgbEdge(y, c, mid16['buf'], *reuses)
            lutRun(mid16['buf'], out, fh, fw)
    state = _ReuseState(rsteps, bool(last)) if reuse else None
    backend = _PlanesBackend(funcs, edge, src, width, height, depth, timing, outBytes, state, views, bool(chroma))
    stream = FrameStream(backend, width, height, bitDepth, depth, nodes, frameBytes=pixfmt.frameBytes(src, width, height))
    stream.edge, stream.reuse = edgeName, (state.stats if reuse else None)
    return stream


def _quantiseInto(bitDepth, dither=None):
    """The unfused output edge: moe_to_output straight on a step's (C, H, W) result.  toFloat's fp32 copy of an fp16 result is skipped: fp16 -> fp32 is exact and the
    kernel widens each value itself, so the samples are toOutput(toFloat(y))'s."""
    lib_dt = _outStorage(bitDepth)[2]
    bits = int(bitDepth) | quant.flags(dither, bitDepth, 'rgb')

    def f(y, out):
        import torch
        if y.dtype not in _DT:
            y = y.float()
        y = y.contiguous()
        C, H, W = y.shape
        if tuple(out.shape) != (H, W, C):
            raise ValueError('frame stream: the chain gave {} where {} was planned'.format((H, W, C), tuple(out.shape)))
        cur = torch.cuda.current_stream(y.device)
        _lib.check(_lib.lib().moe_to_output(y.data_ptr(), _DT[y.dtype], H, W, C, bits, out.data_ptr(), lib_dt, y.device.index or 0, cur.cuda_stream))
        y.record_stream(cur)
    return f


def genFrameStream(steps, width, height, depth=2, timing=False, reuse=False, views=False):
    """genProcess for a video source as a stream: `steps` as genProcess takes them, steps[0] = {'op': 'buffer', 'bitDepth': 8 | 16}; frames are width x height x 3.
    Returns a FrameStream: push(raw) -> list of finished frames' bytes (input order; [] for an empty buffer), flush(), close(), nodes.  The last compute step decides
    the output edge, named by the stream's `edge`: 'crop' -- an SR without ensemble or a DN of strength 1 folds its tiles straight into the encoder's samples
    (doCropOut: the canvas never exists); 'filter' -- a DN of any other finite strength does the same with the blend inside the fold (filterOut, under
    config.filterOnDevice); 'quantise' -- after a resize, an ensemble or otherwise the step's result is quantised in place.  Same bytes as genProcess + runFrames.
    With an {'op': 'output', 'pixFmt': ..} step the finished frames are the encoder's planar Y'CbCr 4:2:0 frames (moephoto_amd/pixfmt.py): the 'crop' edge folds its
    tiles straight into them (doCropYuv); every other chain ends in toYuv on the step's result (a 'filter' chain blends in RGBFilter first).
    With steps[0] = {'op': 'buffer', 'pixFmt': ..} the frames pushed are the decoder's planar Y'CbCr 4:2:0 frames (pixfmt.frameBytes bytes, even width and height), the
    chain runs on Y' and on Cb / Cr as two images and the finished frames are planar again, at the source's format or the output step's: 'crop' -- two doCropPlanes
    folds write straight into the frame -- or 'quantise' (toPlanes); no resize step, no matrix / order (ValueError before a model is loaded).
    reuse=True (either source kind, every edge): the stream keeps each step's tile pool from the previous frame and runs only the tiles whose input changed bit for
    bit -- frames shown twice, static shots, slides; the finished frames are the same bytes.  `stream.reuse` then holds the counters (tiles
    planned / run per step and image, plane-tile pixels planned / run over the stream; None without reuse).
    With 'chroma': 'nearest' | 'bilinear' | 'bicubic' on a planar source step (and 'chromaLoc': 'center' | 'left', the horizontal siting) the chain is luma-only: it
    runs on Y' exactly as above and the frame's Cb / Cr planes are written by one moe_chroma_resample from the source's chroma codes (pixfmt.resampleChroma: integers,
    byte for byte); 'chroma': 'net', the default, is the two-image form.  With reuse the change map and `stream.reuse` cover Y only.
    views=True: push / flush return read-only memoryviews (flat, format 'B') of the ring's pinned output buffers instead of bytes -- no copy is made.  A view is valid
    until the NEXT push, flush or close on this stream: frame k's slot is next written by the download that push(k + depth) enqueues, and that push is the first call
    after the one that returned frame k.  Whoever needs a frame for longer copies it (bytes(view)); stats['tobytes_ms'] then reads about 0.
    With {'op': 'output', 'width': W, 'height': H, 'fit': 'nearest' | 'bilinear' | 'bicubic'} on a planar chain ('fit' defaults to 'bicubic', 'pixFmt' stays optional)
    the finished frames are W x H: the edge runs at 16 bits into one intermediate of the chain's own size and one moe_fit_run per image (Y'; Cb / Cr) writes the
    slot's frame -- a rational integer polyphase filter that antialiases where it shrinks (pixfmt.fitPlanes: integers, byte for byte); `edge` reads 'crop+fit' or
    'quantise+fit'.  A luma-only chain fits Cb / Cr in one pass from the source's codes instead.  W and H are positive even ints within 4 down and 16 up of the chain's
    own size (ValueError before a model is loaded); on a chain whose source is not planar the three keys are refused -- it has a resize step.
    With 'chroma': 'nearest' | 'bilinear' | 'bicubic' on an SR or DN step of a chain whose source is NOT planar (and 'chromaMatrix': 'bt709' | 'bt601' | 'bt2020nc',
    'order': 'bgr' -- the default behind a buffer -- | 'rgb') that step is luma-only: it runs on Y' = (kr r + kg g) + kb b alone and the full-range Cb / Cr planes go to
    its output size through moe_resize with the method named (moephoto_amd/luma.py is the definition).  A last step that is an SR without ensemble or a DN of strength 1
    keeps edge 'crop': its fold merges Y' with the resized chroma planes and writes the encoder's samples (doCropLuma); every other position or form -- a step that is
    not last, an ensemble, a blended DN, a chain with an {'op': 'output', 'pixFmt': ..} step -- merges unfused (lumaMerge) and the edge is what it is without the key
    for that chain's tail ('quantise').  'chroma': 'net', the default, is today's path; 'chromaMatrix' / 'order' beside it, unknown values, and any of the three keys on
    a step of a planar chain raise ValueError naming the key before a model is loaded.  reuse=True works unchanged: the change map applies to Y' as it is
    (DESIGN.md section 17).
    With {'op': 'output', 'dither': 'round' | 'ordered'} whichever edge the chain ends in rounds to nearest or adds the 8 x 8 ordered dither instead of truncating
    (_outputDither; moephoto_amd/quant.py): at every ring depth, with reuse and with views, the same bytes as genProcess + runFrames.  On a luma-only planar chain the key
    governs Y' alone (Cb / Cr come from the integer filter, which rounds to nearest); beside 'width' / 'height' / 'fit' it is refused.
    With {'op': 'resize', 'width': W, 'height': H, 'fit': 'nearest' | 'bilinear' | 'bicubic'} (or 'scaleW' / 'scaleH') as the last compute step of a chain whose source
    is not planar the finished frames are W x H x 3 at the chain's bitDepth: the edge the chain ends in without that step ('crop', 'filter' or 'quantise') writes 16-bit
    samples of the chain's own size into one more device buffer per slot, and one moe_fit_run on the interleaved frame writes the slot's frame -- pixfmt.fitPixels of
    those samples, byte for byte; `edge` reads 'crop+fit', 'filter+fit' or 'quantise+fit'.  reuse and views work unchanged.  Refused by key before a model is loaded:
    such a step anywhere else, 'method' beside 'fit', an unknown 'fit', an axis without a size, 'dither' or 'pixFmt' on the output step, a ratio beyond 4 down or 16 up
    of the chain's own size -- known from the step dicts alone (_chainSize: the SR steps' scales, the resize steps' sizes) -- (DESIGN.md section 19).
    With 'chroma': 'guided' on a planar source step (and 'chromaLoc') the chain is luma-only as with 'bicubic', and the frame's Cb / Cr planes are written by one
    moe_chroma_guided behind the Y edge, on the compute stream: a joint bilateral filter over the source's chroma codes, steered by the source's Y' and by the Y' plane
    the edge has just written into the slot's frame (pixfmt.guidedChroma: integers, byte for byte).  It runs every frame; reuse, views and every ring depth work
    unchanged.  Refused before a model is loaded: a chain of total scale 1 and 'width' / 'height' / 'fit' on the output step.
    With {'op': 'output', 'pixFmt': 'bgr24' | 'rgb24' | 'bgr48le' | 'rgb48le'} on a planar chain the finished frames are interleaved RGB, 3 W H samples of 8 or 16
    bits: the chain's edge -- 'crop', 'quantise', the chroma pass, the fit -- runs at 16 bits into one intermediate planar frame (compute queue only) and one
    moe_planes_to_rgb writes the slot's frame, every frame: pixfmt.toRGB of the frame the same list yields with 'yuv420p16le', byte for byte; `edge` gains '+rgb'.
    Beside such a pixFmt the step takes 'matrix' ('bt709'), 'chromaUp' ('nearest' | 'bilinear' | 'bicubic': the final x2 of the chroma planes), 'chromaLoc' ('center' |
    'left': H.264 / HEVC material is 'left') and 'dither', which then governs the conversion's rounding; 'order' stays refused (the format's name carries it), so do
    'chromaUp' / 'chromaLoc' without an RGB pixFmt and unknown values, before a model is loaded.  reuse and views work unchanged.
    With {'op': 'lut', 'file': path} or {'op': 'lut', 'table': array, 'vertices': array} (and 'strength') as the last compute step of a chain whose frames are
    interleaved RGB samples -- an RGB source, or a planar one with an RGB pixFmt on the output step -- the chain ends in a 3D LUT: the edge the chain ends in without
    the step (the fold, the quantiser, the 'fit' kernel, moe_planes_to_rgb) writes 16-bit samples into one intermediate (allocated at the first frame, compute queue
    only) and one moe_lut3d_run writes the slot's frame at the depth asked for, every frame: lut3d.apply of the 16-bit frame the same list yields without the step,
    byte for byte; `edge` gains '+lut'.  'dither' on the output step governs the step's one quantisation.  reuse and views work unchanged.  Refused by key before a
    model is loaded: a 'lut' step that is not the last compute step, two of them, both or neither of 'file' / 'table', 'vertices' without 'table', a planar Y'CbCr
    sink, a strength that is not finite, a table lut3d.check refuses."""
    steps = [dict(s) for s in steps]
    if not steps or steps[0].get('op') != 'buffer':
        raise ValueError("frame stream: the first step must be {'op': 'buffer', 'bitDepth': 8 | 16}")
    planar = _planeFormats(steps, width, height)
    _lumaCheck(steps, bool(planar))
    dither = _outputDither(steps)          # (before any model is loaded)
    if planar:          # {'op': 'buffer', 'pixFmt': ..}: the decoder's own Y'CbCr 4:2:0 planes in, planar frames out ('crop' or 'quantise'; a blended DN is a 'quantise' chain)
        return _genFrameStreamPlanes(_withoutLut(steps), planar, width, height, depth, timing, reuse, views, dither, _lutStep(steps, planar))
    _refuseFit(steps)
    bitDepth = int(steps[0].get('bitDepth', 16))
    lut = _lutStep(steps, None, bitDepth)          # (before any model is loaded)
    steps = _withoutLut(steps)
    if lut:          # the chain's edge writes 16-bit samples without 'dither': the key governs the step's quantiser
        lutDither, dither = dither, None
    _checkRing(depth, bitDepth)          # (before any model is loaded)
    yuv = _outputFormat(steps)           # (likewise)
    _checkReuse(reuse)                   # (likewise)
    _checkViews(views)                   # (likewise)
    fit = _pixelFit(steps, bitDepth)     # (likewise)
    edgeDepth = 16 if fit or lut else bitDepth          # (a 'fit' resize step: the edge writes 16-bit samples of the chain's own size, the slot's frame is the filter's; a 'lut' step likewise)
    yuvOf = toYuv(*yuv, dither=dither) if yuv else None
    work = [s for s in steps if s['op'] not in ('file', 'buffer', 'output') and s is not fit]
    for opt in work:
        if opt['op'] not in stepOpts:
            raise NotImplementedError('op "{}" is not part of the SR/DN hot path this engine implements'.format(opt['op']))
    funcs, nodes, edge, edgeName, rsteps = [], [], None, 'quantise', []
    h, w = int(height), int(width)
    if fit and _chainSize(work, h, w):          # the fit's ratio against the chain's own size, known here from the step dicts: refused before any model is loaded
        _pixelFitSize(fit, *_chainSize(work, h, w))
    for k, opt in enumerate(work):
        op, last = opt['op'], k == len(work) - 1
        so = stepOpts[op]
        convertValues(int, opt, so.get('toInt', []))
        convertValues(float, opt, so.get('toFloat', []))
        if op == 'resize':
            funcs.append(resize(opt, dict(source=True)))
            rsteps.append(('resize', funcs[-1], opt))
            h = round(h * opt['scaleH']) if 'scaleH' in opt else opt['height']
            w = round(w * opt['scaleW']) if 'scaleW' in opt else opt['width']
            nodes.append(dict(op='resize', mode=opt['method']))
            continue
        o = so['getOpt'].getOpt(opt)
        if o is None:
            raise ValueError('unknown model for step {}'.format(opt))
        opt['opt'] = o
        if op == 'SR' and not opt['scale'] > 1:
            raise TypeError('Invalid scale setting for SR.')
        if _isLuma(o):          # a luma-only step: the merge rides in the last fold where that fold writes the samples; every other position or form merges unfused
            if last and not yuv and (o.ensemble == 0 if op == 'SR' else o.strength == 1):
                edge, edgeName = (lambda x, out, reuse=None, o=o, prepare=o.prepare if op == 'DN' else identity:
                                  doCropLuma(o, prepare(x), o.chroma, o.chromaMatrix, o.order, edgeDepth, out, reuse=reuse, dither=dither)), 'crop'
            else:
                f, r = _lumaStep(op, o)
                funcs.append(f)
                rsteps.append(r)
            if op == 'SR':
                h, w = h * opt['scale'], w * opt['scale']
        elif op == 'SR':
            if last and o.ensemble == 0:
                edge, edgeName = (lambda x, out, reuse=None, o=o: doCropYuv(o, x, yuv[0], out, *yuv[1:], reuse=reuse, dither=dither) if yuv
                                  else doCropOut(o, x, edgeDepth, out, reuse=reuse, dither=dither)), 'crop'
            else:
                funcs.append(runSR.sr(o))
                rsteps.append(_reuseSR(o, funcs[-1]))
            h, w = h * opt['scale'], w * opt['scale']
        elif last and o.strength == 1:         # RGBFilter on three planes with nothing to blend: prepare, doCrop
            edge, edgeName = (lambda x, out, reuse=None, o=o: doCropYuv(o, o.prepare(x), yuv[0], out, *yuv[1:], reuse=reuse, dither=dither) if yuv
                              else doCropOut(o, o.prepare(x), edgeDepth, out, reuse=reuse, dither=dither)), 'crop'
        elif last and config.filterOnDevice and isinstance(o.strength, (int, float)) and math.isfinite(o.strength):      # the blend with the frame inside the fold
            edge, edgeName = (lambda x, out, reuse=None, o=o: yuvOf(_RGBFilter(o, x, reuse), out) if yuv else filterOut(o, x, edgeDepth, out, reuse=reuse, dither=dither)), 'filter'
        else:
            funcs.append(RGBFilter(o))
            rsteps.append(_reuseDN(o))
        nodes.append(dict(op=op, model=opt.get('model'), scale=opt.get('scale', 1)))
    tiledEdge = edge is not None
    if edge is None:
        edge = yuvOf or _quantiseInto(edgeDepth, dither)
    outHW, fitted = (h, w), None
    if fit:          # the edge above fills the slot's 16-bit samples of h x w; one moe_fit_run from them writes the slot's frame, behind everything reuse touches
        outHW = _pixelFitSize(fit, h, w)
        fitted = ((h, w), fitPixels(16, 16 if lut else bitDepth, 3, h, w, outHW[0], outHW[1], fit['fit']))
        edgeName += '+fit'
        nodes.append(dict(op='resize', mode=fit['fit']))
    if lut:          # the edge (and the fit) above write one intermediate frame at 16 bits (compute queue only); one moe_lut3d_run from it writes the slot's frame, every frame
        import torch
        lutRun, mid16, (lh, lw) = _lutRunner(lut, 16, bitDepth, lutDither), {}, outHW
        edgeName += lut['edge']
        nodes.append(dict(op=lut['op']))

        def lutMid(dev):
            if 'buf' not in mid16:          # allocated once, at the first frame
                mid16['buf'] = torch.empty((lh, lw, 3), dtype=_outStorage(16)[0], device=dev)
            return mid16['buf']
        if fit:
            fitRun = fitted[1]

            def fitThenLut(mid, out):
                buf = lutMid(out.device)
                fitRun(mid, _flatBytes(buf))
                lutRun(_flatBytes(buf), out, lh, lw)
            fitted = (fitted[0], fitThenLut)
        else:
            plainEdge = edge

            def edge(x, out, *reuses):
                buf = lutMid(out.device)
                plainEdge(x, buf, *reuses)
                lutRun(_flatBytes(buf), _flatBytes(out), lh, lw)
    state = _ReuseState(rsteps, tiledEdge) if reuse else None
    backend = _DeviceBackend(funcs, edge, bitDepth, width, height, outHW, depth, timing, pixfmt.frameBytes(yuv[0], w, h) if yuv else None, state, views, fitted)
    stream = FrameStream(backend, width, height, bitDepth, depth, nodes)
    stream.edge, stream.reuse = edgeName, (state.stats if reuse else None)
    return stream


def runFramesStreamed(stream, read, write, start=0, stop=-1):
    """runFrames over a FrameStream: the same frames reach `write` in the same order and the same count is returned; they arrive up to depth - 1 reads later.  A short
    frame raises the same ValueError after every frame already pushed has been written.  A stream built with views=True hands `write` read-only memoryviews of the
    ring's pinned buffers: each is valid only until the next push / flush on the stream, and every frame is written here before the next push -- a `write` that keeps a
    frame beyond its own call must copy it."""
    i = n = 0

    def hand(bufs):
        nonlocal n
        for buf in bufs:
            if buf:
                write(buf)
                n += 1
    while stop < 0 or i <= stop:
        raw = read(stream.frameBytes)
        if len(raw) == 0:
            break
        if len(raw) != stream.frameBytes:
            hand(stream.flush())
            raise ValueError('short frame: {} of {} bytes'.format(len(raw), stream.frameBytes))
        if i >= start:
            hand(stream.push(raw))
        i += 1
    hand(stream.flush())
    return n
